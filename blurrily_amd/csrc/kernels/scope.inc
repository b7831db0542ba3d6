// kernels/scope.inc -- scoped find (blurrily_storage_find_in / _find_batch_in[_device], DESIGN.md section 12).
// Part of find_kernels.hip (timed build only: included in namespace blurrily, in front of the launch functions).
//
//   scope_mask_kernel   the mask strategy's bitmaps: a member refs_lookup_kernel found clears its rank's bit in its
//                       image's mask (the launch sets every bit first).  Deleted ranks were never found, so the mask
//                       excludes them as the tombstone bitmap would.
//   scope_find_kernel   the direct strategy: one workgroup per needle.  The needle is tokenised straight into an LDS
//                       bitmap of kNumCodes bits (duplicates fall together); lanes walk the members' code lists (member
//                       per lane, L2-resident for the scopes this serves) and keep each member's matches as a byte in
//                       LDS with a histogram of the values.  A suffix scan of the histogram gives the limit's threshold
//                       value t: every member above t is a row, and of the members at t the first ones in member order
//                       -- (weight, reference) order, the rows' order among equal matches -- fill the rest, counted by
//                       ballots chunk after chunk.  At most `limit` candidates remain; each finds its row by counting
//                       the candidates in front of it.  Exact by construction: no pool to overflow, no second pass.
//   scope_each_kernel   the same find with a scope of its own per needle (DESIGN.md section 13): one launch for every
//                       needle served directly, whatever its scope; the needle a string or a reference's codes.
//   scope_gather_*, scope_scatter_kernel   the needles of a group the sweeps serve compacted, and their rows put back.

namespace {

constexpr uint32_t kScopeThreads  = 256;
constexpr uint32_t kScopeMapWords = (kNumCodes + 31) / 32;   // 686: the needle's code set

__global__ void scope_mask_kernel(const ScopeMaskArgs A) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const uint2 loc = A.loc[i];
  if (loc.x == 0xFFFFFFFFu) return;                     // not held (never put, or deleted)
  const uint32_t k = (A.n_img > 1 && loc.x >= A.win0[1]) ? 1u : 0u;
  const uint32_t rank = (loc.x - A.win0[k]) * kWindowRanks + loc.y;
  atomicAnd(&A.mask[k][rank >> 5], ~(1u << (rank & 31u)));
}

// The LDS a direct find works in: the needle's code set, the histogram of the members' matches and its suffix scan,
// the candidates, and the select's scalars.
struct ScopeScalars {
  uint32_t len, thr, above, need, taken, n_pool, wave[kScopeThreads / 64];
};

// The needle's code set from its string (a C string within cap bytes, storage.c:480): "**" + s + "*", the trigram at k
// is sym(s[k-2]) + 28 sym(s[k-1]) + 784 sym(s[k]), '*' outside s (tokeniser.c:62-75).  Clears s_hist; ends at a barrier.
__device__ __forceinline__ void scope_map_string(uint32_t* s_map, uint32_t* s_hist, ScopeScalars& S, const char* s,
                                                 uint32_t cap, uint32_t tid) {
  for (uint32_t w = tid; w < kScopeMapWords; w += kScopeThreads) s_map[w] = 0u;
  s_hist[tid] = 0u;
  if (tid == 0) { S.len = cap; S.taken = 0u; S.n_pool = 0u; }
  __syncthreads();
  for (uint32_t k = tid; k < cap; k += kScopeThreads)
    if (s[k] == 0) atomicMin(&S.len, k);
  __syncthreads();
  const uint32_t len = S.len;
  for (uint32_t k = tid; k <= len; k += kScopeThreads) {
    const uint32_t a = k >= 2 ? dev_symbol((unsigned char)s[k - 2]) : 0u;
    const uint32_t b = k >= 1 ? dev_symbol((unsigned char)s[k - 1]) : 0u;
    const uint32_t c = k < len ? dev_symbol((unsigned char)s[k]) : 0u;
    const uint32_t code = a + 28u * b + 784u * c;
    atomicOr(&s_map[code >> 5], 1u << (code & 31u));
  }
  __syncthreads();
}

// ... or from a reference's extracted codes (refs_extract: distinct, ntri of them).  Ends at a barrier.
__device__ __forceinline__ void scope_map_codes(uint32_t* s_map, uint32_t* s_hist, ScopeScalars& S, const uint16_t* codes,
                                                uint32_t ntri, uint32_t tid) {
  for (uint32_t w = tid; w < kScopeMapWords; w += kScopeThreads) s_map[w] = 0u;
  s_hist[tid] = 0u;
  if (tid == 0) { S.taken = 0u; S.n_pool = 0u; }
  __syncthreads();
  for (uint32_t k = tid; k < ntri; k += kScopeThreads) {
    const uint32_t code = codes[k];
    atomicOr(&s_map[code >> 5], 1u << (code & 31u));
  }
  __syncthreads();
}

// Every member's matches against the needle's code set, the limit's threshold, and the rows: rows[0, n_rows), *count.
__device__ __forceinline__ void scope_score_rows(const uint32_t* s_map, uint32_t* s_hist, uint32_t* s_suf,
                                                 uint32_t* s_pool, ScopeScalars& S, uint8_t* s_match,
                                                 const uint32_t* m_off, const uint16_t* m_codes, const uint32_t* m_ref,
                                                 const uint32_t* m_weight, uint32_t n_members, uint32_t limit,
                                                 trigram_match_t* rows, uint32_t* count, uint32_t tid) {
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  // every member's matches: the needle's codes among its own (distinct, at most kScopeMaxMemberCodes of them)
  for (uint32_t i = tid; i < n_members; i += kScopeThreads) {
    const uint32_t b0 = m_off[i], b1 = m_off[i + 1];
    uint32_t c = 0;
    for (uint32_t j = b0; j < b1; ++j) {
      const uint32_t code = m_codes[j];
      c += (s_map[code >> 5] >> (code & 31u)) & 1u;
    }
    s_match[i] = uint8_t(c);
    if (c) atomicAdd(&s_hist[c], 1u);
  }
  __syncthreads();
  // s_suf[v]: members with at least v matches (v >= 1)
  s_suf[tid] = tid ? s_hist[tid] : 0u;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint32_t v = tid + d < 256 ? s_suf[tid + d] : 0u;
    __syncthreads();
    s_suf[tid] += v;
    __syncthreads();
  }
  // the threshold: the largest t >= 1 with at least `limit` members at t or above (t = 1 when there are fewer)
  const bool at_or_above = tid >= 1 && s_suf[tid] >= limit;
  const bool next_below = tid == 255 || s_suf[tid + 1] < limit;
  if ((at_or_above && next_below) || (tid == 1 && s_suf[1] < limit)) {
    const uint32_t above = tid == 255 ? 0u : s_suf[tid + 1];
    S.thr = tid; S.above = above; S.need = min(limit - above, s_hist[tid]);
  }
  __syncthreads();
  const uint32_t thr = S.thr, above = S.above, need = S.need;
  // every member above the threshold (fewer than `limit`)
  for (uint32_t i = tid; i < n_members; i += kScopeThreads)
    if (s_match[i] > thr) s_pool[atomicAdd(&S.n_pool, 1u)] = i;
  // ... and the first `need` members at it, in member order
  for (uint32_t base = 0; base < n_members; base += kScopeThreads) {
    if (S.taken >= need) break;                         // (uniform: written before the last barrier)
    const uint32_t i = base + tid;
    const bool at = i < n_members && s_match[i] == thr;
    const unsigned long long bal = __ballot(at);
    if (lane == 0) S.wave[wave] = uint32_t(__popcll(bal));
    __syncthreads();
    uint32_t pos = S.taken;
    for (uint32_t w = 0; w < wave; ++w) pos += S.wave[w];
    pos += uint32_t(__popcll(bal & ((1ull << lane) - 1ull)));
    if (at && pos < need) s_pool[above + pos] = i;
    __syncthreads();
    if (tid == 0) {
      uint32_t t = S.taken;
      for (uint32_t w = 0; w < kScopeThreads / 64; ++w) t += S.wave[w];
      S.taken = t;
    }
    __syncthreads();
  }
  __syncthreads();
  // rows: a candidate's place is the number of candidates before it (matches descending, member order)
  const uint32_t n_rows = above + need;
  for (uint32_t j = tid; j < n_rows; j += kScopeThreads) {
    const uint32_t i = s_pool[j], mi = s_match[i];
    uint32_t rank = 0;
    for (uint32_t k = 0; k < n_rows; ++k) {
      const uint32_t o = s_pool[k], mo = s_match[o];
      rank += (mo > mi || (mo == mi && o < i)) ? 1u : 0u;
    }
    trigram_match_t* row = rows + rank;
    row->reference = m_ref[i];
    row->matches = mi;
    row->weight = m_weight[i];
  }
  if (tid == 0) *count = n_rows;
}

__global__ __launch_bounds__(kScopeThreads) void scope_find_kernel(const ScopeFindArgs A) {
  __shared__ uint32_t s_map[kScopeMapWords];
  __shared__ uint32_t s_hist[256], s_suf[256];
  __shared__ uint32_t s_pool[kScopeMaxKeep];
  __shared__ ScopeScalars S;
  extern __shared__ uint8_t s_match[];                  // [n_members] matches of every member
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  const uint64_t beg = A.offsets[q];
  const uint32_t cap = uint32_t(min<uint64_t>(A.offsets[q + 1] - beg, 0xFFFFFFF0ull));
  scope_map_string(s_map, s_hist, S, A.packed + beg, cap, tid);
  scope_score_rows(s_map, s_hist, s_suf, s_pool, S, s_match, A.m_off, A.m_codes, A.m_ref, A.m_weight, A.n_members,
                   A.limit, A.results + size_t(q) * A.limit, A.counts + q, tid);
}

// Each needle against its own scope: workgroup b serves needle order[b].x with scope order[b].y's direct form (the
// host orders the workgroups by descending member count, so the longest ones start first).  Dynamic LDS: a byte per
// member of the largest scope in the launch.
__global__ __launch_bounds__(kScopeThreads) void scope_each_kernel(const ScopeEachArgs A) {
  __shared__ uint32_t s_map[kScopeMapWords];
  __shared__ uint32_t s_hist[256], s_suf[256];
  __shared__ uint32_t s_pool[kScopeMaxKeep];
  __shared__ ScopeScalars S;
  extern __shared__ uint8_t s_match[];                  // [n_members of this workgroup's scope]
  const uint32_t tid = threadIdx.x;
  const uint2 job = A.order[blockIdx.x];
  const uint32_t q = job.x;
  const ScopeDirect D = A.scopes[job.y];
  if (A.codes) {
    scope_map_codes(s_map, s_hist, S, A.codes + (A.qoff[q] + q), A.ntri[q], tid);
  } else {
    const uint64_t beg = A.offsets[q];
    const uint32_t cap = uint32_t(min<uint64_t>(A.offsets[q + 1] - beg, 0xFFFFFFF0ull));
    scope_map_string(s_map, s_hist, S, A.packed + beg, cap, tid);
  }
  scope_score_rows(s_map, s_hist, s_suf, s_pool, S, s_match, D.m_off, D.m_codes, D.m_ref, D.m_weight, D.n_members,
                   A.limit, A.results + size_t(q) * A.limit, A.counts + q, tid);
}

// Groups served by the sweeps: their needles compacted in front of the launches (strings: byte ranges to the offsets
// the host computed; references: the extracted descriptors, the codes left where they are), and their rows and counts
// put back in the caller's order.
__global__ void scope_gather_strings_kernel(const char* __restrict__ packed, const uint64_t* __restrict__ offsets,
                                            const uint32_t* __restrict__ idx, const uint64_t* __restrict__ out_off,
                                            uint32_t n, char* __restrict__ out) {
  for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
    const uint64_t src = offsets[idx[k]], dst = out_off[k], len = out_off[k + 1] - dst;
    for (uint64_t b = threadIdx.x; b < len; b += blockDim.x) out[dst + b] = packed[src + b];
  }
}

__global__ void scope_gather_refs_kernel(const RefNeedles R, const uint32_t* __restrict__ idx, uint32_t n,
                                         uint64_t* __restrict__ qoff, uint32_t* __restrict__ ntri,
                                         uint32_t* __restrict__ weight) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t q = idx[k];
  qoff[k] = R.qoff[q] + q - k;                          // (codes + qoff[k] + k: reference q's codes; never below the pad)
  ntri[k] = R.ntri[q];
  weight[k] = R.weight[q];
}

__global__ void scope_scatter_kernel(const trigram_match_t* __restrict__ rows, const uint32_t* __restrict__ counts,
                                     const uint32_t* __restrict__ idx, uint32_t n, uint32_t limit,
                                     trigram_match_t* __restrict__ out_rows, uint32_t* __restrict__ out_counts) {
  for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
    const uint32_t q = idx[k], c = counts[k];
    if (threadIdx.x == 0) out_counts[q] = c;
    for (uint32_t j = threadIdx.x; j < c; j += blockDim.x) out_rows[size_t(q) * limit + j] = rows[size_t(k) * limit + j];
  }
}

}  // namespace

// ------------------------------------------------------------------ launch ---

int launch_scope_mask(const ScopeMaskArgs& a, hipStream_t stream) {
  for (uint32_t k = 0; k < a.n_img; ++k)
    BLURRILY_HIP_TRY(hipMemsetAsync(a.mask[k], 0xFF, size_t(a.mask_words[k]) * sizeof(uint32_t), stream));
  if (a.n == 0) return 0;
  hipLaunchKernelGGL(scope_mask_kernel, dim3((a.n + 255) / 256), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_scope_find(const ScopeFindArgs& a, hipStream_t stream) {
  if (a.n == 0) return 0;
  if (a.limit == 0 || a.limit > kScopeMaxKeep || a.n_members > kScopeMaxMembers) { errno = EINVAL; return -1; }
  note_launch("scope_find_kernel");
  const size_t lds = (size_t(a.n_members) + 3) & ~size_t(3);
  hipLaunchKernelGGL(scope_find_kernel, dim3(a.n), dim3(kScopeThreads), lds, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_scope_each(const ScopeEachArgs& a, hipStream_t stream) {
  if (a.n == 0) return 0;
  if (a.limit == 0 || a.limit > kScopeMaxKeep || a.max_members > kScopeMaxMembers) { errno = EINVAL; return -1; }
  note_launch("scope_each_kernel");
  const size_t lds = (size_t(a.max_members) + 3) & ~size_t(3);
  hipLaunchKernelGGL(scope_each_kernel, dim3(a.n), dim3(kScopeThreads), lds, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_scope_gather_strings(const char* packed, const uint64_t* offsets, const uint32_t* idx, const uint64_t* out_off,
                                uint32_t n, char* out, hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(scope_gather_strings_kernel, dim3(std::min<uint32_t>(n, 65536u)), dim3(64), 0, stream, packed,
                     offsets, idx, out_off, n, out);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_scope_gather_refs(const RefNeedles& r, const uint32_t* idx, uint32_t n, uint64_t* qoff, uint32_t* ntri,
                             uint32_t* weight, hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(scope_gather_refs_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, r, idx, n, qoff, ntri, weight);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_scope_scatter(const trigram_match_t* rows, const uint32_t* counts, const uint32_t* idx, uint32_t n,
                         uint32_t limit, trigram_match_t* out_rows, uint32_t* out_counts, hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(scope_scatter_kernel, dim3(std::min<uint32_t>(n, 65536u)), dim3(64), 0, stream, rows, counts, idx, n,
                     limit, out_rows, out_counts);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}
