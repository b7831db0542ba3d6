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

__global__ __launch_bounds__(kScopeThreads) void scope_find_kernel(const ScopeFindArgs A) {
  __shared__ uint32_t s_map[kScopeMapWords];
  __shared__ uint32_t s_hist[256], s_suf[256];
  __shared__ uint32_t s_pool[kScopeMaxKeep];
  __shared__ uint32_t s_len, s_thr, s_above, s_need, s_taken, s_n_pool, s_wave[kScopeThreads / 64];
  extern __shared__ uint8_t s_match[];                  // [n_members] matches of every member
  const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t beg = A.offsets[q];
  const uint32_t cap = uint32_t(min<uint64_t>(A.offsets[q + 1] - beg, 0xFFFFFFF0ull));
  const char* s = A.packed + beg;
  for (uint32_t w = tid; w < kScopeMapWords; w += kScopeThreads) s_map[w] = 0u;
  s_hist[tid] = 0u;
  if (tid == 0) { s_len = cap; s_taken = 0u; s_n_pool = 0u; }
  __syncthreads();
  for (uint32_t k = tid; k < cap; k += kScopeThreads)   // a needle is a C string (storage.c:480)
    if (s[k] == 0) atomicMin(&s_len, k);
  __syncthreads();
  // "**" + s + "*": the trigram at k is sym(s[k-2]) + 28 sym(s[k-1]) + 784 sym(s[k]), '*' outside s (tokeniser.c:62-75)
  const uint32_t len = s_len;
  for (uint32_t k = tid; k <= len; k += kScopeThreads) {
    const uint32_t a = k >= 2 ? dev_symbol((unsigned char)s[k - 2]) : 0u;
    const uint32_t b = k >= 1 ? dev_symbol((unsigned char)s[k - 1]) : 0u;
    const uint32_t c = k < len ? dev_symbol((unsigned char)s[k]) : 0u;
    const uint32_t code = a + 28u * b + 784u * c;
    atomicOr(&s_map[code >> 5], 1u << (code & 31u));
  }
  __syncthreads();
  // every member's matches: the needle's codes among its own (distinct, at most kScopeMaxMemberCodes of them)
  for (uint32_t i = tid; i < A.n_members; i += kScopeThreads) {
    const uint32_t b0 = A.m_off[i], b1 = A.m_off[i + 1];
    uint32_t c = 0;
    for (uint32_t j = b0; j < b1; ++j) {
      const uint32_t code = A.m_codes[j];
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
  const uint32_t limit = A.limit;
  const bool at_or_above = tid >= 1 && s_suf[tid] >= limit;
  const bool next_below = tid == 255 || s_suf[tid + 1] < limit;
  if ((at_or_above && next_below) || (tid == 1 && s_suf[1] < limit)) {
    const uint32_t above = tid == 255 ? 0u : s_suf[tid + 1];
    s_thr = tid; s_above = above; s_need = min(limit - above, s_hist[tid]);
  }
  __syncthreads();
  const uint32_t thr = s_thr, above = s_above, need = s_need;
  // every member above the threshold (fewer than `limit`)
  for (uint32_t i = tid; i < A.n_members; i += kScopeThreads)
    if (s_match[i] > thr) s_pool[atomicAdd(&s_n_pool, 1u)] = i;
  // ... and the first `need` members at it, in member order
  for (uint32_t base = 0; base < A.n_members; base += kScopeThreads) {
    if (s_taken >= need) break;                         // (uniform: written before the last barrier)
    const uint32_t i = base + tid;
    const bool at = i < A.n_members && s_match[i] == thr;
    const unsigned long long bal = __ballot(at);
    if (lane == 0) s_wave[wave] = uint32_t(__popcll(bal));
    __syncthreads();
    uint32_t pos = s_taken;
    for (uint32_t w = 0; w < wave; ++w) pos += s_wave[w];
    pos += uint32_t(__popcll(bal & ((1ull << lane) - 1ull)));
    if (at && pos < need) s_pool[above + pos] = i;
    __syncthreads();
    if (tid == 0) {
      uint32_t t = s_taken;
      for (uint32_t w = 0; w < kScopeThreads / 64; ++w) t += s_wave[w];
      s_taken = t;
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
    trigram_match_t* row = A.results + size_t(q) * limit + rank;
    row->reference = A.m_ref[i];
    row->matches = mi;
    row->weight = A.m_weight[i];
  }
  if (tid == 0) A.counts[q] = n_rows;
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
