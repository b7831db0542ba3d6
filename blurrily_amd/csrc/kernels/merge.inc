// kernels/merge.inc -- latency mode's merge of per-range lists, and the merge of base and delta rows.
// Part of find_kernels.hip (included inside namespace blurrily, BLURRILY_KERNELS_BEGIN, the anonymous namespace).
// ---- latency mode, second half: merge the per-range candidates of every needle -------------
// One workgroup per needle: the best `keep` of the union of the per-range best `keep` keys is
// the needle's result (every range keeps its own top `keep`, so nothing can be lost).
template <int NT>
__global__ __launch_bounds__(NT) void merge_parts_kernel(const FindArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* pool = reinterpret_cast<unsigned long long*>(smem);
  Control* ctl = reinterpret_cast<Control*>(pool + A.pool_cap);
  const uint32_t tid = threadIdx.x;
  const uint32_t item = blockIdx.x, R = A.ranges;
  const uint32_t q = A.work_list ? A.work_list[item] : item;
  if (tid == 0) { ctl->pool_n = 0; ctl->overflow = 0; ctl->thr = kKeyInf; ctl->adm_n = 0; }
  __syncthreads();
  for (uint32_t r = 0; r < R; ++r) {
    const uint32_t slot = item * R + r;
    const uint32_t n = A.part_count[slot];
    if (tid < n) pool[atomicAdd(&ctl->pool_n, 1u)] = A.part_keys[size_t(slot) * A.keep + tid];
  }
  __syncthreads();
  compact_pool<NT>(pool, ctl, A.pool_cap, A.keep);
  const uint32_t nres = ctl->pool_n;
  const uint32_t T = A.q_ntri[q];
  trigram_match_t* out = A.results + size_t(q) * A.limit;
  for (uint32_t i = tid; i < nres; i += NT) {
    const unsigned long long key = pool[i];
    const uint32_t rk = uint32_t(key);
    trigram_match_t row;
    row.reference = A.ref_of_rank[rk];
    row.matches = T - uint32_t(key >> 32);
    row.weight = A.weight_of_rank[rk];
    out[i] = row;
  }
  if (tid == 0) A.counts[q] = nres;
}

// The same merge for a handful of needles tokenised on the host (host_batch.hip: find_few's latency-mode half): the rows go
// straight into host-coherent pinned memory -- rows[needle][kOneMaxKeep], words[needle] = {count, the launch's sequence
// word}, the word stored last and behind a system-scope fence; the host polls it (find_one_kernel's protocol) -- so that
// such a batch costs two launches and no copy, no stream synchronise.  Workgroup 0 hands the find launch's queue word
// back as zero.
template <int NT>
__global__ __launch_bounds__(NT) void merge_parts_pinned_kernel(const FindArgs A, trigram_match_t* rows, uint32_t* words,
                                                                const uint32_t seq) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* pool = reinterpret_cast<unsigned long long*>(smem);
  Control* ctl = reinterpret_cast<Control*>(pool + A.pool_cap);
  const uint32_t tid = threadIdx.x;
  const uint32_t q = blockIdx.x, R = A.ranges;
  if (tid == 0) { ctl->pool_n = 0; ctl->overflow = 0; ctl->thr = kKeyInf; ctl->adm_n = 0; }
  __syncthreads();
  for (uint32_t r = 0; r < R; ++r) {
    const uint32_t slot = q * R + r;
    const uint32_t n = A.part_count[slot];
    if (tid < n) pool[atomicAdd(&ctl->pool_n, 1u)] = A.part_keys[size_t(slot) * A.keep + tid];
  }
  __syncthreads();
  compact_pool<NT>(pool, ctl, A.pool_cap, A.keep);
  const uint32_t nres = ctl->pool_n;
  const uint32_t T = A.q_ntri[q];
  trigram_match_t* out = rows + size_t(q) * kOneMaxKeep;
  if (tid < nres) {                                       // (keep <= kOneMaxKeep < NT)
    const unsigned long long key = pool[tid];
    const uint32_t rk = uint32_t(key);
    trigram_match_t row;
    row.reference = A.ref_of_rank[rk];
    row.matches = T - uint32_t(key >> 32);
    row.weight = A.weight_of_rank[rk];
    out[tid] = row;
  }
  if (tid == 0) words[2 * q] = nres;
  if (tid < ((nres + 63u) & ~63u) || tid < 64) __threadfence_system();   // rows and count are in host memory before the sequence word
  __syncthreads();
  if (tid == 0) {
    __hip_atomic_store(&words[2 * q + 1], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (q == 0) *A.queue = 0;
  }
}

// Small limits (<= 64 rows, <= 256 ranges): the per-range lists are already sorted, so one wave
// merges them by repeated minimum extraction -- every lane watches the heads of up to four
// lists, a wave-wide minimum picks the winner, the winning lane advances -- instead of sorting
// all ranges x keep keys (1 290 keys for a single needle at Geonames scale).
__global__ __launch_bounds__(64) void merge_parts_small_kernel(const FindArgs A) {
  __shared__ unsigned long long s_win[64];
  const uint32_t lane = threadIdx.x;
  const uint32_t item = blockIdx.x, R = A.ranges, keep = A.keep;
  const uint32_t q = A.work_list ? A.work_list[item] : item;
  const uint32_t s0 = item * R + lane, s1 = s0 + 64, s2 = s0 + 128, s3 = s0 + 192;
  const uint32_t n0 = lane < R ? A.part_count[s0] : 0u, n1 = lane + 64 < R ? A.part_count[s1] : 0u;
  const uint32_t n2 = lane + 128 < R ? A.part_count[s2] : 0u, n3 = lane + 192 < R ? A.part_count[s3] : 0u;
  uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0;
  auto head = [&](uint32_t slot, uint32_t p, uint32_t n) {
    return p < n ? A.part_keys[size_t(slot) * keep + p] : kKeyInf;
  };
  unsigned long long h0 = head(s0, 0, n0), h1 = head(s1, 0, n1), h2 = head(s2, 0, n2), h3 = head(s3, 0, n3);
  uint32_t nres = 0;
  for (uint32_t k = 0; k < keep; ++k) {
    const unsigned long long mine = min(min(h0, h1), min(h2, h3));
    unsigned long long best = mine;
#pragma unroll
    for (int d = 32; d; d >>= 1) {
      const uint32_t lo = __shfl_xor(uint32_t(best), d), hi = __shfl_xor(uint32_t(best >> 32), d);
      const unsigned long long other = (static_cast<unsigned long long>(hi) << 32) | lo;
      best = min(best, other);
    }
    if (best == kKeyInf) break;
    if (mine == best) {                      // keys are distinct (distinct ranks): exactly one lane, one list
      if (h0 == best)      h0 = head(s0, ++p0, n0);
      else if (h1 == best) h1 = head(s1, ++p1, n1);
      else if (h2 == best) h2 = head(s2, ++p2, n2);
      else                 h3 = head(s3, ++p3, n3);
    }
    if (lane == 0) s_win[k] = best;
    ++nres;
  }
  __syncthreads();
  const uint32_t T = A.q_ntri[q];
  trigram_match_t* out = A.results + size_t(q) * A.limit;
  if (lane < nres) {
    const unsigned long long key = s_win[lane];
    const uint32_t rk = uint32_t(key);
    trigram_match_t row;
    row.reference = A.ref_of_rank[rk];
    row.matches = T - uint32_t(key >> 32);
    row.weight = A.weight_of_rank[rk];
    out[lane] = row;
  }
  if (lane == 0) A.counts[q] = nres;
}

// ---- base + delta: merge two per-needle result lists in result order ----------------------
// (matches descending, weight ascending, reference ascending; the two images hold disjoint
// references, so the first `limit` rows of the merge are the answer).  One lane per needle.
__global__ void merge_rows_kernel(const trigram_match_t* __restrict__ a_rows, const uint32_t* __restrict__ a_counts,
                                  const trigram_match_t* __restrict__ b_rows, const uint32_t* __restrict__ b_counts,
                                  uint32_t n, uint32_t limit, trigram_match_t* __restrict__ out,
                                  uint32_t* __restrict__ out_counts) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const trigram_match_t* a = a_rows + size_t(q) * limit;
  const trigram_match_t* b = b_rows + size_t(q) * limit;
  trigram_match_t* o = out + size_t(q) * limit;
  const uint32_t na = a_counts[q], nb = b_counts[q];
  uint32_t i = 0, j = 0, k = 0;
  while (k < limit && (i < na || j < nb)) {
    bool take_a;
    if (i >= na) take_a = false;
    else if (j >= nb) take_a = true;
    else {
      const trigram_match_t x = a[i], y = b[j];
      if (x.matches != y.matches) take_a = x.matches > y.matches;
      else if (x.weight != y.weight) take_a = x.weight < y.weight;
      else take_a = x.reference < y.reference;
    }
    o[k++] = take_a ? a[i++] : b[j++];
  }
  out_counts[q] = k;
}
