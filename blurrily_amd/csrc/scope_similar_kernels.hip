// scope_similar_kernels.hip -- the scoped similarity find's direct strategy (launch code:
// scope_similar.hip).
//
// scope_similar_kernel / scope_similar_each_kernel: one workgroup of 256 lanes per needle over a scope's direct form
// (the held members' code lists in (weight, reference) order).  The needle's code set goes into an LDS bitmap, from its
// string or from an extracted reference's codes; T is the bitmap's population count, or the reference's count.  Lanes
// walk the members (member per lane): m from the bitmap, R = m_off[i + 1] - m_off[i], the floor tested exactly in
// integers.  A member that is a row keeps m as a byte in LDS, any other keeps 0 -- the only pass over the code lists.
//
// A row's rank is decided by K = (floor(m 2^32 / u) - 1) << 8 | m, u = T + R - m < 2^16: the fixed-point quotient is
// exact and order-preserving for such denominators (similar.h), K < 2^40, and equal K means equal m and equal u, so
// equal R: member order is then the rows' order.  The best `limit` K are found by a radix select, a byte a step from
// the top: a histogram of the byte over the members that tie on the bytes above, a suffix scan, the byte value t where
// the count reaches what is still needed; the members above t are rows, those at t tie on one byte more.  It ends as
// soon as the ties are no more than are needed -- at once when fewer members pass the floor than `limit` -- or after
// the fifth byte, when the ties have equal K and the first ones in member order fill the rest, counted by ballots
// chunk after chunk.  A step recomputes K from the m byte and m_off (two 32-bit divisions); no member's codes are read
// twice, there is no pool that could overflow, no bar, no floating point.  At most `limit` candidates remain; each
// finds its row by counting the candidates in front of it.
//
// R is read again from m_off in each step instead of being kept as a second LDS byte per member: the LDS stays what
// the scoped find's is (a byte a member: 62 KiB at the cap of 57 344 members, two workgroups a CU, where two bytes
// would leave one), a step touches m_off only for members that passed the floor, and those eight bytes a member come
// from L2, where the scoring pass has just put them.
#include "scope_similar.h"
#include "hip_try.h"

namespace blurrily {

namespace {

constexpr uint32_t kSsThreads  = 256;
constexpr uint32_t kSsMapWords = (kNumCodes + 31) / 32;       // the needle's code set

__device__ __forceinline__ uint32_t ss_symbol(unsigned char c) {
  return (c >= 'a' && c <= 'z') ? uint32_t(c - 'a' + 1) : 0u;   // tokeniser.c:21-31
}

struct SsScalars {
  uint32_t len, T;
  unsigned long long prefix;     // the bytes of K decided so far
  uint32_t shift;                // ... which are K >> shift
  uint32_t above, need, ties, done;
  uint32_t taken, n_pool, wave[kSsThreads / 64];
};

// K of a row (m >= 1, u = T + R - m < 2^16)
__device__ __forceinline__ unsigned long long ss_key(uint32_t m, uint32_t T, uint32_t R) {
  const uint32_t u = T + R - m;
  const uint32_t q1 = (m << 16) / u, r1 = (m << 16) - q1 * u;   // m <= 255; r1 < u
  const uint32_t q2 = (r1 << 16) / u;                            // < 2^16
  const unsigned long long s = ((unsigned long long)q1 << 16) + q2;   // floor(m * 2^32 / u): 2^16 .. 2^32
  return ((s - 1ull) << 8) | m;
}

// The needle's code set from its string (a C string within cap bytes): "**" + s + "*", the trigram at k is
// sym(s[k-2]) + 28 sym(s[k-1]) + 784 sym(s[k]), '*' outside s (tokeniser.c:62-75).  Ends at a barrier.
__device__ __forceinline__ void ss_map_string(uint32_t* s_map, SsScalars& S, const char* s, uint32_t cap, uint32_t tid) {
  if (tid == 0) S.len = cap;
  __syncthreads();
  for (uint32_t k = tid; k < cap; k += kSsThreads)
    if (s[k] == 0) atomicMin(&S.len, k);
  __syncthreads();
  const uint32_t len = S.len;
  for (uint32_t k = tid; k <= len; k += kSsThreads) {
    const uint32_t a = k >= 2 ? ss_symbol((unsigned char)s[k - 2]) : 0u;
    const uint32_t b = k >= 1 ? ss_symbol((unsigned char)s[k - 1]) : 0u;
    const uint32_t c = k < len ? ss_symbol((unsigned char)s[k]) : 0u;
    const uint32_t code = a + 28u * b + 784u * c;
    atomicOr(&s_map[code >> 5], 1u << (code & 31u));
  }
  __syncthreads();
  uint32_t t = 0;
  for (uint32_t w = tid; w < kSsMapWords; w += kSsThreads) t += uint32_t(__popc(s_map[w]));
  if (t) atomicAdd(&S.T, t);
  __syncthreads();
}

// One needle (q: string or reference) against one direct form; rows at slot `out`.
__device__ __forceinline__ void ss_body(const ScopeSimilarArgs& A, uint32_t q, const ScopeDirect& D, uint32_t out) {
  __shared__ uint32_t s_map[kSsMapWords];
  __shared__ unsigned long long s_work[256];            // the select's histogram and suffix scan; then the candidates' K
  __shared__ uint32_t s_pool[kScopeMaxKeep];
  __shared__ SsScalars S;
  extern __shared__ uint8_t s_match[];                  // [n_members] m of every member that is a row, 0 of the others
  uint32_t* s_hist = reinterpret_cast<uint32_t*>(s_work);
  uint32_t* s_suf = s_hist + 256;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n_members = D.n_members, limit = A.limit;

  for (uint32_t w = tid; w < kSsMapWords; w += kSsThreads) s_map[w] = 0u;
  s_hist[tid] = 0u;
  if (tid == 0) {
    S.T = 0u; S.prefix = 0ull; S.shift = 40u; S.above = 0u; S.need = limit; S.ties = 0u; S.done = 0u;
    S.taken = 0u; S.n_pool = 0u;
  }
  __syncthreads();
  if (A.codes) {
    const uint16_t* codes = A.codes + (A.qoff[q] + q);
    const uint32_t ntri = A.ntri[q];
    for (uint32_t k = tid; k < ntri; k += kSsThreads) {
      const uint32_t code = codes[k];
      atomicOr(&s_map[code >> 5], 1u << (code & 31u));
    }
    if (tid == 0) S.T = ntri;
    __syncthreads();
  } else {
    const uint64_t beg = A.offsets[q];
    const uint32_t cap = uint32_t(min<uint64_t>(A.offsets[q + 1] - beg, 0xFFFFFFF0ull));
    ss_map_string(s_map, S, A.packed + beg, cap, tid);
  }
  const uint32_t T = S.T;
  if (T == 0) {                                         // (uniform) no trigram: no rows
    if (tid == 0) A.counts[out] = 0u;
    return;
  }

  // every member's m, the floor, and the first step's histogram: K's top byte
  for (uint32_t i = tid; i < n_members; i += kSsThreads) {
    const uint32_t b0 = D.m_off[i], b1 = D.m_off[i + 1];
    uint32_t c = 0;
    for (uint32_t j = b0; j < b1; ++j) {
      const uint32_t code = D.m_codes[j];
      c += (s_map[code >> 5] >> (code & 31u)) & 1u;
    }
    const uint32_t R = b1 - b0;
    const bool row = c >= 1u && 1000ull * c >= (unsigned long long)A.min_permille * (T + R - c);
    s_match[i] = row ? uint8_t(c) : uint8_t(0);
    if (row) atomicAdd(&s_hist[uint32_t(ss_key(c, T, R) >> 32)], 1u);
  }
  __syncthreads();

  // the select: s_hist holds, of the members that tie on K >> shift == prefix, the histogram of the next byte
  for (;;) {
    s_suf[tid] = s_hist[tid];
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {              // s_suf[v]: ties whose next byte is at least v
      const uint32_t v = tid + d < 256 ? s_suf[tid + d] : 0u;
      __syncthreads();
      s_suf[tid] += v;
      __syncthreads();
    }
    const uint32_t need = S.need, above = S.above, shift = S.shift, total = s_suf[0];
    const unsigned long long prefix = S.prefix;
    __syncthreads();
    if (total <= need) {                                 // every tie is a row
      if (tid == 0) { S.ties = total; S.done = 1u; }
    } else if (s_suf[tid] >= need && (tid == 255 || s_suf[tid + 1] < need)) {   // (one lane: need >= 1)
      const uint32_t up = tid == 255 ? 0u : s_suf[tid + 1];
      S.above = above + up; S.need = need - up; S.ties = s_hist[tid];
      S.prefix = (prefix << 8) | tid; S.shift = shift - 8u;
      S.done = (s_hist[tid] == need - up || shift == 8u) ? 1u : 0u;
    }
    __syncthreads();
    if (S.done) break;
    const uint32_t sh = S.shift;
    const unsigned long long pre = S.prefix;
    s_hist[tid] = 0u;
    __syncthreads();
    for (uint32_t i = tid; i < n_members; i += kSsThreads) {
      const uint32_t c = s_match[i];
      if (!c) continue;
      const unsigned long long K = ss_key(c, T, D.m_off[i + 1] - D.m_off[i]);
      if ((K >> sh) == pre) atomicAdd(&s_hist[uint32_t(K >> (sh - 8u)) & 255u], 1u);
    }
    __syncthreads();
  }
  const uint32_t sh = S.shift, above = S.above, need = min(S.need, S.ties);
  const unsigned long long pre = S.prefix;
  __syncthreads();                                       // (s_work changes hands: every lane has left the select)
  // every member above the ties (fewer than `limit`)
  for (uint32_t i = tid; i < n_members; i += kSsThreads) {
    const uint32_t c = s_match[i];
    if (!c) continue;
    const unsigned long long K = ss_key(c, T, D.m_off[i + 1] - D.m_off[i]);
    if ((K >> sh) > pre) {
      const uint32_t at = atomicAdd(&S.n_pool, 1u);
      s_pool[at] = i;
      s_work[at] = K;
    }
  }
  // ... and the first `need` ties, in member order
  for (uint32_t base = 0; base < n_members; base += kSsThreads) {
    if (S.taken >= need) break;                         // (uniform: written before the last barrier)
    const uint32_t i = base + tid;
    const uint32_t c = i < n_members ? s_match[i] : 0u;
    unsigned long long K = 0ull;
    if (c) K = ss_key(c, T, D.m_off[i + 1] - D.m_off[i]);
    const bool at = c && (K >> sh) == pre;
    const unsigned long long bal = __ballot(at);
    if (lane == 0) S.wave[wave] = uint32_t(__popcll(bal));
    __syncthreads();
    uint32_t pos = S.taken;
    for (uint32_t w = 0; w < wave; ++w) pos += S.wave[w];
    pos += uint32_t(__popcll(bal & ((1ull << lane) - 1ull)));
    if (at && pos < need) { s_pool[above + pos] = i; s_work[above + pos] = K; }
    __syncthreads();
    if (tid == 0) {
      uint32_t t = S.taken;
      for (uint32_t w = 0; w < kSsThreads / 64; ++w) t += S.wave[w];
      S.taken = t;
    }
    __syncthreads();
  }
  __syncthreads();
  // rows: a candidate's place is the number of candidates before it (K descending, member order)
  const uint32_t n_rows = above + need;
  trigram_match_t* rows = A.rows + size_t(out) * limit;
  for (uint32_t j = tid; j < n_rows; j += kSsThreads) {
    const uint32_t i = s_pool[j];
    const unsigned long long Ki = s_work[j];
    uint32_t rank = 0;
    for (uint32_t k = 0; k < n_rows; ++k) {
      const unsigned long long Ko = s_work[k];
      rank += (Ko > Ki || (Ko == Ki && s_pool[k] < i)) ? 1u : 0u;
    }
    trigram_match_t* row = rows + rank;
    row->reference = D.m_ref[i];
    row->matches = uint32_t(Ki & 255ull);
    row->weight = D.m_weight[i];
    if (A.row_ntri) A.row_ntri[size_t(out) * limit + rank] = D.m_off[i + 1] - D.m_off[i];
  }
  if (tid == 0) A.counts[out] = n_rows;
}

__global__ __launch_bounds__(kSsThreads) void scope_similar_kernel(const ScopeSimilarArgs A) {
  ss_body(A, blockIdx.x, A.one, blockIdx.x);
}

// Each needle against its own scope (the host orders the workgroups by descending member count, so the longest ones
// start first).  Dynamic LDS: a byte per member of the largest scope in the launch.
__global__ __launch_bounds__(kSsThreads) void scope_similar_each_kernel(const ScopeSimilarArgs A) {
  const uint2 job = A.order[blockIdx.x];
  const ScopeDirect D = A.scopes[job.y];
  ss_body(A, job.x, D, blockIdx.x);
}

__global__ void scope_similar_gather_kernel(const uint64_t* __restrict__ qoff, const uint32_t* __restrict__ ntri,
                                            const uint32_t* __restrict__ idx, uint32_t n, uint64_t* __restrict__ gq,
                                            uint32_t* __restrict__ gn) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t q = idx[k];
  gq[k] = qoff[q] + q - k;
  gn[k] = ntri[q];
}

}  // namespace

int launch_scope_similar(const ScopeSimilarArgs& a, hipStream_t stream) {
  if (a.n == 0) return 0;
  if (a.limit == 0 || a.limit > kScopeMaxKeep || a.max_members > kScopeMaxMembers || a.min_permille > 1000) {
    errno = EINVAL;
    return -1;
  }
  const size_t lds = (size_t(a.max_members) + 3) & ~size_t(3);
  if (a.order) {
    note_launch("scope_similar_each_kernel");
    hipLaunchKernelGGL(scope_similar_each_kernel, dim3(a.n), dim3(kSsThreads), lds, stream, a);
  } else {
    note_launch("scope_similar_kernel");
    hipLaunchKernelGGL(scope_similar_kernel, dim3(a.n), dim3(kSsThreads), lds, stream, a);
  }
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_scope_similar_gather(const uint64_t* qoff, const uint32_t* ntri, const uint32_t* idx, uint32_t n,
                                uint64_t* gq, uint32_t* gn, hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(scope_similar_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, qoff, ntri, idx, n, gq, gn);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
