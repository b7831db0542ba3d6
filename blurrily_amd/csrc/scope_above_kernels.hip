// scope_above_kernels.hip -- the scoped threshold find's direct strategy (launch code:
// scope_above.hip).
//
// scope_above_kernel / scope_above_each_kernel: one workgroup of 256 lanes per needle over a scope's direct form (the
// held members' code lists in (weight, reference) order).  The needle's code set goes into an LDS bitmap, from its
// string or from an extracted reference's codes (the framing is scope_similar_kernels.hip's); T is the bitmap's
// population count, or the reference's count, and the bar t = above_bar(T, min_matches, min_permille).  A member has at
// most 255 codes, so a bar above 255 -- or above T -- ends the workgroup there with no rows.
//
// The rows' order is matches descending, then (weight, reference) ascending -- and the members already stand in
// (weight, reference) order.  So a row's place is decided by a STABLE COUNTING SORT on the one byte m:
//   each of the four waves owns a contiguous quarter of the members (a slab) and scores it, member per lane: m from the
//   bitmap, kept as a byte in LDS, 0 when m < t; the wave counts its slab's m values in 256 bins of its own.
//   The count launch ends here: the sum of the bins is the needle's row count.
//   The emit launch scores again, then turns the bins into base[w][v] = the rows with more than v matches + the rows of
//   value v in the slabs below w; each wave walks its slab in order, 64 members a step, and for every distinct v among
//   the step's rows a lane's slot is the wave's cursor for v plus the population count of the ballot "m == v" below the
//   lane; the cursor advances by the ballot's count.  Rows of one v keep member order within a step (lane order),
//   across steps (the cursor), across slabs (the base); rows of different v never share a slot range.
// The row goes straight to rows[seg + slot]: no keys, no sort kernel, no second rows kernel, and members the base image
// and the delta image hold are one list already.
#include "scope_above.h"
#include "above.h"
#include "hip_try.h"

namespace blurrily {

namespace {

constexpr uint32_t kSaThreads  = 256;
constexpr uint32_t kSaWaves    = kSaThreads / 64;
constexpr uint32_t kSaMapWords = (kNumCodes + 31) / 32;       // the needle's code set

__device__ __forceinline__ uint32_t sa_symbol(unsigned char c) {
  return (c >= 'a' && c <= 'z') ? uint32_t(c - 'a' + 1) : 0u;   // tokeniser.c:21-31
}

struct SaScalars {
  uint32_t len, T, total;
};

// The needle's code set from its string (a C string within cap bytes): "**" + s + "*", the trigram at k is
// sym(s[k-2]) + 28 sym(s[k-1]) + 784 sym(s[k]), '*' outside s (tokeniser.c:62-75).  Ends at a barrier.
__device__ __forceinline__ void sa_map_string(uint32_t* s_map, SaScalars& S, const char* s, uint32_t cap, uint32_t tid) {
  if (tid == 0) S.len = cap;
  __syncthreads();
  for (uint32_t k = tid; k < cap; k += kSaThreads)
    if (s[k] == 0) atomicMin(&S.len, k);
  __syncthreads();
  const uint32_t len = S.len;
  for (uint32_t k = tid; k <= len; k += kSaThreads) {
    const uint32_t a = k >= 2 ? sa_symbol((unsigned char)s[k - 2]) : 0u;
    const uint32_t b = k >= 1 ? sa_symbol((unsigned char)s[k - 1]) : 0u;
    const uint32_t c = k < len ? sa_symbol((unsigned char)s[k]) : 0u;
    const uint32_t code = a + 28u * b + 784u * c;
    atomicOr(&s_map[code >> 5], 1u << (code & 31u));
  }
  __syncthreads();
  uint32_t t = 0;
  for (uint32_t w = tid; w < kSaMapWords; w += kSaThreads) t += uint32_t(__popc(s_map[w]));
  if (t) atomicAdd(&S.T, t);
  __syncthreads();
}

// Job `job` (needle q, string or reference) against one direct form; workgroup b of the launch.
__device__ __forceinline__ void sa_body(const ScopeAboveArgs& A, uint32_t q, const ScopeDirect& D, uint32_t job, uint32_t b) {
  __shared__ uint32_t s_map[kSaMapWords];
  __shared__ uint32_t s_cnt[kSaWaves][256];             // per wave: its slab's count of each m; then its cursor for each m
  __shared__ uint32_t s_suf[256];
  __shared__ SaScalars S;
  extern __shared__ uint8_t s_match[];                  // (emit) [n_members] m of every member that is a row, 0 of the others
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n_members = min(D.n_members, A.max_members);
  const bool emit = A.seg != nullptr;
  uint32_t cap = 0;
  if (emit) {
    cap = A.counts[job];
    if (cap == 0) return;                               // (uniform) the count launch found no row
  }

  for (uint32_t w = tid; w < kSaMapWords; w += kSaThreads) s_map[w] = 0u;
  for (uint32_t w = 0; w < kSaWaves; ++w) s_cnt[w][tid] = 0u;
  if (tid == 0) { S.T = 0u; S.total = 0u; }
  __syncthreads();
  if (A.codes) {
    const uint16_t* codes = A.codes + (A.qoff[q] + q);
    const uint32_t ntri = A.ntri[q];
    for (uint32_t k = tid; k < ntri; k += kSaThreads) {
      const uint32_t code = codes[k];
      atomicOr(&s_map[code >> 5], 1u << (code & 31u));
    }
    if (tid == 0) S.T = ntri;
    __syncthreads();
  } else {
    const uint64_t beg = A.offsets[q];
    const uint32_t cap_bytes = uint32_t(min<uint64_t>(A.offsets[q + 1] - beg, 0xFFFFFFF0ull));
    sa_map_string(s_map, S, A.packed + beg, cap_bytes, tid);
  }
  const uint32_t T = S.T;
  const uint32_t t = above_bar(T, A.min_matches, A.min_permille);
  if (T == 0 || t > T || t > kScopeMaxMemberCodes) {    // (uniform) no member can reach the bar
    if (!emit && tid == 0) A.counts[job] = 0u;
    return;
  }

  // the wave's slab, a whole number of 64-member steps; every member's m
  const uint32_t per = (((n_members + kSaWaves - 1u) / kSaWaves) + 63u) & ~63u;
  const uint32_t lo = min(wave * per, n_members), hi = min(lo + per, n_members);
  uint32_t mine = 0;
  for (uint32_t i = lo + lane; i < hi; i += 64u) {
    const uint32_t b0 = D.m_off[i], b1 = D.m_off[i + 1];
    uint32_t c = 0;
    for (uint32_t j = b0; j < b1; ++j) {
      const uint32_t code = D.m_codes[j];
      c += (s_map[code >> 5] >> (code & 31u)) & 1u;
    }
    const uint32_t m = c >= t ? c : 0u;                 // (c <= 255: a member has at most kScopeMaxMemberCodes codes)
    if (emit) {
      s_match[i] = uint8_t(m);
      if (m) atomicAdd(&s_cnt[wave][m & 255u], 1u);
    } else {
      mine += m ? 1u : 0u;
    }
  }
  if (!emit) {
    if (mine) atomicAdd(&S.total, mine);
    __syncthreads();
    if (tid == 0) A.counts[job] = S.total;
    return;
  }
  __syncthreads();

  // base: lane v owns column v of the four waves' bins
  {
    uint32_t c[kSaWaves], tot = 0;
    for (uint32_t w = 0; w < kSaWaves; ++w) { c[w] = s_cnt[w][tid]; tot += c[w]; }
    s_suf[tid] = tot;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {            // s_suf[v]: rows of at least v matches
      const uint32_t up = tid + d < 256 ? s_suf[tid + d] : 0u;
      __syncthreads();
      s_suf[tid] += up;
      __syncthreads();
    }
    uint32_t at = s_suf[tid] - tot;                     // rows of more than v matches
    for (uint32_t w = 0; w < kSaWaves; ++w) { s_cnt[w][tid] = at; at += c[w]; }
  }
  __syncthreads();

  // placement: the wave walks its slab in member order
  trigram_match_t* rows = A.rows + A.seg[b];
  for (uint32_t base = lo; base < hi; base += 64u) {    // (uniform in the wave)
    const uint32_t i = base + lane;
    const uint32_t m = i < hi ? s_match[i] : 0u;
    unsigned long long todo = __ballot(m != 0u);
    while (todo) {
      const int first = __ffsll((long long)todo) - 1;
      const uint32_t v = uint32_t(__shfl(int(m), first));
      const unsigned long long same = __ballot(m == v);
      uint32_t cur = 0;
      if (int(lane) == first) cur = atomicAdd(&s_cnt[wave][v], uint32_t(__popcll(same)));
      cur = uint32_t(__shfl(int(cur), first));
      if (m == v) {
        const uint32_t slot = cur + uint32_t(__popcll(same & ((1ull << lane) - 1ull)));
        if (slot < cap) {                               // (always: the count launch saw the same members)
          trigram_match_t* row = rows + slot;
          row->reference = D.m_ref[i];
          row->matches = m;
          row->weight = D.m_weight[i];
        }
      }
      todo &= ~same;
    }
  }
}

__global__ __launch_bounds__(kSaThreads) void scope_above_kernel(const ScopeAboveArgs A) {
  const uint32_t job = A.first + blockIdx.x;
  sa_body(A, job, A.one, job, blockIdx.x);
}

// Each needle against its own scope (the host orders the jobs by descending member count, so the longest ones start
// first).  Dynamic LDS of an emit launch: a byte per member of the largest scope in the call.
__global__ __launch_bounds__(kSaThreads) void scope_above_each_kernel(const ScopeAboveArgs A) {
  const uint32_t job = A.first + blockIdx.x;
  const uint2 who = A.order[job];
  const ScopeDirect D = A.scopes[who.y];
  sa_body(A, who.x, D, job, blockIdx.x);
}

}  // namespace

int launch_scope_above(const ScopeAboveArgs& a, hipStream_t stream) {
  if (a.n == 0) return 0;
  if (a.max_members > kScopeMaxMembers || a.min_permille > 1000 || !a.counts || (a.seg && !a.rows)) {
    errno = EINVAL;
    return -1;
  }
  const size_t lds = a.seg ? (size_t(a.max_members) + 3) & ~size_t(3) : 0;   // (the count launch keeps no m)
  if (a.order) {
    note_launch("scope_above_each_kernel");
    hipLaunchKernelGGL(scope_above_each_kernel, dim3(a.n), dim3(kSaThreads), lds, stream, a);
  } else {
    note_launch("scope_above_kernel");
    hipLaunchKernelGGL(scope_above_kernel, dim3(a.n), dim3(kSaThreads), lds, stream, a);
  }
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
