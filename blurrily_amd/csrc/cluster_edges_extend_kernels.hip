// cluster_edges_extend_kernels.hip -- the kernel of blurrily_storage_cluster_edges_extend and
// blurrily_storage_cluster_edges_between (launch code: cluster_edges_extend.hip): the similarity
// graph's edges that have a new end, or an end on each side of two lists, each once, as keys for cluster_edges.hip's
// sort and rows.
//
// cluster_edges_extend_sweep_kernel: cluster_sweep_kernel's sweep (cluster_kernels.hip: a window's postings counted into
// LDS, bytes or 16-bit halves; the floor's bars t and [rlo, rhi]; windows passed over by win_min_tri / win_max_tri; the
// t - 1 largest dense slices left out and asked through their bitmaps; a needle's windows shared among workgroups) with
// cluster_extend_sweep_kernel's range (cluster_extend_kernels.hip: the needles come through a list of numbers, a needle
// sweeps every window of both images, and a candidate that is the needle is skipped) and cluster_edges_sweep_kernel's
// ending (cluster_edges_kernels.hip: a candidate that passes the exact floor test and is a node is united with nothing
// -- its key is appended).  Which candidates a needle keeps is one bitmap and one flag: `side` has a bit per number,
// every needle of a call lies on one side, and a candidate on the needle's side is passed over when `between` is set
// (only edges across the sides) and otherwise when it lies at a higher position than the needle -- an edge between two
// needles is its higher end's to find, across images too, so absolute positions are compared.  A candidate on the other
// side is never a needle, so the edge is this end's wherever the candidate lies.  The body is a copy, as the other
// entries' are, so that their device code stays as it was.
//
// The append is cluster_edges_kernels.hip's, and its rules hold here as there: one 64-bit cursor per call; a wave
// reserves room for all its lanes' edges at once (an inclusive prefix sum through __shfl_up, ONE agent-scope relaxed
// fetch_add by lane 0, the base handed round by __shfl); a key is stored only when its slot lies below
// ClusterEdgesOut::room, and the cursor counts on regardless.  The cross-lane steps need every lane of the wave: the
// harvest takes every lane through kCluWords / kCluThreads trips and predicates its body instead of leaving early,
// every `continue` and `return` in front of it is uniform across the workgroup, and a wave in which no lane found an
// edge skips the reservation on a ballot all 64 lanes take.
#include "cluster.h"
#include "cluster_forest.h"
#include "find_kernels.h"
#include "hip_try.h"
#include "map_internal.h"

namespace blurrily {

namespace {

// (every launch of a call is named, as cluster_edges_kernels.hip names its own: a sweep per image can be counted)
void note_each_launch(const char* kernel_name) {
  std::string* s = detail::launch_names();
  if (!s) return;
  if (!s->empty()) *s += '+';
  *s += kernel_name;
}

// the height, floor(1000 m / (T + R - m)): m, T, R <= kNumCodes, so 32 bits hold it exactly
__device__ __forceinline__ unsigned long long edge_key(uint32_t m, uint32_t T, uint32_t R, uint32_t u, uint32_t v) {
  const unsigned long long down = 1000u - (1000u * m) / (T + R - m);
  return down << 54 | static_cast<unsigned long long>(min(u, v) & kTreeNumberMask) << kTreeNumberBits |
         (max(u, v) & kTreeNumberMask);
}

// Room for `mine` keys of this lane among its wave's: the first slot.  EVERY lane of the wave calls it.
__device__ __forceinline__ unsigned long long edges_reserve(const ClusterEdgesOut& o, uint32_t lane, uint32_t mine) {
  uint32_t incl = mine;
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t below = __shfl_up(incl, d);
    if (lane >= d) incl += below;
  }
  const uint32_t total = __shfl(incl, 63);
  unsigned long long base = 0;
  if (lane == 0)
    base = __hip_atomic_fetch_add(o.cursor, static_cast<unsigned long long>(total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  base = __shfl(base, 0);
  return base + (incl - mine);
}

static_assert(kCluWords % kCluThreads == 0, "the harvest takes every lane through the same number of counter words");
static_assert(kCluThreads % 64 == 0, "whole waves");

__global__ __launch_bounds__(kCluThreads) void cluster_edges_extend_sweep_kernel(const ClusterEdgesExtendSweepArgs A) {
  const ClusterSweepArgs& a = A.s;
  __shared__ uint32_t cnt[kCluWords];
  __shared__ uint32_t left[(kNumCodes + 31) / 32];            // codes left out of this window's count
  __shared__ uint32_t d_len[kCluMaxDense], d_at[kCluMaxDense], d_code[kCluMaxDense], leave_at[kCluMaxDense];
  __shared__ uint32_t s_nd, s_any;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tasks = (a.n_windows + a.per - 1u) / a.per;
  const uint32_t qi = blockIdx.x / tasks, wr = blockIdx.x % tasks;
  if (qi >= a.n) return;
  const uint32_t q = A.needles[a.q_base + qi];                // (a number of the swept side)
  if (q >= a.n_nodes) return;
  const uint32_t T = a.q_ntri[q];
  if (T == 0) return;                                         // (the map does not hold it: no node)
  const uint32_t qside = (A.side[q >> 5] >> (q & 31u)) & 1u;
  const uint2 qloc = a.loc[q];
  const uint64_t qpos = uint64_t(qloc.x) * kWindowRanks + qloc.y;
  // every window of the image, in front of the needle and behind it: a node of the other side may lie anywhere
  const uint32_t w_begin = wr * a.per, w_end = min(a.n_windows, (wr + 1u) * a.per);
  if (w_begin >= w_end) return;
  const uint32_t p = a.min_permille;
  const uint16_t* codes = a.qcodes + a.qoff[q] + uint64_t(q);
  const bool wide = T > 255u;                                 // byte counters hold at most 255 matches
  // the floor's bars: m >= ceil(p T / 1000), ceil(p T / 1000) <= R <= floor(1000 T / p)
  const uint32_t t = max(1u, uint32_t((uint64_t(p) * T + 999u) / 1000u));
  const uint32_t rlo = t;
  const uint32_t rhi = p ? uint32_t(min<uint64_t>(1000ull * T / p, 0xFFFFFFFFull)) : 0xFFFFFFFFu;
  for (uint32_t i = tid; i < kCluWords; i += kCluThreads) cnt[i] = 0;
  for (uint32_t i = tid; i < (kNumCodes + 31) / 32; i += kCluThreads) left[i] = 0;
  __syncthreads();

  for (uint32_t w = w_begin; w < w_end; ++w) {
    const uint32_t wmin = a.win_min_tri[w], wmax = a.win_max_tri[w];
    if (wmax < rlo || wmin > rhi) continue;                   // no reference of the window has an R the floor allows
    __syncthreads();                                          // (the previous window is done with the lists)
    if (tid == 0) { s_nd = 0; s_any = 0; }
    __syncthreads();
    const uint2* se_w = a.slice_se + size_t(w) * kNumCodes;
    if (a.dense_min8 && t > 1u) {
      for (uint32_t i = tid; i < T; i += kCluThreads) {
        const uint2 se = se_w[codes[i]];
        if (se.y - se.x >= a.dense_min8) {
          const uint32_t k = atomicAdd(&s_nd, 1u);
          if (k < kCluMaxDense) { d_len[k] = se.y - se.x; d_at[k] = se.x; d_code[k] = codes[i]; }
        }
      }
      __syncthreads();
    }
    const uint32_t nd = min(s_nd, kCluMaxDense);
    const uint32_t L = min(t - 1u, nd);
    // the L largest dense slices (lower code first among equal lengths) are left out
    if (tid < nd) {
      uint32_t r = 0;
      for (uint32_t j = 0; j < nd; ++j)
        r += d_len[j] > d_len[tid] || (d_len[j] == d_len[tid] && d_code[j] < d_code[tid]);
      if (r < L) { leave_at[r] = d_at[tid]; atomicOr(&left[d_code[tid] >> 5], 1u << (d_code[tid] & 31u)); }
    }
    __syncthreads();
    const uint32_t hthr = max(1u, t - L);                     // counted matches a rank needs to be asked about
    const uint64_t pos0 = uint64_t(a.win0 + w) * kWindowRanks;

    for (uint32_t half = 0; half < (wide ? 2u : 1u); ++half) {
      const uint32_t lo = half * (kWindowSize / 2);
      // count: one slice per wave, 8 postings a lane per 16-byte load
      for (uint32_t i = wave; i < T; i += kCluWaves) {
        const uint32_t code = codes[i];
        if ((left[code >> 5] >> (code & 31u)) & 1u) continue;
        const uint2 se = se_w[code];
        const uint32_t groups = (se.y - se.x) / 8u;
        if (groups == 0) continue;
        if (lane == 0) s_any = 1;
        const uint4* pp = reinterpret_cast<const uint4*>(a.ent + se.x);
        for (uint32_t g = lane; g < groups; g += 64u) {
          const uint4 v = pp[g];
          const uint32_t h[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const uint32_t r = (h[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
            if (r == kPadRank) continue;
            if (!wide) {
              atomicAdd(&cnt[r >> 2], 1u << ((r & 3u) * 8u));
            } else {
              const uint32_t x = r - lo;
              if (x < kWindowSize / 2) atomicAdd(&cnt[x >> 1], 1u << ((x & 1u) * 16u));
            }
          }
        }
      }
      __syncthreads();
      if (!s_any) continue;                                   // (uniform: nothing was counted, the counters are still zero)
      const uint32_t per_word = wide ? 2u : 4u, bits = wide ? 16u : 8u, mask = wide ? 0xFFFFu : 0xFFu;
      // the harvest: the same trips in every lane, so that the reservation below meets whole waves
      for (uint32_t w0 = 0; w0 < kCluWords; w0 += kCluThreads) {
        const uint32_t wi = w0 + tid;
        const uint32_t x = cnt[wi];
        unsigned long long found[4];                          // this word's edges, by counter (statically indexed)
        uint32_t hits = 0;                                    // bit s: counter s of the word is an edge
        if (x) {
          cnt[wi] = 0;
#pragma unroll
          for (uint32_t s = 0; s < 4u; ++s) {
            found[s] = 0;
            if (s >= per_word) continue;
            const uint32_t c = (x >> (s * bits)) & mask;
            if (c < hthr) continue;
            const uint32_t r = wide ? lo + wi * 2u + s : wi * 4u + s;
            if (r >= kWindowRanks || pos0 + r == qpos) continue;   // (the needle itself)
            const uint32_t g = w * kWindowRanks + r;
            if (g >= a.n_refs) continue;
            uint32_t m = c;
            for (uint32_t l = 0; l < L; ++l) {
              const uint32_t* bm = reinterpret_cast<const uint32_t*>(a.ent + (leave_at[l] - kBitmapSlots));
              m += (bm[r >> 5] >> (r & 31u)) & 1u;
            }
            if (m < t) continue;
            const uint32_t R = a.ntri_of_rank[g];
            if (R < rlo || R > rhi) continue;
            if (1000ull * m < uint64_t(p) * (uint64_t(T) + R - m)) continue;   // the floor, exactly
            const uint32_t other = a.node_of_pos[pos0 + r];
            if (other == kNoNode || other >= a.n_nodes) continue;   // held but not listed (or deleted): no node, no bridge
            // the other side's node is no needle: the edge is this end's to find.  On the needle's own side there is
            // no edge to report (between), or it is the higher end's.
            if ((((A.side[other >> 5] >> (other & 31u)) & 1u) == qside) && (A.between || pos0 + r > qpos)) continue;
            found[s] = edge_key(m, T, R, q, other);
            hits |= 1u << s;
          }
        }
        if (__ballot(hits != 0u) == 0ull) continue;           // (uniform across the wave: no lane of it has an edge)
        const unsigned long long at = edges_reserve(A.out, lane, __popc(hits));
#pragma unroll
        for (uint32_t s = 0; s < 4u; ++s) {
          const unsigned long long slot = at + __popc(hits & ((1u << s) - 1u));
          if (((hits >> s) & 1u) && slot < A.out.room) A.out.keys[slot].k = found[s];
        }
      }
      __syncthreads();
    }
    if (tid < nd) atomicAnd(&left[d_code[tid] >> 5], ~(1u << (d_code[tid] & 31u)));   // (cleared for the next window)
  }
}

}  // namespace

int launch_cluster_edges_extend_sweep(const ClusterEdgesExtendSweepArgs& a, hipStream_t stream) {
  const ClusterSweepArgs& s = a.s;
  if (s.n == 0 || s.n_windows == 0) return 0;
  const uint64_t grid = uint64_t(s.n) * ((s.n_windows + s.per - 1u) / s.per);
  if (grid > 0x7FFFFFFFull || s.n_nodes > kTreeMaxNodes || !a.needles || !a.side || !a.out.cursor ||
      (a.out.room && !a.out.keys)) {
    errno = EINVAL;
    return -1;
  }
  note_each_launch("cluster_edges_extend_sweep_kernel");
  hipLaunchKernelGGL(cluster_edges_extend_sweep_kernel, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
