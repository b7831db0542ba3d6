// cluster_extend_kernels.hip -- the kernels of blurrily_storage_cluster_extend (launch code:
// cluster_extend.hip): the clusters of old and new references together, from the labels the caller holds for the old
// ones and a sweep of the new ones alone.
//
// cluster_extend_seed_kernel: one lane per old element.  The element and the node holding its label are united, unless
// either is no node (not held) or is new; the label is looked up among the ascending references by binary search.
// cluster_extend_sweep_kernel: cluster_sweep_kernel's sweep (cluster_kernels.hip: byte counters or 16-bit halves, the
// bars t and [rlo, rhi], windows passed over by win_min_tri / win_max_tri, the t - 1 largest dense slices left out and
// asked through their bitmaps, a needle's windows shared among workgroups) with three differences: the needles are the
// new nodes, through the list of their numbers; a needle sweeps every window of both images; and the ending -- a
// candidate that is the needle is skipped, an old node is united wherever it lies, a new node only from the end at
// the higher position, so that every edge with a new end is found once and the edges stay a plain count.
//
// The forest is cluster_kernels.hip's, and its argument holds with seeds as it stands: a seed is one more call of
// pf_unite, which hooks the root with the larger number under the smaller by a compare-and-swap that saw it a root.
// So parent[x] <= x, every value stored in parent[x] is an ancestor of x for ever, and a component's root is its lowest
// number, whichever of seeds and edges made it.  Inside the two launches every access to parent[] is one of
// cluster_forest.h's agent-scope atomics; the seeds run in a launch of their own before the sweeps.
#include "cluster.h"
#include "cluster_forest.h"
#include "find_kernels.h"
#include "hip_try.h"

namespace blurrily {

namespace {

__global__ __launch_bounds__(256) void cluster_extend_seed_kernel(const ClusterExtendSeedArgs A) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_old) return;
  uint32_t v = A.inv ? A.inv[i] : i;
  if (A.ntri[v] == 0 || ((A.is_new[v >> 5] >> (v & 31u)) & 1u)) return;   // not held, or named by the new list
  const uint32_t label = A.old_labels[i];
  if (label == A.refs[v]) return;                             // (its own label: nothing to look up or unite)
  uint32_t lo = 0, hi = A.n_nodes;                            // the first number whose reference is >= label
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (A.refs[mid] < label) lo = mid + 1u; else hi = mid;
  }
  if (lo >= A.n_nodes || A.refs[lo] != label) return;         // the label is not listed
  if (A.ntri[lo] == 0 || ((A.is_new[lo >> 5] >> (lo & 31u)) & 1u)) return;   // ... or not held, or new
  uint64_t budget = 4ull * A.n_nodes + 64u;
  if (!pf_unite(A.parent, &v, lo, &budget)) atomicOr(&A.totals->error, 1u);
}

__global__ __launch_bounds__(kCluThreads) void cluster_extend_sweep_kernel(const ClusterExtendSweepArgs A) {
  const ClusterSweepArgs& a = A.s;
  __shared__ uint32_t cnt[kCluWords];
  __shared__ uint32_t left[(kNumCodes + 31) / 32];            // codes left out of this window's count
  __shared__ uint32_t d_len[kCluMaxDense], d_at[kCluMaxDense], d_code[kCluMaxDense], leave_at[kCluMaxDense];
  __shared__ uint32_t s_nd, s_any, s_edges, s_err;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tasks = (a.n_windows + a.per - 1u) / a.per;
  const uint32_t qi = blockIdx.x / tasks, wr = blockIdx.x % tasks;
  if (qi >= a.n) return;
  const uint32_t q = A.new_nodes[a.q_base + qi];              // (a new node's number)
  const uint32_t T = a.q_ntri[q];
  if (T == 0) return;                                         // (the map does not hold it: no node)
  const uint2 qloc = a.loc[q];
  const uint64_t qpos = uint64_t(qloc.x) * kWindowRanks + qloc.y;
  // every window of the image, in front of the needle and behind it: an old node may lie anywhere
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
  if (tid == 0) { s_edges = 0; s_err = 0; }
  __syncthreads();

  uint32_t root = q;                                          // the needle's root as far as this lane knows
  uint32_t mine = 0;                                          // edges this lane found
  bool ok = true;
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
      for (uint32_t wi = tid; wi < kCluWords; wi += kCluThreads) {
        const uint32_t x = cnt[wi];
        if (!x) continue;
        cnt[wi] = 0;
        for (uint32_t s = 0; s < per_word; ++s) {
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
          if (other == kNoNode) continue;                     // held but not listed (or deleted): no node, no bridge
          // an old node is no needle: the edge is this end's to find.  Between two new nodes it is the higher end's.
          if (pos0 + r > qpos && ((A.is_new[other >> 5] >> (other & 31u)) & 1u)) continue;
          ++mine;
          if (ok) {
            uint64_t budget = 4ull * a.n_nodes + 64u;
            ok = pf_unite(a.parent, &root, other, &budget);
          }
        }
      }
      __syncthreads();
    }
    if (tid < nd) atomicAnd(&left[d_code[tid] >> 5], ~(1u << (d_code[tid] & 31u)));   // (cleared for the next window)
  }
  if (mine) atomicAdd(&s_edges, mine);
  if (!ok) s_err = 1;
  __syncthreads();
  if (tid == 0) {
    if (s_edges) atomicAdd(&a.totals->edges, static_cast<unsigned long long>(s_edges));
    if (s_err) atomicOr(&a.totals->error, 1u);
  }
}

}  // namespace

int launch_cluster_extend_seed(const ClusterExtendSeedArgs& a, hipStream_t stream) {
  if (a.n_old == 0) return 0;
  note_launch("cluster_extend_seed_kernel");
  hipLaunchKernelGGL(cluster_extend_seed_kernel, dim3((a.n_old + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_extend_sweep(const ClusterExtendSweepArgs& a, hipStream_t stream) {
  if (a.s.n == 0 || a.s.n_windows == 0) return 0;
  const uint64_t grid = uint64_t(a.s.n) * ((a.s.n_windows + a.s.per - 1u) / a.s.per);
  if (grid > 0x7FFFFFFFull) { errno = EINVAL; return -1; }
  note_launch("cluster_extend_sweep_kernel");
  hipLaunchKernelGGL(cluster_extend_sweep_kernel, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
