// cluster_tree_kernels.hip -- the kernels of blurrily_storage_cluster_tree (launch code:
// cluster_tree.hip): the maximum spanning forest of the similarity graph by Boruvka rounds, a round being one sweep
// that chooses, one merge and one flatten.
//
// cluster_tree_sweep_kernel is cluster_sweep_kernel's sweep (cluster_kernels.hip: the counters, the floor's bars t and
// [rlo, rhi], the windows passed over, the dense slices left out, each edge found from its end at the higher position)
// with another ending: a rank that passes the exact floor test and is a node is not united with the needle's node.
// Its ends' components are looked up in comp[], and if they differ the edge's key (cluster.h) is offered to best[] of
// both.  The body is a copy of cluster_sweep_kernel's, as that one is of similar_sweep_kernel's all mode, so that the
// device code of the others stays as it was.
//
// The memory model.  comp[] and closed[] are written by no thread while a sweep runs (the flatten and the merge wrote
// them launches ago), so they are read plainly.  best[] is touched, inside the sweep, only by agent-scope relaxed
// 64-bit fetch_max and by the relaxed load in front of it that spares the atomic when the word already holds as much:
// a key only rises, so a stale load costs one atomic that changes nothing, and the maximum of a set does not depend
// on the order of its elements.  best[cq], cq the needle's component, is one word for the whole workgroup: a lane keeps
// its maximum in registers, the workgroup's is taken in LDS at the end (in counter words that every harvest leaves
// zero), and one lane offers it.  The merge and the flatten meet best[] and parent[] across launch boundaries.
//
// The merge: thread i with best[i] != 0 holds the best edge leaving component i (its root's number when the round
// began) and unites its ends with cluster_forest.h's pf_unite, in the forest of cluster_kernels.hip, whose argument
// holds here unchanged: every access to parent[] inside the merge is an agent-scope relaxed atomic, hooks put the
// higher number under the lower, a step budget sets the error word.  The thread whose compare-and-swap made the hook
// writes the edge down.  That every chosen edge is written exactly once:
//   * the keys are a strict total order of the edges (height, then lower number, then higher number; two edges
//     differ in one of the numbers), so the best edge leaving a component is one edge;
//   * the edges chosen in a round form no cycle.  Take a cycle of components, each joined to the next by a chosen
//     edge, and the cycle's LOWEST edge e under the order.  e was chosen by one of the two components it joins, say X;
//     X's other cycle edge leaves X too and is higher, so X would have chosen that one.  (Two components may choose
//     the SAME edge from both sides: that is one edge, not a cycle.)
//   * so the distinct chosen edges extend the forest whatever the order of the unions: an edge's ends are under
//     different roots until that very edge is hooked.  pf_unite returns without a hook only when it saw both ends
//     under one root, which then is the same edge's hook by the thread of its other side; and a compare-and-swap
//     succeeds once per root.  Hence one record per distinct chosen edge: n_merges == nodes - components in the end.
// A root with best[i] == 0 when the merge reads it had no edge leaving its component in this sweep; components only
// grow by hooks along such edges, so nothing ever hooks it, it stays its component's number, and closed[i] is final.
//
// The flatten: comp[i] = root of i, for the next sweep, by plain loads (the merge is a launch behind).
#include "cluster.h"
#include "cluster_forest.h"
#include "find_kernels.h"
#include "hip_try.h"
#include "map_internal.h"

namespace blurrily {

namespace {

// note_launch keeps distinct names; a tree call launches the same kernels round after round, and blurrily_storage_last_kernels
// names every one of these launches: the rounds can be counted from it.
void note_each_launch(const char* kernel_name) {
  std::string* s = detail::launch_names();
  if (!s) return;
  if (!s->empty()) *s += '+';
  *s += kernel_name;
}

__device__ __forceinline__ void best_raise(unsigned long long* p, unsigned long long key) {
  if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= key) return;
  (void)__hip_atomic_fetch_max(p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kCluThreads) void cluster_tree_sweep_kernel(const ClusterTreeSweepArgs A) {
  const ClusterSweepArgs& a = A.s;
  __shared__ __attribute__((aligned(8))) uint32_t cnt[kCluWords];   // (two of its words end as one 64-bit key)
  __shared__ uint32_t left[(kNumCodes + 31) / 32];            // codes left out of this window's count
  __shared__ uint32_t d_len[kCluMaxDense], d_at[kCluMaxDense], d_code[kCluMaxDense], leave_at[kCluMaxDense];
  __shared__ uint32_t s_nd, s_any;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tasks = (a.n_windows + a.per - 1u) / a.per;
  const uint32_t qi = blockIdx.x / tasks, wr = blockIdx.x % tasks;
  if (qi >= a.n) return;
  const uint32_t q = a.q_base + qi;
  const uint32_t T = a.q_ntri[q];
  if (T == 0) return;                                         // (the map does not hold it: no node)
  const uint2 qloc = a.loc[q];
  if (qloc.x < a.win0) return;                                // (this image lies behind the needle's)
  const uint64_t qpos = uint64_t(qloc.x) * kWindowRanks + qloc.y;
  // the windows in front of the needle's position: up to its own, of which the ranks below its own count
  const uint32_t w_begin = wr * a.per, w_end = min(min(a.n_windows, (wr + 1u) * a.per), qloc.x - a.win0 + 1u);
  if (w_begin >= w_end) return;
  const uint32_t cq = A.comp[q];                              // the needle's component: frozen for the launch
  const bool counting = A.round == 1u;                        // (the edges are counted once, as cluster_sweep_kernel counts them)
  if (!counting && A.closed[cq]) return;                      // no edge leaves it: none of the needle's can
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

  unsigned long long mine_best = 0;                           // the best key this lane has for best[cq]
  uint32_t mine = 0;                                          // edges this lane found
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
          if (r >= kWindowRanks || pos0 + r >= qpos) continue;   // (an edge is its higher end's to find)
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
          mine += counting;
          const uint32_t co = A.comp[other];
          if (co == cq) continue;                             // inside a component: no edge of the forest any more
          // the height, floor(1000 m / (T + R - m)): m, T, R <= kNumCodes, so 32 bits hold it exactly
          const unsigned long long h = (1000u * m) / (T + R - m);
          const uint32_t e_lo = min(q, other), e_hi = max(q, other);
          const unsigned long long key = h << 54 | static_cast<unsigned long long>(~e_lo & kTreeNumberMask) << kTreeNumberBits |
                                         (~e_hi & kTreeNumberMask);
          mine_best = max(mine_best, key);
          best_raise(A.best + co, key);
        }
      }
      __syncthreads();
    }
    if (tid < nd) atomicAnd(&left[d_code[tid] >> 5], ~(1u << (d_code[tid] & 31u)));   // (cleared for the next window)
  }
  // the workgroup's count and its best key in the first words of the counters (every harvest leaves them zero)
  __syncthreads();
  unsigned long long* s_best = reinterpret_cast<unsigned long long*>(&cnt[2]);
  if (mine) atomicAdd(&cnt[0], mine);
  if (mine_best) atomicMax(s_best, mine_best);
  __syncthreads();
  if (tid == 0) {
    if (cnt[0]) atomicAdd(&a.totals->edges, static_cast<unsigned long long>(cnt[0]));
    if (*s_best) best_raise(A.best + cq, *s_best);
  }
}

__global__ __launch_bounds__(256) void cluster_tree_merge_kernel(const ClusterTreeRoundArgs A) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_nodes) return;
  const unsigned long long key = A.best[i];
  if (key == 0) {
    if (pf_load(A.parent + i) == i) A.closed[i] = 1;          // a root that no edge leaves (or a number that is no node)
    return;
  }
  A.best[i] = 0;                                              // (for the next round's sweep)
  const uint32_t h = uint32_t(key >> 54);
  const uint32_t lo = ~uint32_t(key >> kTreeNumberBits) & kTreeNumberMask, hi = ~uint32_t(key) & kTreeNumberMask;
  if (lo >= hi || hi >= A.n_nodes) { atomicOr(&A.totals->error, 1u); return; }   // (no key the sweep builds)
  uint64_t budget = 4ull * A.n_nodes + 64u;
  uint32_t root = lo;
  bool hooked;
  if (!pf_unite(A.parent, &root, hi, &budget, &hooked)) { atomicOr(&A.totals->error, 1u); return; }
  if (!hooked) return;                                        // (the same edge, chosen from its other side, made the hook)
  const uint32_t slot = atomicAdd(A.n_merges, 1u);
  if (slot >= A.n_nodes) { atomicOr(&A.totals->error, 1u); return; }   // (a forest has fewer edges than nodes)
  A.merges[slot] = {A.refs[lo], A.refs[hi], h};
}

__global__ __launch_bounds__(256) void cluster_tree_flatten_kernel(const ClusterTreeRoundArgs A) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_nodes) return;
  uint32_t v = i, steps = 0;
  for (uint32_t up = A.parent[v]; up < v; up = A.parent[v]) {   // (at most n_nodes links: the chain descends)
    v = up;
    if (++steps > A.n_nodes) { atomicOr(&A.totals->error, 1u); break; }
  }
  A.comp[i] = v;
}

}  // namespace

int launch_cluster_tree_sweep(const ClusterTreeSweepArgs& a, hipStream_t stream) {
  if (a.s.n == 0 || a.s.n_windows == 0) return 0;
  const uint64_t grid = uint64_t(a.s.n) * ((a.s.n_windows + a.s.per - 1u) / a.s.per);
  if (grid > 0x7FFFFFFFull || a.s.n_nodes > kTreeMaxNodes || a.round == 0) { errno = EINVAL; return -1; }
  note_each_launch("cluster_tree_sweep_kernel");
  hipLaunchKernelGGL(cluster_tree_sweep_kernel, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_tree_merge(const ClusterTreeRoundArgs& a, hipStream_t stream) {
  if (a.n_nodes == 0) return 0;
  note_each_launch("cluster_tree_merge_kernel");
  hipLaunchKernelGGL(cluster_tree_merge_kernel, dim3((a.n_nodes + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_tree_flatten(const ClusterTreeRoundArgs& a, hipStream_t stream) {
  if (a.n_nodes == 0) return 0;
  note_each_launch("cluster_tree_flatten_kernel");
  hipLaunchKernelGGL(cluster_tree_flatten_kernel, dim3((a.n_nodes + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
