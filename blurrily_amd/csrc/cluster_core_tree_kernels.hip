// cluster_core_tree_kernels.hip -- the kernels of blurrily_storage_cluster_core_tree (launch
// code: cluster_core_tree.hip): the core heights by histogram refinement, then the cluster tree's Boruvka rounds over
// the edges between numbers that have one, heights capped.  The merge, the flatten and the labels are
// cluster_tree_kernels.hip's and cluster_kernels.hip's as they are.
//
// Both sweeps are cluster_sweep_kernel's sweep (cluster_kernels.hip: the counters, the floor's bars t and [rlo, rhi],
// the windows passed over, the dense slices left out, each edge found from its end at the higher position) with
// another ending, one body with two endings here; it is a copy, as cluster_tree_sweep_kernel's is, so that the device
// code of the others stays as it was.
//
// The height ending (cluster_core_height_sweep_kernel).  An edge of height h adds 1 to counter (h - core[x]) / width
// of each end x with h - core[x] < span: one agent-scope relaxed 32-bit add per end, and nothing else is written.
// core[] and above[] are written by no thread while a sweep runs (the settle wrote them a launch ago), so both ends'
// brackets are read plainly.  Integer adds commute: a counter ends as the number of the node's edges in its heights,
// whatever the order of arrival, and the settle reads it across a launch boundary.  A needle without a bracket still
// sweeps, since its edges are found from its end alone and count at the other.
//
// The settle's invariant (cluster_core_height_settle_kernel, a thread per number, plain loads and stores: nobody else
// touches its words in that launch).  For a node with a bracket [lo, lo + span): above = its edges of a height above
// the bracket, above < min_degree <= above + its edges inside the bracket -- the min_degree-th largest height lies in
// the bracket.  The first bracket is every height an edge can have, [min_permille, 1000], with above = 0, so after the
// first sweep the invariant holds or the node has fewer than min_degree edges and no core height.  Walking the
// counters from the top with the running count starting at above, the first counter at which the count reaches
// min_degree holds the min_degree-th largest, ties counted as often as they occur; it becomes the bracket, the count
// in front of it becomes above, and the invariant holds again.  A bracket of one height is the core height.
//
// The tree ending (cluster_core_tree_sweep_kernel) is cluster_tree_sweep_kernel's -- its memory model and the merge's
// argument hold unchanged, the keys being a strict total order of whatever edges are offered -- with three
// differences: a workgroup whose needle has no core height returns at once, an edge to a number without one is passed
// over, and the key's height is min(h, core[q], core[other]).  core[] is final launches before the first round.
#include "cluster.h"
#include "cluster_forest.h"
#include "find_kernels.h"
#include "hip_try.h"
#include "map_internal.h"

namespace blurrily {

namespace {

// (as cluster_tree_kernels.hip's: every launch is named, so that the sweeps and the rounds can be counted)
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

__device__ __forceinline__ const ClusterSweepArgs& sweep_args(const ClusterCoreHeightSweepArgs& A) { return A.s; }
__device__ __forceinline__ const ClusterSweepArgs& sweep_args(const ClusterCoreTreeSweepArgs& A) { return A.t.s; }

template <bool kTree, class Args>
__device__ __forceinline__ void core_sweep(const Args& A) {
  const ClusterSweepArgs& a = sweep_args(A);
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
  const uint32_t core_q = A.core[q];                          // frozen for the launch
  if (kTree && core_q == kNoCore) return;                     // no edge of the needle's is in the tree
  const uint2 qloc = a.loc[q];
  if (qloc.x < a.win0) return;                                // (this image lies behind the needle's)
  const uint64_t qpos = uint64_t(qloc.x) * kWindowRanks + qloc.y;
  // the windows in front of the needle's position: up to its own, of which the ranks below its own count
  const uint32_t w_begin = wr * a.per, w_end = min(min(a.n_windows, (wr + 1u) * a.per), qloc.x - a.win0 + 1u);
  if (w_begin >= w_end) return;
  uint32_t cq = 0;                                            // the needle's component: frozen for the launch
  bool counting;                                              // (the edges are counted once)
  if constexpr (kTree) {
    cq = A.t.comp[q];
    counting = A.t.round == 1u;
    if (!counting && A.t.closed[cq]) return;                  // no edge leaves it: none of the needle's can
  } else {
    counting = A.count_edges != 0u;
  }
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
  uint32_t mine = 0;                                          // edges this lane found (the tree's: between two core heights)
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
          // the height, floor(1000 m / (T + R - m)): m, T, R <= kNumCodes, so 32 bits hold it exactly
          const uint32_t h = (1000u * m) / (T + R - m);
          const uint32_t core_o = A.core[other];
          if constexpr (kTree) {
            if (core_o == kNoCore) continue;                  // not an edge of the tree
            mine += counting;
            const uint32_t co = A.t.comp[other];
            if (co == cq) continue;                           // inside a component: no edge of the forest any more
            const unsigned long long H = min(h, min(core_q, core_o));
            const uint32_t e_lo = min(q, other), e_hi = max(q, other);
            const unsigned long long key = H << 54 | static_cast<unsigned long long>(~e_lo & kTreeNumberMask) << kTreeNumberBits |
                                           (~e_hi & kTreeNumberMask);
            mine_best = max(mine_best, key);
            best_raise(A.t.best + co, key);
          } else {
            mine += counting;
            // (h - core wraps far above span for a height under the bracket; kNoCore would wrap to h + 1)
            const uint32_t dq = h - core_q, dn = h - core_o;
            if (core_q != kNoCore && dq < A.span)
              (void)__hip_atomic_fetch_add(A.hist + size_t(q) * kCoreBuckets + dq / A.width, 1u, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            if (core_o != kNoCore && dn < A.span)
              (void)__hip_atomic_fetch_add(A.hist + size_t(other) * kCoreBuckets + dn / A.width, 1u, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
          }
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
  if (kTree && mine_best) atomicMax(s_best, mine_best);
  __syncthreads();
  if (tid == 0) {
    if constexpr (kTree) {
      if (cnt[0]) {
        atomicAdd(&A.totals->core_edges, static_cast<unsigned long long>(cnt[0]));
        if (A.count_edges) atomicAdd(&A.totals->t.edges, static_cast<unsigned long long>(cnt[0]));
      }
      if (*s_best) best_raise(A.t.best + cq, *s_best);
    } else {
      if (cnt[0]) atomicAdd(&A.totals->t.edges, static_cast<unsigned long long>(cnt[0]));
    }
  }
}

__global__ __launch_bounds__(kCluThreads) void cluster_core_height_sweep_kernel(const ClusterCoreHeightSweepArgs A) {
  core_sweep<false>(A);
}

__global__ __launch_bounds__(kCluThreads) void cluster_core_tree_sweep_kernel(const ClusterCoreTreeSweepArgs A) {
  core_sweep<true>(A);
}

__global__ __launch_bounds__(256) void cluster_core_height_settle_kernel(const ClusterCoreHeightSettleArgs A) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_nodes) return;
  if (A.pass == 0) {
    A.core[i] = A.ntri[i] == 0 ? kNoCore : A.min_degree == 0 ? 1000u : A.min_permille;
    A.above[i] = 0;
    return;
  }
  const uint32_t lo = A.core[i];
  if (lo == kNoCore) return;                                  // (nothing was added to its counters)
  uint32_t* mine = A.hist + size_t(i) * kCoreBuckets;
  uint32_t run = A.above[i], found = kCoreBuckets;            // the edges above counter j, the counter that holds the height
  for (uint32_t j = kCoreBuckets; j-- > 0;) {
    const uint32_t c = mine[j];
    mine[j] = 0;                                              // (for the next sweep)
    if (found != kCoreBuckets) continue;
    if (run + c >= A.min_degree) found = j; else run += c;    // (run + c <= the node's edges < n_nodes)
  }
  if (found != kCoreBuckets) {
    A.core[i] = lo + found * A.width;
    A.above[i] = run;
  } else {
    A.core[i] = kNoCore;                                      // fewer than min_degree edges: the first sweep tells ...
    if (A.pass > 1) atomicOr(&A.totals->t.error, 1u);         // ... a later one cannot (the invariant is broken)
  }
}

int check_sweep(const ClusterSweepArgs& s, uint64_t* grid) {
  *grid = uint64_t(s.n) * ((s.n_windows + s.per - 1u) / s.per);
  if (*grid > 0x7FFFFFFFull || s.n_nodes > kTreeMaxNodes) { errno = EINVAL; return -1; }
  return 0;
}

}  // namespace

int launch_cluster_core_height_sweep(const ClusterCoreHeightSweepArgs& a, hipStream_t stream) {
  if (a.s.n == 0 || a.s.n_windows == 0) return 0;
  uint64_t grid;
  if (check_sweep(a.s, &grid) < 0) return -1;
  // (what keeps a counter's index inside a number's kCoreBuckets: (span - 1) / width < kCoreBuckets)
  if (a.span == 0 || a.span > 1001u || a.width != (a.span + kCoreBuckets - 1u) / kCoreBuckets) { errno = EINVAL; return -1; }
  note_each_launch("cluster_core_height_sweep_kernel");
  hipLaunchKernelGGL(cluster_core_height_sweep_kernel, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_core_height_settle(const ClusterCoreHeightSettleArgs& a, hipStream_t stream) {
  if (a.n_nodes == 0) return 0;
  note_each_launch("cluster_core_height_settle_kernel");
  hipLaunchKernelGGL(cluster_core_height_settle_kernel, dim3((a.n_nodes + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_core_tree_sweep(const ClusterCoreTreeSweepArgs& a, hipStream_t stream) {
  if (a.t.s.n == 0 || a.t.s.n_windows == 0) return 0;
  uint64_t grid;
  if (check_sweep(a.t.s, &grid) < 0 || a.t.round == 0) { errno = EINVAL; return -1; }
  note_each_launch("cluster_core_tree_sweep_kernel");
  hipLaunchKernelGGL(cluster_core_tree_sweep_kernel, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
