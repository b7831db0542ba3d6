// cluster_kernels.hip -- the clustering kernels (launch code: cluster.hip).
//
// cluster_nodes_kernel: the node tables (cluster.h).
// cluster_sweep_kernel: similar_sweep_kernel's all mode (similar_kernels.hip: a window's postings counted into LDS,
// bytes or 16-bit halves; the floor's bars t and [rlo, rhi]; windows passed over by win_min_tri / win_max_tri; the
// t - 1 largest dense slices left out and asked through their bitmaps) with another ending: a rank in front of the
// needle's own position that passes the exact floor test and is a node is united with the needle's node, counted, and
// forgotten.  A deleted rank is no node (the extraction passes it over), so the tombstones are not read.
// cluster_label_kernel: every node's root, after the last sweep.
//
// The union-find forest, parent[]: hooking always puts the root with the larger number under the smaller, so
//   (1) parent[x] <= x at all times, and every write lowers a word: a chain of parents strictly descends, has no
//       cycle and at most n_nodes links;
//   (2) a component's root is its lowest number, which -- the numbering being the references ascending -- holds its
//       smallest reference: the label, whatever the order of the unions.
// Workgroups all over the chip read and write the same words during one sweep.  A CU's L1 is never refreshed by other
// CUs' stores and the XCDs' L2s are not coherent, so inside the sweep EVERY access to parent[] is an agent-scope
// atomic (pf_load, pf_cas, pf_min below; nothing else touches it).  No access is ordered against any other and none
// needs to be, because every value ever stored in parent[x] is an ancestor of x (or x itself) and stays one for ever:
// links only change from x -> p to x -> (an ancestor of p), and a root only stops being one by a compare-and-swap
// that saw it as a root.  Hence
//   * a find that follows values read at any time, however old, walks up x's true chain and ends at a number that
//     was x's root when read; "a and b reach the same number" proves them connected for good, so skipping that union
//     is right;
//   * "different roots" may be out of date, which costs a compare-and-swap: it succeeds only if parent[hi] is still hi
//     at the coherence point (hi still a root: the hook loses nothing and keeps (1)), and otherwise returns the
//     word's current value, an ancestor of hi, from which the loop goes on;
//   * path halving stores by atomic min: of two ancestors of x the lower-numbered is the farther, still an ancestor.
// Nothing waits for another workgroup.  Every loop is bounded by (1): a find takes at most n_nodes steps and every
// lost compare-and-swap lowers the root in hand; the step budget below is a multiple of that, and running out of it
// sets ClusterTotals::error instead of spinning.  The kernels before and after the sweeps meet parent[] across launch
// boundaries and use plain accesses.
#include "cluster.h"
#include "find_kernels.h"
#include "hip_try.h"

namespace blurrily {

namespace {

constexpr uint32_t kCluThreads  = 512;
constexpr uint32_t kCluWaves    = kCluThreads / 64;
constexpr uint32_t kCluWords    = kWindowSize / 4;            // 64 KiB of counters: a window in bytes, half a window in 16 bits
constexpr uint32_t kCluMaxDense = 64;                         // dense slices of a (needle, window) that may be left out

__device__ __forceinline__ uint32_t pf_load(uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// parent[x]: want -> to if it still holds `want`; returns what it held
__device__ __forceinline__ uint32_t pf_cas(uint32_t* p, uint32_t want, uint32_t to) {
  __hip_atomic_compare_exchange_strong(p, &want, to, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return want;
}
__device__ __forceinline__ void pf_min(uint32_t* p, uint32_t v) {
  (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// x's root as far as this lane can tell, halving the path on the way; false: the budget ran out
__device__ inline bool pf_find(uint32_t* parent, uint32_t* x, uint64_t* budget) {
  uint32_t v = *x;
  for (;;) {
    const uint32_t p = pf_load(parent + v);
    if (p >= v) { *x = v; return true; }                      // (p == v: a root; above v nothing is ever stored)
    const uint32_t g = pf_load(parent + p);
    if (g < p) pf_min(parent + v, g);
    v = g < p ? g : p;
    if ((*budget)-- == 0) return false;
  }
}

// a and b in one tree; *a ends as their root as far as this lane can tell (the next union of a starts there)
__device__ inline bool pf_unite(uint32_t* parent, uint32_t* a, uint32_t b, uint64_t* budget) {
  for (;;) {
    if (!pf_find(parent, a, budget) || !pf_find(parent, &b, budget)) return false;
    if (*a == b) return true;
    const uint32_t hi = max(*a, b), lo = min(*a, b);
    const uint32_t was = pf_cas(parent + hi, hi, lo);
    if (was == hi) { *a = lo; return true; }
    *a = lo; b = was;                                         // hi was hooked meanwhile: on from where it hangs now
    if ((*budget)-- == 0) return false;
  }
}

__global__ void cluster_nodes_kernel(const ClusterNodesArgs A) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  A.parent[i] = i;
  if (A.ntri[i] == 0) return;
  const uint2 loc = A.loc[i];
  A.node_of_pos[size_t(loc.x) * kWindowRanks + loc.y] = i;
}

__global__ __launch_bounds__(kCluThreads) void cluster_sweep_kernel(const ClusterSweepArgs a) {
  __shared__ uint32_t cnt[kCluWords];
  __shared__ uint32_t left[(kNumCodes + 31) / 32];            // codes left out of this window's count
  __shared__ uint32_t d_len[kCluMaxDense], d_at[kCluMaxDense], d_code[kCluMaxDense], leave_at[kCluMaxDense];
  __shared__ uint32_t s_nd, s_any, s_edges, s_err;
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

// (one launch: thread i < n_nodes counts node i if it is a root, thread i < n labels the caller's element i)
__global__ __launch_bounds__(256) void cluster_label_kernel(const ClusterLabelArgs A) {
  __shared__ uint32_t s_roots, s_err;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (threadIdx.x == 0) { s_roots = 0; s_err = 0; }
  __syncthreads();
  if (i < A.n_nodes && A.ntri[i] && A.parent[i] == i) atomicAdd(&s_roots, 1u);
  if (i < A.n) {
    uint32_t v = A.inv ? A.inv[i] : i, label = kNoNode;
    if (A.ntri[v]) {
      uint32_t steps = 0;
      for (uint32_t up = A.parent[v]; up < v; up = A.parent[v]) {   // (at most n_nodes links: the chain descends)
        v = up;
        if (++steps > A.n_nodes) { s_err = 1; break; }
      }
      label = A.refs[v];
    }
    A.labels[i] = label;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_roots) atomicAdd(&A.totals->clusters, s_roots);
    if (s_err) atomicOr(&A.totals->error, 1u);
  }
}

}  // namespace

int launch_cluster_nodes(const ClusterNodesArgs& a, hipStream_t stream) {
  if (a.n == 0) return 0;
  note_launch("cluster_nodes_kernel");
  hipLaunchKernelGGL(cluster_nodes_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_sweep(const ClusterSweepArgs& a, hipStream_t stream) {
  if (a.n == 0 || a.n_windows == 0) return 0;
  const uint64_t grid = uint64_t(a.n) * ((a.n_windows + a.per - 1u) / a.per);
  if (grid > 0x7FFFFFFFull) { errno = EINVAL; return -1; }
  note_launch("cluster_sweep_kernel");
  hipLaunchKernelGGL(cluster_sweep_kernel, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_label(const ClusterLabelArgs& a, hipStream_t stream) {
  const uint32_t n = a.n > a.n_nodes ? a.n : a.n_nodes;
  if (n == 0) return 0;
  note_launch("cluster_label_kernel");
  hipLaunchKernelGGL(cluster_label_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
