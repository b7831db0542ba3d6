// cluster_centres_kernels.hip -- the kernels of blurrily_storage_cluster_centres (launch code:
// cluster_centres.hip): per node its degree, per component its centre (the member with the most edges, the smallest
// reference among equals), per node whether an edge of its own reaches that centre.
//
// cluster_centres_sweep_kernel<kMark> is cluster_sweep_kernel's sweep (cluster_kernels.hip: the counters, the floor's
// bars t and [rlo, rhi], the windows passed over, the dense slices left out, each edge found from its end at the
// higher position) as a copy, so that the device code of that kernel stays as it was, with one of two endings:
//   count (kMark == false): the edge (q, other) is united as there, and counted at both ends: one relaxed agent-scope
//     add to degree[other] per edge, and the workgroup's edges -- all of them the needle's -- added once to degree[q]
//     beside the add to totals->edges.  Nothing reads a degree word inside the launch, so no add is ordered against
//     anything; the adds commute, and the launch boundary makes the sums visible to the kernels behind it.
//   mark (kMark == true), after cluster_centres_kernel: no unions, no counting.  An edge whose one end is the other's
//     centre stores 1 to the other's attached word: a plain vector store of one value, from however many workgroups,
//     read only behind the launch boundary.  Only two kinds of needle can meet such an edge from their side: a centre
//     (any lower neighbour of its component is attached by it) and a node whose centre lies at a lower position (in
//     that centre's window, nowhere else).  Everything else leaves at once, singletons (degree 0) first.
// cluster_centres_kernel<kPhase>, after cluster_label_kernel, when parent[] is final (plain accesses):
//   phase 0: every node walks to its root and raises best[root] to degree << 32 | (0xFFFFFFFF - number) by a 64-bit
//     atomic max: the highest degree wins, and among equals the lowest number, which -- the numbering being the
//     references ascending -- holds the smallest reference;
//   phase 1, across a launch boundary: centre_of[u] and attached[u] = (u is its centre) for every number, and the
//     caller's elements' centres and degrees, through inv as the labels go.
// The walks are bounded as cluster_label_kernel's is; running out sets ClusterTotals::error.
#include "cluster.h"
#include "cluster_forest.h"
#include "find_kernels.h"
#include "hip_try.h"

namespace blurrily {

namespace {

template <bool kMark>
__global__ __launch_bounds__(kCluThreads) void cluster_centres_sweep_kernel(const ClusterCentresSweepArgs A) {
  const ClusterSweepArgs& a = A.s;
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
  uint32_t w_begin = wr * a.per, w_end = min(min(a.n_windows, (wr + 1u) * a.per), qloc.x - a.win0 + 1u);
  uint32_t q_centre = q;
  if (kMark) {
    if (A.degree[q] == 0) return;                             // (a singleton: its own centre, marked already)
    q_centre = A.centre_of[q];
    if (q_centre != q) {                                      // no centre: only the edge to its centre matters here
      const uint2 cloc = a.loc[q_centre];
      if (uint64_t(cloc.x) * kWindowRanks + cloc.y >= qpos || cloc.x < a.win0) return;   // (the centre's to find; another image)
      w_begin = max(w_begin, cloc.x - a.win0);
      w_end = min(w_end, cloc.x - a.win0 + 1u);
    }
  }
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
          if (kMark) {
            if (q_centre == other) A.attached[q] = 1u;
            if (A.centre_of[other] == q) A.attached[other] = 1u;
          } else {
            ++mine;
            (void)__hip_atomic_fetch_add(A.degree + other, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ok) {
              uint64_t budget = 4ull * a.n_nodes + 64u;
              ok = pf_unite(a.parent, &root, other, &budget);
            }
          }
        }
      }
      __syncthreads();
    }
    if (tid < nd) atomicAnd(&left[d_code[tid] >> 5], ~(1u << (d_code[tid] & 31u)));   // (cleared for the next window)
  }
  if (kMark) return;
  if (mine) atomicAdd(&s_edges, mine);
  if (!ok) s_err = 1;
  __syncthreads();
  if (tid == 0) {
    if (s_edges) {
      atomicAdd(&a.totals->edges, static_cast<unsigned long long>(s_edges));
      (void)__hip_atomic_fetch_add(A.degree + q, s_edges, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (s_err) atomicOr(&a.totals->error, 1u);
  }
}

// v's root (at most n_nodes links: the chain descends); false: the walk ran out
__device__ __forceinline__ bool final_root(const uint32_t* parent, uint32_t n_nodes, uint32_t* v) {
  uint32_t steps = 0;
  for (uint32_t up = parent[*v]; up < *v; up = parent[*v]) {
    *v = up;
    if (++steps > n_nodes) return false;
  }
  return true;
}

// (one launch per phase: thread i < n_nodes serves number i, in phase 1 thread i < n also the caller's element i)
template <int kPhase>
__global__ __launch_bounds__(256) void cluster_centres_kernel(const ClusterCentresArgs A) {
  __shared__ uint32_t s_err;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (threadIdx.x == 0) s_err = 0;
  __syncthreads();
  if (i < A.n_nodes) {
    uint32_t r = i, centre = kNoNode;
    if (A.ntri[i]) {
      if (!final_root(A.parent, A.n_nodes, &r)) s_err = 1;
      if (kPhase == 0)
        atomicMax(A.best + r, (static_cast<unsigned long long>(A.degree[i]) << 32) | (0xFFFFFFFFu - i));
      else
        centre = 0xFFFFFFFFu - uint32_t(A.best[r]);
    }
    if (kPhase == 1) { A.centre_of[i] = centre; A.attached[i] = centre == i ? 1u : 0u; }
  }
  if (kPhase == 1 && i < A.n) {
    uint32_t v = A.inv ? A.inv[i] : i, centre = kNoNode, degree = 0;
    if (A.ntri[v]) {
      degree = A.degree[v];
      if (!final_root(A.parent, A.n_nodes, &v)) s_err = 1;
      centre = A.refs[0xFFFFFFFFu - uint32_t(A.best[v])];
    }
    A.centres[i] = centre;
    A.degrees[i] = degree;
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_err) atomicOr(&A.totals->error, 1u);
}

}  // namespace

int launch_cluster_centres_sweep(const ClusterCentresSweepArgs& a, bool mark, hipStream_t stream) {
  if (a.s.n == 0 || a.s.n_windows == 0) return 0;
  const uint64_t grid = uint64_t(a.s.n) * ((a.s.n_windows + a.s.per - 1u) / a.s.per);
  if (grid > 0x7FFFFFFFull) { errno = EINVAL; return -1; }
  if (mark) {
    note_launch("cluster_centres_sweep_kernel<mark>");
    hipLaunchKernelGGL(cluster_centres_sweep_kernel<true>, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  } else {
    note_launch("cluster_centres_sweep_kernel");
    hipLaunchKernelGGL(cluster_centres_sweep_kernel<false>, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  }
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_centres(const ClusterCentresArgs& a, hipStream_t stream) {
  const uint32_t n = a.n > a.n_nodes ? a.n : a.n_nodes;
  if (n == 0) return 0;
  note_launch("cluster_centres_kernel");
  hipLaunchKernelGGL(cluster_centres_kernel<0>, dim3((a.n_nodes + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(cluster_centres_kernel<1>, dim3((n + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
