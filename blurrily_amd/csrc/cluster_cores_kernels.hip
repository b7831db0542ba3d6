// cluster_cores_kernels.hip -- the kernels of blurrily_storage_cluster_cores (launch code:
// cluster_cores.hip): density-based clusters over the edges of blurrily_storage_cluster.  A node with at least
// min_degree edges is a core; only an edge between two cores unites; a node that is no core takes the label of its
// anchor -- its core neighbour of the highest degree, the smallest reference among equals -- and is a border, or has
// no core neighbour and is noise.
//
// cluster_cores_sweep_kernel<kUnite> is cluster_centres_sweep_kernel's sweep (cluster_centres_kernels.hip: the
// counters, the floor's bars t and [rlo, rhi], the windows passed over, the dense slices left out, each edge found
// from its end at the higher position), written once here with one of two endings, so that the device code of the
// three older sweep kernels stays as it was:
//   degree (kUnite == false), the first sweep: the edge (q, other) is counted at both ends and nothing else -- one
//     relaxed agent-scope add to degree[other] per edge, and the workgroup's edges, all of them the needle's, added
//     once to degree[q] beside the add to totals->t.edges.  No union, no access to parent[].  Nothing reads a degree
//     word inside the launch; the adds commute, and the launch boundary makes the sums visible behind it.
//   unite (kUnite == true), the second sweep, across that boundary: degree[] is final and read by plain loads.  A
//     needle without an edge leaves at once.  With cq = degree[q] >= min_degree (uniform in the workgroup) and co the
//     same of `other`: both cores -- pf_unite as cluster_sweep_kernel does, and a core edge counted; cq alone --
//     anchor[other] is raised to q's key degree[q] << 32 | (0xFFFFFFFF - q) by a relaxed agent-scope 64-bit max; co
//     alone -- other's key is a candidate for anchor[q]: each lane keeps its highest, the workgroup reduces them in
//     LDS and issues one global max; neither -- nothing.  Nothing reads an anchor word inside the launch; max is
//     commutative and idempotent.  A key is never 0: an anchor has an edge, so its degree, on top, is at least 1.
// cluster_cores_label_kernel, after the last sweep, when parent[], degree[] and anchor[] are final (plain accesses):
// the cores that are their own root are the clusters (cluster_label_kernel counts every root among the nodes, and a
// node that is no core stays its own root), and every element of the caller's gets its label, degree and kind through
// inv as cluster_centres_kernel's outputs go.  The walks are bounded as there; running out sets ClusterTotals::error.
#include "cluster.h"
#include "cluster_forest.h"
#include "find_kernels.h"
#include "hip_try.h"

namespace blurrily {

namespace {

// what anchor[] is raised to for a core neighbour u: the highest degree wins, and among equals the lowest number,
// which -- the numbering being the references ascending -- holds the smallest reference
__device__ __forceinline__ unsigned long long anchor_key(uint32_t degree, uint32_t u) {
  return (static_cast<unsigned long long>(degree) << 32) | (0xFFFFFFFFu - u);
}
__device__ __forceinline__ void anchor_raise(unsigned long long* p, unsigned long long key) {
  (void)__hip_atomic_fetch_max(p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool kUnite>
__global__ __launch_bounds__(kCluThreads) void cluster_cores_sweep_kernel(const ClusterCoresSweepArgs A) {
  const ClusterSweepArgs& a = A.s;
  __shared__ uint32_t cnt[kCluWords];
  __shared__ uint32_t left[(kNumCodes + 31) / 32];            // codes left out of this window's count
  __shared__ uint32_t d_len[kCluMaxDense], d_at[kCluMaxDense], d_code[kCluMaxDense], leave_at[kCluMaxDense];
  __shared__ uint32_t s_nd, s_any, s_edges, s_err;
  __shared__ unsigned long long s_anchor;               // unite: the highest key among the needle's core neighbours
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
  const uint32_t q_degree = kUnite ? A.degree[q] : 0u;
  if (kUnite && q_degree == 0) return;                        // (no edge: nothing to unite, nobody's anchor)
  const bool cq = q_degree >= A.min_degree;                   // unite: the needle is a core
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
  if (tid == 0) { s_edges = 0; s_err = 0; s_anchor = 0; }
  __syncthreads();

  uint32_t root = q;                                          // the needle's root as far as this lane knows
  uint32_t mine = 0;                                          // edges this lane found (unite: between two cores)
  unsigned long long best = 0;                                // unite: the highest key of this lane's core neighbours
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
          if (!kUnite) {
            ++mine;
            (void)__hip_atomic_fetch_add(A.degree + other, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
          }
          const uint32_t o_degree = A.degree[other];
          const bool co = o_degree >= A.min_degree;
          if (cq && co) {
            ++mine;
            if (ok) {
              uint64_t budget = 4ull * a.n_nodes + 64u;
              ok = pf_unite(a.parent, &root, other, &budget);
            }
          } else if (cq) {
            anchor_raise(A.anchor + other, anchor_key(q_degree, q));
          } else if (co) {
            best = max(best, anchor_key(o_degree, other));
          }
        }
      }
      __syncthreads();
    }
    if (tid < nd) atomicAnd(&left[d_code[tid] >> 5], ~(1u << (d_code[tid] & 31u)));   // (cleared for the next window)
  }
  if (mine) atomicAdd(&s_edges, mine);
  if (best) atomicMax(&s_anchor, best);
  if (!ok) s_err = 1;
  __syncthreads();
  if (tid == 0) {
    if (!kUnite) {
      if (s_edges) {
        atomicAdd(&A.totals->t.edges, static_cast<unsigned long long>(s_edges));
        (void)__hip_atomic_fetch_add(A.degree + q, s_edges, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    } else {
      if (s_edges) atomicAdd(&A.totals->core_edges, static_cast<unsigned long long>(s_edges));
      if (s_anchor) anchor_raise(A.anchor + q, s_anchor);
    }
    if (s_err) atomicOr(&A.totals->t.error, 1u);
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

// (one launch: thread i < n_nodes counts number i if it is a core and its own root, thread i < n serves the caller's
// element i)
__global__ __launch_bounds__(256) void cluster_cores_label_kernel(const ClusterCoresLabelArgs A) {
  __shared__ uint32_t s_roots, s_err;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (threadIdx.x == 0) { s_roots = 0; s_err = 0; }
  __syncthreads();
  if (i < A.n_nodes && A.ntri[i] && A.degree[i] >= A.min_degree && A.parent[i] == i) atomicAdd(&s_roots, 1u);
  if (i < A.n) {
    uint32_t v = A.inv ? A.inv[i] : i, label = kNoNode, degree = 0;
    uint8_t kind = kKindNone;
    if (A.ntri[v]) {
      degree = A.degree[v];
      const unsigned long long key = A.anchor[v];
      kind = degree >= A.min_degree ? kKindCore : key ? kKindBorder : kKindNoise;
      if (kind == kKindBorder) v = 0xFFFFFFFFu - uint32_t(key);   // (the anchor: a core)
      if (kind != kKindNoise && !final_root(A.parent, A.n_nodes, &v)) s_err = 1;
      label = A.refs[v];
    }
    A.labels[i] = label;
    A.degrees[i] = degree;
    A.kinds[i] = kind;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_roots) atomicAdd(&A.totals->t.clusters, s_roots);
    if (s_err) atomicOr(&A.totals->t.error, 1u);
  }
}

}  // namespace

int launch_cluster_cores_sweep(const ClusterCoresSweepArgs& a, bool unite, hipStream_t stream) {
  if (a.s.n == 0 || a.s.n_windows == 0) return 0;
  const uint64_t grid = uint64_t(a.s.n) * ((a.s.n_windows + a.s.per - 1u) / a.s.per);
  if (grid > 0x7FFFFFFFull) { errno = EINVAL; return -1; }
  if (unite) {
    note_launch("cluster_cores_sweep_kernel<unite>");
    hipLaunchKernelGGL(cluster_cores_sweep_kernel<true>, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  } else {
    note_launch("cluster_cores_sweep_kernel");
    hipLaunchKernelGGL(cluster_cores_sweep_kernel<false>, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  }
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_cores_label(const ClusterCoresLabelArgs& a, hipStream_t stream) {
  const uint32_t n = a.n > a.n_nodes ? a.n : a.n_nodes;
  if (n == 0) return 0;
  note_launch("cluster_cores_label_kernel");
  hipLaunchKernelGGL(cluster_cores_label_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
