// cluster_cores_within_kernels.hip -- the kernels of blurrily_storage_cluster_cores_within (launch
// code: cluster_cores_within.hip): blurrily_storage_cluster_cores' cores, borders and noise where an edge also needs
// both ends under one block key.  A block is served by one of two kernels, as cluster_within serves it, and each kernel
// has cluster_cores' two endings: the degrees first, then, across a launch boundary, the unions between cores and the
// borders' anchors.  The bodies are copies, as the others' are, so that the device code of the others stays as it was.
//
// cluster_cores_within_kernel<kUnite>: cluster_within_kernel's direct form (cluster_within_kernels.hip: one workgroup
// per tile of up to kClusterWithinTile places of one block, the tile's needles TRANSPOSED in LDS, a 16-bit word per
// code, the hull of the needles' R bars, a member a lane, byte counters emptied every 255 codes, the exact floor test,
// an edge found from its end at the higher place only) with one of two endings:
//   degree (kUnite == false): no union, no access to parent[].  A lane counts the tile's needles that pass against
//     its member v and issues one relaxed agent-scope add to degree[v] for the member; each passing needle k gets an
//     LDS add to s_deg[k], and after the member loop one lane per needle with a count issues one global add.  The
//     tile's edges, the sum of s_deg[], go to totals->t.edges.  Nothing reads a degree word inside the launch; the adds
//     commute, and the launch boundary makes the sums visible behind it.
//   unite (kUnite == true), across that boundary: degree[] is final and read by plain loads.  Each needle's degree
//     and whether it is a core stand in LDS beside s_T.  For a pair (member v, needle q) that passes: both cores --
//     pf_unite under cluster_within_kernel's budget, and a core edge counted; q alone -- q's key is a candidate for
//     anchor[v], of which the lane keeps the highest over the tile's needles and issues one anchor_raise per member;
//     v alone -- v's key goes into s_anchor[k] by a 64-bit LDS max, and after the member loop one lane per needle with
//     a key issues one anchor_raise; neither -- nothing.  Nothing reads an anchor word inside the launch; max is
//     commutative and idempotent.  A key is never 0: an anchor has an edge, so its degree, on top, is at least 1.
//   The second pass skips what cannot matter; each skip stands with its reason where it is made.
// Every return in front of a barrier is uniform across the workgroup: the plan's check before any barrier, "no needle
// with an edge" (unite) right behind the first, "no needle held" right behind the third.  Nothing spins.
//
// cluster_cores_within_sweep_kernel<kUnite>: cluster_cores_sweep_kernel<kUnite> (cluster_cores_kernels.hip) with
// cluster_within_sweep_kernel's two differences: the needles are the numbers of the swept blocks, through the list of
// them, and a candidate node under another key than the needle's is passed over before anything is counted or raised.
//
// A swept block and a directly scored block never share an edge, so the two kernels add into the same degree[],
// anchor[], forest and totals in stream order with nothing between them.  The forest is cluster_kernels.hip's and its
// argument holds as it stands: both kernels touch parent[] through cluster_forest.h's agent-scope atomics alone.
#include "cluster.h"
#include "cluster_forest.h"
#include "find_kernels.h"
#include "hip_try.h"

namespace blurrily {

namespace {

// what anchor[] is raised to for a core neighbour u (cluster_cores_kernels.hip's): the highest degree wins, and among
// equals the lowest number, which -- the numbering being the references ascending, number_nodes_keyed's as
// number_nodes' -- holds the smallest reference
__device__ __forceinline__ unsigned long long anchor_key(uint32_t degree, uint32_t u) {
  return (static_cast<unsigned long long>(degree) << 32) | (0xFFFFFFFFu - u);
}
__device__ __forceinline__ void anchor_raise(unsigned long long* p, unsigned long long key) {
  (void)__hip_atomic_fetch_max(p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr uint32_t kCcwThreads    = 256;
constexpr uint32_t kCcwG          = kClusterWithinTile;
constexpr uint32_t kCcwImageWords = (kNumCodes + 1) / 2;      // a 16-bit word per code, two to a word
static_assert(kCcwG == 16, "a code's word of the transposed image has a bit per needle of the tile");
static_assert(kCcwThreads == 16 * kCcwG, "the image is filled by 16 lanes per needle");
static_assert(kCcwG <= 64, "the tile's needles are looked at by lanes of one wave");

template <bool kUnite>
__global__ __launch_bounds__(kCcwThreads) void cluster_cores_within_kernel(const ClusterCoresWithinArgs A) {
  const ClusterWithinArgs& a = A.w;
  __shared__ uint32_t img[kCcwImageWords];
  __shared__ unsigned long long s_anchor[kCcwG];              // unite: the highest key among each needle's core members
  __shared__ uint32_t s_num[kCcwG], s_T[kCcwG];
  __shared__ uint32_t s_deg[kCcwG];                           // degree: the edges found for each needle; unite: its degree
  __shared__ uint32_t s_core[kCcwG];                          // unite: the needle is a core
  __shared__ uint32_t s_lo, s_hi, s_edges, s_err, s_open, s_any_core;
  const uint32_t tid = threadIdx.x;
  if (blockIdx.x >= a.n_tiles) return;
  const ClusterWithinTile tile = a.tiles[blockIdx.x];
  if (tile.count == 0 || tile.count > kCcwG || tile.first < tile.begin || tile.first > a.n_order ||
      tile.count > a.n_order - tile.first)
    return;                                                   // (uniform: no such tile is planned)
  const uint32_t p = a.min_permille;
  if (tid < kCcwG) {
    uint32_t u = kNoNode, T = 0, d = 0;
    if (tid < tile.count) {
      u = a.order[tile.first + tid];
      T = u < a.n_nodes ? a.q_ntri[u] : 0u;
      if (kUnite && T) {
        d = A.degree[u];                                      // final: the degree launches lie behind a boundary
        // A needle with degree 0 is not put into the image.  Exact: its degree counts every pair of this block that
        // passes the floor with it as an end, so no member passes against it, and a pair that does not pass does
        // nothing below.
        if (d == 0) T = 0;
      }
    }
    const bool core = kUnite && T && d >= A.min_degree;
    s_num[tid] = u;
    s_T[tid] = T;
    s_deg[tid] = d;
    s_core[tid] = core;
    s_anchor[tid] = 0;
    const bool any = __ballot(T != 0) != 0, any_core = __ballot(core) != 0;   // (the tile's lanes are the first of one wave)
    if (tid == 0) { s_lo = 0xFFFFFFFFu; s_hi = 0; s_edges = 0; s_err = 0; s_open = any; s_any_core = any_core; }
  }
  __syncthreads();
  // A tile whose needles all have degree 0 (or are not held) returns.  Exact: every needle has left the image for the
  // reason above, so no pair of this tile could pass.  Uniform: s_open is one LDS word read behind a barrier.
  if (kUnite && !s_open) return;
  for (uint32_t i = tid; i < kCcwImageWords; i += kCcwThreads) img[i] = 0;
  __syncthreads();
  {
    // needle k by lanes 16 k .. 16 k + 15: its bars into the hull, its codes into the image
    const uint32_t k = tid >> 4, T = s_T[k];
    if (T) {
      if ((tid & 15u) == 0) {
        atomicMin(&s_lo, max(1u, uint32_t((uint64_t(p) * T + 999u) / 1000u)));
        atomicMax(&s_hi, p ? uint32_t(min<uint64_t>(1000ull * T / p, 0xFFFFFFFFull)) : 0xFFFFFFFFu);
      }
      const uint32_t u = s_num[k];
      const uint16_t* codes = a.qcodes + a.qoff[u] + uint64_t(u);
      for (uint32_t i = tid & 15u; i < T; i += 16u) {
        const uint32_t c = codes[i];
        if (c < kNumCodes) atomicOr(&img[c >> 1], (1u << k) << ((c & 1u) * 16u));
      }
    }
  }
  __syncthreads();
  const uint32_t lo = s_lo, hi = s_hi;
  if (hi == 0) return;                                        // (uniform: the map holds none of the tile's needles)
  const bool any_core = s_any_core != 0;

  uint32_t mine = 0;                                          // unite: edges between two cores this lane found
  bool ok = true;
  // the members in front of the tile's last place (that place itself is in front of no needle of the tile)
  const uint32_t end = tile.first + tile.count - 1u;
  for (uint32_t place = tile.begin + tid; place < end; place += kCcwThreads) {
    const uint32_t v = a.order[place];
    if (v >= a.n_nodes) continue;
    const uint32_t R = a.q_ntri[v];
    if (R == 0 || R < lo || R > hi) continue;                 // no node, or no needle's floor allows this R
    uint32_t dv = 0;
    bool cv = false;
    if (kUnite) {
      dv = A.degree[v];
      // A member with degree 0 is skipped before it is scored.  Exact: it is an end of no pair that passes.
      if (dv == 0) continue;
      cv = dv >= A.min_degree;
      // A non-core member in front of a tile without a core needle is skipped.  Exact: of the four cases below, "both
      // cores" and "v alone" need v a core, "q alone" needs a core needle, and "neither" does nothing.
      if (!cv && !any_core) continue;
    }
    const uint16_t* mc = a.qcodes + a.qoff[v] + uint64_t(v);
    uint32_t cnt[kCcwG];
#pragma unroll
    for (uint32_t k = 0; k < kCcwG; ++k) cnt[k] = 0;
    for (uint32_t c0 = 0; c0 < R; c0 += 255u) {               // (a byte counts 255 codes at most)
      const uint32_t c1 = min(R, c0 + 255u);
      uint32_t acc[4] = {0, 0, 0, 0};
      for (uint32_t j = c0; j < c1; ++j) {
        const uint32_t c = mc[j];
        if (c >= kNumCodes) continue;
        const uint32_t bits = (img[c >> 1] >> ((c & 1u) * 16u)) & 0xFFFFu;
        if (!bits) continue;
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w)                       // bits 4 w .. 4 w + 3 to the low bit of a byte each
          acc[w] += (((bits >> (4u * w)) & 0xFu) * 0x00204081u) & 0x01010101u;
      }
#pragma unroll
      for (uint32_t k = 0; k < kCcwG; ++k) cnt[k] += (acc[k >> 2] >> ((k & 3u) * 8u)) & 0xFFu;
    }
    uint32_t root = v;                                        // unite: the member's root as far as this lane knows
    uint32_t passed = 0;                                      // degree: the tile's needles that pass against the member
    unsigned long long best = 0;                              // unite: the highest key among the member's core needles
#pragma unroll
    for (uint32_t k = 0; k < kCcwG; ++k) {
      const uint32_t m = cnt[k], T = s_T[k];
      if (m == 0 || T == 0 || place >= tile.first + k) continue;   // (an edge is its higher end's to find)
      if (1000ull * m < uint64_t(p) * (uint64_t(T) + R - m)) continue;   // the floor, exactly
      if (!kUnite) {
        ++passed;
        atomicAdd(&s_deg[k], 1u);
        continue;
      }
      const bool cq = s_core[k] != 0;
      if (cq && cv) {
        ++mine;
        if (ok) {
          uint64_t budget = 4ull * a.n_nodes + 64u;
          ok = pf_unite(a.parent, &root, s_num[k], &budget);
        }
      } else if (cq) {
        best = max(best, anchor_key(s_deg[k], s_num[k]));
      } else if (cv) {
        (void)__hip_atomic_fetch_max(&s_anchor[k], anchor_key(dv, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    if (passed) (void)__hip_atomic_fetch_add(A.degree + v, passed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (best) anchor_raise(A.anchor + v, best);
  }
  if (mine) atomicAdd(&s_edges, mine);
  if (!ok) s_err = 1;
  __syncthreads();
  if (tid < kCcwG) {
    if (!kUnite) {
      const uint32_t found = s_deg[tid];
      if (found) {
        (void)__hip_atomic_fetch_add(A.degree + s_num[tid], found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicAdd(&s_edges, found);                           // (read by lane 0 behind the barrier below)
      }
    } else if (s_anchor[tid]) {
      anchor_raise(A.anchor + s_num[tid], s_anchor[tid]);
    }
  }
  __syncthreads();
  if (tid == 0) {
    if (s_edges) atomicAdd(kUnite ? &A.totals->core_edges : &A.totals->t.edges, static_cast<unsigned long long>(s_edges));
    if (s_err) atomicOr(&A.totals->t.error, 1u);
  }
}

template <bool kUnite>
__global__ __launch_bounds__(kCluThreads) void cluster_cores_within_sweep_kernel(const ClusterCoresWithinSweepArgs W) {
  const ClusterCoresSweepArgs& A = W.c;
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
  const uint32_t q = W.needles[a.q_base + qi];                // (a number of a swept block)
  if (q >= a.n_nodes) return;
  const uint32_t T = a.q_ntri[q];
  if (T == 0) return;                                         // (the map does not hold it: no node)
  const uint32_t qblock = W.block_of[q];
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
          if (W.block_of[other] != qblock) continue;          // another block's: no edge, no degree, nobody's anchor
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

}  // namespace

int launch_cluster_cores_within(const ClusterCoresWithinArgs& a, bool unite, hipStream_t stream) {
  if (a.w.n_tiles == 0) return 0;
  if (a.w.n_tiles > 0x7FFFFFFFu) { errno = EINVAL; return -1; }
  if (unite) {
    note_launch("cluster_cores_within_kernel<unite>");
    hipLaunchKernelGGL(cluster_cores_within_kernel<true>, dim3(a.w.n_tiles), dim3(kCcwThreads), 0, stream, a);
  } else {
    note_launch("cluster_cores_within_kernel");
    hipLaunchKernelGGL(cluster_cores_within_kernel<false>, dim3(a.w.n_tiles), dim3(kCcwThreads), 0, stream, a);
  }
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_cores_within_sweep(const ClusterCoresWithinSweepArgs& a, bool unite, hipStream_t stream) {
  if (a.c.s.n == 0 || a.c.s.n_windows == 0) return 0;
  const uint64_t grid = uint64_t(a.c.s.n) * ((a.c.s.n_windows + a.c.s.per - 1u) / a.c.s.per);
  if (grid > 0x7FFFFFFFull) { errno = EINVAL; return -1; }
  if (unite) {
    note_launch("cluster_cores_within_sweep_kernel<unite>");
    hipLaunchKernelGGL(cluster_cores_within_sweep_kernel<true>, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  } else {
    note_launch("cluster_cores_within_sweep_kernel");
    hipLaunchKernelGGL(cluster_cores_within_sweep_kernel<false>, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  }
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
