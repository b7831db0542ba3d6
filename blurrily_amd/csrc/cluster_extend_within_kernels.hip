// cluster_extend_within_kernels.hip -- the kernels of blurrily_storage_cluster_extend_within (DESIGN.md section 45;
// launch code: cluster_extend_within.hip): blurrily_storage_cluster_extend's forest -- seeds for the old nodes, only the
// new ones looked at -- where a seed and an edge also need both ends under one block key.
//
// cluster_extend_within_seed_kernel: cluster_extend_seed_kernel's lane per old element with one test more: an element
// and the node holding its label are united only when both carry the same key.
//
// cluster_extend_within_kernel: the direct form, for blocks small enough to score their new members against every
// member.  It reads no image: ClusterCall::begin has extracted every number's distinct codes, and the kernel works on
// those.  One workgroup per tile of up to kClusterWithinTile consecutive places of new_order, all NEW numbers of one
// block (cluster_plan.h).  The tile's needles go into LDS TRANSPOSED as in cluster_within_kernel: one 16-bit word per
// trigram code, bit k set when needle k of the tile holds the code (21 952 codes, 43 904 bytes: three workgroups a CU).
// Then one pass over ALL of the block's places, a member a lane: a member whose R lies outside the hull of the
// needles' [ceil(pT/1000), floor(1000T/p)] is dropped by R alone; otherwise each of its codes costs one LDS read that
// answers for all 16 needles, the bits spread into four words of byte counters (emptied into 32-bit counts every 255
// codes, so any T and any R count exactly).  For needle u and a member v that passes the exact floor test: v == u is
// the needle itself; an OLD v is an edge, found here and nowhere else because v is no needle of any tile; a NEW v is a
// needle of some tile too, and the edge is the end's with the higher number to find (v < u).  So every edge with a new
// end is found exactly once.
//
// cluster_extend_within_sweep_kernel: cluster_extend_sweep_kernel's sweep (the needles are new numbers through a list,
// every window of both images, old candidates wherever they lie, new ones from the higher position only) with
// cluster_within_sweep_kernel's one line: a candidate node under another key than the needle's is passed over before
// the edge is counted.
//
// A block is served by one of the two as a whole, so every pair of it falls under one of the two once-rules, never
// both.  That matters: between two new nodes the direct kernel gives the edge to the higher NUMBER, the sweep to the
// higher POSITION in the images, and the two orders need not agree -- a block split between the kernels could count
// such a pair twice or not at all.  plan_extend_within_blocks (cluster_plan.h) gives a block's new numbers to tiles
// or to the needle list, never to both, and tests/cpp/cluster_extend_within_plan_check.cpp holds it to that.
//
// The forest is cluster_kernels.hip's and its argument holds with seeds as cluster_extend_kernels.hip states it: all
// three kernels touch parent[] through cluster_forest.h's agent-scope atomics alone, so they may share one forest in
// stream order or side by side.
#include "cluster.h"
#include "cluster_forest.h"
#include "find_kernels.h"
#include "hip_try.h"

namespace blurrily {

namespace {

constexpr uint32_t kCxwThreads    = 256;
constexpr uint32_t kCxwG          = kClusterWithinTile;
constexpr uint32_t kCxwImageWords = (kNumCodes + 1) / 2;      // a 16-bit word per code, two to a word
static_assert(kCxwG == 16, "a code's word of the transposed image has a bit per needle of the tile");
static_assert(kCxwThreads == 16 * kCxwG, "the image is filled by 16 lanes per needle");

__global__ __launch_bounds__(256) void cluster_extend_within_seed_kernel(const ClusterExtendWithinSeedArgs B) {
  const ClusterExtendSeedArgs& A = B.s;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_old) return;
  uint32_t v = A.inv ? A.inv[i] : i;
  if (v >= A.n_nodes) return;
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
  if (B.block_of[v] != B.block_of[lo]) return;                // ... or under another key: no such seed
  uint64_t budget = 4ull * A.n_nodes + 64u;
  if (!pf_unite(A.parent, &v, lo, &budget)) atomicOr(&A.totals->error, 1u);
}

__global__ __launch_bounds__(kCxwThreads) void cluster_extend_within_kernel(const ClusterExtendWithinArgs a) {
  __shared__ uint32_t img[kCxwImageWords];
  __shared__ uint32_t s_num[kCxwG], s_T[kCxwG];
  __shared__ uint32_t s_lo, s_hi, s_edges, s_err;
  const uint32_t tid = threadIdx.x;
  if (blockIdx.x >= a.n_tiles) return;
  const ClusterExtendWithinTile tile = a.tiles[blockIdx.x];
  if (tile.count == 0 || tile.count > kCxwG || tile.begin > tile.end || tile.end > a.n_order ||
      tile.first > a.n_new_order || tile.count > a.n_new_order - tile.first)
    return;                                                   // (uniform: no such tile is planned)
  const uint32_t p = a.min_permille;
  for (uint32_t i = tid; i < kCxwImageWords; i += kCxwThreads) img[i] = 0;
  if (tid < kCxwG) {
    uint32_t u = kNoNode, T = 0;
    if (tid < tile.count) {
      u = a.new_order[tile.first + tid];
      T = u < a.n_nodes ? a.q_ntri[u] : 0u;
    }
    s_num[tid] = u;
    s_T[tid] = T;
  }
  if (tid == 0) { s_lo = 0xFFFFFFFFu; s_hi = 0; s_edges = 0; s_err = 0; }
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

  uint32_t mine = 0;                                          // edges this lane found
  bool ok = true;
  // every member of the block, old and new, in front of the needles and behind them
  for (uint32_t place = tile.begin + tid; place < tile.end; place += kCxwThreads) {
    const uint32_t v = a.order[place];
    if (v >= a.n_nodes) continue;
    const uint32_t R = a.q_ntri[v];
    if (R == 0 || R < lo || R > hi) continue;                 // no node, or no needle's floor allows this R
    const uint16_t* mc = a.qcodes + a.qoff[v] + uint64_t(v);
    uint32_t cnt[kCxwG];
#pragma unroll
    for (uint32_t k = 0; k < kCxwG; ++k) cnt[k] = 0;
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
      for (uint32_t k = 0; k < kCxwG; ++k) cnt[k] += (acc[k >> 2] >> ((k & 3u) * 8u)) & 0xFFu;
    }
    const bool v_new = (a.is_new[v >> 5] >> (v & 31u)) & 1u;
    uint32_t root = v;                                        // the member's root as far as this lane knows
#pragma unroll
    for (uint32_t k = 0; k < kCxwG; ++k) {
      const uint32_t m = cnt[k], T = s_T[k], u = s_num[k];
      if (m == 0 || T == 0 || v == u) continue;               // (no needle, or the needle itself)
      if (v_new && v > u) continue;                           // (between two new numbers the edge is the higher one's)
      if (1000ull * m < uint64_t(p) * (uint64_t(T) + R - m)) continue;   // the floor, exactly
      ++mine;
      if (ok) {
        uint64_t budget = 4ull * a.n_nodes + 64u;
        ok = pf_unite(a.parent, &root, u, &budget);
      }
    }
  }
  if (mine) atomicAdd(&s_edges, mine);
  if (!ok) s_err = 1;
  __syncthreads();
  if (tid == 0) {
    if (s_edges) atomicAdd(&a.totals->edges, static_cast<unsigned long long>(s_edges));
    if (s_err) atomicOr(&a.totals->error, 1u);
  }
}

__global__ __launch_bounds__(kCluThreads) void cluster_extend_within_sweep_kernel(const ClusterExtendWithinSweepArgs A) {
  const ClusterSweepArgs& a = A.s;
  __shared__ uint32_t cnt[kCluWords];
  __shared__ uint32_t left[(kNumCodes + 31) / 32];            // codes left out of this window's count
  __shared__ uint32_t d_len[kCluMaxDense], d_at[kCluMaxDense], d_code[kCluMaxDense], leave_at[kCluMaxDense];
  __shared__ uint32_t s_nd, s_any, s_edges, s_err;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tasks = (a.n_windows + a.per - 1u) / a.per;
  const uint32_t qi = blockIdx.x / tasks, wr = blockIdx.x % tasks;
  if (qi >= a.n) return;
  const uint32_t q = A.needles[a.q_base + qi];                // (a new number of a swept block)
  if (q >= a.n_nodes) return;
  const uint32_t T = a.q_ntri[q];
  if (T == 0) return;                                         // (the map does not hold it: no node)
  const uint32_t qblock = A.block_of[q];
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
          if (A.block_of[other] != qblock) continue;          // another block's: no edge
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

int launch_cluster_extend_within_seed(const ClusterExtendWithinSeedArgs& a, hipStream_t stream) {
  if (a.s.n_old == 0) return 0;
  note_launch("cluster_extend_within_seed_kernel");
  hipLaunchKernelGGL(cluster_extend_within_seed_kernel, dim3((a.s.n_old + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_extend_within(const ClusterExtendWithinArgs& a, hipStream_t stream) {
  if (a.n_tiles == 0) return 0;
  if (a.n_tiles > 0x7FFFFFFFu) { errno = EINVAL; return -1; }
  note_launch("cluster_extend_within_kernel");
  hipLaunchKernelGGL(cluster_extend_within_kernel, dim3(a.n_tiles), dim3(kCxwThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_extend_within_sweep(const ClusterExtendWithinSweepArgs& a, hipStream_t stream) {
  if (a.s.n == 0 || a.s.n_windows == 0) return 0;
  const uint64_t grid = uint64_t(a.s.n) * ((a.s.n_windows + a.s.per - 1u) / a.s.per);
  if (grid > 0x7FFFFFFFull) { errno = EINVAL; return -1; }
  note_launch("cluster_extend_within_sweep_kernel");
  hipLaunchKernelGGL(cluster_extend_within_sweep_kernel, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
