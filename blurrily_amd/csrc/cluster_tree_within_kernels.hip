// cluster_tree_within_kernels.hip -- the kernels of blurrily_storage_cluster_tree_within (launch
// code: cluster_tree_within.hip): the cluster tree where an edge also needs both ends under one block key.  A Boruvka
// round of cluster_tree_kernels.hip takes its edges from two kernels here, which choose where cluster_within's unite:
// whoever finds an edge between two components raises best[] of both, and that file's merge and flatten do the rest as
// they are.
//
// cluster_tree_within_kernel: cluster_within_kernel's direct form (cluster_within_kernels.hip: one workgroup per tile of
// up to kClusterWithinTile places of one block, the tile's needles TRANSPOSED in LDS, a 16-bit word per code, the hull of
// the needles' R bars, a member a lane, byte counters emptied every 255 codes, the exact floor test, an edge found from
// its end at the higher place only) with the tree's ending.  A pair that passes is not united: the ends' components are
// read from comp[], and if they differ the edge's key (cluster.h) is offered to both.  The needle's component takes it
// through one of 16 64-bit LDS words, a word per needle of the tile, which one lane per needle offers to best[] at the
// end; the member's takes the best of the lane's up to 16 keys through best_raise.  Round 1 counts the edges and skips
// nothing.  From round 2 a needle or a member whose component is closed takes no part (no edge leaves a closed
// component, so every edge of such a node lies inside it), and a tile without a needle left returns before it fills
// the image.  Every early return is uniform across the workgroup and stands in front of the first barrier it would
// otherwise miss: the plan's check before any barrier, "no needle left" right behind the first, "no needle held"
// right behind the third.  Nothing spins.
//
// cluster_tree_within_sweep_kernel: cluster_tree_sweep_kernel's sweep (cluster_tree_kernels.hip) with
// cluster_within_sweep_kernel's two differences: the needles are the numbers of the swept blocks, through the list of
// them, and a candidate node under another key than the needle's is passed over before the edge is counted and before
// comp[] is read.  The bodies are copies, as the others' are, so that the device code of the others stays as it was.
//
// The memory model is cluster_tree_kernels.hip's.  comp[] and closed[] are written by no thread while either kernel
// runs (the flatten and the merge wrote them launches ago), so they are read plainly.  best[] is touched, in both, only
// by agent-scope relaxed 64-bit fetch_max and by the relaxed load in front of it that spares the atomic when the word
// already holds as much: a key only rises, and the maximum of a set does not depend on the order of its elements.
// Blocks are disjoint and a component never spans two, so the two kernels of a round may run in stream order, or side
// by side, into the one best[]; the merge reads it a launch later.
#include "cluster.h"
#include "cluster_forest.h"
#include "find_kernels.h"
#include "hip_try.h"
#include "map_internal.h"

namespace blurrily {

namespace {

// (every launch of a call is named, as cluster_tree_kernels.hip names its own: the rounds can be counted)
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

constexpr uint32_t kCtwThreads    = 256;
constexpr uint32_t kCtwG          = kClusterWithinTile;
constexpr uint32_t kCtwImageWords = (kNumCodes + 1) / 2;      // a 16-bit word per code, two to a word
static_assert(kCtwG == 16, "a code's word of the transposed image has a bit per needle of the tile");
static_assert(kCtwThreads == 16 * kCtwG, "the image is filled by 16 lanes per needle");
static_assert(kCtwG <= 64, "the tile's needles are looked at by lanes of one wave");

__global__ __launch_bounds__(kCtwThreads) void cluster_tree_within_kernel(const ClusterTreeWithinArgs A) {
  const ClusterWithinArgs& a = A.w;
  __shared__ uint32_t img[kCtwImageWords];
  __shared__ unsigned long long s_best[kCtwG];                // the best key found for each needle's component
  __shared__ uint32_t s_num[kCtwG], s_T[kCtwG], s_comp[kCtwG];
  __shared__ uint32_t s_lo, s_hi, s_edges, s_open;
  const uint32_t tid = threadIdx.x;
  if (blockIdx.x >= a.n_tiles) return;
  const ClusterWithinTile tile = a.tiles[blockIdx.x];
  if (tile.count == 0 || tile.count > kCtwG || tile.first < tile.begin || tile.first > a.n_order ||
      tile.count > a.n_order - tile.first)
    return;                                                   // (uniform: no such tile is planned)
  const uint32_t p = a.min_permille;
  const bool counting = A.round == 1u;                        // (the edges are counted once, as cluster_within_kernel counts them)
  if (tid < kCtwG) {
    // a needle takes part with T != 0: the map holds it, and from round 2 its component is not closed
    uint32_t u = kNoNode, T = 0, cu = kNoNode;
    if (tid < tile.count) {
      u = a.order[tile.first + tid];
      if (u < a.n_nodes) {
        T = a.q_ntri[u];
        cu = A.comp[u];                                       // frozen for the launch
        if (T && !counting && A.closed[cu]) T = 0;            // no edge leaves it: none of the needle's can
      }
    }
    s_num[tid] = u;
    s_T[tid] = T;
    s_comp[tid] = cu;
    s_best[tid] = 0;
    const bool any = __ballot(T != 0) != 0;                   // (the tile's lanes are the first of one wave)
    if (tid == 0) { s_lo = 0xFFFFFFFFu; s_hi = 0; s_edges = 0; s_open = any; }
  }
  __syncthreads();
  if (!s_open) return;                                        // (uniform: no needle of the tile takes part)
  for (uint32_t i = tid; i < kCtwImageWords; i += kCtwThreads) img[i] = 0;
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
  if (hi == 0) return;                                        // (uniform: s_open says a needle has T != 0, so hi >= 1)

  uint32_t mine = 0;                                          // edges this lane found
  // the members in front of the tile's last place (that place itself is in front of no needle of the tile)
  const uint32_t end = tile.first + tile.count - 1u;
  for (uint32_t place = tile.begin + tid; place < end; place += kCtwThreads) {
    const uint32_t v = a.order[place];
    if (v >= a.n_nodes) continue;
    const uint32_t R = a.q_ntri[v];
    if (R == 0 || R < lo || R > hi) continue;                 // no node, or no needle's floor allows this R
    const uint32_t cv = A.comp[v];
    if (!counting && A.closed[cv]) continue;                  // no edge leaves the member's component
    const uint16_t* mc = a.qcodes + a.qoff[v] + uint64_t(v);
    uint32_t cnt[kCtwG];
#pragma unroll
    for (uint32_t k = 0; k < kCtwG; ++k) cnt[k] = 0;
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
      for (uint32_t k = 0; k < kCtwG; ++k) cnt[k] += (acc[k >> 2] >> ((k & 3u) * 8u)) & 0xFFu;
    }
    unsigned long long member_best = 0;                       // the best key this lane has for best[cv]
#pragma unroll
    for (uint32_t k = 0; k < kCtwG; ++k) {
      const uint32_t m = cnt[k], T = s_T[k];
      if (m == 0 || T == 0 || place >= tile.first + k) continue;   // (an edge is its higher end's to find)
      if (1000ull * m < uint64_t(p) * (uint64_t(T) + R - m)) continue;   // the floor, exactly
      mine += counting;
      if (s_comp[k] == cv) continue;                          // inside a component: no edge of the forest any more
      // the height, floor(1000 m / (T + R - m)): m, T, R <= kNumCodes, so 32 bits hold it exactly
      const unsigned long long h = (1000u * m) / (T + R - m);
      const uint32_t q = s_num[k];
      const uint32_t e_lo = min(q, v), e_hi = max(q, v);
      const unsigned long long key = h << 54 | static_cast<unsigned long long>(~e_lo & kTreeNumberMask) << kTreeNumberBits |
                                     (~e_hi & kTreeNumberMask);
      member_best = max(member_best, key);
      // (the relaxed load spares the atomic when the word already holds as much, as best_raise's does)
      if (__hip_atomic_load(&s_best[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < key)
        (void)__hip_atomic_fetch_max(&s_best[k], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (member_best) best_raise(A.best + cv, member_best);
  }
  if (mine) atomicAdd(&s_edges, mine);
  __syncthreads();
  if (tid < kCtwG && s_best[tid]) best_raise(A.best + s_comp[tid], s_best[tid]);
  if (tid == 0 && s_edges) atomicAdd(&a.totals->edges, static_cast<unsigned long long>(s_edges));
}

__global__ __launch_bounds__(kCluThreads) void cluster_tree_within_sweep_kernel(const ClusterTreeWithinSweepArgs W) {
  const ClusterTreeSweepArgs& A = W.t;
  const ClusterSweepArgs& a = A.s;
  __shared__ __attribute__((aligned(8))) uint32_t cnt[kCluWords];   // (two of its words end as one 64-bit key)
  __shared__ uint32_t left[(kNumCodes + 31) / 32];            // codes left out of this window's count
  __shared__ uint32_t d_len[kCluMaxDense], d_at[kCluMaxDense], d_code[kCluMaxDense], leave_at[kCluMaxDense];
  __shared__ uint32_t s_nd, s_any;
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
  if (w_begin >= w_end) return;
  const uint32_t cq = A.comp[q];                              // the needle's component: frozen for the launch
  const bool counting = A.round == 1u;                        // (the edges are counted once, as cluster_within_sweep_kernel counts them)
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
          if (W.block_of[other] != qblock) continue;          // another block's: no edge
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

}  // namespace

int launch_cluster_tree_within(const ClusterTreeWithinArgs& a, hipStream_t stream) {
  if (a.w.n_tiles == 0) return 0;
  if (a.w.n_tiles > 0x7FFFFFFFu || a.w.n_nodes > kTreeMaxNodes || a.round == 0) { errno = EINVAL; return -1; }
  note_each_launch("cluster_tree_within_kernel");
  hipLaunchKernelGGL(cluster_tree_within_kernel, dim3(a.w.n_tiles), dim3(kCtwThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_tree_within_sweep(const ClusterTreeWithinSweepArgs& a, hipStream_t stream) {
  const ClusterSweepArgs& s = a.t.s;
  if (s.n == 0 || s.n_windows == 0) return 0;
  const uint64_t grid = uint64_t(s.n) * ((s.n_windows + s.per - 1u) / s.per);
  if (grid > 0x7FFFFFFFull || s.n_nodes > kTreeMaxNodes || a.t.round == 0) { errno = EINVAL; return -1; }
  note_each_launch("cluster_tree_within_sweep_kernel");
  hipLaunchKernelGGL(cluster_tree_within_sweep_kernel, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
