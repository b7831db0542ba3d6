// cluster_core_tree_within_kernels.hip -- the kernels of blurrily_storage_cluster_core_tree_within (DESIGN.md section
// 44; launch code: cluster_core_tree_within.hip): the cluster core tree where an edge also needs both ends under one
// block key, so a core height ranks those edges only.  A block is served by one of two kernels, as cluster_within
// serves it, and each kernel has the core tree's two endings: the height ending, which sorts every edge into its ends'
// brackets for cluster_core_height_settle_kernel (cluster_core_tree_kernels.hip, as it is), and the tree ending, which
// offers a Boruvka round its edges for cluster_tree_kernels.hip's merge and flatten (as they are).  The bodies are
// copies, as the others' are, so that the device code of the others stays as it was.
//
// cluster_core_tree_within_kernel<kTree>: cluster_tree_within_kernel's tile (cluster_tree_within_kernels.hip: one
// workgroup per tile of up to kClusterWithinTile places of one block, the tile's needles TRANSPOSED in LDS, a 16-bit
// word per code, the hull of the needles' R bars, a member a lane, byte counters emptied every 255 codes, the exact
// floor test, a pair found from its end at the higher place only) with one of two endings:
//   height (kTree == false): nothing is united and nothing offered.  A pair of height h that passes adds 1 to counter
//     (h - core[x]) / width of each end x with h - core[x] < span.  The needle's end goes to an LDS histogram of
//     16 x kCoreBuckets words by a workgroup-scope add, and after the member loop one lane per non-zero word issues one
//     relaxed agent-scope add to hist[].  The member's end goes straight to hist[v] by one relaxed agent-scope add per
//     pair.  A lane does not merge its up to 16 adds per counter first: that needs kCoreBuckets more registers a lane
//     (or a 16 x 16 compare network) on top of the 16 match counts the body holds, and on the inputs measured a member
//     passes against fewer than one needle of a tile on average, so there is next to nothing to merge.  The first pass
//     counts the pairs that pass into totals->t.edges.  A needle without a bracket stays in the image: its pairs count
//     at their other end.
//   tree (kTree == true): cluster_tree_within_kernel's offer -- s_best[16] by 64-bit LDS max, one best_raise per
//     member, one per needle at the end -- with the core tree's three differences: a needle without a core height
//     takes no part (T = 0 in LDS), a member without one is passed over before its codes are read, and the key's
//     height is min(h, core[q], core[v]).  Round 1 counts the tree edges into totals->core_edges, and into
//     totals->t.edges too when no height pass ran; from round 2 a needle or a member whose component is closed takes
//     no part, as there.
// Every return is uniform across the workgroup and stands in front of the first barrier it would otherwise miss: the
// plan's check before any barrier, "no needle takes part" right behind the first (s_open is one LDS word read behind
// it), "no needle held" right behind the third (s_hi likewise).  The member loop holds no barrier, so a lane that
// passes a member over misses none.  Nothing spins, and no workgroup waits for another.
//
// cluster_core_tree_within_sweep_kernel<kTree>: core_sweep<kTree> of cluster_core_tree_kernels.hip with the keyed
// sweeps' two differences: the needle is needles[q_base + qi], and a candidate whose block_of differs from the needle's
// is passed over before anything is counted, added or offered.
//
// The memory model is the two files' these are copied from.  core[] and above[] are written by no thread while either
// kernel runs (the settle wrote them a launch ago), comp[] and closed[] likewise (the flatten and the merge), so all
// four are read plainly.  hist[] is touched by relaxed agent-scope adds alone and read by the settle a launch later:
// integer adds commute.  best[] is touched by agent-scope relaxed 64-bit fetch_max and the relaxed load in front of it:
// a key only rises, and a maximum does not depend on the order of its elements.  A swept block and a directly scored
// one share no edge, so both kernels of a pass add into the same hist[], best[] and totals in stream order.
#include "cluster.h"
#include "cluster_forest.h"
#include "find_kernels.h"
#include "hip_try.h"
#include "map_internal.h"

namespace blurrily {

namespace {

// (every launch of a call is named, as cluster_tree_kernels.hip names its own: the passes and rounds can be counted)
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

constexpr uint32_t kCtcThreads    = 256;
constexpr uint32_t kCtcG          = kClusterWithinTile;
constexpr uint32_t kCtcImageWords = (kNumCodes + 1) / 2;      // a 16-bit word per code, two to a word
constexpr uint32_t kCtcHistWords  = kCtcG * kCoreBuckets;     // the needles' counters of one height pass
static_assert(kCtcG == 16, "a code's word of the transposed image has a bit per needle of the tile");
static_assert(kCtcThreads == 16 * kCtcG, "the image is filled by 16 lanes per needle");
static_assert(kCtcG <= 64, "the tile's needles are looked at by lanes of one wave");
static_assert((kCoreBuckets & (kCoreBuckets - 1u)) == 0, "a word of the LDS histogram splits into needle and counter by shifts");

template <bool kTree>
__global__ __launch_bounds__(kCtcThreads) void cluster_core_tree_within_kernel(const ClusterCoreTreeWithinArgs A) {
  const ClusterWithinArgs& a = A.w;
  __shared__ uint32_t img[kCtcImageWords];
  __shared__ unsigned long long s_best[kTree ? kCtcG : 1];    // tree: the best key found for each needle's component
  __shared__ uint32_t s_hist[kTree ? 1 : kCtcHistWords];      // height: needle k's counters at [k * kCoreBuckets ..)
  __shared__ uint32_t s_num[kCtcG], s_T[kCtcG], s_comp[kCtcG], s_core[kCtcG];
  __shared__ uint32_t s_lo, s_hi, s_edges, s_open, s_any_bracket;
  const uint32_t tid = threadIdx.x;
  if (blockIdx.x >= a.n_tiles) return;
  const ClusterWithinTile tile = a.tiles[blockIdx.x];
  if (tile.count == 0 || tile.count > kCtcG || tile.first < tile.begin || tile.first > a.n_order ||
      tile.count > a.n_order - tile.first)
    return;                                                   // (uniform: no such tile is planned)
  const uint32_t p = a.min_permille;
  // the pairs are counted once: by the first height pass, or by round 1 (which counts the tree edges)
  const bool counting = kTree ? A.round == 1u : A.count_edges != 0u;
  if (tid < kCtcG) {
    // a needle takes part with T != 0: the map holds it; tree: it has a core height, and from round 2 its component
    // is not closed
    uint32_t u = kNoNode, T = 0, cu = kNoNode, core_u = kNoCore;
    if (tid < tile.count) {
      u = a.order[tile.first + tid];
      if (u < a.n_nodes) {
        T = a.q_ntri[u];
        core_u = A.core[u];                                   // frozen for the launch (kNoCore where T == 0)
        if (kTree && T) {
          if (core_u == kNoCore) {
            T = 0;                                            // no edge of the needle's is in the tree
          } else {
            cu = A.comp[u];                                   // frozen for the launch
            if (!counting && A.closed[cu]) T = 0;             // no edge leaves it: none of the needle's can
          }
        }
      }
    }
    s_num[tid] = u;
    s_T[tid] = T;
    s_comp[tid] = cu;
    s_core[tid] = core_u;
    if (kTree) s_best[tid] = 0;
    // (the tile's lanes are the first of one wave)
    const bool any = __ballot(T != 0) != 0, any_bracket = __ballot(T != 0 && core_u != kNoCore) != 0;
    if (tid == 0) { s_lo = 0xFFFFFFFFu; s_hi = 0; s_edges = 0; s_open = any; s_any_bracket = any_bracket; }
  }
  __syncthreads();
  if (!s_open) return;                                        // (uniform: no needle of the tile takes part)
  for (uint32_t i = tid; i < kCtcImageWords; i += kCtcThreads) img[i] = 0;
  if (!kTree)
    for (uint32_t i = tid; i < kCtcHistWords; i += kCtcThreads) s_hist[i] = 0;
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
  const bool any_bracket = s_any_bracket != 0;

  uint32_t mine = 0;                                          // pairs this lane counted
  // the members in front of the tile's last place (that place itself is in front of no needle of the tile)
  const uint32_t end = tile.first + tile.count - 1u;
  for (uint32_t place = tile.begin + tid; place < end; place += kCtcThreads) {
    const uint32_t v = a.order[place];
    if (v >= a.n_nodes) continue;
    const uint32_t R = a.q_ntri[v];
    if (R == 0 || R < lo || R > hi) continue;                 // no node, or no needle's floor allows this R
    const uint32_t core_v = A.core[v];                        // frozen for the launch
    uint32_t cv = 0;
    if (kTree) {
      if (core_v == kNoCore) continue;                        // not an end of any tree edge
      cv = A.comp[v];
      if (!counting && A.closed[cv]) continue;                // no edge leaves the member's component
    } else {
      // A member without a bracket in front of a tile none of whose needles has one is passed over, unless the pairs
      // are being counted.  Exact: a pair that passes adds to an end's counter only where that end has a bracket, and
      // here neither end of any of the member's pairs with this tile has one.
      if (!counting && core_v == kNoCore && !any_bracket) continue;
    }
    const uint16_t* mc = a.qcodes + a.qoff[v] + uint64_t(v);
    uint32_t cnt[kCtcG];
#pragma unroll
    for (uint32_t k = 0; k < kCtcG; ++k) cnt[k] = 0;
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
      for (uint32_t k = 0; k < kCtcG; ++k) cnt[k] += (acc[k >> 2] >> ((k & 3u) * 8u)) & 0xFFu;
    }
    unsigned long long member_best = 0;                       // tree: the best key this lane has for best[cv]
#pragma unroll
    for (uint32_t k = 0; k < kCtcG; ++k) {
      const uint32_t m = cnt[k], T = s_T[k];
      if (m == 0 || T == 0 || place >= tile.first + k) continue;   // (a pair is its higher end's to find)
      if (1000ull * m < uint64_t(p) * (uint64_t(T) + R - m)) continue;   // the floor, exactly
      mine += counting;
      // the height, floor(1000 m / (T + R - m)): m, T, R <= kNumCodes, so 32 bits hold it exactly
      const uint32_t h = (1000u * m) / (T + R - m);
      const uint32_t core_q = s_core[k];
      if constexpr (kTree) {
        if (s_comp[k] == cv) continue;                        // inside a component: no edge of the forest any more
        const unsigned long long H = min(h, min(core_q, core_v));
        const uint32_t q = s_num[k];
        const uint32_t e_lo = min(q, v), e_hi = max(q, v);
        const unsigned long long key = H << 54 | static_cast<unsigned long long>(~e_lo & kTreeNumberMask) << kTreeNumberBits |
                                       (~e_hi & kTreeNumberMask);
        member_best = max(member_best, key);
        // (the relaxed load spares the atomic when the word already holds as much, as best_raise's does)
        if (__hip_atomic_load(&s_best[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < key)
          (void)__hip_atomic_fetch_max(&s_best[k], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else {
        // (h - core wraps far above span for a height under the bracket; kNoCore would wrap to h + 1, hence the test.
        // A counter's index stays below kCoreBuckets: d < span and width = ceil(span / kCoreBuckets), checked at launch)
        const uint32_t dq = h - core_q, dv = h - core_v;
        if (core_q != kNoCore && dq < A.span)
          (void)__hip_atomic_fetch_add(&s_hist[k * kCoreBuckets + dq / A.width], 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
        if (core_v != kNoCore && dv < A.span)
          (void)__hip_atomic_fetch_add(A.hist + size_t(v) * kCoreBuckets + dv / A.width, 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (kTree && member_best) best_raise(A.best + cv, member_best);
  }
  if (mine) atomicAdd(&s_edges, mine);
  __syncthreads();
  if constexpr (kTree) {
    if (tid < kCtcG && s_best[tid]) best_raise(A.best + s_comp[tid], s_best[tid]);
    if (tid == 0 && s_edges) {
      atomicAdd(&A.totals->core_edges, static_cast<unsigned long long>(s_edges));
      if (A.count_edges) atomicAdd(&A.totals->t.edges, static_cast<unsigned long long>(s_edges));
    }
  } else {
    // one lane per non-zero word of the needles' histogram (a word's needle has T != 0, so its number is a node's)
    for (uint32_t i = tid; i < kCtcHistWords; i += kCtcThreads) {
      const uint32_t c = s_hist[i];
      if (c)
        (void)__hip_atomic_fetch_add(A.hist + size_t(s_num[i / kCoreBuckets]) * kCoreBuckets + (i % kCoreBuckets), c,
                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 0 && s_edges) atomicAdd(&A.totals->t.edges, static_cast<unsigned long long>(s_edges));
  }
}

template <bool kTree>
__global__ __launch_bounds__(kCluThreads) void cluster_core_tree_within_sweep_kernel(const ClusterCoreTreeWithinSweepArgs A) {
  const ClusterSweepArgs& a = A.s;
  __shared__ __attribute__((aligned(8))) uint32_t cnt[kCluWords];   // (two of its words end as one 64-bit key)
  __shared__ uint32_t left[(kNumCodes + 31) / 32];            // codes left out of this window's count
  __shared__ uint32_t d_len[kCluMaxDense], d_at[kCluMaxDense], d_code[kCluMaxDense], leave_at[kCluMaxDense];
  __shared__ uint32_t s_nd, s_any;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tasks = (a.n_windows + a.per - 1u) / a.per;
  const uint32_t qi = blockIdx.x / tasks, wr = blockIdx.x % tasks;
  if (qi >= a.n) return;
  const uint32_t q = A.needles[a.q_base + qi];                // (a number of a swept block)
  if (q >= a.n_nodes) return;
  const uint32_t T = a.q_ntri[q];
  if (T == 0) return;                                         // (the map does not hold it: no node)
  const uint32_t core_q = A.core[q];                          // frozen for the launch
  if (kTree && core_q == kNoCore) return;                     // no edge of the needle's is in the tree
  const uint32_t qblock = A.block_of[q];
  const uint2 qloc = a.loc[q];
  if (qloc.x < a.win0) return;                                // (this image lies behind the needle's)
  const uint64_t qpos = uint64_t(qloc.x) * kWindowRanks + qloc.y;
  // the windows in front of the needle's position: up to its own, of which the ranks below its own count
  const uint32_t w_begin = wr * a.per, w_end = min(min(a.n_windows, (wr + 1u) * a.per), qloc.x - a.win0 + 1u);
  if (w_begin >= w_end) return;
  uint32_t cq = 0;                                            // the needle's component: frozen for the launch
  bool counting;                                              // (the edges are counted once)
  if constexpr (kTree) {
    cq = A.comp[q];
    counting = A.round == 1u;
    if (!counting && A.closed[cq]) return;                    // no edge leaves it: none of the needle's can
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
          if (A.block_of[other] != qblock) continue;          // another block's: no edge
          // the height, floor(1000 m / (T + R - m)): m, T, R <= kNumCodes, so 32 bits hold it exactly
          const uint32_t h = (1000u * m) / (T + R - m);
          const uint32_t core_o = A.core[other];
          if constexpr (kTree) {
            if (core_o == kNoCore) continue;                  // not an edge of the tree
            mine += counting;
            const uint32_t co = A.comp[other];
            if (co == cq) continue;                           // inside a component: no edge of the forest any more
            const unsigned long long H = min(h, min(core_q, core_o));
            const uint32_t e_lo = min(q, other), e_hi = max(q, other);
            const unsigned long long key = H << 54 | static_cast<unsigned long long>(~e_lo & kTreeNumberMask) << kTreeNumberBits |
                                           (~e_hi & kTreeNumberMask);
            mine_best = max(mine_best, key);
            best_raise(A.best + co, key);
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
      if (*s_best) best_raise(A.best + cq, *s_best);
    } else {
      if (cnt[0]) atomicAdd(&A.totals->t.edges, static_cast<unsigned long long>(cnt[0]));
    }
  }
}

// (what keeps a counter's index inside a number's kCoreBuckets: (span - 1) / width < kCoreBuckets)
bool brackets_fit(uint32_t span, uint32_t width) {
  return span != 0 && span <= 1001u && width == (span + kCoreBuckets - 1u) / kCoreBuckets;
}

}  // namespace

int launch_cluster_core_tree_within(const ClusterCoreTreeWithinArgs& a, bool tree, hipStream_t stream) {
  if (a.w.n_tiles == 0) return 0;
  if (a.w.n_tiles > 0x7FFFFFFFu || a.w.n_nodes > kTreeMaxNodes || (tree ? a.round == 0 : !brackets_fit(a.span, a.width))) {
    errno = EINVAL;
    return -1;
  }
  if (tree) {
    note_each_launch("cluster_core_tree_within_kernel<tree>");
    hipLaunchKernelGGL(cluster_core_tree_within_kernel<true>, dim3(a.w.n_tiles), dim3(kCtcThreads), 0, stream, a);
  } else {
    note_each_launch("cluster_core_tree_within_kernel<height>");
    hipLaunchKernelGGL(cluster_core_tree_within_kernel<false>, dim3(a.w.n_tiles), dim3(kCtcThreads), 0, stream, a);
  }
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_core_tree_within_sweep(const ClusterCoreTreeWithinSweepArgs& a, bool tree, hipStream_t stream) {
  const ClusterSweepArgs& s = a.s;
  if (s.n == 0 || s.n_windows == 0) return 0;
  const uint64_t grid = uint64_t(s.n) * ((s.n_windows + s.per - 1u) / s.per);
  if (grid > 0x7FFFFFFFull || s.n_nodes > kTreeMaxNodes || (tree ? a.round == 0 : !brackets_fit(a.span, a.width))) {
    errno = EINVAL;
    return -1;
  }
  if (tree) {
    note_each_launch("cluster_core_tree_within_sweep_kernel<tree>");
    hipLaunchKernelGGL(cluster_core_tree_within_sweep_kernel<true>, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  } else {
    note_each_launch("cluster_core_tree_within_sweep_kernel<height>");
    hipLaunchKernelGGL(cluster_core_tree_within_sweep_kernel<false>, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  }
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
