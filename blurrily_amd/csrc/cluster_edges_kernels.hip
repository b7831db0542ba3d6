// cluster_edges_kernels.hip -- the kernels of blurrily_storage_cluster_edges and blurrily_storage_cluster_edges_within
// (launch code: cluster_edges.hip): the similarity graph's edges themselves, each once, as sorted
// records.
//
// cluster_edges_sweep_kernel: cluster_sweep_kernel's sweep (cluster_kernels.hip: a window's postings counted into LDS,
// bytes or 16-bit halves; the floor's bars t and [rlo, rhi]; windows passed over by win_min_tri / win_max_tri; the
// t - 1 largest dense slices left out and asked through their bitmaps; a needle's windows shared among workgroups; only
// positions in front of the needle's own) with another ending: a candidate that passes the exact floor test and is a
// node is not united with anything -- its key (cluster.h) is appended.  With a needle list and block_of[] it is
// cluster_within_sweep_kernel's sweep: the needles are the swept blocks' numbers, and a candidate under another key is
// passed over before the edge is counted.  The body is a copy, as the other entries' are, so that their device code
// stays as it was.
//
// cluster_edges_within_kernel: cluster_within_kernel's direct form (cluster_within_kernels.hip: one workgroup per tile of
// up to kClusterWithinTile places of one block, the tile's needles TRANSPOSED in LDS, the hull of the needles' R bars, a
// member a lane, byte counters emptied every 255 codes, an edge found from its end at the higher place only) with the
// same ending.
//
// The append.  One 64-bit cursor per call, in device memory, shared by every launch of the call.  A wave reserves room
// for all its lanes' edges at once: an inclusive prefix sum of the lanes' edge counts through __shfl_up, ONE agent-scope
// relaxed fetch_add of the wave's total by lane 0, the base handed round by __shfl; lane l's keys go to base + (the
// edges of the lanes below l) + j.  A key is stored only when its slot lies below ClusterEdgesOut::room; the cursor
// counts on regardless, so after the last launch it holds the edge count in every mode, also when nothing is stored,
// and nothing else counts: the count cannot disagree with what was written.  Slots are handed out once each, so no
// two stores meet, and the keys are read a launch later (the sort, or the rows kernel): nothing here needs an order.
// The cross-lane steps need every lane of the wave: the loops they stand in -- the harvest over the counters, the
// direct kernel's walk over the members -- have the SAME trip count in every lane (a multiple of the workgroup's
// threads; kCluWords is one already) and predicate their bodies instead of leaving early, every `continue` and `return`
// in front of them is uniform across the workgroup, and a wave in which no lane found an edge skips the reservation on
// a ballot all 64 lanes take.  The order in which waves reserve is not reproducible; the sort makes the bytes so.
//
// cluster_edges_tiles_kernel: above_tiles_kernel's bitonic sort of a tile in LDS, on this key.  The merge passes are
// segsort.h's seg_merge_kernel.  cluster_edges_rows_kernel: key i to record i.
#include "cluster.h"
#include "cluster_forest.h"
#include "find_kernels.h"
#include "hip_try.h"
#include "map_internal.h"

namespace blurrily {

namespace {

// (every launch of a call is named, as cluster_tree_kernels.hip names its own: a sweep per image can be counted)
void note_each_launch(const char* kernel_name) {
  std::string* s = detail::launch_names();
  if (!s) return;
  if (!s->empty()) *s += '+';
  *s += kernel_name;
}

// the height, floor(1000 m / (T + R - m)): m, T, R <= kNumCodes, so 32 bits hold it exactly
__device__ __forceinline__ unsigned long long edge_key(uint32_t m, uint32_t T, uint32_t R, uint32_t u, uint32_t v) {
  const unsigned long long down = 1000u - (1000u * m) / (T + R - m);
  return down << 54 | static_cast<unsigned long long>(min(u, v) & kTreeNumberMask) << kTreeNumberBits |
         (max(u, v) & kTreeNumberMask);
}

// Room for `mine` keys of this lane among its wave's: the first slot.  EVERY lane of the wave calls it.
__device__ __forceinline__ unsigned long long edges_reserve(const ClusterEdgesOut& o, uint32_t lane, uint32_t mine) {
  uint32_t incl = mine;
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t below = __shfl_up(incl, d);
    if (lane >= d) incl += below;
  }
  const uint32_t total = __shfl(incl, 63);
  unsigned long long base = 0;
  if (lane == 0)
    base = __hip_atomic_fetch_add(o.cursor, static_cast<unsigned long long>(total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  base = __shfl(base, 0);
  return base + (incl - mine);
}

static_assert(kCluWords % kCluThreads == 0, "the harvest takes every lane through the same number of counter words");
static_assert(kCluThreads % 64 == 0, "whole waves");

__global__ __launch_bounds__(kCluThreads) void cluster_edges_sweep_kernel(const ClusterEdgesSweepArgs A) {
  const ClusterSweepArgs& a = A.s;
  __shared__ uint32_t cnt[kCluWords];
  __shared__ uint32_t left[(kNumCodes + 31) / 32];            // codes left out of this window's count
  __shared__ uint32_t d_len[kCluMaxDense], d_at[kCluMaxDense], d_code[kCluMaxDense], leave_at[kCluMaxDense];
  __shared__ uint32_t s_nd, s_any;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tasks = (a.n_windows + a.per - 1u) / a.per;
  const uint32_t qi = blockIdx.x / tasks, wr = blockIdx.x % tasks;
  if (qi >= a.n) return;
  const bool blocked = A.needles != nullptr;
  const uint32_t q = blocked ? A.needles[a.q_base + qi] : a.q_base + qi;   // (a number of a swept block, or of the list)
  if (q >= a.n_nodes) return;
  const uint32_t T = a.q_ntri[q];
  if (T == 0) return;                                         // (the map does not hold it: no node)
  const uint32_t qblock = blocked ? A.block_of[q] : 0u;
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
  __syncthreads();

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
      // the harvest: the same trips in every lane, so that the reservation below meets whole waves
      for (uint32_t w0 = 0; w0 < kCluWords; w0 += kCluThreads) {
        const uint32_t wi = w0 + tid;
        const uint32_t x = cnt[wi];
        unsigned long long found[4];                          // this word's edges, by counter (statically indexed)
        uint32_t hits = 0;                                    // bit s: counter s of the word is an edge
        if (x) {
          cnt[wi] = 0;
#pragma unroll
          for (uint32_t s = 0; s < 4u; ++s) {
            found[s] = 0;
            if (s >= per_word) continue;
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
            if (other == kNoNode || other >= a.n_nodes) continue;   // held but not listed (or deleted): no node, no bridge
            if (blocked && A.block_of[other] != qblock) continue;   // another block's: no edge
            found[s] = edge_key(m, T, R, q, other);
            hits |= 1u << s;
          }
        }
        if (__ballot(hits != 0u) == 0ull) continue;           // (uniform across the wave: no lane of it has an edge)
        const unsigned long long at = edges_reserve(A.out, lane, __popc(hits));
#pragma unroll
        for (uint32_t s = 0; s < 4u; ++s) {
          const unsigned long long slot = at + __popc(hits & ((1u << s) - 1u));
          if (((hits >> s) & 1u) && slot < A.out.room) A.out.keys[slot].k = found[s];
        }
      }
      __syncthreads();
    }
    if (tid < nd) atomicAnd(&left[d_code[tid] >> 5], ~(1u << (d_code[tid] & 31u)));   // (cleared for the next window)
  }
}

constexpr uint32_t kCeThreads    = 256;
constexpr uint32_t kCeG          = kClusterWithinTile;
constexpr uint32_t kCeImageWords = (kNumCodes + 1) / 2;       // a 16-bit word per code, two to a word
static_assert(kCeG == 16, "a code's word of the transposed image has a bit per needle of the tile");
static_assert(kCeThreads == 16 * kCeG, "the image is filled by 16 lanes per needle");
static_assert(kCeThreads % 64 == 0, "whole waves");

__global__ __launch_bounds__(kCeThreads) void cluster_edges_within_kernel(const ClusterEdgesWithinArgs A) {
  const ClusterWithinArgs& a = A.w;
  __shared__ uint32_t img[kCeImageWords];
  __shared__ uint32_t s_num[kCeG], s_T[kCeG];
  __shared__ uint32_t s_lo, s_hi;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  if (blockIdx.x >= a.n_tiles) return;
  const ClusterWithinTile tile = a.tiles[blockIdx.x];
  if (tile.count == 0 || tile.count > kCeG || tile.first < tile.begin || tile.first > a.n_order ||
      tile.count > a.n_order - tile.first)
    return;                                                   // (uniform: no such tile is planned)
  const uint32_t p = a.min_permille;
  for (uint32_t i = tid; i < kCeImageWords; i += kCeThreads) img[i] = 0;
  if (tid < kCeG) {
    uint32_t u = kNoNode, T = 0;
    if (tid < tile.count) {
      u = a.order[tile.first + tid];
      T = u < a.n_nodes ? a.q_ntri[u] : 0u;
    }
    s_num[tid] = u;
    s_T[tid] = T;
  }
  if (tid == 0) { s_lo = 0xFFFFFFFFu; s_hi = 0; }
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

  // the members in front of the tile's last place (that place itself is in front of no needle of the tile), the same
  // trips in every lane, so that the reservation below meets whole waves
  const uint32_t end = tile.first + tile.count - 1u;
  for (uint32_t place0 = tile.begin; place0 < end; place0 += kCeThreads) {
    const uint32_t place = place0 + tid;
    uint32_t cnt[kCeG];
#pragma unroll
    for (uint32_t k = 0; k < kCeG; ++k) cnt[k] = 0;
    uint32_t v = kNoNode, R = 0;
    if (place < end) {
      v = a.order[place];
      R = v < a.n_nodes ? a.q_ntri[v] : 0u;
      if (R < lo || R > hi) R = 0;                            // no node, or no needle's floor allows this R
    }
    if (R) {
      const uint16_t* mc = a.qcodes + a.qoff[v] + uint64_t(v);
      for (uint32_t c0 = 0; c0 < R; c0 += 255u) {             // (a byte counts 255 codes at most)
        const uint32_t c1 = min(R, c0 + 255u);
        uint32_t acc[4] = {0, 0, 0, 0};
        for (uint32_t j = c0; j < c1; ++j) {
          const uint32_t c = mc[j];
          if (c >= kNumCodes) continue;
          const uint32_t bits = (img[c >> 1] >> ((c & 1u) * 16u)) & 0xFFFFu;
          if (!bits) continue;
#pragma unroll
          for (uint32_t w = 0; w < 4; ++w)                     // bits 4 w .. 4 w + 3 to the low bit of a byte each
            acc[w] += (((bits >> (4u * w)) & 0xFu) * 0x00204081u) & 0x01010101u;
        }
#pragma unroll
        for (uint32_t k = 0; k < kCeG; ++k) cnt[k] += (acc[k >> 2] >> ((k & 3u) * 8u)) & 0xFFu;
      }
    }
    uint32_t hits = 0;                                        // bit k: the member and needle k of the tile share an edge
    if (R) {
#pragma unroll
      for (uint32_t k = 0; k < kCeG; ++k) {
        const uint32_t m = cnt[k], T = s_T[k];
        if (m == 0 || T == 0 || place >= tile.first + k) continue;   // (an edge is its higher end's to find)
        if (1000ull * m < uint64_t(p) * (uint64_t(T) + R - m)) continue;   // the floor, exactly
        hits |= 1u << k;
      }
    }
    if (__ballot(hits != 0u) == 0ull) continue;               // (uniform across the wave: no lane of it has an edge)
    const unsigned long long at = edges_reserve(A.out, lane, __popc(hits));
#pragma unroll
    for (uint32_t k = 0; k < kCeG; ++k) {
      const unsigned long long slot = at + __popc(hits & ((1u << k) - 1u));
      if (((hits >> k) & 1u) && slot < A.out.room) A.out.keys[slot].k = edge_key(cnt[k], s_T[k], R, s_num[k], v);
    }
  }
}

// one tile per workgroup: bitonic sort over the next power of two at or above its length, padded with ~0 (no key:
// a key's top ten bits are at most 1000)
__global__ __launch_bounds__(256) void cluster_edges_tiles_kernel(const SegTile* tiles, const ClusterEdgeKey* in,
                                                                  ClusterEdgeKey* out) {
  __shared__ unsigned long long s[kClusterEdgesTile];
  const SegTile tl = tiles[blockIdx.x];
  if (tl.len > kClusterEdgesTile) return;                     // (uniform: no such tile is cut)
  uint32_t P = 1;
  while (P < tl.len) P <<= 1;
  for (uint32_t i = threadIdx.x; i < P; i += 256u) s[i] = i < tl.len ? in[size_t(tl.start) + i].k : ~0ull;
  __syncthreads();
  for (uint32_t k = 2; k <= P; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < P; i += 256u) {
        const uint32_t x = i ^ j;
        if (x > i) {
          const unsigned long long a = s[i], b = s[x];
          if ((a > b) == ((i & k) == 0)) { s[i] = b; s[x] = a; }
        }
      }
      __syncthreads();
    }
  for (uint32_t i = threadIdx.x; i < tl.len; i += 256u) out[size_t(tl.start) + i].k = s[i];
}

__global__ __launch_bounds__(256) void cluster_edges_rows_kernel(const ClusterEdgesRowsArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_keys) return;
  const unsigned long long key = a.keys[i].k;
  const uint32_t lo = uint32_t(key >> kTreeNumberBits) & kTreeNumberMask, hi = uint32_t(key) & kTreeNumberMask;
  a.rows[i] = ClusterTreeMerge{lo < a.n_nodes ? a.refs[lo] : kNoNode, hi < a.n_nodes ? a.refs[hi] : kNoNode,
                               1000u - uint32_t(key >> 54)};
}

}  // namespace

int launch_cluster_edges_sweep(const ClusterEdgesSweepArgs& a, hipStream_t stream) {
  const ClusterSweepArgs& s = a.s;
  if (s.n == 0 || s.n_windows == 0) return 0;
  const uint64_t grid = uint64_t(s.n) * ((s.n_windows + s.per - 1u) / s.per);
  if (grid > 0x7FFFFFFFull || s.n_nodes > kTreeMaxNodes || !a.out.cursor || (a.out.room && !a.out.keys) ||
      (a.needles && !a.block_of)) {
    errno = EINVAL;
    return -1;
  }
  note_each_launch("cluster_edges_sweep_kernel");
  hipLaunchKernelGGL(cluster_edges_sweep_kernel, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_edges_within(const ClusterEdgesWithinArgs& a, hipStream_t stream) {
  if (a.w.n_tiles == 0) return 0;
  if (a.w.n_tiles > 0x7FFFFFFFu || a.w.n_nodes > kTreeMaxNodes || !a.out.cursor || (a.out.room && !a.out.keys)) {
    errno = EINVAL;
    return -1;
  }
  note_each_launch("cluster_edges_within_kernel");
  hipLaunchKernelGGL(cluster_edges_within_kernel, dim3(a.w.n_tiles), dim3(kCeThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_edges_tiles(const SegTile* tiles, uint32_t n_tiles, const ClusterEdgeKey* in, ClusterEdgeKey* out,
                               hipStream_t stream) {
  if (n_tiles == 0) return 0;
  note_launch("cluster_edges_tiles_kernel");
  hipLaunchKernelGGL(cluster_edges_tiles_kernel, dim3(n_tiles), dim3(256), 0, stream, tiles, in, out);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_edges_merge(const SegMergeArgs<ClusterEdgeKey>& a, hipStream_t stream) {
  if (a.n_elems == 0) return 0;
  note_launch("cluster_edges_merge_kernel");
  hipLaunchKernelGGL(seg_merge_kernel<ClusterEdgeKey>, dim3((a.n_elems + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_edges_rows(const ClusterEdgesRowsArgs& a, hipStream_t stream) {
  if (a.n_keys == 0) return 0;
  note_launch("cluster_edges_rows_kernel");
  hipLaunchKernelGGL(cluster_edges_rows_kernel, dim3((a.n_keys + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
