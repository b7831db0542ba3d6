// cluster_levels_kernels.hip -- the sweep of blurrily_storage_cluster_levels (launch code:
// cluster_levels.hip): one sweep at the lowest floor, one union-find forest per floor.
//
// cluster_levels_sweep_kernel is cluster_sweep_kernel's sweep (cluster_kernels.hip: the counters, the floor's bars t
// and [rlo, rhi], the windows passed over, the dense slices left out, each edge found from its end at the higher
// position) run with p = floors[0] -- an edge at a higher floor is an edge at every lower one, so this sweep meets
// every level's edges, each with its exact m, T and R in registers -- and with another ending: a rank that passes
// floor 0's exact test and is a node gets its level lv, the number of floors k with 1000 m >= floors[k] (T + R - m),
// is counted for levels 0 .. lv - 1 and united with the needle's node in forests 0 .. lv - 1.  The body is a copy of
// cluster_sweep_kernel's, as that one is of similar_sweep_kernel's all mode, so that the device code of both stays
// as it was.  The node tables and the labels are cluster_kernels.hip's kernels, launched once per level.
//
// Per-level state lives in registers: the needle's last known root and a count per level, in arrays of
// kClusterMaxLevels words that only unrolled loops index, the walk down the forests included, so that nothing goes
// to scratch.  The counts are a histogram over lv; the workgroup's sum of it is taken from each level upwards
// at the end, in the first words of the LDS counters, which every harvest leaves zero.
//
// Each forest by itself is cluster_kernels.hip's forest, and that file's argument applies to it unchanged: inside
// the sweep every access to a parent word is an agent-scope relaxed atomic (cluster_forest.h), hooks put the higher
// number under the lower, path halving stores by atomic min, and a step budget sets the error word when it runs out.
//
// The unions go from the top level down and stop early: a lane with an edge of level lv unites its ends in forest
// lv - 1 first, then lv - 2, ..., and stops at the first forest in which it finds both ends under one root already.
// That the forests below then hold the ends together too, once the sweeps are done:
//   * a hook in forest k is only ever made by a lane whose edge passed floor k;
//   * a lane that has hooked in forest k goes on to forest k - 1, where it unites the same ends or finds them
//     together -- so when its launch ends, the ends of every edge behind a hook of forest k are connected in forest
//     k - 1;
//   * two nodes under one root in forest k are joined by a path of such hooked edges, hence connected in forest
//     k - 1 when the launches that made the hooks have ended; by induction downwards, in every forest below k.
// So "one root in forest k" lets the lane leave forests k - 1 .. 0 to the lanes that built that path (or to those
// that built theirs), and the label kernel, which runs only after the last sweep, sees every forest complete.  A
// lane whose budget runs out stops too, and the call fails.  The early stop does not touch the edge counts: they come
// from lv alone.  BLURRILY_LEVELS_EARLY_STOP=0 builds the plain form (every forest 0 .. lv - 1 visited), which
// DESIGN.md section 18 measures against.
#include "cluster.h"
#include "cluster_forest.h"
#include "find_kernels.h"
#include "hip_try.h"

#ifndef BLURRILY_LEVELS_EARLY_STOP
#define BLURRILY_LEVELS_EARLY_STOP 1
#endif

namespace blurrily {

namespace {

__global__ __launch_bounds__(kCluThreads) void cluster_levels_sweep_kernel(const ClusterLevelsSweepArgs A) {
  const ClusterSweepArgs& a = A.s;
  __shared__ uint32_t cnt[kCluWords];
  __shared__ uint32_t left[(kNumCodes + 31) / 32];            // codes left out of this window's count
  __shared__ uint32_t d_len[kCluMaxDense], d_at[kCluMaxDense], d_code[kCluMaxDense], leave_at[kCluMaxDense];
  __shared__ uint32_t s_nd, s_any, s_err;
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
  const uint32_t p = A.floors[0];                             // the sweep is the lowest floor's: it meets every level's edges
  const uint16_t* codes = a.qcodes + a.qoff[q] + uint64_t(q);
  const bool wide = T > 255u;                                 // byte counters hold at most 255 matches
  // the floor's bars: m >= ceil(p T / 1000), ceil(p T / 1000) <= R <= floor(1000 T / p)
  const uint32_t t = max(1u, uint32_t((uint64_t(p) * T + 999u) / 1000u));
  const uint32_t rlo = t;
  const uint32_t rhi = p ? uint32_t(min<uint64_t>(1000ull * T / p, 0xFFFFFFFFull)) : 0xFFFFFFFFu;
  for (uint32_t i = tid; i < kCluWords; i += kCluThreads) cnt[i] = 0;
  for (uint32_t i = tid; i < (kNumCodes + 31) / 32; i += kCluThreads) left[i] = 0;
  if (tid == 0) s_err = 0;
  __syncthreads();

  uint32_t root[kClusterMaxLevels];                           // the needle's root in each forest as far as this lane knows
  uint32_t hist[kClusterMaxLevels];                           // edges this lane found, by level: hist[k] of them have lv == k + 1
#pragma unroll
  for (uint32_t k = 0; k < kClusterMaxLevels; ++k) { root[k] = q; hist[k] = 0; }
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
          // the edge's level: the floors it passes are a prefix, the floors ascending
          uint32_t lv = 1;
#pragma unroll
          for (uint32_t k = 1; k < kClusterMaxLevels; ++k)
            lv += k < A.n_floors && 1000ull * m >= uint64_t(A.floors[k]) * (uint64_t(T) + R - m);
#pragma unroll
          for (uint32_t k = 0; k < kClusterMaxLevels; ++k) hist[k] += lv == k + 1u;
          bool go = ok;                                       // forests lv - 1 down to 0
#pragma unroll
          for (uint32_t i = 0; i < kClusterMaxLevels; ++i) {
            const uint32_t k = kClusterMaxLevels - 1u - i;
            if (!go || k >= lv) continue;
            uint64_t budget = 4ull * a.n_nodes + 64u;
            bool hooked;
            ok = pf_unite(a.parent + size_t(k) * a.n_nodes, &root[k], other, &budget, &hooked);
            go = ok && (hooked || !BLURRILY_LEVELS_EARLY_STOP);   // (together here: together in every forest below, see above)
          }
        }
      }
      __syncthreads();
    }
    if (tid < nd) atomicAnd(&left[d_code[tid] >> 5], ~(1u << (d_code[tid] & 31u)));   // (cleared for the next window)
  }
  // the workgroup's histogram in the first words of the counters (every harvest leaves them zero), summed from each
  // level upwards: an edge of level lv counts for levels 0 .. lv - 1
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < kClusterMaxLevels; ++k)
    if (hist[k]) atomicAdd(&cnt[k], hist[k]);
  if (!ok) s_err = 1;
  __syncthreads();
  if (tid < A.n_floors) {
    uint32_t edges = 0;
    for (uint32_t k = tid; k < kClusterMaxLevels; ++k) edges += cnt[k];
    if (edges) atomicAdd(&a.totals[tid].edges, static_cast<unsigned long long>(edges));
  }
  if (tid == 0 && s_err) atomicOr(&a.totals[0].error, 1u);
}

}  // namespace

int launch_cluster_levels_sweep(const ClusterLevelsSweepArgs& a, hipStream_t stream) {
  if (a.s.n == 0 || a.s.n_windows == 0) return 0;
  const uint64_t grid = uint64_t(a.s.n) * ((a.s.n_windows + a.s.per - 1u) / a.s.per);
  if (grid > 0x7FFFFFFFull || a.n_floors == 0 || a.n_floors > kClusterMaxLevels) { errno = EINVAL; return -1; }
  note_launch("cluster_levels_sweep_kernel");
  hipLaunchKernelGGL(cluster_levels_sweep_kernel, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
