// cluster_tree_extend_kernels.hip -- the kernels of blurrily_storage_cluster_tree_extend (launch
// code: cluster_tree_extend.hip): the cluster tree of old and new references together, from the records the caller
// holds for the old ones and sweeps of the new ones alone.  The candidate edges of the forest are of two kinds, the old
// records and the similarity edges with a new end, and a Boruvka round of cluster_tree_kernels.hip takes both: whoever
// offers an edge raises best[] of the two components it joins, and that file's merge and flatten do the rest as they
// are.
//
// cluster_tree_extend_resolve_kernel, once per call: one thread per old record.  Both references are looked up among
// the ascending refs[] by binary search, as cluster_extend_seed_kernel looks a label up, and the record's key (cluster.h)
// is written, or 0 for a record that is no candidate: an end not listed, not held or new, or a height below the floor.
// The height is the caller's; nothing is computed again.
// cluster_tree_extend_offer_kernel, every round after the sweeps and before the merge: one thread per old record.  A
// record whose ends lie in different components offers its key to best[] of both.
// cluster_tree_extend_sweep_kernel: cluster_tree_sweep_kernel's sweep (cluster_tree_kernels.hip) with
// cluster_extend_sweep_kernel's three differences (cluster_extend_kernels.hip): the needles are the new nodes, through
// the list of their numbers; a needle sweeps every window of both images; and a candidate that is the needle, or a new
// node at a higher position, is skipped -- in every round, so that an edge between two new nodes costs one pair of
// atomics and round 1's count names every edge with a new end once.  The body is a copy, as the others' are, so that
// the device code of the others stays as it was.
//
// The memory model is cluster_tree_kernels.hip's.  comp[] and closed[] are written by no thread while the sweeps and the
// offer run, and are read plainly; best[] is touched by both only through agent-scope relaxed 64-bit fetch_max behind
// the relaxed load that spares it, so the sweeps of a round and its offer need no order among themselves: the maximum of
// a set does not depend on who offered which element when.  The merge reads best[] a launch later.
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

// the number of `ref` among the ascending refs[0 .. n), or n
__device__ __forceinline__ uint32_t number_of(const uint32_t* refs, uint32_t n, uint32_t ref) {
  uint32_t lo = 0, hi = n;                                    // the first number whose reference is >= ref
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (refs[mid] < ref) lo = mid + 1u; else hi = mid;
  }
  return lo < n && refs[lo] == ref ? lo : n;
}

__global__ __launch_bounds__(256) void cluster_tree_extend_resolve_kernel(const ClusterTreeExtendRecordsArgs A) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_records) return;
  const ClusterTreeMerge rec = A.records[i];
  unsigned long long key = 0;
  if (rec.permille >= A.min_permille && rec.permille <= 1000u && rec.a < rec.b) {
    const uint32_t lo = number_of(A.refs, A.n_nodes, rec.a), hi = number_of(A.refs, A.n_nodes, rec.b);
    if (lo < A.n_nodes && hi < A.n_nodes && A.ntri[lo] != 0 && A.ntri[hi] != 0 &&
        !((A.is_new[lo >> 5] >> (lo & 31u)) & 1u) && !((A.is_new[hi >> 5] >> (hi & 31u)) & 1u))
      key = static_cast<unsigned long long>(rec.permille) << 54 |
            static_cast<unsigned long long>(~lo & kTreeNumberMask) << kTreeNumberBits | (~hi & kTreeNumberMask);
  }
  A.keys[i] = key;
}

__global__ __launch_bounds__(256) void cluster_tree_extend_offer_kernel(const ClusterTreeExtendRecordsArgs A) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_records) return;
  const unsigned long long key = A.keys[i];
  if (key == 0) return;                                       // no candidate
  const uint32_t lo = ~uint32_t(key >> kTreeNumberBits) & kTreeNumberMask, hi = ~uint32_t(key) & kTreeNumberMask;
  const uint32_t cl = A.comp[lo], ch = A.comp[hi];            // (the resolve saw both below n_nodes)
  if (cl == ch) return;                                       // inside a component: no edge of the forest any more
  best_raise(A.best + cl, key);
  best_raise(A.best + ch, key);
}

__global__ __launch_bounds__(kCluThreads) void cluster_tree_extend_sweep_kernel(const ClusterTreeExtendSweepArgs A) {
  const ClusterSweepArgs& a = A.t.s;
  __shared__ __attribute__((aligned(8))) uint32_t cnt[kCluWords];   // (two of its words end as one 64-bit key)
  __shared__ uint32_t left[(kNumCodes + 31) / 32];            // codes left out of this window's count
  __shared__ uint32_t d_len[kCluMaxDense], d_at[kCluMaxDense], d_code[kCluMaxDense], leave_at[kCluMaxDense];
  __shared__ uint32_t s_nd, s_any;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tasks = (a.n_windows + a.per - 1u) / a.per;
  const uint32_t qi = blockIdx.x / tasks, wr = blockIdx.x % tasks;
  if (qi >= a.n) return;
  const uint32_t q = A.new_nodes[a.q_base + qi];              // (a new node's number)
  const uint32_t T = a.q_ntri[q];
  if (T == 0) return;                                         // (the map does not hold it: no node)
  const uint2 qloc = a.loc[q];
  const uint64_t qpos = uint64_t(qloc.x) * kWindowRanks + qloc.y;
  // every window of the image, in front of the needle and behind it: an old node may lie anywhere
  const uint32_t w_begin = wr * a.per, w_end = min(a.n_windows, (wr + 1u) * a.per);
  if (w_begin >= w_end) return;
  const uint32_t cq = A.t.comp[q];                            // the needle's component: frozen for the launch
  const bool counting = A.t.round == 1u;                      // (the edges with a new end are counted once)
  if (!counting && A.t.closed[cq]) return;                    // no edge leaves it: none of the needle's can
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
          // an old node is no needle: the edge is this end's to find.  Between two new nodes it is the higher end's.
          if (pos0 + r > qpos && ((A.is_new[other >> 5] >> (other & 31u)) & 1u)) continue;
          mine += counting;
          const uint32_t co = A.t.comp[other];
          if (co == cq) continue;                             // inside a component: no edge of the forest any more
          // the height, floor(1000 m / (T + R - m)): m, T, R <= kNumCodes, so 32 bits hold it exactly
          const unsigned long long h = (1000u * m) / (T + R - m);
          const uint32_t e_lo = min(q, other), e_hi = max(q, other);
          const unsigned long long key = h << 54 | static_cast<unsigned long long>(~e_lo & kTreeNumberMask) << kTreeNumberBits |
                                         (~e_hi & kTreeNumberMask);
          mine_best = max(mine_best, key);
          best_raise(A.t.best + co, key);
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
    if (*s_best) best_raise(A.t.best + cq, *s_best);
  }
}

}  // namespace

int launch_cluster_tree_extend_sweep(const ClusterTreeExtendSweepArgs& a, hipStream_t stream) {
  const ClusterSweepArgs& s = a.t.s;
  if (s.n == 0 || s.n_windows == 0) return 0;
  const uint64_t grid = uint64_t(s.n) * ((s.n_windows + s.per - 1u) / s.per);
  if (grid > 0x7FFFFFFFull || s.n_nodes > kTreeMaxNodes || a.t.round == 0) { errno = EINVAL; return -1; }
  note_each_launch("cluster_tree_extend_sweep_kernel");
  hipLaunchKernelGGL(cluster_tree_extend_sweep_kernel, dim3(uint32_t(grid)), dim3(kCluThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_tree_extend_resolve(const ClusterTreeExtendRecordsArgs& a, hipStream_t stream) {
  if (a.n_records == 0) return 0;
  note_each_launch("cluster_tree_extend_resolve_kernel");
  hipLaunchKernelGGL(cluster_tree_extend_resolve_kernel, dim3((a.n_records + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_cluster_tree_extend_offer(const ClusterTreeExtendRecordsArgs& a, hipStream_t stream) {
  if (a.n_records == 0) return 0;
  note_each_launch("cluster_tree_extend_offer_kernel");
  hipLaunchKernelGGL(cluster_tree_extend_offer_kernel, dim3((a.n_records + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
