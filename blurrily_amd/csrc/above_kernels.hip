// above_kernels.hip -- the threshold find's kernels (launch code: above.hip).
//
// above_sweep_kernel: one workgroup per (needle, run of windows).  The bar t is known before the first window, so a
// window whose win_max_tri is below it is passed over, and up to t - 1 of the needle's dense slices -- the largest --
// are left out of the count (a rank with t matches has at least one hit among the counted slices: prefix filtering).
// The counted slices are added into the window's counters in LDS (bytes; 16 bits over two half windows when the
// needle has more than 255 distinct trigrams); a rank with at least t - L counted matches asks the left-out slices'
// bitmaps about itself, and is a row when its total reaches t and it is not deleted.  The same launch counts a
// needle's rows (count pass) or writes its keys (emit pass, into the segment the count pass sized).
// Each needle's keys are then sorted (above_tiles_kernel: bitonic sort of up to kAboveTile keys in LDS;
// segsort.h's seg_merge_kernel: merge passes over the few segments longer than a tile), and above_rows_kernel merges the base
// and delta images' rows per needle.
#include "above.h"
#include "find_kernels.h"
#include "hip_try.h"

namespace blurrily {

namespace {

constexpr uint32_t kAboveThreads  = 512;
constexpr uint32_t kAboveWaves    = kAboveThreads / 64;
constexpr uint32_t kAboveWords    = kWindowSize / 4;          // 64 KiB of counters: a window in bytes, half a window in 16 bits
constexpr uint32_t kAboveMaxDense = 64;                       // dense slices of a (needle, window) that may be left out

__global__ __launch_bounds__(kAboveThreads) void above_sweep_kernel(AboveArgs a) {
  __shared__ uint32_t cnt[kAboveWords];
  __shared__ uint32_t left[(kNumCodes + 31) / 32];            // codes left out of this window's count
  __shared__ uint32_t d_len[kAboveMaxDense], d_at[kAboveMaxDense], d_code[kAboveMaxDense], leave_at[kAboveMaxDense];
  __shared__ uint32_t s_nd, s_any, s_rows;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tasks = (a.n_windows + a.per - 1u) / a.per;
  const uint32_t q = blockIdx.x / tasks, wr = blockIdx.x % tasks;
  if (q >= a.n) return;
  const uint32_t T = a.q_ntri[q];
  const uint32_t t = above_bar(T, a.min_matches, a.min_permille);
  if (T == 0 || t > T) return;
  const uint16_t* codes = a.qcodes + a.qoff[q] + (uint64_t(a.q_base) + q);
  const bool wide = T > 255u;                                 // byte counters hold at most 255 matches
  const bool emit = a.keys != nullptr;
  const uint32_t w_end = min(a.n_windows, (wr + 1u) * a.per);
  for (uint32_t i = tid; i < kAboveWords; i += kAboveThreads) cnt[i] = 0;
  for (uint32_t i = tid; i < (kNumCodes + 31) / 32; i += kAboveThreads) left[i] = 0;
  if (tid == 0) s_rows = 0;
  uint32_t seg = 0, cap = 0;
  if (emit) { seg = a.seg[q]; cap = a.counts[q]; }

  for (uint32_t w = wr * a.per; w < w_end; ++w) {
    if (a.win_max_tri[w] < t) continue;                       // no reference of the window has t trigrams
    __syncthreads();                                          // (the previous window is done with the lists)
    if (tid == 0) { s_nd = 0; s_any = 0; }
    __syncthreads();
    const uint2* se_w = a.slice_se + size_t(w) * kNumCodes;
    if (a.dense_min8 && t > 1u) {
      for (uint32_t i = tid; i < T; i += kAboveThreads) {
        const uint2 se = se_w[codes[i]];
        if (se.y - se.x >= a.dense_min8) {
          const uint32_t k = atomicAdd(&s_nd, 1u);
          if (k < kAboveMaxDense) { d_len[k] = se.y - se.x; d_at[k] = se.x; d_code[k] = codes[i]; }
        }
      }
      __syncthreads();
    }
    const uint32_t nd = min(s_nd, kAboveMaxDense);
    const uint32_t L = min(t - 1u, nd);
    // the L largest dense slices (lower code first among equal lengths) are left out: a fixed choice, whatever the
    // order the list was filled in
    if (tid < nd) {
      uint32_t r = 0;
      for (uint32_t j = 0; j < nd; ++j)
        r += d_len[j] > d_len[tid] || (d_len[j] == d_len[tid] && d_code[j] < d_code[tid]);
      if (r < L) { leave_at[r] = d_at[tid]; atomicOr(&left[d_code[tid] >> 5], 1u << (d_code[tid] & 31u)); }
    }
    __syncthreads();
    const uint32_t hthr = max(1u, t - L);                     // counted matches a rank needs to be asked about

    for (uint32_t half = 0; half < (wide ? 2u : 1u); ++half) {
      const uint32_t lo = half * (kWindowSize / 2);
      // count: one slice per wave, 8 postings a lane per 16-byte load
      for (uint32_t i = wave; i < T; i += kAboveWaves) {
        const uint32_t code = codes[i];
        if ((left[code >> 5] >> (code & 31u)) & 1u) continue;
        const uint2 se = se_w[code];
        const uint32_t groups = (se.y - se.x) / 8u;
        if (groups == 0) continue;
        if (lane == 0) s_any = 1;
        const uint4* p = reinterpret_cast<const uint4*>(a.ent + se.x);
        for (uint32_t g = lane; g < groups; g += 64u) {
          const uint4 v = p[g];
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
      // scan: a thread reads words tid, tid + 512, ...; the rows of its words, counted first, then (emit) written
      const uint32_t per_word = wide ? 2u : 4u, bits = wide ? 16u : 8u, mask = wide ? 0xFFFFu : 0xFFu;
      auto row_of = [&](uint32_t x, uint32_t wi, uint32_t s, unsigned long long* key) -> bool {
        const uint32_t c = (x >> (s * bits)) & mask;
        if (c < hthr) return false;
        const uint32_t r = wide ? lo + wi * 2u + s : wi * 4u + s;
        if (r >= kWindowRanks) return false;
        const uint32_t g = w * kWindowRanks + r;
        if (g >= a.n_refs) return false;
        uint32_t total = c;
        for (uint32_t l = 0; l < L; ++l) {                   // (exact: the key carries the matches)
          const uint32_t* bm = reinterpret_cast<const uint32_t*>(a.ent + (leave_at[l] - kBitmapSlots));
          total += (bm[r >> 5] >> (r & 31u)) & 1u;
        }
        if (total < t) return false;
        if (a.tomb && ((a.tomb[g >> 5] >> (g & 31u)) & 1u)) return false;
        *key = (static_cast<unsigned long long>(T - total) << 32) | g;
        return true;
      };
      uint32_t mine = 0;
      unsigned long long key;
      for (uint32_t wi = tid; wi < kAboveWords; wi += kAboveThreads) {
        const uint32_t x = cnt[wi];
        if (!x) continue;
        for (uint32_t s = 0; s < per_word; ++s) mine += row_of(x, wi, s, &key);
        if (!emit) cnt[wi] = 0;
      }
      if (!emit) {
        if (mine) atomicAdd(&s_rows, mine);
      } else {
        // a wave's rows go to one run of the needle's segment: an inclusive scan over the lanes, one atomic a wave
        uint32_t incl = mine;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
          const uint32_t y = __shfl_up(incl, d, 64);
          if (lane >= d) incl += y;
        }
        const uint32_t wave_total = __shfl(incl, 63, 64);
        uint32_t base = 0;
        if (lane == 0 && wave_total) base = atomicAdd(&a.cursor[q], wave_total);
        base = __shfl(base, 0, 64);
        uint32_t at = base + incl - mine;
        for (uint32_t wi = tid; wi < kAboveWords; wi += kAboveThreads) {
          const uint32_t x = cnt[wi];
          if (!x) continue;
          for (uint32_t s = 0; s < per_word; ++s)
            if (row_of(x, wi, s, &key)) {
              if (at < cap) a.keys[size_t(seg) + at] = key;   // (the count pass found as many: never past the segment)
              ++at;
            }
          cnt[wi] = 0;
        }
      }
      __syncthreads();
    }
    if (tid < nd) atomicAnd(&left[d_code[tid] >> 5], ~(1u << (d_code[tid] & 31u)));   // (cleared for the next window)
  }
  __syncthreads();
  if (!emit && tid == 0 && s_rows) atomicAdd(&a.counts[q], s_rows);
}

// one tile per workgroup: bitonic sort over the next power of two at or above its length, padded with ~0
__global__ __launch_bounds__(256) void above_tiles_kernel(const SegTile* tiles, const unsigned long long* in,
                                                          unsigned long long* out) {
  __shared__ unsigned long long s[kAboveTile];
  const SegTile tl = tiles[blockIdx.x];
  uint32_t P = 1;
  while (P < tl.len) P <<= 1;
  for (uint32_t i = threadIdx.x; i < P; i += 256u) s[i] = i < tl.len ? in[size_t(tl.start) + i] : ~0ull;
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
  for (uint32_t i = threadIdx.x; i < tl.len; i += 256u) out[size_t(tl.start) + i] = s[i];
}

// result order of two rows: matches descending, weight ascending, reference ascending
__device__ inline bool above_before(uint32_t m1, uint32_t w1, uint32_t r1, uint32_t m2, uint32_t w2, uint32_t r2) {
  return m1 != m2 ? m1 > m2 : w1 != w2 ? w1 < w2 : r1 < r2;
}

__global__ __launch_bounds__(256) void above_rows_kernel(AboveRowsArgs a) {
  const uint64_t k0 = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const uint32_t img = k0 < a.n_keys[0] ? 0u : 1u;
  if (img >= a.n_img || k0 >= uint64_t(a.n_keys[0]) + (a.n_img > 1 ? a.n_keys[1] : 0u)) return;
  const uint32_t k = uint32_t(img ? k0 - a.n_keys[0] : k0);
  const uint32_t* off = a.off[img];
  uint32_t lo = 0, hi = a.n;                                  // the needle: the last q with off[q] <= k
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) / 2u;
    if (off[mid] <= k) lo = mid; else hi = mid;
  }
  const uint32_t q = lo, T = a.q_ntri[q];
  const unsigned long long key = a.keys[img][k];
  const uint32_t rank = uint32_t(key), m = T - uint32_t(key >> 32);
  const uint32_t ref = a.ref_of_rank[img][rank], wgt = a.weight_of_rank[img][rank];
  uint32_t before = 0;                                        // rows of the other image in front of this one
  if (a.n_img > 1) {
    const uint32_t o = img ^ 1u;
    uint32_t b = a.off[o][q], e = a.off[o][q + 1];
    const uint32_t first = b;
    while (b < e) {
      const uint32_t mid = (b + e) / 2u;
      const unsigned long long ok = a.keys[o][mid];
      const uint32_t orank = uint32_t(ok), om = T - uint32_t(ok >> 32);
      if (above_before(om, a.weight_of_rank[o][orank], a.ref_of_rank[o][orank], m, wgt, ref)) b = mid + 1u; else e = mid;
    }
    before = b - first;
  }
  const uint64_t at = uint64_t(a.off[0][q]) + (a.n_img > 1 ? a.off[1][q] : 0u) + (k - off[q]) + before;
  a.rows[at] = trigram_match_t{ref, m, wgt};
}

}  // namespace

int launch_above_sweep(const AboveArgs& a, hipStream_t stream) {
  if (a.n == 0 || a.n_windows == 0) return 0;
  const uint64_t grid = uint64_t(a.n) * ((a.n_windows + a.per - 1u) / a.per);
  if (grid > 0x7FFFFFFFull) { errno = EINVAL; return -1; }
  note_launch("above_sweep_kernel");
  hipLaunchKernelGGL(above_sweep_kernel, dim3(uint32_t(grid)), dim3(kAboveThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_above_tiles(const SegTile* tiles, uint32_t n_tiles, const unsigned long long* in, unsigned long long* out,
                       hipStream_t stream) {
  if (n_tiles == 0) return 0;
  note_launch("above_tiles_kernel");
  hipLaunchKernelGGL(above_tiles_kernel, dim3(n_tiles), dim3(256), 0, stream, tiles, in, out);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_above_merge(const SegMergeArgs<unsigned long long>& a, hipStream_t stream) {
  if (a.n_elems == 0) return 0;
  note_launch("above_merge_kernel");
  hipLaunchKernelGGL(seg_merge_kernel<unsigned long long>, dim3((a.n_elems + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_above_rows(const AboveRowsArgs& a, hipStream_t stream) {
  const uint64_t n_keys = uint64_t(a.n_keys[0]) + (a.n_img > 1 ? a.n_keys[1] : 0u);
  if (n_keys == 0) return 0;
  note_launch("above_rows_kernel");
  hipLaunchKernelGGL(above_rows_kernel, dim3(uint32_t((n_keys + 255) / 256)), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
