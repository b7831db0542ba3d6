// similar_kernels.hip -- the similarity find's kernels (launch code: similar.hip).
//
// similar_ntri_kernel: an image's per-rank trigram counts R, counted from its own postings (one workgroup per half
// window, 16-bit counters in LDS), and each window's fewest.
// similar_sweep_kernel: one workgroup per (needle, run of windows), counting a window's postings into LDS counters as
// above_sweep_kernel does.  J >= j bounds both the matches (m >= j * T) and the reference's size (j * T <= R <= T / j),
// so a window whose [win_min_tri, win_max_tri] misses the allowed range of R is passed over, and up to t - 1 dense
// slices are left out of the count (t: the match bar) and asked about candidate ranks only.  A rank's R comes from
// ntri_of_rank and the floor is tested exactly.  List mode keeps the workgroup's best `limit` rows in LDS under the
// exact key (similar.h); once the list is full its worst row m_k / u_k raises the bar (t = ceil(m_k T / u_k),
// ceil(m_k T / u_k) <= R <= floor(T u_k / m_k)), and the windows whose range of R holds T are visited first so that
// it rises early.  All mode (large limits) counts, then writes, every row at or above the floor.
// similar_tiles_kernel / seg_merge_kernel (segsort.h) sort key segments, and similar_rows_kernel merges the base and delta
// images per needle and writes the first `limit` rows.
#include "similar.h"
#include "find_kernels.h"
#include "hip_try.h"

namespace blurrily {

namespace {

constexpr uint32_t kSimThreads  = 512;
constexpr uint32_t kSimWaves    = kSimThreads / 64;
constexpr uint32_t kSimWords    = kWindowSize / 4;            // 64 KiB of counters: a window in bytes, half a window in 16 bits
constexpr uint32_t kSimMaxDense = 64;                         // dense slices of a (needle, window) that may be left out

__device__ inline bool key_less(const SimilarKey& a, const SimilarKey& b) {
  return SegKey<SimilarKey>::less(a, b);
}

__global__ __launch_bounds__(kSimThreads) void similar_ntri_kernel(const uint2* slice_se, const uint16_t* ent,
                                                                   uint32_t n_refs, uint16_t* ntri, uint32_t* win_min) {
  __shared__ uint32_t cnt[kSimWords];                         // 16-bit counters over half a window
  __shared__ uint32_t s_min;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t w = blockIdx.x >> 1, lo = (blockIdx.x & 1u) * (kWindowSize / 2);
  for (uint32_t i = tid; i < kSimWords; i += kSimThreads) cnt[i] = 0;
  if (tid == 0) s_min = 0xFFFFFFFFu;
  __syncthreads();
  const uint2* se_w = slice_se + size_t(w) * kNumCodes;
  for (uint32_t code = wave; code < kNumCodes; code += kSimWaves) {
    const uint2 se = se_w[code];                              // (a dense slice's x is past its bitmap)
    const uint32_t groups = (se.y - se.x) / 8u;
    const uint4* p = reinterpret_cast<const uint4*>(ent + se.x);
    for (uint32_t g = lane; g < groups; g += 64u) {
      const uint4 v = p[g];
      const uint32_t h[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t r = (h[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
        const uint32_t x = r - lo;
        if (r != kPadRank && x < kWindowSize / 2) atomicAdd(&cnt[x >> 1], 1u << ((x & 1u) * 16u));
      }
    }
  }
  __syncthreads();
  uint32_t mn = 0xFFFFFFFFu;
  for (uint32_t x = tid; x < kWindowSize / 2; x += kSimThreads) {
    const uint32_t r = lo + x;
    if (r >= kWindowRanks) continue;
    const uint32_t g = w * kWindowRanks + r;
    if (g >= n_refs) continue;
    const uint32_t c = (cnt[x >> 1] >> ((x & 1u) * 16u)) & 0xFFFFu;
    ntri[g] = uint16_t(c);
    mn = min(mn, c);
  }
  if (mn != 0xFFFFFFFFu) atomicMin(&s_min, mn);
  __syncthreads();
  if (tid == 0 && s_min != 0xFFFFFFFFu) atomicMin(&win_min[w], s_min);
}

// CAP > 0: list mode with a list of CAP slots (limit <= CAP / 2); CAP == 0: all mode
template <uint32_t CAP>
__global__ __launch_bounds__(kSimThreads) void similar_sweep_kernel(SimilarArgs a) {
  constexpr bool kList = CAP > 0;
  constexpr uint32_t kSlots = kList ? CAP : 1u;
  __shared__ uint32_t cnt[kSimWords];
  __shared__ uint32_t left[(kNumCodes + 31) / 32];            // codes left out of this window's count
  __shared__ uint32_t d_len[kSimMaxDense], d_at[kSimMaxDense], d_code[kSimMaxDense], leave_at[kSimMaxDense];
  __shared__ unsigned long long s_hi[kSlots], s_lo[kSlots];
  __shared__ uint32_t s_nd, s_any, s_rows, s_n, s_sorted, s_ovf, s_full, s_mk, s_uk;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tasks = (a.n_windows + a.per - 1u) / a.per;
  const uint32_t q = blockIdx.x / tasks, wr = blockIdx.x % tasks;
  if (q >= a.n) return;
  const uint32_t T = a.q_ntri[q];
  if (T == 0) return;
  const uint32_t p = a.min_permille;
  const uint16_t* codes = a.qcodes + a.qoff[q] + (uint64_t(a.q_base) + q);
  const bool wide = T > 255u;                                 // byte counters hold at most 255 matches
  const bool emit = !kList && a.keys != nullptr;
  const uint32_t w_begin = wr * a.per, w_end = min(a.n_windows, (wr + 1u) * a.per);
  // the floor's bars: m >= ceil(p T / 1000), ceil(p T / 1000) <= R <= floor(1000 T / p)
  const uint32_t f_t = max(1u, uint32_t((uint64_t(p) * T + 999u) / 1000u));
  const uint32_t f_rhi = p ? uint32_t(min<uint64_t>(1000ull * T / p, 0xFFFFFFFFull)) : 0xFFFFFFFFu;
  for (uint32_t i = tid; i < kSimWords; i += kSimThreads) cnt[i] = 0;
  for (uint32_t i = tid; i < (kNumCodes + 31) / 32; i += kSimThreads) left[i] = 0;
  if (tid == 0) { s_rows = 0; s_n = 0; s_sorted = 0; s_ovf = 0; s_full = 0; s_mk = 0; s_uk = 1; }
  uint32_t seg = 0, cap = 0;
  if (emit) { seg = a.seg[q]; cap = a.counts[q]; }
  __syncthreads();

  // the current bar (uniform: read from LDS after a barrier)
  uint32_t t = f_t, rlo = f_t, rhi = f_rhi, full = 0, mk = 0, uk = 1;
  auto bounds = [&]() {
    t = f_t; rlo = f_t; rhi = f_rhi;
    full = kList ? s_full : 0u;
    if (full) {
      mk = s_mk; uk = s_uk;
      const uint32_t tl = uint32_t((uint64_t(mk) * T + uk - 1u) / uk);
      t = max(t, tl);
      rlo = max(rlo, tl);
      rhi = min(rhi, uint32_t(uint64_t(T) * uk / mk));
    }
    rlo = max(rlo, t);                                        // (R >= m)
  };

  // the list's flush: sort the CAP slots (the empty ones as kSimNone), keep the best `limit`, raise the bar
  auto flush = [&]() {
    __syncthreads();
    const uint32_t n = min(s_n, kSlots);
    for (uint32_t i = tid; i < kSlots; i += kSimThreads)
      if (i >= n) { s_hi[i] = kSimNone; s_lo[i] = kSimNone; }
    __syncthreads();
    for (uint32_t k = 2; k <= kSlots; k <<= 1)
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t i = tid; i < kSlots; i += kSimThreads) {
          const uint32_t x = i ^ j;
          if (x > i) {
            const SimilarKey u{s_hi[i], s_lo[i]}, v{s_hi[x], s_lo[x]};
            if (key_less(v, u) == ((i & k) == 0)) { s_hi[i] = v.hi; s_lo[i] = v.lo; s_hi[x] = u.hi; s_lo[x] = u.lo; }
          }
        }
        __syncthreads();
      }
    if (tid == 0) {
      const uint32_t keep = min(n, a.limit);
      s_n = keep; s_sorted = keep; s_ovf = 0;
      if (keep == a.limit) {
        const unsigned long long hi = s_hi[keep - 1u];
        const uint32_t m = similar_m(hi), R = similar_r(hi);
        s_full = 1; s_mk = m; s_uk = T + R - m;
      }
    }
    __syncthreads();
    bounds();
  };

  for (uint32_t phase = 0; phase < (kList ? 2u : 1u); ++phase)
    for (uint32_t w = w_begin; w < w_end; ++w) {
      const uint32_t wmin = a.win_min_tri[w], wmax = a.win_max_tri[w];
      if (kList && (wmin <= T && T <= wmax) != (phase == 0)) continue;   // windows whose range of R holds T first
      bounds();
      if (wmax < rlo || wmin > rhi) continue;                 // no reference of the window has an R the bar allows
      __syncthreads();                                        // (the previous window is done with the lists)
      if (tid == 0) { s_nd = 0; s_any = 0; }
      __syncthreads();
      const uint2* se_w = a.slice_se + size_t(w) * kNumCodes;
      if (a.dense_min8 && t > 1u) {
        for (uint32_t i = tid; i < T; i += kSimThreads) {
          const uint2 se = se_w[codes[i]];
          if (se.y - se.x >= a.dense_min8) {
            const uint32_t k = atomicAdd(&s_nd, 1u);
            if (k < kSimMaxDense) { d_len[k] = se.y - se.x; d_at[k] = se.x; d_code[k] = codes[i]; }
          }
        }
        __syncthreads();
      }
      const uint32_t nd = min(s_nd, kSimMaxDense);
      const uint32_t L = min(t - 1u, nd);
      // the L largest dense slices (lower code first among equal lengths) are left out
      if (tid < nd) {
        uint32_t r = 0;
        for (uint32_t j = 0; j < nd; ++j)
          r += d_len[j] > d_len[tid] || (d_len[j] == d_len[tid] && d_code[j] < d_code[tid]);
        if (r < L) { leave_at[r] = d_at[tid]; atomicOr(&left[d_code[tid] >> 5], 1u << (d_code[tid] & 31u)); }
      }
      __syncthreads();
      const uint32_t hthr = max(1u, t - L);                   // counted matches a rank needs to be asked about

      for (uint32_t half = 0; half < (wide ? 2u : 1u); ++half) {
        const uint32_t lo = half * (kWindowSize / 2);
        // count: one slice per wave, 8 postings a lane per 16-byte load
        for (uint32_t i = wave; i < T; i += kSimWaves) {
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
        if (!s_any) continue;                                 // (uniform: nothing was counted, the counters are still zero)
        const uint32_t per_word = wide ? 2u : 4u, bits = wide ? 16u : 8u, mask = wide ? 0xFFFFu : 0xFFu;
        // a row of the window: slot s of counter word wi, at the current bar
        auto row_of = [&](uint32_t x, uint32_t wi, uint32_t s, SimilarKey* key) -> bool {
          const uint32_t c = (x >> (s * bits)) & mask;
          if (c < hthr) return false;
          const uint32_t r = wide ? lo + wi * 2u + s : wi * 4u + s;
          if (r >= kWindowRanks) return false;
          const uint32_t g = w * kWindowRanks + r;
          if (g >= a.n_refs) return false;
          uint32_t m = c;
          for (uint32_t l = 0; l < L; ++l) {
            const uint32_t* bm = reinterpret_cast<const uint32_t*>(a.ent + (leave_at[l] - kBitmapSlots));
            m += (bm[r >> 5] >> (r & 31u)) & 1u;
          }
          if (m < t) return false;
          if (a.tomb && ((a.tomb[g >> 5] >> (g & 31u)) & 1u)) return false;
          const uint32_t R = a.ntri_of_rank[g];
          if (R < rlo || R > rhi) return false;
          const uint64_t u = uint64_t(T) + R - m;
          if (1000ull * m < uint64_t(p) * u) return false;   // the floor, exactly
          if (full && uint64_t(m) * uk < uint64_t(mk) * u) return false;   // below the list's worst (ties enter)
          key->hi = similar_hi(m, T, R);
          key->lo = (static_cast<unsigned long long>(a.weight_of_rank[g]) << 32) | a.ref_of_rank[g];
          return true;
        };
        SimilarKey key;
        if (kList) {
          // a thread reads words tid, tid + 512, ... (the same number of rounds for every thread: the barriers below)
          for (uint32_t wi = tid; wi < kSimWords; wi += kSimThreads) {
            const uint32_t x = cnt[wi];
            uint32_t pend = 0;
            auto offer = [&](uint32_t s) {
              if (!row_of(x, wi, s, &key)) return;
              const uint32_t at = atomicAdd(&s_n, 1u);
              if (at < kSlots) { s_hi[at] = key.hi; s_lo[at] = key.lo; }
              else { pend |= 1u << s; s_ovf = 1; }
            };
            if (x) {
              for (uint32_t s = 0; s < per_word; ++s) offer(s);
              cnt[wi] = 0;
            }
            __syncthreads();
            while (true) {                                    // a full list: flush it, offer what did not fit again
              const uint32_t ovf = s_ovf;
              __syncthreads();
              if (!ovf) break;
              flush();
              const uint32_t again = pend;
              pend = 0;
              for (uint32_t s = 0; s < per_word; ++s)
                if ((again >> s) & 1u) offer(s);
              __syncthreads();
            }
          }
        } else {
          uint32_t mine = 0;
          for (uint32_t wi = tid; wi < kSimWords; wi += kSimThreads) {
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
            for (uint32_t wi = tid; wi < kSimWords; wi += kSimThreads) {
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
        }
        __syncthreads();
      }
      if (tid < nd) atomicAnd(&left[d_code[tid] >> 5], ~(1u << (d_code[tid] & 31u)));   // (cleared for the next window)
      if (kList) {                                            // the window's rows sorted in: the bar for the next one
        __syncthreads();
        const uint32_t unsorted = s_n != s_sorted;
        __syncthreads();
        if (unsorted) flush();
      }
    }
  __syncthreads();
  if (kList) {
    if (s_n != s_sorted) flush();
    const size_t out = (size_t(q) * tasks + wr) * a.limit;
    for (uint32_t i = tid; i < s_n; i += kSimThreads) a.keys[out + i] = SimilarKey{s_hi[i], s_lo[i]};
  } else if (!emit && tid == 0 && s_rows) {
    atomicAdd(&a.counts[q], s_rows);
  }
}

// one tile per workgroup: bitonic sort over the next power of two at or above its length, padded with kSimNone
__global__ __launch_bounds__(256) void similar_tiles_kernel(const SegTile* tiles, const SimilarKey* in,
                                                            SimilarKey* out) {
  __shared__ unsigned long long s_hi[kSimTile], s_lo[kSimTile];
  const SegTile tl = tiles[blockIdx.x];
  uint32_t P = 1;
  while (P < tl.len) P <<= 1;
  for (uint32_t i = threadIdx.x; i < P; i += 256u) {
    const SimilarKey k = i < tl.len ? in[size_t(tl.start) + i] : SimilarKey{kSimNone, kSimNone};
    s_hi[i] = k.hi; s_lo[i] = k.lo;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= P; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < P; i += 256u) {
        const uint32_t x = i ^ j;
        if (x > i) {
          const SimilarKey u{s_hi[i], s_lo[i]}, v{s_hi[x], s_lo[x]};
          if (key_less(v, u) == ((i & k) == 0)) { s_hi[i] = v.hi; s_lo[i] = v.lo; s_hi[x] = u.hi; s_lo[x] = u.lo; }
        }
      }
      __syncthreads();
    }
  for (uint32_t i = threadIdx.x; i < tl.len; i += 256u) out[size_t(tl.start) + i] = SimilarKey{s_hi[i], s_lo[i]};
}

__global__ __launch_bounds__(256) void similar_rows_kernel(SimilarRowsArgs a) {
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
  const uint32_t q = lo;
  const SimilarKey key = a.keys[img][k];
  if (key.hi == kSimNone) return;
  uint32_t before = 0;                                        // rows of the other image in front of this one
  if (a.n_img > 1) {
    const uint32_t o = img ^ 1u;
    uint32_t b = a.off[o][q], e = a.off[o][q + 1];
    const uint32_t first = b;
    while (b < e) {
      const uint32_t mid = (b + e) / 2u;
      if (key_less(a.keys[o][mid], key)) b = mid + 1u; else e = mid;
    }
    before = b - first;
  }
  const uint32_t at = (k - off[q]) + before;
  if (at >= a.limit) return;
  const size_t slot = size_t(q) * a.limit + at;
  a.rows[slot] = trigram_match_t{uint32_t(key.lo), similar_m(key.hi), uint32_t(key.lo >> 32)};
  if (a.row_ntri) a.row_ntri[slot] = similar_r(key.hi);
  atomicMax(&a.counts[q], at + 1u);
}

}  // namespace

int launch_similar_ntri(const DeviceIndex& ix, const SimilarTable& t, hipStream_t stream) {
  if (ix.n_windows == 0) return 0;
  BLURRILY_HIP_TRY(hipMemsetAsync(t.win_min_tri, 0xFF, size_t(ix.n_windows) * 4, stream));
  if (ix.n_refs) BLURRILY_HIP_TRY(hipMemsetAsync(t.ntri_of_rank, 0, size_t(ix.n_refs) * 2, stream));
  note_launch("similar_ntri_kernel");
  hipLaunchKernelGGL(similar_ntri_kernel, dim3(ix.n_windows * 2u), dim3(kSimThreads), 0, stream, ix.d_slice_se, ix.d_ent,
                     ix.n_refs, t.ntri_of_rank, t.win_min_tri);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_similar_sweep(const SimilarArgs& a, hipStream_t stream) {
  if (a.n == 0 || a.n_windows == 0) return 0;
  if (!a.all && (a.limit == 0 || a.limit > kSimListMax)) { errno = EINVAL; return -1; }
  const uint64_t grid = uint64_t(a.n) * ((a.n_windows + a.per - 1u) / a.per);
  if (grid > 0x7FFFFFFFull) { errno = EINVAL; return -1; }
  note_launch("similar_sweep_kernel");
  if (a.all)
    hipLaunchKernelGGL(similar_sweep_kernel<0>, dim3(uint32_t(grid)), dim3(kSimThreads), 0, stream, a);
  else if (a.limit <= kSimListSmall)
    hipLaunchKernelGGL(similar_sweep_kernel<2 * kSimListSmall>, dim3(uint32_t(grid)), dim3(kSimThreads), 0, stream, a);
  else
    hipLaunchKernelGGL(similar_sweep_kernel<2 * kSimListMax>, dim3(uint32_t(grid)), dim3(kSimThreads), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_similar_tiles(const SegTile* tiles, uint32_t n_tiles, const SimilarKey* in, SimilarKey* out, hipStream_t stream) {
  if (n_tiles == 0) return 0;
  note_launch("similar_tiles_kernel");
  hipLaunchKernelGGL(similar_tiles_kernel, dim3(n_tiles), dim3(256), 0, stream, tiles, in, out);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_similar_merge(const SegMergeArgs<SimilarKey>& a, hipStream_t stream) {
  if (a.n_elems == 0) return 0;
  note_launch("similar_merge_kernel");
  hipLaunchKernelGGL(seg_merge_kernel<SimilarKey>, dim3((a.n_elems + 255u) / 256u), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_similar_rows(const SimilarRowsArgs& a, hipStream_t stream) {
  const uint64_t n_keys = uint64_t(a.n_keys[0]) + (a.n_img > 1 ? a.n_keys[1] : 0u);
  if (n_keys == 0 || a.limit == 0) return 0;
  note_launch("similar_rows_kernel");
  hipLaunchKernelGGL(similar_rows_kernel, dim3(uint32_t((n_keys + 255) / 256)), dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace blurrily
