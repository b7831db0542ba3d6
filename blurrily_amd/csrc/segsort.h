// segsort.h -- sorting key segments ascending, shared by the threshold and similarity finds (above.h, similar.h).
// Keys are distinct within a segment.  A segment is cut into tiles of at most SegKey<Key>::kTile keys from its start;
// the key's own tile kernel sorts every tile in LDS (above_tiles_kernel, similar_tiles_kernel: written per key -- one
// templated on the key with the LDS layout as a trait compiled to other instructions for both keys);
// seg_merge_kernel is one pass over the segments longer than a tile -- every pair of sorted runs of `width` keys
// merged from in to out, a run without a partner copied.  segmented_sort drives both.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "hip_try.h"

namespace blurrily {

struct SegTile {
  uint32_t start, len;
};
template <class Key>
struct SegMergeArgs {
  const uint32_t* seg_start;   // [n_segs] the long segments
  const uint32_t* seg_len;
  const uint32_t* elem_off;    // [n_segs + 1] exclusive scan of seg_len
  uint32_t        n_segs;
  uint32_t        n_elems;
  uint32_t        width;
  const Key*      in;
  Key*            out;
};

// Per key type, specialised beside the key (above.h, similar.h):
//   kTile                           keys per tile
//   tiles(...), merge(...)          the launches (above_kernels.hip, similar_kernels.hip: they note their kernels' names)
//   less(a, b)                      (device) the order
template <class Key>
struct SegKey;

// Sort the segments [off[q], off[q + 1]) of keys, q < nc (off: host), into `sorted`; `keys` is scratch afterwards.
// min_len: shorter segments are left alone (copy_first: all keys are copied to `sorted` before, so that those are in
// place too).  tables: device scratch for the tile and long-segment tables.
template <class Key, class Buffer>
int segmented_sort(Key* keys, Key* sorted, const uint32_t* off, size_t nc, uint32_t min_len, bool copy_first,
                   Buffer& tables, hipStream_t stream) {
  constexpr uint32_t kTile = SegKey<Key>::kTile;
  std::vector<SegTile> tiles;
  std::vector<uint32_t> longs, ln, eo{0};                     // seg_start | seg_len | elem_off, each of n_long (+1)
  uint32_t max_len = 0;
  for (size_t q = 0; q < nc; ++q) {
    const uint32_t len = off[q + 1] - off[q];
    if (len < min_len) continue;
    for (uint32_t t0 = 0; t0 < len; t0 += kTile) tiles.push_back(SegTile{off[q] + t0, std::min(kTile, len - t0)});
    if (len > kTile) { longs.push_back(off[q]); ln.push_back(len); eo.push_back(eo.back() + len); }
    max_len = std::max(max_len, len);
  }
  const uint32_t n_long = uint32_t(ln.size());
  longs.insert(longs.end(), ln.begin(), ln.end());
  longs.insert(longs.end(), eo.begin(), eo.end());
  const size_t tile_bytes = (tiles.size() * sizeof(SegTile) + 255) / 256 * 256;
  if (tables.reserve(tile_bytes + longs.size() * 4 + 256, stream) < 0) return -1;
  SegTile* d_tiles = static_cast<SegTile*>(tables.p);
  uint32_t* d_longs = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(tables.p) + tile_bytes);
  if (copy_first)
    BLURRILY_HIP_TRY(hipMemcpyAsync(sorted, keys, size_t(off[nc]) * sizeof(Key), hipMemcpyDeviceToDevice, stream));
  if (!tiles.empty())
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(SegTile), hipMemcpyHostToDevice, stream));
  BLURRILY_HIP_TRY(hipMemcpyAsync(d_longs, longs.data(), longs.size() * 4, hipMemcpyHostToDevice, stream));
  if (SegKey<Key>::tiles(d_tiles, uint32_t(tiles.size()), keys, sorted, stream) < 0) return -1;
  if (n_long) {
    SegMergeArgs<Key> g{d_longs, d_longs + n_long, d_longs + 2 * n_long, n_long, eo.back(), kTile, sorted, keys};
    for (; g.width < max_len; g.width *= 2) {
      if (SegKey<Key>::merge(g, stream) < 0) return -1;
      std::swap(const_cast<Key*&>(g.in), g.out);
    }
    if (g.in != sorted) {                                     // (an odd number of passes: copied back)
      g.width = 1u << 31;
      if (SegKey<Key>::merge(g, stream) < 0) return -1;
    }
  }
  return 0;
}

#ifdef __HIPCC__
namespace {   // (kernels of the translation unit that launches them: above_kernels.hip, similar_kernels.hip)

// one thread per key of the long segments: its place in the merge of its run with the partner run
template <class Key>
__global__ __launch_bounds__(256) void seg_merge_kernel(SegMergeArgs<Key> a) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n_elems) return;
  uint32_t lo = 0, hi = a.n_segs;                             // the segment: the last k with elem_off[k] <= e
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) / 2u;
    if (a.elem_off[mid] <= e) lo = mid; else hi = mid;
  }
  const uint32_t base = a.seg_start[lo], len = a.seg_len[lo], i = e - a.elem_off[lo];
  const uint32_t b = i / a.width, p = b ^ 1u;
  const Key x = a.in[size_t(base) + i];
  uint32_t rank = 0;
  if (size_t(p) * a.width < len) {
    uint32_t f = p * a.width, l = min(len, f + a.width);
    const uint32_t first = f;
    while (f < l) {                                           // partner keys below x (keys are distinct)
      const uint32_t mid = (f + l) / 2u;
      if (SegKey<Key>::less(a.in[size_t(base) + mid], x)) f = mid + 1u; else l = mid;
    }
    rank = f - first;
  }
  a.out[size_t(base) + min(b, p) * a.width + (i - b * a.width) + rank] = x;
}

}  // namespace
#endif

}  // namespace blurrily
