// above.h -- launch interface of the threshold find (above_kernels.hip): every row of a needle
// with at least its bar of matches, bar = max(1, min_matches, ceil(min_permille * T / 1000)), T its distinct trigrams.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/blurrily_storage.h"
#include "device_index.h"
#include "segsort.h"

namespace blurrily {

// One image, a chunk of needles [0, n): needle q's T = q_ntri[q] distinct codes at qcodes + qoff[q] + (q_base + q)
// (the front ends' layout: tokenise_kernel, ref_needles_kernel).  Workgroup b sweeps windows [wr * per, wr * per + per)
// of needle b / tasks, wr = b % tasks, tasks = ceil(n_windows / per).
struct AboveArgs {
  const uint2*    slice_se;
  const uint16_t* ent;
  const uint32_t* win_max_tri;
  const uint32_t* tomb;          // deleted ranks (nullptr: none)
  uint32_t        n_windows;
  uint32_t        n_refs;
  uint32_t        dense_min8;
  uint32_t        per;           // windows per workgroup
  const uint16_t* qcodes;
  const uint64_t* qoff;
  const uint32_t* q_ntri;
  uint32_t        q_base;
  uint32_t        n;
  uint32_t        min_matches;
  uint32_t        min_permille;
  // count pass (keys == nullptr): counts[q] += rows found.  Emit pass: keys (T - matches) << 32 | rank of needle q
  // go to keys[seg[q] ..], at most counts[q] of them (what the count pass found), cursor[q] zeroed before the launch.
  uint32_t*           counts;
  const uint32_t*     seg;
  uint32_t*           cursor;
  unsigned long long* keys;
};
int launch_above_sweep(const AboveArgs& a, hipStream_t stream);

// Sorting a chunk's key segments ascending (segsort.h; keys are distinct within a segment: the rank is in the low bits).
constexpr uint32_t kAboveTile = 4096;
int launch_above_tiles(const SegTile* tiles, uint32_t n_tiles, const unsigned long long* in, unsigned long long* out,
                       hipStream_t stream);
int launch_above_merge(const SegMergeArgs<unsigned long long>& a, hipStream_t stream);
template <>
struct SegKey<unsigned long long> {
  static constexpr uint32_t kTile = kAboveTile;
  static int tiles(const SegTile* t, uint32_t n, const unsigned long long* in, unsigned long long* out, hipStream_t s) {
    return launch_above_tiles(t, n, in, out, s);
  }
  static int merge(const SegMergeArgs<unsigned long long>& a, hipStream_t s) { return launch_above_merge(a, s); }
#ifdef __HIPCC__
  __device__ static bool less(unsigned long long a, unsigned long long b) { return a < b; }
#endif
};

// Rows from the sorted keys of up to two images (base, delta: disjoint references), merged per needle in result
// order: needle q's rows at rows + off[0][q] + off[1][q], off[1][q + 1] - off[1][q] of them from the delta image.
struct AboveRowsArgs {
  const unsigned long long* keys[2];
  const uint32_t*           off[2];          // [n + 1] each
  const uint32_t*           ref_of_rank[2];
  const uint32_t*           weight_of_rank[2];
  uint32_t                  n_keys[2];
  uint32_t                  n_img;
  const uint32_t*           q_ntri;          // [n]
  uint32_t                  n;
  trigram_match_t*          rows;
};
int launch_above_rows(const AboveRowsArgs& a, hipStream_t stream);

// (host and device) the bar of a needle of T distinct trigrams
__host__ __device__ inline uint32_t above_bar(uint32_t T, uint32_t min_matches, uint32_t min_permille) {
  const uint64_t p = (uint64_t(min_permille) * T + 999u) / 1000u;
  uint32_t t = min_matches > 1u ? min_matches : 1u;
  return p > t ? uint32_t(p) : t;
}

}  // namespace blurrily
