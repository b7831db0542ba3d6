// similar.h -- launch interface of the similarity find (similar_kernels.hip): a needle's top
// `limit` rows by trigram Jaccard similarity J = m / (T + R - m) at or above min_permille / 1000, T the needle's
// distinct trigrams, R the reference's, m their common ones.  Order: J descending, then find's order (matches
// descending, weight ascending, reference ascending).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/blurrily_storage.h"
#include "device_index.h"
#include "segsort.h"

namespace blurrily {

// A row's sort key: ascending (hi, lo) is result order, across images too.
//   hi = (2^32 - floor(m * 2^32 / u)) << 30 | (0x7FFF - m) << 15 | R     (u = T + R - m < 2^16: m, T, R < 2^15)
//   lo = weight << 32 | reference
// floor(m * 2^32 / u) is exact and order-preserving: two distinct fractions with denominators below 2^16 differ by
// more than 2^-32, and equal fractions give equal values.  R sits below m: for one needle, equal J and equal m imply
// equal u, so equal R -- it never decides the order, it only travels with the row.  ~0 (both words) is no row.
struct SimilarKey {
  unsigned long long hi, lo;
};
constexpr unsigned long long kSimNone = ~0ull;

// (host and device) the key of a row, and its parts back
__host__ __device__ inline unsigned long long similar_hi(uint32_t m, uint32_t T, uint32_t R) {
  const uint64_t u = uint64_t(T) + R - m;
  const uint64_t s = (uint64_t(m) << 32) / u;                  // 1 .. 2^32
  return (((1ull << 32) - s) << 30) | (uint64_t(0x7FFFu - m) << 15) | R;
}
__host__ __device__ inline uint32_t similar_m(unsigned long long hi) { return 0x7FFFu - uint32_t((hi >> 15) & 0x7FFFu); }
__host__ __device__ inline uint32_t similar_r(unsigned long long hi) { return uint32_t(hi & 0x7FFFu); }

// Per-rank trigram counts of one image, built on the device from its own postings (similar_ntri_kernel):
// ntri_of_rank[g] = R of rank g, win_min_tri[w] = the fewest any rank of window w has.
struct SimilarTable {
  uint16_t* ntri_of_rank = nullptr;   // [n_refs]
  uint32_t* win_min_tri  = nullptr;   // [n_windows]
};
int launch_similar_ntri(const DeviceIndex& ix, const SimilarTable& t, hipStream_t stream);

// One image, a chunk of needles [0, n) in the front ends' layout (needle q's T = q_ntri[q] codes at
// qcodes + qoff[q] + (q_base + q)).  Workgroup b sweeps windows [wr * per, wr * per + per) of needle q = b / tasks,
// wr = b % tasks, tasks = ceil(n_windows / per).
//   list mode (limit <= kSimListMax): each workgroup keeps its best `limit` rows in LDS and writes them, best first and
//     padded with kSimNone, to keys[(q * tasks + wr) * limit ..].
//   all mode (keys_all): every row at or above the floor -- count pass (keys == nullptr): counts[q] += rows; emit pass:
//     keys[seg[q] + ..], at most counts[q] of them, cursor[q] zeroed before the launch.
struct SimilarArgs {
  const uint2*    slice_se;
  const uint16_t* ent;
  const uint32_t* win_max_tri;
  const uint32_t* win_min_tri;
  const uint16_t* ntri_of_rank;
  const uint32_t* ref_of_rank;
  const uint32_t* weight_of_rank;
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
  uint32_t        limit;
  uint32_t        min_permille;
  bool            all;           // all mode
  uint32_t*       counts;
  const uint32_t* seg;
  uint32_t*       cursor;
  SimilarKey*     keys;
};
constexpr uint32_t kSimListSmall = 256;    // limits served by the 8 KiB list (two workgroups a CU)
constexpr uint32_t kSimListMax   = 1024;   // ... by the 32 KiB list (one a CU); above: all mode
int launch_similar_sweep(const SimilarArgs& a, hipStream_t stream);

// Sorting key segments ascending (segsort.h; keys are distinct within a segment: the reference is in lo).
constexpr uint32_t kSimTile = 2048;
int launch_similar_tiles(const SegTile* tiles, uint32_t n_tiles, const SimilarKey* in, SimilarKey* out, hipStream_t stream);
int launch_similar_merge(const SegMergeArgs<SimilarKey>& a, hipStream_t stream);
template <>
struct SegKey<SimilarKey> {
  static constexpr uint32_t kTile = kSimTile;
  static int tiles(const SegTile* t, uint32_t n, const SimilarKey* in, SimilarKey* out, hipStream_t s) {
    return launch_similar_tiles(t, n, in, out, s);
  }
  static int merge(const SegMergeArgs<SimilarKey>& a, hipStream_t s) { return launch_similar_merge(a, s); }
#ifdef __HIPCC__
  __device__ static bool less(const SimilarKey& a, const SimilarKey& b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }
#endif
};

// Rows from the sorted segments of up to two images, merged per needle and cut at `limit`: needle q's segment in
// image i is keys[i][off[i][q] .. off[i][q + 1]) (kSimNone keys are no rows).  Row k of needle q goes to
// rows[q * limit + k] (row_ntri likewise, when given); counts[q] (zeroed before the launch) ends as the rows written.
struct SimilarRowsArgs {
  const SimilarKey* keys[2];
  const uint32_t*   off[2];      // [n + 1] each
  uint32_t          n_keys[2];
  uint32_t          n_img;
  uint32_t          n;
  uint32_t          limit;
  trigram_match_t*  rows;
  uint32_t*         row_ntri;
  uint32_t*         counts;
};
int launch_similar_rows(const SimilarRowsArgs& a, hipStream_t stream);

}  // namespace blurrily
