// above.hip -- the threshold find's entry points (include/blurrily_storage.h).  They drive the
// map's internals (map_internal.h: the mutation log, the device images, the string and by-reference front ends);
// the kernels are above_kernels.hip's.  The find runs in two steps, above_count and above_emit (map_internal.h), which
// the scoped threshold find (scope_above.hip; section 27) runs apart, with a scope's masks.
#include "above.h"
#include "map_internal.h"

using namespace blurrily;
using namespace blurrily::detail;

namespace blurrily {
namespace detail {

namespace {

// one image's launch arguments for needles [s, s + nc) of the call
AboveArgs above_args(trigram_map m, const MapImages& I, const ScopeMasks* sm, uint32_t i, const NeedleView& N, size_t s,
                     size_t nc, uint32_t min_matches, uint32_t min_permille) {
  const DeviceIndex& ix = *I.img[i];
  AboveArgs a{};
  a.slice_se = ix.d_slice_se; a.ent = ix.d_ent; a.win_max_tri = ix.d_win_max_tri;
  a.tomb = sm ? (i ? sm->delta : sm->base) : I.tomb[i];
  a.n_windows = ix.n_windows; a.n_refs = ix.n_refs; a.dense_min8 = ix.dense_min8; a.per = windows_per_workgroup(m, ix, nc);
  a.qcodes = N.codes; a.qoff = N.qoff + s; a.q_ntri = N.ntri + s; a.q_base = uint32_t(s); a.n = uint32_t(nc);
  a.min_matches = min_matches; a.min_permille = min_permille;
  return a;
}

}  // namespace

int above_count(trigram_map m, size_t n, const NeedleView& N, uint32_t min_matches, uint32_t min_permille,
                hipStream_t stream, const ScopeMasks* sm, AboveCounted* C) {
  const MapImages I = map_images(m);
  const uint32_t n_img = I.n;
  C->n = n;
  C->n_img = n_img;
  if (C->d_counts.reserve(std::max<size_t>(size_t(n_img) * n * 4, 16), stream) < 0) return -1;
  uint32_t* d_counts = static_cast<uint32_t*>(C->d_counts.p);
  BLURRILY_HIP_TRY(hipMemsetAsync(d_counts, 0, size_t(n_img) * n * 4, stream));
  for (uint32_t i = 0; i < n_img; ++i)
    for (size_t s = 0; s < n; s += kAboveChunkNeedles) {
      AboveArgs a = above_args(m, I, sm, i, N, s, std::min(kAboveChunkNeedles, n - s), min_matches, min_permille);
      a.counts = d_counts + size_t(i) * n + s;
      if (launch_above_sweep(a, stream) < 0) return -1;
    }
  C->cnt.resize(size_t(n_img) * n);
  BLURRILY_HIP_TRY(hipMemcpyAsync(C->cnt.data(), d_counts, C->cnt.size() * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

int above_emit(trigram_map m, const NeedleView& N, uint32_t min_matches, uint32_t min_permille, const AboveCounted& C,
               const uint64_t* row_off, trigram_match results, hipStream_t stream, AboveScratch& S,
               const ScopeMasks* sm) {
  const MapImages I = map_images(m);
  const size_t n = C.n;
  const uint32_t n_img = C.n_img;
  DeviceIndex* const* img = I.img;
  const std::vector<uint32_t>& cnt = C.cnt;
  uint32_t* d_counts = static_cast<uint32_t*>(C.d_counts.p);
  auto args_of = [&](uint32_t i, size_t s, size_t nc) {
    return above_args(m, I, sm, i, N, s, nc, min_matches, min_permille);
  };
  // emit, sort and write, in chunks of needles whose rows fit the chunk's scratch
  size_t s = 0;
  while (s < n) {
    const size_t e = above_chunk_end(row_off, n, s);
    const size_t nc = e - s;
    const uint64_t rows = row_off[e] - row_off[s];
    if (rows == 0) { s = e; continue; }
    if (rows > 0x7FFFFFFFull) { errno = ENOMEM; return -1; }
    // segments per image, chunk-local
    std::vector<uint32_t> off(size_t(n_img) * (nc + 1));
    uint32_t n_keys[2] = {0, 0};
    for (uint32_t i = 0; i < n_img; ++i) {
      uint32_t* o = off.data() + size_t(i) * (nc + 1);
      o[0] = 0;
      for (size_t q = 0; q < nc; ++q) o[q + 1] = o[q] + cnt[size_t(i) * n + s + q];
      n_keys[i] = o[nc];
    }
    const size_t key_bytes = align_up(size_t(rows) * 8, 256), off_bytes = align_up(off.size() * 4, 256);
    const size_t cur_bytes = align_up(size_t(n_img) * nc * 4, 256);
    if (S.b[1].reserve(key_bytes, stream) < 0 || S.b[2].reserve(key_bytes, stream) < 0 ||
        S.b[3].reserve(off_bytes + cur_bytes, stream) < 0 ||
        S.b[5].reserve(size_t(rows) * sizeof(trigram_match_t), stream) < 0)
      return -1;
    unsigned long long* keys = static_cast<unsigned long long*>(S.b[1].p);
    unsigned long long* sorted = static_cast<unsigned long long*>(S.b[2].p);
    uint32_t* d_off = static_cast<uint32_t*>(S.b[3].p);
    uint32_t* d_cur = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(S.b[3].p) + off_bytes);
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, stream));
    BLURRILY_HIP_TRY(hipMemsetAsync(d_cur, 0, size_t(n_img) * nc * 4, stream));
    AboveRowsArgs r{};
    for (uint32_t i = 0; i < n_img; ++i) {
      const size_t kb = i ? n_keys[0] : 0;                     // the delta image's keys behind the base image's
      AboveArgs a = args_of(i, s, nc);
      a.counts = d_counts + size_t(i) * n + s;
      a.seg = d_off + size_t(i) * (nc + 1);
      a.cursor = d_cur + size_t(i) * nc;
      a.keys = keys + kb;
      if (n_keys[i] && launch_above_sweep(a, stream) < 0) return -1;
      // sort: tiles in LDS, then merge passes over the long segments (the two images' tables: b[4], b[7])
      if (n_keys[i] && segmented_sort(keys + kb, sorted + kb, off.data() + size_t(i) * (nc + 1), nc, 1, false,
                                      S.b[i ? 7 : 4], stream) < 0)
        return -1;
      r.keys[i] = sorted + kb; r.off[i] = a.seg; r.n_keys[i] = n_keys[i];
      r.ref_of_rank[i] = img[i]->d_ref_of_rank; r.weight_of_rank[i] = img[i]->d_weight_of_rank;
    }
    r.n_img = n_img; r.q_ntri = N.ntri + s; r.n = uint32_t(nc);
    r.rows = static_cast<trigram_match>(S.b[5].p);
    if (launch_above_rows(r, stream) < 0) return -1;
    BLURRILY_HIP_TRY(hipMemcpyAsync(results + row_off[s], r.rows, size_t(rows) * sizeof(trigram_match_t),
                                    hipMemcpyDeviceToHost, stream));
    BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
    s = e;
  }
  return 0;
}

}  // namespace detail
}  // namespace blurrily

namespace {

// Count (and, when results is given, write) the rows of n needles over the map as it is now.  row_off: n + 1 offsets.
int above_run(trigram_map m, size_t n, const NeedleView& N, uint32_t min_matches, uint32_t min_permille,
              trigram_match results, uint64_t capacity, uint64_t* row_off, hipStream_t stream, AboveScratch& S) {
  AboveCounted C;
  if (above_count(m, n, N, min_matches, min_permille, stream, nullptr, &C) < 0) return -1;
  const int go = above_row_off(n, [&](size_t q) { return C.rows(q); }, results, capacity, row_off);
  if (go <= 0) return go;
  return above_emit(m, N, min_matches, min_permille, C, row_off, results, stream, S, nullptr);
}

}  // namespace

extern "C" {

int blurrily_storage_find_batch_above(trigram_map m, const char* packed, const uint64_t* offsets, size_t n,
                                      uint32_t min_matches, uint32_t min_permille, trigram_match results,
                                      uint64_t capacity, uint64_t* row_off) {
  if (!m || !row_off || min_permille > 1000 || (n && (!packed || !offsets)) || n > kMaxBatchNeedles) {
    errno = EINVAL;
    return -1;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();
  row_off[0] = 0;
  if (n == 0) return 0;
  AboveScratch S;
  NeedleView N;
  if (stage_string_needles(m, packed, offsets, n, S.b[6], stream, &N) < 0) return -1;
  return above_run(m, n, N, min_matches, min_permille, results, capacity, row_off, stream, S);
}

int blurrily_storage_find_above(trigram_map m, const char* needle, uint32_t min_matches, uint32_t min_permille,
                                trigram_match results, uint64_t capacity, uint64_t* total) {
  if (!needle) { errno = EINVAL; return -1; }
  const uint64_t offsets[2] = {0, std::strlen(needle)};
  uint64_t row_off[2] = {0, 0};
  const int res = blurrily_storage_find_batch_above(m, needle, offsets, 1, min_matches, min_permille, results, capacity,
                                                    row_off);
  if (total && (res == 0 || errno == ERANGE)) *total = row_off[1];
  return res;
}

int blurrily_storage_find_references_above(trigram_map m, const uint32_t* references, size_t n, uint32_t min_matches,
                                           uint32_t min_permille, trigram_match results, uint64_t capacity,
                                           uint64_t* row_off, uint32_t* nb_trigrams) {
  if (!m || !row_off || min_permille > 1000 || (n && !references) || n > kMaxBatchNeedles) {
    errno = EINVAL;
    return -1;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();
  row_off[0] = 0;
  if (n == 0) return 0;
  AboveScratch S;
  NeedleView N;
  if (stage_reference_needles(m, references, n, S.b[6], stream, nb_trigrams, &N) < 0) return -1;
  return above_run(m, n, N, min_matches, min_permille, results, capacity, row_off, stream, S);
}

}  // extern "C"
