// similar.hip -- the similarity find's entry points (include/blurrily_storage.h).  They drive the
// map's internals (map_internal.h: the mutation log, the device images, the string and by-reference front ends);
// the kernels are similar_kernels.hip's.
#include <mutex>

#include "map_internal.h"
#include "similar.h"

using namespace blurrily;
using namespace blurrily::detail;

namespace {

constexpr size_t   kSimChunkNeedles = size_t(1) << 20;   // needles per sweep launch
constexpr uint64_t kSimChunkKeys    = uint64_t(1) << 24; // keys (16 B, twice: keys and sorted keys) or rows per chunk

// ---- per-rank trigram counts, one table per device image -------------------------------------------------------------
// A table is built at the first similarity call on an image and kept beside it: an image that never serves one holds
// what it held before.  An image is known by the allocation of its postings, under the runtime's process-wide buffer
// id -- a rebuilt image (new postings), or a closed map's, no longer matches, and its table is freed at the next
// similarity call on any map.  Where the runtime gives no ids, a call builds the tables it needs and frees them.
std::mutex                     g_sim_mu;
std::vector<SimilarTableEntry> g_sim_tables;

bool buffer_id(const void* p, unsigned long long* id) {
  unsigned long long v = 0;
  if (hipPointerGetAttribute(&v, HIP_POINTER_ATTRIBUTE_BUFFER_ID, const_cast<void*>(p)) != hipSuccess) {
    (void)hipGetLastError();                            // (a freed allocation: not an error of this call)
    return false;
  }
  *id = v;
  return true;
}

void free_table(SimilarTableEntry& e) {
  DeviceScope scope(e.device);
  if (e.t.ntri_of_rank) (void)hipFree(e.t.ntri_of_rank);
  if (e.t.win_min_tri) (void)hipFree(e.t.win_min_tri);
  e.t = SimilarTable();
}

}  // namespace

namespace blurrily {
namespace detail {

SimilarTables::~SimilarTables() { for (auto& e : own) free_table(e); }

int similar_table(DeviceIndex* ix, hipStream_t stream, SimilarTables& call, SimilarTable* out) {
  std::lock_guard<std::mutex> lock(g_sim_mu);
  for (size_t i = 0; i < g_sim_tables.size();) {             // tables of images that are gone
    unsigned long long id = 0;
    SimilarTableEntry& e = g_sim_tables[i];
    if (buffer_id(e.ent, &id) && id == e.ent_id) { ++i; continue; }
    free_table(e);
    g_sim_tables[i] = g_sim_tables.back();
    g_sim_tables.pop_back();
  }
  unsigned long long id = 0, other = 0;
  // ids are usable when two allocations of the image have different ones
  const bool keep = buffer_id(ix->d_ent, &id) && buffer_id(ix->d_slice_se, &other) && id != other;
  if (keep)
    for (const SimilarTableEntry& e : g_sim_tables)
      if (e.ix == ix && e.ent == ix->d_ent && e.ent_id == id) { *out = e.t; return 0; }
  SimilarTableEntry e{ix, ix->d_ent, id, ix->device, SimilarTable(), 0};
  const size_t b_ntri = std::max<size_t>(ix->n_refs, 1) * 2, b_win = std::max<size_t>(ix->n_windows, 1) * 4;
  if (hipMalloc(reinterpret_cast<void**>(&e.t.ntri_of_rank), b_ntri) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&e.t.win_min_tri), b_win) != hipSuccess) {
    (void)hipGetLastError();
    free_table(e);
    errno = ENOMEM;
    return -1;
  }
  e.bytes = b_ntri + b_win;
  if (launch_similar_ntri(*ix, e.t, stream) < 0) { free_table(e); return -1; }
  *out = e.t;
  if (keep) {
    g_sim_tables.push_back(e);
    ix->device_bytes += e.bytes;
  } else {
    call.own.push_back(e);
  }
  return 0;
}

}  // namespace detail
}  // namespace blurrily

namespace {

// ---- the search -----------------------------------------------------------------------------------------------------
// The sorted segments of a chunk's needles, one per image: sort what is not sorted yet (tiles in LDS, then merge passes
// over the segments longer than a tile), then write the rows.  off[i]: nc + 1 offsets into keys[i] (device and host).
int similar_finish(uint32_t n_img, SimilarKey* const keys[2], SimilarKey* const sorted[2], const uint32_t* const d_off[2],
                   const std::vector<uint32_t>* const h_off, const bool need_sort[2], size_t nc, uint32_t limit,
                   SimilarScratch& S, trigram_match d_rows, uint32_t* d_rntri, uint32_t* d_counts, hipStream_t stream) {
  SimilarRowsArgs r{};
  for (uint32_t i = 0; i < n_img; ++i) {
    r.keys[i] = keys[i]; r.off[i] = d_off[i]; r.n_keys[i] = h_off[i][nc];
    if (!need_sort[i] || h_off[i][nc] == 0) continue;
    // (the segments shorter than two keys are copied as they are; the two images' tables: b[4], b[7])
    if (segmented_sort(keys[i], sorted[i], h_off[i].data(), nc, 2, true, S.b[i ? 7 : 4], stream) < 0) return -1;
    r.keys[i] = sorted[i];
  }
  r.n_img = n_img; r.n = uint32_t(nc); r.limit = limit;
  r.rows = d_rows; r.row_ntri = d_rntri; r.counts = d_counts;
  return launch_similar_rows(r, stream);
}

}  // namespace

// The top-`limit` rows of n needles over the map as it is now: results / row_ntri [n * limit], counts [n].  sm: a
// scoped call's masks, in the tombstone bitmaps' place (they exclude the deleted ranks too).
int blurrily::detail::similar_run(trigram_map m, size_t n, const NeedleView& N, uint32_t limit, uint32_t min_permille,
                                  trigram_match results, uint32_t* counts, uint32_t* row_ntri, hipStream_t stream,
                                  SimilarScratch& S, const ScopeMasks* sm) {
  const MapImages I = map_images(m);
  const uint32_t n_img = I.n;
  const bool with_delta = n_img > 1;
  DeviceIndex* const* img = I.img;
  const uint32_t* const masks[2] = {sm ? sm->base : nullptr, sm ? sm->delta : nullptr};
  const uint32_t* const* tomb = sm ? masks : I.tomb;
  SimilarTables call;
  SimilarTable tab[2];
  for (uint32_t i = 0; i < n_img; ++i)
    if (similar_table(img[i], stream, call, &tab[i]) < 0) return -1;
  const bool all = limit > kSimListMax;
  // windows per workgroup: in list mode a needle's lists (tasks * limit keys) fit one tile
  auto per_of = [&](const DeviceIndex& ix, size_t nc) {
    return windows_per_workgroup(m, ix, nc, all ? 1 : (ix.n_windows + kSimTile / limit - 1) / (kSimTile / limit));
  };
  auto args_of = [&](uint32_t i, size_t s, size_t nc) {
    const DeviceIndex& ix = *img[i];
    SimilarArgs a{};
    a.slice_se = ix.d_slice_se; a.ent = ix.d_ent; a.win_max_tri = ix.d_win_max_tri; a.win_min_tri = tab[i].win_min_tri;
    a.ntri_of_rank = tab[i].ntri_of_rank; a.ref_of_rank = ix.d_ref_of_rank; a.weight_of_rank = ix.d_weight_of_rank;
    a.tomb = tomb[i]; a.n_windows = ix.n_windows; a.n_refs = ix.n_refs; a.dense_min8 = ix.dense_min8; a.per = per_of(ix, nc);
    a.qcodes = N.codes; a.qoff = N.qoff + s; a.q_ntri = N.ntri + s; a.q_base = uint32_t(s); a.n = uint32_t(nc);
    a.limit = limit; a.min_permille = min_permille; a.all = all;
    return a;
  };
  auto tasks_of = [&](uint32_t i, size_t nc) {
    const uint32_t per = per_of(*img[i], nc);
    return (img[i]->n_windows + per - 1u) / per;
  };
  // the rows of a chunk, written on the device and copied out
  auto rows_out = [&](size_t s, size_t nc, trigram_match* d_rows, uint32_t** d_rntri, uint32_t** d_cnt) -> int {
    const size_t rows_bytes = align_up(nc * limit * sizeof(trigram_match_t), 256), rn_bytes = align_up(nc * limit * 4, 256);
    if (S.b[5].reserve(rows_bytes + rn_bytes + align_up(nc * 4, 256), stream) < 0) return -1;
    unsigned char* b = static_cast<unsigned char*>(S.b[5].p);
    *d_rows = reinterpret_cast<trigram_match>(b);
    *d_rntri = row_ntri ? reinterpret_cast<uint32_t*>(b + rows_bytes) : nullptr;
    *d_cnt = reinterpret_cast<uint32_t*>(b + rows_bytes + rn_bytes);
    BLURRILY_HIP_TRY(hipMemsetAsync(b, 0, rows_bytes + rn_bytes + nc * 4, stream));
    (void)s;
    return 0;
  };
  auto copy_out = [&](size_t s, size_t nc, trigram_match d_rows, const uint32_t* d_rntri, const uint32_t* d_cnt) -> int {
    BLURRILY_HIP_TRY(hipMemcpyAsync(counts + s, d_cnt, nc * 4, hipMemcpyDeviceToHost, stream));
    BLURRILY_HIP_TRY(hipMemcpyAsync(results + s * limit, d_rows, nc * limit * sizeof(trigram_match_t), hipMemcpyDeviceToHost, stream));
    if (row_ntri) BLURRILY_HIP_TRY(hipMemcpyAsync(row_ntri + s * limit, d_rntri, nc * limit * 4, hipMemcpyDeviceToHost, stream));
    BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  };

  if (!all) {
    // list mode: every workgroup's best `limit` rows, then per needle the best `limit` of its lists in both images
    size_t s = 0;
    while (s < n) {
      size_t nc = std::min(kSimChunkNeedles, n - s);
      auto keys_of = [&](size_t c) {
        uint64_t k = 0;
        for (uint32_t i = 0; i < n_img; ++i) k += uint64_t(c) * tasks_of(i, c) * limit;
        return k;
      };
      while (nc > 1 && keys_of(nc) > kSimChunkKeys) nc = (nc + 1) / 2;
      uint32_t tasks[2] = {0, 0};
      std::vector<uint32_t> h_off[2];
      size_t key_bytes = 0, off_bytes = 0;
      for (uint32_t i = 0; i < n_img; ++i) {
        tasks[i] = tasks_of(i, nc);
        h_off[i].resize(nc + 1);
        for (size_t q = 0; q <= nc; ++q) h_off[i][q] = uint32_t(q * tasks[i] * limit);
        key_bytes += align_up(size_t(h_off[i][nc]) * sizeof(SimilarKey), 256);
        off_bytes += align_up((nc + 1) * 4, 256);
      }
      if (S.b[1].reserve(key_bytes, stream) < 0 || S.b[2].reserve(key_bytes, stream) < 0 ||
          S.b[3].reserve(off_bytes, stream) < 0)
        return -1;
      SimilarKey* keys[2] = {static_cast<SimilarKey*>(S.b[1].p), nullptr};
      SimilarKey* sorted[2] = {static_cast<SimilarKey*>(S.b[2].p), nullptr};
      uint32_t* d_off[2] = {static_cast<uint32_t*>(S.b[3].p), nullptr};
      if (n_img > 1) {
        const size_t k0 = align_up(size_t(h_off[0][nc]) * sizeof(SimilarKey), 256);
        keys[1] = reinterpret_cast<SimilarKey*>(static_cast<unsigned char*>(S.b[1].p) + k0);
        sorted[1] = reinterpret_cast<SimilarKey*>(static_cast<unsigned char*>(S.b[2].p) + k0);
        d_off[1] = d_off[0] + align_up((nc + 1) * 4, 256) / 4;
      }
      BLURRILY_HIP_TRY(hipMemsetAsync(S.b[1].p, 0xFF, key_bytes, stream));   // (kSimNone: no row)
      bool need_sort[2] = {false, false};
      for (uint32_t i = 0; i < n_img; ++i) {
        BLURRILY_HIP_TRY(hipMemcpyAsync(d_off[i], h_off[i].data(), (nc + 1) * 4, hipMemcpyHostToDevice, stream));
        SimilarArgs a = args_of(i, s, nc);
        a.keys = keys[i];
        if (launch_similar_sweep(a, stream) < 0) return -1;
        need_sort[i] = tasks[i] > 1;                          // (one list a needle: sorted already)
      }
      trigram_match d_rows;
      uint32_t *d_rntri, *d_cnt;
      if (rows_out(s, nc, &d_rows, &d_rntri, &d_cnt) < 0) return -1;
      if (similar_finish(n_img, keys, sorted, d_off, h_off, need_sort, nc, limit, S, d_rows, d_rntri, d_cnt, stream) < 0)
        return -1;
      if (copy_out(s, nc, d_rows, d_rntri, d_cnt) < 0) return -1;
      s += nc;
    }
    return 0;
  }

  // all mode: count every needle's rows at or above the floor, then write, sort and cut them in chunks
  if (S.b[0].reserve(std::max<size_t>(size_t(n_img) * n * 4, 16), stream) < 0) return -1;
  uint32_t* d_counts = static_cast<uint32_t*>(S.b[0].p);
  BLURRILY_HIP_TRY(hipMemsetAsync(d_counts, 0, size_t(n_img) * n * 4, stream));
  for (uint32_t i = 0; i < n_img; ++i)
    for (size_t s = 0; s < n; s += kSimChunkNeedles) {
      SimilarArgs a = args_of(i, s, std::min(kSimChunkNeedles, n - s));
      a.counts = d_counts + size_t(i) * n + s;
      if (launch_similar_sweep(a, stream) < 0) return -1;
    }
  std::vector<uint32_t> cnt(size_t(n_img) * n);
  BLURRILY_HIP_TRY(hipMemcpyAsync(cnt.data(), d_counts, cnt.size() * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  size_t s = 0;
  while (s < n) {
    auto rows_of = [&](size_t q) { return uint64_t(cnt[q]) + (with_delta ? cnt[n + q] : 0u); };
    size_t e = s + 1;
    uint64_t rows = rows_of(s);
    while (e < n && e - s < kSimChunkNeedles && rows + rows_of(e) <= kSimChunkKeys && (e + 1 - s) * limit <= kSimChunkKeys)
      rows += rows_of(e++);
    const size_t nc = e - s;
    if (rows > 0x7FFFFFFFull) { errno = ENOMEM; return -1; }
    std::vector<uint32_t> h_off[2];
    size_t key_bytes = 0;
    for (uint32_t i = 0; i < n_img; ++i) {
      h_off[i].resize(nc + 1);
      h_off[i][0] = 0;
      for (size_t q = 0; q < nc; ++q) h_off[i][q + 1] = h_off[i][q] + cnt[size_t(i) * n + s + q];
      key_bytes += align_up(std::max<size_t>(h_off[i][nc], 1) * sizeof(SimilarKey), 256);
    }
    const size_t off_bytes = align_up((nc + 1) * 4, 256), cur_bytes = align_up(nc * 4, 256);
    if (S.b[1].reserve(key_bytes, stream) < 0 || S.b[2].reserve(key_bytes, stream) < 0 ||
        S.b[3].reserve(n_img * (off_bytes + cur_bytes), stream) < 0)
      return -1;
    SimilarKey* keys[2] = {static_cast<SimilarKey*>(S.b[1].p), nullptr};
    SimilarKey* sorted[2] = {static_cast<SimilarKey*>(S.b[2].p), nullptr};
    unsigned char* ob = static_cast<unsigned char*>(S.b[3].p);
    uint32_t* d_off[2] = {reinterpret_cast<uint32_t*>(ob), reinterpret_cast<uint32_t*>(ob + off_bytes)};
    uint32_t* d_cur = reinterpret_cast<uint32_t*>(ob + n_img * off_bytes);
    if (n_img > 1) {
      const size_t k0 = align_up(std::max<size_t>(h_off[0][nc], 1) * sizeof(SimilarKey), 256);
      keys[1] = reinterpret_cast<SimilarKey*>(static_cast<unsigned char*>(S.b[1].p) + k0);
      sorted[1] = reinterpret_cast<SimilarKey*>(static_cast<unsigned char*>(S.b[2].p) + k0);
    }
    BLURRILY_HIP_TRY(hipMemsetAsync(d_cur, 0, n_img * cur_bytes, stream));
    bool need_sort[2] = {true, true};
    for (uint32_t i = 0; i < n_img; ++i) {
      BLURRILY_HIP_TRY(hipMemcpyAsync(d_off[i], h_off[i].data(), (nc + 1) * 4, hipMemcpyHostToDevice, stream));
      if (h_off[i][nc] == 0) continue;
      SimilarArgs a = args_of(i, s, nc);
      a.counts = d_counts + size_t(i) * n + s;
      a.seg = d_off[i];
      a.cursor = d_cur + size_t(i) * (cur_bytes / 4);
      a.keys = keys[i];
      if (launch_similar_sweep(a, stream) < 0) return -1;
    }
    trigram_match d_rows;
    uint32_t *d_rntri, *d_cnt;
    if (rows_out(s, nc, &d_rows, &d_rntri, &d_cnt) < 0) return -1;
    if (similar_finish(n_img, keys, sorted, d_off, h_off, need_sort, nc, limit, S, d_rows, d_rntri, d_cnt, stream) < 0)
      return -1;
    if (copy_out(s, nc, d_rows, d_rntri, d_cnt) < 0) return -1;
    s = e;
  }
  return 0;
}

extern "C" {

int blurrily_storage_find_batch_similar(trigram_map m, const char* packed, const uint64_t* offsets, size_t n,
                                        uint16_t limit, uint32_t min_permille, trigram_match results, uint32_t* counts,
                                        uint32_t* row_ntri) {
  if (!m || !counts || min_permille > 1000 || (n && limit && !results) || (n && (!packed || !offsets)) ||
      n > kMaxBatchNeedles) {
    errno = EINVAL;
    return -1;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  if (n == 0) return 0;
  if (limit == 0) { std::memset(counts, 0, n * 4); return 0; }
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();
  SimilarScratch S;
  NeedleView N;
  if (stage_string_needles(m, packed, offsets, n, S.b[6], stream, &N) < 0) return -1;
  return similar_run(m, n, N, limit, min_permille, results, counts, row_ntri, stream, S);
}

int blurrily_storage_find_similar(trigram_map m, const char* needle, uint16_t limit, uint32_t min_permille,
                                  trigram_match results, uint32_t* row_ntri) {
  if (!needle) { errno = EINVAL; return -1; }
  const uint64_t offsets[2] = {0, std::strlen(needle)};
  uint32_t count = 0;
  if (blurrily_storage_find_batch_similar(m, needle, offsets, 1, limit, min_permille, results, &count, row_ntri) < 0)
    return -1;
  return int(count);
}

int blurrily_storage_find_references_similar(trigram_map m, const uint32_t* references, size_t n, uint16_t limit,
                                             uint32_t min_permille, trigram_match results, uint32_t* counts,
                                             uint32_t* row_ntri, uint32_t* nb_trigrams) {
  if (!m || !counts || min_permille > 1000 || (n && limit && !results) || (n && !references) || n > kMaxBatchNeedles) {
    errno = EINVAL;
    return -1;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  if (n == 0) return 0;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();
  SimilarScratch S;
  NeedleView N;
  if (stage_reference_needles(m, references, n, S.b[6], stream, nb_trigrams, &N) < 0) return -1;
  if (limit == 0) { std::memset(counts, 0, n * 4); return 0; }
  return similar_run(m, n, N, limit, min_permille, results, counts, row_ntri, stream, S);
}

}  // extern "C"
