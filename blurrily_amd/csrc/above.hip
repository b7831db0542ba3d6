// above.hip -- the threshold find's entry points (include/blurrily_storage.h).  Compiled as
// one translation unit with c_abi.hip, whose map internals (the mutation log, the device images, the by-reference
// extraction) they drive; the kernels are above_kernels.hip's.
#include "c_abi.hip"

#include "above.h"

namespace {

constexpr size_t   kAboveChunkNeedles = size_t(1) << 20;   // needles per sweep launch
constexpr uint64_t kAboveChunkRows    = uint64_t(1) << 24; // rows per emit chunk (keys, sorted keys, rows: 28 B each)

// device scratch of one call, freed on the way out
struct AboveScratch {
  DeviceBuffer b[8];
  ~AboveScratch() { for (auto& x : b) x.release(); }
};

// The needles of a call as the sweeps read them: needle q's ntri[q] codes at codes + qoff[q] + q.
struct AboveNeedles {
  const uint16_t* codes;
  const uint64_t* qoff;
  const uint32_t* ntri;
};

// Count (and, when results is given, write) the rows of n needles over the map as it is now.  row_off: n + 1 offsets.
int above_run(trigram_map m, size_t n, const AboveNeedles& N, uint32_t min_matches, uint32_t min_permille,
              trigram_match results, uint64_t capacity, uint64_t* row_off, hipStream_t stream, AboveScratch& S) {
  const bool with_delta = !log_of(m)->pending.empty() && m->delta.device >= 0;
  const uint32_t n_img = with_delta ? 2u : 1u;
  const DeviceIndex* img[2] = {&m->dev, &m->delta};
  const uint32_t* tomb[2] = {log_of(m)->n_tomb ? m->dev.d_tomb : nullptr, nullptr};
  // windows per workgroup: a small batch spreads each needle's windows over the GPU, a large one gives a needle one workgroup
  auto per_of = [&](const DeviceIndex& ix, size_t nc) {
    const uint64_t want = uint64_t(std::max(m->n_cus, 1)) * 8u;
    const uint64_t per = uint64_t(ix.n_windows) * nc / want;
    return uint32_t(std::min<uint64_t>(std::max<uint64_t>(per, 1), std::max<uint32_t>(ix.n_windows, 1)));
  };
  auto args_of = [&](uint32_t i, size_t s, size_t nc) {
    const DeviceIndex& ix = *img[i];
    AboveArgs a{};
    a.slice_se = ix.d_slice_se; a.ent = ix.d_ent; a.win_max_tri = ix.d_win_max_tri; a.tomb = tomb[i];
    a.n_windows = ix.n_windows; a.n_refs = ix.n_refs; a.dense_min8 = ix.dense_min8; a.per = per_of(ix, nc);
    a.qcodes = N.codes; a.qoff = N.qoff + s; a.q_ntri = N.ntri + s; a.q_base = uint32_t(s); a.n = uint32_t(nc);
    a.min_matches = min_matches; a.min_permille = min_permille;
    return a;
  };

  // 1. count
  if (S.b[0].reserve(std::max<size_t>(size_t(n_img) * n * 4, 16), stream) < 0) return -1;
  uint32_t* d_counts = static_cast<uint32_t*>(S.b[0].p);
  BLURRILY_HIP_TRY(hipMemsetAsync(d_counts, 0, size_t(n_img) * n * 4, stream));
  for (uint32_t i = 0; i < n_img; ++i)
    for (size_t s = 0; s < n; s += kAboveChunkNeedles) {
      AboveArgs a = args_of(i, s, std::min(kAboveChunkNeedles, n - s));
      a.counts = d_counts + size_t(i) * n + s;
      if (launch_above_sweep(a, stream) < 0) return -1;
    }
  std::vector<uint32_t> cnt(size_t(n_img) * n);
  BLURRILY_HIP_TRY(hipMemcpyAsync(cnt.data(), d_counts, cnt.size() * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  row_off[0] = 0;
  for (size_t q = 0; q < n; ++q) row_off[q + 1] = row_off[q] + cnt[q] + (with_delta ? cnt[n + q] : 0u);
  if (!results) return 0;
  if (capacity < row_off[n]) { errno = ERANGE; return -1; }

  // 2. emit, sort and write, in chunks of needles whose rows fit the chunk's scratch
  size_t s = 0;
  while (s < n) {
    size_t e = s + 1;
    while (e < n && e - s < kAboveChunkNeedles && row_off[e + 1] - row_off[s] <= kAboveChunkRows) ++e;
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
    // the sort's tables: every image's tiles, and its segments longer than a tile
    std::vector<AboveTile> tiles[2];
    std::vector<uint32_t> longs[2];                           // seg_start | seg_len | elem_off, each of n_long (+1)
    uint32_t max_len[2] = {0, 0};
    for (uint32_t i = 0; i < n_img; ++i) {
      const uint32_t* o = off.data() + size_t(i) * (nc + 1);
      std::vector<uint32_t> st, ln, eo{0};
      for (size_t q = 0; q < nc; ++q) {
        const uint32_t len = o[q + 1] - o[q];
        for (uint32_t t0 = 0; t0 < len; t0 += kAboveTile) tiles[i].push_back(AboveTile{o[q] + t0, std::min(kAboveTile, len - t0)});
        if (len > kAboveTile) { st.push_back(o[q]); ln.push_back(len); eo.push_back(eo.back() + len); }
        max_len[i] = std::max(max_len[i], len);
      }
      longs[i] = st;
      longs[i].insert(longs[i].end(), ln.begin(), ln.end());
      longs[i].insert(longs[i].end(), eo.begin(), eo.end());
    }
    const size_t tab_bytes = align_up((tiles[0].size() + tiles[1].size()) * sizeof(AboveTile), 256) +
                             align_up((longs[0].size() + longs[1].size()) * 4, 256) + 256;
    if (S.b[1].reserve(key_bytes, stream) < 0 || S.b[2].reserve(key_bytes, stream) < 0 ||
        S.b[3].reserve(off_bytes + cur_bytes, stream) < 0 || S.b[4].reserve(tab_bytes, stream) < 0 ||
        S.b[5].reserve(size_t(rows) * sizeof(trigram_match_t), stream) < 0)
      return -1;
    unsigned long long* keys = static_cast<unsigned long long*>(S.b[1].p);
    unsigned long long* sorted = static_cast<unsigned long long*>(S.b[2].p);
    uint32_t* d_off = static_cast<uint32_t*>(S.b[3].p);
    uint32_t* d_cur = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(S.b[3].p) + off_bytes);
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, stream));
    BLURRILY_HIP_TRY(hipMemsetAsync(d_cur, 0, size_t(n_img) * nc * 4, stream));
    AboveTile* d_tiles = static_cast<AboveTile*>(S.b[4].p);
    uint32_t* d_longs = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(S.b[4].p) +
                                                    align_up((tiles[0].size() + tiles[1].size()) * sizeof(AboveTile), 256));
    if (!tiles[0].empty())
      BLURRILY_HIP_TRY(hipMemcpyAsync(d_tiles, tiles[0].data(), tiles[0].size() * sizeof(AboveTile), hipMemcpyHostToDevice, stream));
    if (!tiles[1].empty())
      BLURRILY_HIP_TRY(hipMemcpyAsync(d_tiles + tiles[0].size(), tiles[1].data(), tiles[1].size() * sizeof(AboveTile),
                                      hipMemcpyHostToDevice, stream));
    if (!longs[0].empty()) BLURRILY_HIP_TRY(hipMemcpyAsync(d_longs, longs[0].data(), longs[0].size() * 4, hipMemcpyHostToDevice, stream));
    if (!longs[1].empty())
      BLURRILY_HIP_TRY(hipMemcpyAsync(d_longs + longs[0].size(), longs[1].data(), longs[1].size() * 4, hipMemcpyHostToDevice, stream));
    AboveRowsArgs r{};
    for (uint32_t i = 0; i < n_img; ++i) {
      const size_t kb = i ? n_keys[0] : 0;                     // the delta image's keys behind the base image's
      AboveArgs a = args_of(i, s, nc);
      a.counts = d_counts + size_t(i) * n + s;
      a.seg = d_off + size_t(i) * (nc + 1);
      a.cursor = d_cur + size_t(i) * nc;
      a.keys = keys + kb;
      if (n_keys[i] && launch_above_sweep(a, stream) < 0) return -1;
      if (n_keys[i]) {                                          // sort: tiles in LDS, then merge passes over the long segments
        const AboveTile* t_i = d_tiles + (i ? tiles[0].size() : 0);
        if (launch_above_tiles(t_i, uint32_t(tiles[i].size()), keys + kb, sorted + kb, stream) < 0) return -1;
        const uint32_t n_long = uint32_t((longs[i].size() - 1) / 3);
        if (n_long) {
          const uint32_t* L = d_longs + (i ? longs[0].size() : 0);
          AboveMergeArgs g{L, L + n_long, L + 2 * n_long, n_long, longs[i][3 * n_long], kAboveTile, sorted + kb, keys + kb};
          for (; g.width < max_len[i]; g.width *= 2) {
            if (launch_above_merge(g, stream) < 0) return -1;
            std::swap(const_cast<unsigned long long*&>(g.in), g.out);
          }
          if (g.in != sorted + kb) {                              // (an odd number of passes: copied back)
            g.width = 1u << 31;
            if (launch_above_merge(g, stream) < 0) return -1;
          }
        }
      }
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

// what every entry does first: the map's pending work, then the device image (ENODEV without a usable GPU)
int above_ready(trigram_map m, hipStream_t stream) {
  if (m->host->dirty_buckets()) m->host->sort_dirty_buckets();
  if (ensure_device(m) < 0) return -1;
  return apply_tombstones(m, stream);
}

}  // namespace

extern "C" {

int blurrily_storage_find_batch_above(trigram_map m, const char* packed, const uint64_t* offsets, size_t n,
                                      uint32_t min_matches, uint32_t min_permille, trigram_match results,
                                      uint64_t capacity, uint64_t* row_off) {
  if (!m || !row_off || min_permille > 1000 || (n && (!packed || !offsets)) || n > 0xFFFFFFF0ull) {
    errno = EINVAL;
    return -1;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (above_ready(m, stream) < 0) return -1;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();
  row_off[0] = 0;
  if (n == 0) return 0;
  AboveScratch S;
  // the needles up, tokenised by the string path's own front end
  const size_t packed_bytes = size_t(offsets[n]);
  const size_t per_n = align_up(n * 4, 256), o_pk = align_up((n + 1) * 8, 256);
  const size_t o_codes = o_pk + align_up(std::max<size_t>(packed_bytes, 16), 256);
  const size_t o_ntri = o_codes + align_up((packed_bytes + n) * 2, 256);
  const size_t bytes = o_ntri + 6 * per_n + 256;
  if (S.b[6].reserve(bytes, stream) < 0) return -1;
  unsigned char* b = static_cast<unsigned char*>(S.b[6].p);
  uint64_t* d_offsets = reinterpret_cast<uint64_t*>(b);
  char* d_packed = reinterpret_cast<char*>(b + o_pk);
  uint16_t* d_codes = reinterpret_cast<uint16_t*>(b + o_codes);
  uint32_t* q = reinterpret_cast<uint32_t*>(b + o_ntri);      // ntri | nb | big | mid | start | (spare) | scalars
  uint32_t* scalars = reinterpret_cast<uint32_t*>(b + o_ntri + 6 * per_n);
  BLURRILY_HIP_TRY(hipMemcpyAsync(d_offsets, offsets, (n + 1) * 8, hipMemcpyHostToDevice, stream));
  if (packed_bytes) BLURRILY_HIP_TRY(hipMemcpyAsync(d_packed, packed, packed_bytes, hipMemcpyHostToDevice, stream));
  BLURRILY_HIP_TRY(hipMemsetAsync(scalars, 0, 256, stream));
  const size_t w = per_n / 4;
  TokeniseArgs t{d_packed, d_offsets, uint32_t(n), m->dev.d_code_total, d_codes, q, q + w, q + 2 * w, scalars,
                 q + 3 * w, scalars + 1, m->dev.d_start_win, q + 4 * w, 0u};
  note_launch("tokenise_kernel");
  if (launch_tokenise(t, stream) < 0) return -1;
  return above_run(m, n, AboveNeedles{d_codes, d_offsets, q}, min_matches, min_permille, results, capacity, row_off,
                   stream, S);
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
  if (!m || !row_off || min_permille > 1000 || (n && !references) || n > 0xFFFFFFF0ull) {
    errno = EINVAL;
    return -1;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (above_ready(m, stream) < 0) return -1;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();
  row_off[0] = 0;
  if (n == 0) return 0;
  AboveScratch S;
  if (S.b[6].reserve(n * 4, stream) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(S.b[6].p, references, n * 4, hipMemcpyHostToDevice, stream));
  RefExtract x;                                                // the by-reference front end (section 11)
  if (refs_extract(m, static_cast<const uint32_t*>(S.b[6].p), n, stream, &x) < 0) return -1;
  if (nb_trigrams) {
    BLURRILY_HIP_TRY(hipMemcpyAsync(nb_trigrams, x.needles.ntri, n * 4, hipMemcpyDeviceToHost, stream));
    BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  }
  const int res = above_run(m, n, AboveNeedles{x.needles.codes, x.needles.qoff, x.needles.ntri}, min_matches,
                            min_permille, results, capacity, row_off, stream, S);
  return res;
}

}  // extern "C"
