// scope_above.hip -- scoped threshold find (blurrily_storage_find_batch_above_in / _find_above_in /
// _find_batch_above_each_in / _find_references_above_each_in).
// The threshold find's rows (section 14) among a scope's members only, the strategies chosen as the scoped find chooses
// them (there is no limit: scope_takes_direct and each_plan are asked with a limit of 1): the threshold sweep with the
// scope's masks in the tombstone bitmaps' place (any scope), or the members scored directly and written in result order
// by a counting sort (scope_above_kernels.hip).  Either way a call counts first -- every needle, whatever serves it --
// lays out row_off in the caller's order, checks the capacity, and only then emits.  The each-in entries group their
// needles with each_plan: the direct ones in one count launch and one emit launch a chunk, a sweep's count and emit per
// masked scope and for the NO_SCOPE group over their compacted needles; the rows are put at the caller's row_off on the
// host.
#include "scope_above.h"
#include "scope_internal.h"

using namespace blurrily;
using namespace blurrily::detail;

namespace {

int above_in_check(const uint64_t* row_off, uint32_t min_permille, size_t n, bool needles) {
  if (!row_off || min_permille > 1000 || (n && !needles) || n > kMaxBatchNeedles) { errno = EINVAL; return -1; }
  return 0;
}

// The direct launches' count step: cnt[j] = job j's rows (a.first, a.n, a.counts and a.seg are set here).
int direct_above_count(ScopeAboveArgs a, size_t jobs, DeviceBuffer& d_counts, std::vector<uint32_t>& cnt, hipStream_t stream) {
  if (d_counts.reserve(std::max<size_t>(jobs * 4, 16), stream) < 0) return -1;
  a.counts = static_cast<uint32_t*>(d_counts.p);
  a.seg = nullptr; a.rows = nullptr;
  for (size_t s = 0; s < jobs; s += kAboveChunkNeedles) {
    a.first = uint32_t(s); a.n = uint32_t(std::min(kAboveChunkNeedles, jobs - s));
    if (launch_scope_above(a, stream) < 0) return -1;
  }
  cnt.resize(jobs);
  BLURRILY_HIP_TRY(hipMemcpyAsync(cnt.data(), a.counts, jobs * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

// ... and their emit step: job j's rows to results + off[j] (off: jobs + 1 offsets that add up cnt), in the threshold
// find's chunks.  d_counts: what the count step left.
int direct_above_emit(ScopeAboveArgs a, size_t jobs, const DeviceBuffer& d_counts, const std::vector<uint32_t>& cnt,
                      const uint64_t* off, trigram_match results, AboveScratch& S, hipStream_t stream) {
  a.counts = static_cast<uint32_t*>(d_counts.p);
  std::vector<uint32_t> seg;
  size_t s = 0;
  while (s < jobs) {
    const size_t e = above_chunk_end(off, jobs, s);
    const size_t nc = e - s;
    const uint64_t rows = off[e] - off[s];
    if (rows == 0) { s = e; continue; }
    if (rows > 0x7FFFFFFFull) { errno = ENOMEM; return -1; }
    seg.resize(nc);
    uint32_t at = 0;
    for (size_t j = 0; j < nc; ++j) { seg[j] = at; at += cnt[s + j]; }
    if (S.b[3].reserve(nc * 4, stream) < 0 || S.b[5].reserve(size_t(rows) * sizeof(trigram_match_t), stream) < 0) return -1;
    BLURRILY_HIP_TRY(hipMemcpyAsync(S.b[3].p, seg.data(), nc * 4, hipMemcpyHostToDevice, stream));
    a.first = uint32_t(s); a.n = uint32_t(nc);
    a.seg = static_cast<const uint32_t*>(S.b[3].p);
    a.rows = static_cast<trigram_match>(S.b[5].p);
    if (launch_scope_above(a, stream) < 0) return -1;
    BLURRILY_HIP_TRY(hipMemcpyAsync(results + off[s], a.rows, size_t(rows) * sizeof(trigram_match_t),
                                    hipMemcpyDeviceToHost, stream));
    BLURRILY_HIP_TRY(hipStreamSynchronize(stream));   // (seg and the rows' scratch are the next chunk's too)
    s = e;
  }
  return 0;
}

// The planned each-in call, rows to host memory at the caller's row_off.
int above_each_run(trigram_map m, const EachPlan& P, const EachNeedles& N, size_t n, uint32_t min_matches,
                   uint32_t min_permille, trigram_match results, uint64_t capacity, uint64_t* row_off, AboveScratch& S,
                   hipStream_t stream) {
  const size_t nd = P.order.size(), ng = P.idx.size(), groups = P.group_scope.size();
  if (!nd && !ng) { std::fill(row_off, row_off + n + 1, uint64_t(0)); return 0; }   // nothing serves any needle
  EachOnDevice D;
  if (D.upload(m, P, nullptr, 0, ng, false, stream) < 0) return -1;

  // 1. count: every needle served directly in one launch, a sweep per group over its needles, compacted
  std::vector<uint64_t> rows_of(n, 0);
  ScopeAboveArgs a{};
  std::vector<uint32_t> d_cnt;
  if (nd) {
    N.into(a);
    a.order = D.d_order; a.scopes = D.d_table;
    a.max_members = P.max_members; a.min_matches = min_matches; a.min_permille = min_permille;
    if (direct_above_count(a, nd, S.b[8], d_cnt, stream) < 0) return -1;
    for (size_t b = 0; b < nd; ++b) rows_of[P.order[b].x] = d_cnt[b];
  }
  std::vector<AboveCounted> C(groups);
  std::vector<SweptGroup> G(groups);
  for (size_t g = 0; g < groups; ++g) {
    if (G[g].gather(P, D, N.V, g, stream) < 0) return -1;
    if (above_count(m, G[g].cnt, G[g].V, min_matches, min_permille, stream, G[g].masks.ptr(), &C[g]) < 0) return -1;
    for (size_t k = 0; k < G[g].cnt; ++k) rows_of[P.idx[G[g].k0 + k]] = C[g].rows(k);
  }
  const int go = above_row_off(n, [&](size_t q) { return rows_of[q]; }, results, capacity, row_off);
  if (go <= 0) return go;

  // 2. emit, launch by launch in its own order; each needle's rows then go where the caller's row_off has them
  std::vector<trigram_match_t> part;
  std::vector<uint64_t> off(std::max(nd, ng) + 1);
  auto put_back = [&](size_t k, uint32_t q) {           // the launch's job k is the caller's q
    if (off[k + 1] > off[k])
      std::memcpy(results + row_off[q], part.data() + off[k], size_t(off[k + 1] - off[k]) * sizeof(trigram_match_t));
  };
  if (nd) {
    rows_to_offsets(nd, [&](size_t b) { return d_cnt[b]; }, off.data());
    part.resize(size_t(off[nd]));
    if (off[nd] && direct_above_emit(a, nd, S.b[8], d_cnt, off.data(), part.data(), S, stream) < 0) return -1;
    for (size_t b = 0; b < nd; ++b) put_back(b, P.order[b].x);
  }
  for (size_t g = 0; g < groups; ++g) {
    const size_t k0 = G[g].k0, cnt = G[g].cnt;
    rows_to_offsets(cnt, [&](size_t k) { return C[g].rows(k); }, off.data());
    if (off[cnt] == 0) continue;
    part.resize(size_t(off[cnt]));
    if (above_emit(m, G[g].V, min_matches, min_permille, C[g], off.data(), part.data(), stream, S, G[g].masks.ptr()) < 0)
      return -1;
    for (size_t k = 0; k < cnt; ++k) put_back(k, P.idx[k0 + k]);
  }
  return 0;
}

}  // namespace

extern "C" {

int blurrily_storage_find_batch_above_in(trigram_map m, blurrily_scope sc, const char* packed, const uint64_t* offsets,
                                         size_t n, uint32_t min_matches, uint32_t min_permille, trigram_match results,
                                         uint64_t capacity, uint64_t* row_off) {
  if (scope_check(m, sc) < 0 || above_in_check(row_off, min_permille, n, packed && offsets) < 0) return -1;
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (scope_prepare(m, sc, stream) < 0) return -1;     // (without a GPU this is what fails, with ENODEV)
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();
  row_off[0] = 0;
  if (n == 0) return 0;
  if (sc->n_held == 0) { std::fill(row_off, row_off + n + 1, uint64_t(0)); return 0; }
  AboveScratch S;
  if (scope_takes_direct(m, sc, 1)) {
    EachNeedles N;
    if (stage_direct_strings(packed, offsets, n, S.b[9], stream, &N) < 0) return -1;
    ScopeAboveArgs a{};
    N.into(a);
    a.one = direct_of(sc);
    a.max_members = sc->n_direct; a.min_matches = min_matches; a.min_permille = min_permille;
    std::vector<uint32_t> cnt;
    if (direct_above_count(a, n, S.b[8], cnt, stream) < 0) return -1;
    const int go = above_row_off(n, [&](size_t q) { return cnt[q]; }, results, capacity, row_off);
    if (go <= 0) return go;
    return direct_above_emit(a, n, S.b[8], cnt, row_off, results, S, stream);
  }
  const ScopeMasksOf sm = masks_of(sc);
  NeedleView N;
  if (stage_string_needles(m, packed, offsets, n, S.b[6], stream, &N) < 0) return -1;
  AboveCounted C;
  if (above_count(m, n, N, min_matches, min_permille, stream, sm.ptr(), &C) < 0) return -1;
  const int go = above_row_off(n, [&](size_t q) { return C.rows(q); }, results, capacity, row_off);
  if (go <= 0) return go;
  return above_emit(m, N, min_matches, min_permille, C, row_off, results, stream, S, sm.ptr());
}

int blurrily_storage_find_above_in(trigram_map m, blurrily_scope sc, const char* needle, uint32_t min_matches,
                                   uint32_t min_permille, trigram_match results, uint64_t capacity, uint64_t* total) {
  if (!needle) { errno = EINVAL; return -1; }
  const uint64_t offsets[2] = {0, std::strlen(needle)};
  uint64_t row_off[2] = {0, 0};
  const int res = blurrily_storage_find_batch_above_in(m, sc, needle, offsets, 1, min_matches, min_permille, results,
                                                       capacity, row_off);
  if (total && (res == 0 || errno == ERANGE)) *total = row_off[1];
  return res;
}

int blurrily_storage_find_batch_above_each_in(trigram_map m, const blurrily_scope* scopes, size_t n_scopes,
                                              const uint32_t* which, const char* packed, const uint64_t* offsets,
                                              size_t n, uint32_t min_matches, uint32_t min_permille,
                                              trigram_match results, uint64_t capacity, uint64_t* row_off) {
  if (each_check(m, scopes, n_scopes) < 0 || above_in_check(row_off, min_permille, n, which && packed && offsets) < 0 ||
      each_check_which(which, n, n_scopes) < 0)
    return -1;
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  m->last_kernels.clear();
  row_off[0] = 0;
  if (n == 0) return 0;
  EachPlan P;
  if (each_plan(m, scopes, n_scopes, which, n, 1, stream, &P) < 0) return -1;
  NameScope names(&m->last_kernels);                     // (the scopes' preparation is no part of the find)
  AboveScratch S;
  EachNeedles N;
  if (stage_each_strings(m, P, packed, offsets, n, S.b[6], S.b[9], stream, &N) < 0) return -1;
  return above_each_run(m, P, N, n, min_matches, min_permille, results, capacity, row_off, S, stream);
}

int blurrily_storage_find_references_above_each_in(trigram_map m, const blurrily_scope* scopes, size_t n_scopes,
                                                   const uint32_t* which, const uint32_t* references, size_t n,
                                                   uint32_t min_matches, uint32_t min_permille, trigram_match results,
                                                   uint64_t capacity, uint64_t* row_off, uint32_t* nb_trigrams) {
  if (each_check(m, scopes, n_scopes) < 0 || above_in_check(row_off, min_permille, n, which && references) < 0 ||
      each_check_which(which, n, n_scopes) < 0)
    return -1;
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  m->last_kernels.clear();
  row_off[0] = 0;
  if (n == 0) return 0;
  EachPlan P;
  if (each_plan(m, scopes, n_scopes, which, n, 1, stream, &P) < 0) return -1;
  AboveScratch S;
  EachNeedles N;                                         // (after every scope's preparation: both use ws_refs)
  if (stage_reference_needles(m, references, n, S.b[6], stream, nb_trigrams, &N.V) < 0) return -1;
  NameScope names(&m->last_kernels);                     // (the preparation and the extraction are no part of the find)
  return above_each_run(m, P, N, n, min_matches, min_permille, results, capacity, row_off, S, stream);
}

}  // extern "C"
