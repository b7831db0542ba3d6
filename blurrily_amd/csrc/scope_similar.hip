// scope_similar.hip -- scoped similarity find (blurrily_storage_find_batch_similar_in / _find_similar_in /
// _find_batch_similar_each_in / _find_references_similar_each_in).
// The similarity find's rows (section 15) among a scope's members only, the strategies chosen as the scoped find
// chooses them: the similarity sweep with the scope's masks in the tombstone bitmaps' place (any scope, any limit), or
// the members scored directly (scope_similar_kernels.hip).  The each-in entries group their needles with each_plan: the
// direct ones in one launch, a sweep per masked scope and one for the NO_SCOPE group over their compacted needles; the
// rows come back to the host per group and are put in the caller's order there.
#include "scope_internal.h"

using namespace blurrily;
using namespace blurrily::detail;

namespace {

int similar_check(const uint32_t* counts, uint32_t min_permille, size_t n, uint16_t limit, const void* results,
                  bool needles) {
  if (!counts || min_permille > 1000 || (n && limit && !results) || (n && !needles) || n > kMaxBatchNeedles) {
    errno = EINVAL;
    return -1;
  }
  return 0;
}

// The direct launch's device output for nd workgroups (zeroed: a needle's rows past its count read 0, as the sweep's do).
struct DirectOut {
  trigram_match rows;
  uint32_t *rntri, *counts;
  size_t rows_bytes, rn_bytes;
  int reserve(DeviceBuffer& b, size_t nd, uint16_t limit, hipStream_t stream) {
    rows_bytes = align_up(std::max<size_t>(nd * limit * sizeof(trigram_match_t), 16), 256);
    rn_bytes = align_up(std::max<size_t>(nd * limit * 4, 16), 256);
    const size_t bytes = rows_bytes + rn_bytes + align_up(nd * 4, 256);
    if (b.reserve(bytes, stream) < 0) return -1;
    unsigned char* p = static_cast<unsigned char*>(b.p);
    rows = reinterpret_cast<trigram_match>(p);
    rntri = reinterpret_cast<uint32_t*>(p + rows_bytes);
    counts = reinterpret_cast<uint32_t*>(p + rows_bytes + rn_bytes);
    BLURRILY_HIP_TRY(hipMemsetAsync(p, 0, bytes, stream));
    return 0;
  }
  // to host arrays of nd needles (waits for the stream)
  int read(size_t nd, uint16_t limit, trigram_match h_rows, uint32_t* h_counts, uint32_t* h_rntri, hipStream_t stream) const {
    BLURRILY_HIP_TRY(hipMemcpyAsync(h_counts, counts, nd * 4, hipMemcpyDeviceToHost, stream));
    BLURRILY_HIP_TRY(hipMemcpyAsync(h_rows, rows, nd * limit * sizeof(trigram_match_t), hipMemcpyDeviceToHost, stream));
    if (h_rntri) BLURRILY_HIP_TRY(hipMemcpyAsync(h_rntri, rntri, nd * limit * 4, hipMemcpyDeviceToHost, stream));
    BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }
};

// The planned each-in call, rows to host memory in the caller's order.
int similar_each_run(trigram_map m, const EachPlan& P, const EachNeedles& N, size_t n, uint16_t limit,
                     uint32_t min_permille, trigram_match results, uint32_t* counts, uint32_t* row_ntri,
                     SimilarScratch& S, hipStream_t stream) {
  const size_t nd = P.order.size(), ng = P.idx.size();
  if (limit == 0 || P.any_empty || (!nd && !ng)) std::memset(counts, 0, n * 4);
  if (limit == 0 || (!nd && !ng)) return 0;             // nothing serves any needle
  std::vector<trigram_match_t> h_rows;
  std::vector<uint32_t> h_counts, h_rntri;
  auto put_back = [&](size_t k, uint32_t q) {           // group-local needle k is the caller's q
    counts[q] = h_counts[k];
    std::memcpy(results + size_t(q) * limit, h_rows.data() + k * limit, size_t(limit) * sizeof(trigram_match_t));
    if (row_ntri) std::memcpy(row_ntri + size_t(q) * limit, h_rntri.data() + k * limit, size_t(limit) * 4);
  };
  auto host_room = [&](size_t k) {
    h_rows.resize(k * limit); h_counts.resize(k);
    if (row_ntri) h_rntri.resize(k * limit);
  };
  EachOnDevice D;
  if (D.upload(m, P, nullptr, 0, ng, false, stream) < 0) return -1;
  // every needle served directly: one launch
  if (nd) {
    DirectOut out;
    if (out.reserve(S.b[9], nd, limit, stream) < 0) return -1;
    ScopeSimilarArgs a{};
    N.into(a);
    a.order = D.d_order; a.scopes = D.d_table;
    a.n = uint32_t(nd); a.max_members = P.max_members; a.limit = limit; a.min_permille = min_permille;
    a.rows = out.rows; a.row_ntri = row_ntri ? out.rntri : nullptr; a.counts = out.counts;
    if (launch_scope_similar(a, stream) < 0) return -1;
    host_room(nd);
    if (out.read(nd, limit, h_rows.data(), h_counts.data(), row_ntri ? h_rntri.data() : nullptr, stream) < 0) return -1;
    for (size_t b = 0; b < nd; ++b) put_back(b, P.order[b].x);
  }
  // a sweep per group over its needles, compacted
  for (size_t g = 0; g < P.group_scope.size(); ++g) {
    SweptGroup G;
    if (G.gather(P, D, N.V, g, stream) < 0) return -1;
    host_room(G.cnt);
    if (similar_run(m, G.cnt, G.V, limit, min_permille, h_rows.data(), h_counts.data(),
                    row_ntri ? h_rntri.data() : nullptr, stream, S, G.masks.ptr()) < 0)
      return -1;
    for (size_t k = 0; k < G.cnt; ++k) put_back(k, P.idx[G.k0 + k]);
  }
  return 0;
}

}  // namespace

extern "C" {

int blurrily_storage_find_batch_similar_in(trigram_map m, blurrily_scope sc, const char* packed, const uint64_t* offsets,
                                           size_t n, uint16_t limit, uint32_t min_permille, trigram_match results,
                                           uint32_t* counts, uint32_t* row_ntri) {
  if (scope_check(m, sc) < 0 || similar_check(counts, min_permille, n, limit, results, packed && offsets) < 0) return -1;
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (scope_prepare(m, sc, stream) < 0) return -1;     // (without a GPU this is what fails, with ENODEV)
  if (n == 0) return 0;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();
  if (limit == 0 || sc->n_held == 0) { std::memset(counts, 0, n * 4); return 0; }
  SimilarScratch S;
  if (scope_takes_direct(m, sc, limit)) {
    EachNeedles N;
    if (stage_direct_strings(packed, offsets, n, S.b[8], stream, &N) < 0) return -1;
    DirectOut out;
    if (out.reserve(S.b[9], n, limit, stream) < 0) return -1;
    ScopeSimilarArgs a{};
    N.into(a);
    a.one = direct_of(sc);
    a.n = uint32_t(n); a.max_members = sc->n_direct; a.limit = limit; a.min_permille = min_permille;
    a.rows = out.rows; a.row_ntri = row_ntri ? out.rntri : nullptr; a.counts = out.counts;
    if (launch_scope_similar(a, stream) < 0) return -1;
    return out.read(n, limit, results, counts, row_ntri, stream);
  }
  NeedleView N;
  if (stage_string_needles(m, packed, offsets, n, S.b[6], stream, &N) < 0) return -1;
  return similar_run(m, n, N, limit, min_permille, results, counts, row_ntri, stream, S, masks_of(sc).ptr());
}

int blurrily_storage_find_similar_in(trigram_map m, blurrily_scope sc, const char* needle, uint16_t limit,
                                     uint32_t min_permille, trigram_match results, uint32_t* row_ntri) {
  if (!needle) { errno = EINVAL; return -1; }
  const uint64_t offsets[2] = {0, std::strlen(needle)};
  uint32_t count = 0;
  if (blurrily_storage_find_batch_similar_in(m, sc, needle, offsets, 1, limit, min_permille, results, &count, row_ntri) < 0)
    return -1;
  return int(count);
}

int blurrily_storage_find_batch_similar_each_in(trigram_map m, const blurrily_scope* scopes, size_t n_scopes,
                                                const uint32_t* which, const char* packed, const uint64_t* offsets,
                                                size_t n, uint16_t limit, uint32_t min_permille, trigram_match results,
                                                uint32_t* counts, uint32_t* row_ntri) {
  if (each_check(m, scopes, n_scopes) < 0 ||
      similar_check(counts, min_permille, n, limit, results, which && packed && offsets) < 0 ||
      each_check_which(which, n, n_scopes) < 0)
    return -1;
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  if (n == 0) return 0;
  m->last_kernels.clear();
  if (limit == 0) { std::memset(counts, 0, n * 4); return 0; }
  EachPlan P;
  if (each_plan(m, scopes, n_scopes, which, n, limit, stream, &P) < 0) return -1;
  NameScope names(&m->last_kernels);                     // (the scopes' preparation is no part of the find)
  SimilarScratch S;
  EachNeedles N;
  if (stage_each_strings(m, P, packed, offsets, n, S.b[6], S.b[8], stream, &N) < 0) return -1;
  return similar_each_run(m, P, N, n, limit, min_permille, results, counts, row_ntri, S, stream);
}

int blurrily_storage_find_references_similar_each_in(trigram_map m, const blurrily_scope* scopes, size_t n_scopes,
                                                     const uint32_t* which, const uint32_t* references, size_t n,
                                                     uint16_t limit, uint32_t min_permille, trigram_match results,
                                                     uint32_t* counts, uint32_t* row_ntri, uint32_t* nb_trigrams) {
  if (each_check(m, scopes, n_scopes) < 0 ||
      similar_check(counts, min_permille, n, limit, results, which && references) < 0 ||
      each_check_which(which, n, n_scopes) < 0)
    return -1;
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  if (n == 0) return 0;
  m->last_kernels.clear();
  EachPlan P;
  if (limit && each_plan(m, scopes, n_scopes, which, n, limit, stream, &P) < 0) return -1;
  SimilarScratch S;
  EachNeedles N;                                         // (after every scope's preparation: both use ws_refs)
  if (stage_reference_needles(m, references, n, S.b[6], stream, nb_trigrams, &N.V) < 0) return -1;
  NameScope names(&m->last_kernels);                     // (the preparation and the extraction are no part of the find)
  return similar_each_run(m, P, N, n, limit, min_permille, results, counts, row_ntri, S, stream);
}

}  // extern "C"
