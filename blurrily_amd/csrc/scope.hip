// scope.hip -- scoped find and a scope per needle (blurrily_scope_*, blurrily_storage_find_in / _find_batch_in[_device],
// _find_batch_each_in[_device], _find_references_each_in; DESIGN.md sections 12 and 13), and what the scoped similarity
// and threshold finds (scope_similar.hip, scope_above.hip) share with them (scope_internal.h).
#include "scope_internal.h"

using namespace blurrily;
using namespace blurrily::detail;

// ---- scoped find (blurrily_scope_* / blurrily_storage_find_in / _find_batch_in[_device]) ---------
namespace {

constexpr size_t kScopePageBytes = size_t(1) << 16;   // small direct batches: needles in, rows out, through mapped memory

// The direct form from an extraction's readback, whose members [at, at + sc->refs.size()) are the scope's: the held
// ones (indices into sc->refs) in (weight, reference) order -- the rows' order among equal matches -- with their
// codes, copied to the device.
int scope_set_direct(blurrily_scope sc, std::vector<uint32_t>& held, const ExtractionOnHost& R, size_t at, uint64_t codes,
                     hipStream_t stream) {
  const uint32_t* ntri = R.ntri.data() + at;
  const uint32_t* wgt = R.weight.data() + at;
  std::sort(held.begin(), held.end(), [&](uint32_t a, uint32_t b) {
    return wgt[a] != wgt[b] ? wgt[a] < wgt[b] : sc->refs[a] < sc->refs[b];
  });
  const size_t nd = held.size();
  const size_t o_ref = align_up((nd + 1) * 4, 256), o_wgt = o_ref + align_up(nd * 4, 256);
  const size_t o_codes = o_wgt + align_up(nd * 4, 256), bytes = o_codes + std::max<size_t>(codes * 2, 16);
  std::vector<unsigned char> h(bytes, 0);
  uint32_t* off = reinterpret_cast<uint32_t*>(h.data());
  uint32_t* ref = reinterpret_cast<uint32_t*>(h.data() + o_ref);
  uint32_t* weight = reinterpret_cast<uint32_t*>(h.data() + o_wgt);
  uint16_t* cd = reinterpret_cast<uint16_t*>(h.data() + o_codes);
  off[0] = 0;
  for (size_t j = 0; j < nd; ++j) {
    const uint32_t i = held[j];
    std::memcpy(cd + off[j], R.codes_of(at + i), size_t(ntri[i]) * sizeof(uint16_t));
    off[j + 1] = off[j] + ntri[i];
    ref[j] = sc->refs[i];
    weight[j] = wgt[i];
  }
  if (sc->d_direct.reserve(bytes, stream) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemcpy(sc->d_direct.p, h.data(), bytes, hipMemcpyHostToDevice));
  unsigned char* d = static_cast<unsigned char*>(sc->d_direct.p);
  sc->m_off = reinterpret_cast<const uint32_t*>(d);
  sc->m_ref = reinterpret_cast<const uint32_t*>(d + o_ref);
  sc->m_weight = reinterpret_cast<const uint32_t*>(d + o_wgt);
  sc->m_codes = reinterpret_cast<const uint16_t*>(d + o_codes);
  sc->n_direct = uint32_t(nd);
  sc->direct_codes = codes;
  sc->direct = true;
  return 0;
}

// A scope's held count and -- when the direct strategy can serve the scope at all -- its direct form, from members
// [at, at + sc->refs.size()) of an extraction whose counts are on the host; the scope is then ready for the map as it
// is now (its masks apart).  The codes are read back here unless the caller has them already.
int scope_from_extraction(trigram_map m, blurrily_scope sc, ExtractionOnHost& R, size_t at, hipStream_t stream) {
  std::vector<uint32_t> held;
  uint64_t codes = 0;
  uint32_t widest = 0;
  for (size_t i = 0; i < sc->refs.size(); ++i)
    if (const uint32_t t = R.ntri[at + i]) { held.push_back(uint32_t(i)); codes += t; widest = std::max(widest, t); }
  sc->n_held = uint32_t(held.size());
  if (!held.empty() && held.size() <= kScopeMaxMembers && widest <= kScopeMaxMemberCodes &&
      (R.read_codes(stream) < 0 || scope_set_direct(sc, held, R, at, codes, stream) < 0))
    return -1;
  sc->built_base = m->base_builds;
  sc->built_log = log_of(m)->log_version;
  sc->ready = true;
  return 0;
}

// The direct form and the held count of every scope in `stale` for the map as it is now: their members uploaded and
// extracted as one list, read back once.  No masks: mask_ready stays false until scope_prepare builds them.
int scopes_prepare_direct(trigram_map m, const std::vector<blurrily_scope>& stale, hipStream_t stream) {
  if (stale.empty()) return 0;
  size_t n = 0;
  for (blurrily_scope sc : stale) {
    n += sc->refs.size();
    sc->ready = false; sc->mask_ready = false; sc->direct = false; sc->n_held = 0;
  }
  if (n > kMaxBatchNeedles) { errno = EINVAL; return -1; }
  ExtractionOnHost R(n);
  if (n) {
    std::vector<uint32_t> refs;
    refs.reserve(n);
    for (blurrily_scope sc : stale) refs.insert(refs.end(), sc->refs.begin(), sc->refs.end());
    if (m->ws_each.reserve(n * sizeof(uint32_t), stream) < 0) return -1;
    BLURRILY_HIP_TRY(hipMemcpyAsync(m->ws_each.p, refs.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    RefExtract x;
    if (refs_extract(m, static_cast<const uint32_t*>(m->ws_each.p), n, stream, &x) < 0) return -1;
    if (R.enqueue_counts(x, stream) < 0 || R.read_codes(stream) < 0) return -1;   // (one readback, whatever the scopes hold)
  }
  size_t at = 0;
  for (blurrily_scope sc : stale) {
    if (scope_from_extraction(m, sc, R, at, stream) < 0) return -1;
    at += sc->refs.size();
  }
  return 0;
}

}  // namespace

int blurrily::detail::scope_prepare(trigram_map m, blurrily_scope sc, hipStream_t stream) {
  if (map_ready(m, stream) < 0) return -1;
  if (sc->ready && sc->mask_ready && sc->built_base == m->base_builds && sc->built_log == log_of(m)->log_version)
    return 0;
  sc->ready = false;
  sc->mask_ready = false;
  sc->direct = false;
  sc->n_held = 0;
  const size_t n = sc->refs.size();
  const bool with_delta = !log_of(m)->pending.empty() && m->delta.device >= 0;
  const uint32_t words[2] = {(m->dev.n_refs + 31u) / 32u + 1u, with_delta ? (m->delta.n_refs + 31u) / 32u + 1u : 1u};
  for (int k = 0; k < 2; ++k)
    if (sc->d_mask[k].reserve(size_t(words[k]) * 4, stream) < 0) return -1;
  sc->has_delta = with_delta;
  ScopeMaskArgs ma{};
  ma.n_img = with_delta ? 2u : 1u;
  ma.win0[0] = 0; ma.win0[1] = m->dev.n_windows;
  ma.mask[0] = static_cast<uint32_t*>(sc->d_mask[0].p); ma.mask[1] = static_cast<uint32_t*>(sc->d_mask[1].p);
  ma.mask_words[0] = words[0]; ma.mask_words[1] = words[1];
  ExtractionOnHost R(n);
  if (n == 0) {
    if (launch_scope_mask(ma, stream) < 0) return -1;
  } else {
    if (sc->d_refs.reserve(n * sizeof(uint32_t), stream) < 0) return -1;
    BLURRILY_HIP_TRY(hipMemcpyAsync(sc->d_refs.p, sc->refs.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    RefExtract x;
    if (refs_extract(m, static_cast<const uint32_t*>(sc->d_refs.p), n, stream, &x) < 0) return -1;
    ma.loc = x.loc; ma.n = uint32_t(n);
    if (launch_scope_mask(ma, stream) < 0) return -1;
    // (the counts alone first: the offsets and the codes travel only if a direct form is possible)
    if (R.enqueue_counts(x, stream) < 0) return -1;
    BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  }
  if (scope_from_extraction(m, sc, R, 0, stream) < 0) return -1;
  sc->mask_ready = true;
  return 0;
}

bool blurrily::detail::scope_takes_direct(const trigram_map_t* m, const blurrily_scope_t* sc, uint16_t limit) {
  if (m->scope_strategy == 1 || !sc->direct || limit == 0 || limit > kScopeMaxKeep) return false;
  return m->scope_strategy == 2 || sc->direct_codes <= m->scope_direct_max;
}

namespace {

// Enqueue a scoped find of n device-resident needles on the prepared scope: rows of only its members.
int scope_run(trigram_map m, blurrily_scope sc, const char* d_packed, size_t packed_bytes, const uint64_t* d_offsets,
              size_t n, uint16_t limit, trigram_match d_results, uint32_t* d_counts, bool maybe_long, bool maybe_mid,
              hipStream_t stream) {
  if (n == 0) return 0;
  if (n > kMaxBatchNeedles) { errno = EINVAL; return -1; }
  const bool no_rows = sc->n_held == 0 || limit == 0;  // nothing in the scope is held
  if (no_rows || scope_takes_direct(m, sc, limit)) {
    NameScope name_scope(&m->last_kernels);
    m->last_kernels.clear();
    m->last_sweep = 0;
    if (no_rows) {
      BLURRILY_HIP_TRY(hipMemsetAsync(d_counts, 0, n * sizeof(uint32_t), stream));
      return 0;
    }
    const ScopeDirect d = direct_of(sc);
    const ScopeFindArgs a{d_packed, d_offsets, uint32_t(n), d.m_off, d.m_codes, d.m_ref, d.m_weight, d.n_members, limit,
                          d_results, d_counts};
    return launch_scope_find(a, stream);
  }
  return run_find(m, d_packed, packed_bytes, d_offsets, n, limit, d_results, d_counts, nullptr, maybe_long, maybe_mid,
                  stream, nullptr, masks_of(sc).ptr());
}

// The pinned page small direct batches go through (m->h_scope, mapped at m->d_scope), made at first use.
int scope_page(trigram_map m) {
  if (m->h_scope) return 0;
  HostPage h;
  unsigned char* d = nullptr;
  if (h.alloc(2 * kScopePageBytes, hipHostMallocMapped | hipHostMallocCoherent) < 0) return -1;
  BLURRILY_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&d), h, 0));
  m->h_scope = std::move(h); m->d_scope = d;
  return 0;
}

}  // namespace

extern "C" {

int blurrily_scope_new(trigram_map m, const uint32_t* references, size_t n, blurrily_scope* scope) {
  if (!m || !scope || (n && !references)) { errno = EINVAL; return -1; }
  blurrily_scope sc = new (std::nothrow) blurrily_scope_t();
  if (!sc) { errno = ENOMEM; return -1; }
  try {
    sc->refs.assign(references, references + n);
  } catch (const std::bad_alloc&) {
    delete sc;
    errno = ENOMEM;
    return -1;
  }
  std::sort(sc->refs.begin(), sc->refs.end());
  sc->refs.erase(std::unique(sc->refs.begin(), sc->refs.end()), sc->refs.end());
  sc->map = m;
  *scope = sc;
  return 0;
}

int blurrily_scope_close(blurrily_scope* scope) {
  if (!scope) { errno = EINVAL; return -1; }
  blurrily_scope sc = *scope;
  if (sc) {
    if (sc->d_refs.p || sc->d_mask[0].p || sc->d_mask[1].p || sc->d_direct.p) (void)hipDeviceSynchronize();
    delete sc;
  }
  *scope = nullptr;
  return 0;
}

int blurrily_scope_members(blurrily_scope scope, uint32_t* held) {
  if (!scope || !held || !scope->map) { errno = EINVAL; return -1; }
  uint32_t k = 0;
  for (uint32_t r : scope->refs) k += scope->map->host->holds(r) ? 1u : 0u;
  *held = k;
  return 0;
}

int blurrily_storage_find_batch_in_device(trigram_map m, blurrily_scope sc, const char* d_packed, size_t packed_bytes,
                                          const uint64_t* d_offsets, size_t n, uint16_t limit,
                                          trigram_match d_results, uint32_t* d_counts, void* stream) {
  if (scope_check(m, sc) < 0) return -1;
  DeviceScope scope(m->dev.device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (scope_prepare(m, sc, st) < 0) return -1;
  return scope_run(m, sc, d_packed, packed_bytes, d_offsets, n, limit, d_results, d_counts, true, true, st);
}

int blurrily_storage_find_batch_in(trigram_map m, blurrily_scope sc, const char* packed, const uint64_t* offsets,
                                   size_t n, uint16_t limit, trigram_match results, uint32_t* counts) {
  if (scope_check(m, sc) < 0) return -1;
  if (n && (!packed || !offsets || !counts || (limit && !results))) { errno = EINVAL; return -1; }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (scope_prepare(m, sc, stream) < 0) return -1;     // (without a GPU this is what fails, with ENODEV)
  if (n == 0) return 0;
  const size_t max_len = longest_needle(packed, offsets, n);
  const BatchBlocks B(n, size_t(offsets[n]), limit, false);
  // a small batch the direct strategy serves: needles read and rows written by the kernel in mapped pinned memory --
  // one launch, no copies
  if (B.in_bytes <= kScopePageBytes && B.out_bytes <= kScopePageBytes && sc->n_held && scope_takes_direct(m, sc, limit)) {
    if (scope_page(m) < 0) return -1;
    B.fill_in(m->h_scope, packed, offsets);
    const BatchBlocks::In in = B.in(m->d_scope);
    const BatchBlocks::Out out = B.out(m->d_scope + kScopePageBytes);
    if (scope_run(m, sc, in.packed, B.packed_bytes, in.offsets, n, limit, out.rows, out.counts, false, false, stream) < 0)
      return -1;
    BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
    B.take_out(B.out(m->h_scope + kScopePageBytes), counts, nullptr, results);
    return 0;
  }
  if (m->ws_io_in.reserve(B.in_bytes, stream) < 0 || m->ws_io_out.reserve(B.out_bytes, stream) < 0) return -1;
  unsigned char* d_in = static_cast<unsigned char*>(m->ws_io_in.p);
  const BatchBlocks::In in = B.in(d_in);
  const BatchBlocks::Out out = B.out(static_cast<unsigned char*>(m->ws_io_out.p));
  if (B.copy_in(d_in, packed, offsets, stream) < 0) return -1;
  if (scope_run(m, sc, in.packed, B.packed_bytes, in.offsets, n, limit, out.rows, out.counts, max_len > 126, max_len > 63,
                stream) < 0)
    return -1;
  return B.copy_out(out.counts, nullptr, out.rows, counts, nullptr, results, stream);
}

int blurrily_storage_find_in(trigram_map m, blurrily_scope sc, const char* needle, uint16_t limit, trigram_match results) {
  if (!needle) { errno = EINVAL; return -1; }
  const uint64_t offsets[2] = {0, std::strlen(needle)};
  uint32_t count = 0;
  if (blurrily_storage_find_batch_in(m, sc, needle, offsets, 1, limit, results, &count) < 0) return -1;
  return int(count);
}

}  // extern "C"

// ---- a scope per needle (blurrily_storage_find_batch_each_in[_device] / _find_references_each_in) -
// Needle i is a scoped find in scopes[which[i]], or a plain find for BLURRILY_NO_SCOPE.  The call groups the needles by
// what serves their scope: every needle the direct strategy serves, whatever its scope, goes into ONE launch of
// scope_each_kernel; each scope the mask serves gets one run_find over its needles, compacted, and so does the NO_SCOPE
// group (unscoped); a scatter puts their rows back in the caller's order.  The stale scopes of a call are prepared
// together (scopes_prepare_direct: one extraction of all their members, one readback); a scope's masks are built only
// when a call serves it through them (scope_prepare).
int blurrily::detail::each_plan(trigram_map m, const blurrily_scope* scopes, size_t n_scopes, const uint32_t* which,
                                size_t n, uint16_t limit, hipStream_t stream, EachPlan* P) {
  std::unordered_map<blurrily_scope, uint32_t> slot_of;    // the distinct scopes (a handle given twice is one)
  std::vector<blurrily_scope> uniq;
  std::vector<uint32_t> slot(n_scopes);
  for (size_t j = 0; j < n_scopes; ++j) {
    auto it = slot_of.emplace(scopes[j], uint32_t(uniq.size()));
    if (it.second) uniq.push_back(scopes[j]);
    slot[j] = it.first->second;
  }
  const uint32_t U = uint32_t(uniq.size());                // slot U: NO_SCOPE
  auto slot_at = [&](size_t i) { return which[i] == BLURRILY_NO_SCOPE ? U : slot[which[i]]; };
  std::vector<uint32_t> per(U + 1, 0);
  for (size_t i = 0; i < n; ++i) ++per[slot_at(i)];
  std::vector<blurrily_scope> stale;
  for (uint32_t u = 0; u < U; ++u) {
    const blurrily_scope sc = uniq[u];
    if (per[u] && !(sc->ready && sc->built_base == m->base_builds && sc->built_log == log_of(m)->log_version))
      stale.push_back(sc);
  }
  if (scopes_prepare_direct(m, stale, stream) < 0) return -1;
  // 0: no rows, 1: direct, 2: through its masks, 3: NO_SCOPE (unscoped)
  std::vector<uint8_t> kind(U + 1, 0);
  kind[U] = 3;
  for (uint32_t u = 0; u < U; ++u) {
    const blurrily_scope sc = uniq[u];
    if (!per[u]) continue;
    if (sc->n_held == 0 || limit == 0) { P->any_empty = true; continue; }
    if (scope_takes_direct(m, sc, limit)) { kind[u] = 1; continue; }
    if (scope_prepare(m, sc, stream) < 0) return -1;      // (builds the masks if this scope has none yet)
    kind[u] = 2;
  }
  std::vector<uint32_t> direct_u, dslot(U + 1, 0);
  for (uint32_t u = 0; u < U; ++u)
    if (kind[u] == 1) direct_u.push_back(u);
  std::stable_sort(direct_u.begin(), direct_u.end(),
                   [&](uint32_t a, uint32_t b) { return uniq[a]->n_direct > uniq[b]->n_direct; });
  std::vector<size_t> cursor(U + 1, 0);
  size_t nd = 0, ng = 0;
  for (uint32_t u : direct_u) {
    const blurrily_scope sc = uniq[u];
    dslot[u] = uint32_t(P->table.size());
    P->table.push_back(direct_of(sc));
    P->max_members = std::max(P->max_members, sc->n_direct);
    cursor[u] = nd;
    nd += per[u];
  }
  for (uint32_t u = 0; u <= U; ++u) {
    if (kind[u] < 2 || !per[u]) continue;
    P->group_start.push_back(ng);
    P->group_scope.push_back(u < U ? uniq[u] : nullptr);
    cursor[u] = ng;
    ng += per[u];
  }
  P->group_start.push_back(ng);
  P->order.resize(nd);
  P->idx.resize(ng);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t u = slot_at(i);
    if (kind[u] == 1) P->order[cursor[u]++] = make_uint2(uint32_t(i), dslot[u]);
    else if (kind[u] >= 2) P->idx[cursor[u]++] = uint32_t(i);
  }
  return 0;
}

int EachOnDevice::upload(trigram_map m, const EachPlan& P, const std::vector<uint64_t>* goff, size_t gpk_bytes,
                         size_t n_desc, bool weights, hipStream_t stream) {
  const size_t nd = P.order.size(), ng = P.idx.size();
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t here = at; at += align_up(std::max<size_t>(bytes, 8), 256); return here; };
  const size_t o_tab = take(P.table.size() * sizeof(ScopeDirect)), o_ord = take(nd * sizeof(uint2));
  const size_t o_idx = take(ng * 4), o_goff = goff ? take(goff->size() * 8) : 0, up = at;
  const size_t o_gpk = goff ? take(gpk_bytes) : 0, o_gq = take(n_desc * 8), o_gn = take(n_desc * 4);
  const size_t o_gw = weights ? take(n_desc * 4) : 0;
  m->h_each.assign(up, 0);                               // (kept: the copy reads it after this returns)
  unsigned char* h = m->h_each.data();
  if (!P.table.empty()) std::memcpy(h + o_tab, P.table.data(), P.table.size() * sizeof(ScopeDirect));
  if (nd) std::memcpy(h + o_ord, P.order.data(), nd * sizeof(uint2));
  if (ng) std::memcpy(h + o_idx, P.idx.data(), ng * 4);
  if (goff && !goff->empty()) std::memcpy(h + o_goff, goff->data(), goff->size() * 8);
  if (m->ws_each.reserve(at, stream) < 0) return -1;
  unsigned char* d = static_cast<unsigned char*>(m->ws_each.p);
  BLURRILY_HIP_TRY(hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, stream));
  d_table = reinterpret_cast<const ScopeDirect*>(d + o_tab); d_order = reinterpret_cast<const uint2*>(d + o_ord);
  d_idx = reinterpret_cast<const uint32_t*>(d + o_idx); d_goff = reinterpret_cast<const uint64_t*>(d + o_goff);
  d_gpk = reinterpret_cast<char*>(d + o_gpk); gq = reinterpret_cast<uint64_t*>(d + o_gq);
  gn = reinterpret_cast<uint32_t*>(d + o_gn); gw = reinterpret_cast<uint32_t*>(d + o_gw);
  return 0;
}

namespace {

int each_launch_direct(const EachPlan& P, const EachNeedles& N, const ScopeDirect* d_table, const uint2* d_order,
                       uint16_t limit, trigram_match d_results, uint32_t* d_counts, hipStream_t stream) {
  ScopeEachArgs a{};
  N.into(a);
  a.order = d_order; a.n = uint32_t(P.order.size()); a.scopes = d_table; a.max_members = P.max_members;
  a.limit = limit; a.results = d_results; a.counts = d_counts;
  return launch_scope_each(a, stream);
}

// Enqueue the planned call on `stream`: rows and counts of needle i at d_results + i * limit, d_counts[i].
// last_kernels: every find kernel the call launched.
int each_run(trigram_map m, const EachPlan& P, const EachNeedles& N, size_t n, uint16_t limit, trigram_match d_results,
             uint32_t* d_counts, bool maybe_long, bool maybe_mid, hipStream_t stream) {
  std::string names;
  const size_t nd = P.order.size(), ng = P.idx.size();
  if (P.any_empty) BLURRILY_HIP_TRY(hipMemsetAsync(d_counts, 0, n * sizeof(uint32_t), stream));
  // the swept groups' strings: where each lands when compacted
  std::vector<uint64_t> goff, off_back;
  if (ng && !N.rn) {
    const uint64_t* off = N.h_offsets;
    if (!off) {
      off_back.resize(n + 1);
      BLURRILY_HIP_TRY(hipMemcpyAsync(off_back.data(), N.d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, stream));
      BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
      off = off_back.data();
    }
    goff.resize(ng + 1);
    goff[0] = 0;
    for (size_t k = 0; k < ng; ++k) goff[k + 1] = goff[k] + (off[P.idx[k] + 1] - off[P.idx[k]]);
  }
  // one upload (table | order | idx | compacted offsets), then the device's own: compacted strings or descriptors
  EachOnDevice D;
  if (D.upload(m, P, &goff, goff.empty() ? 0 : goff[ng], N.rn ? ng : 0, true, stream) < 0) return -1;
  // every needle served directly: one launch
  if (nd) {
    NameScope name_scope(&names);
    if (each_launch_direct(P, N, D.d_table, D.d_order, limit, d_results, d_counts, stream) < 0) return -1;
  }
  if (ng) {
    const size_t row_bytes = align_up(std::max<size_t>(ng * size_t(limit) * sizeof(trigram_match_t), 16), 256);
    if (m->ws_each_rows.reserve(row_bytes + ng * 4, stream) < 0) return -1;
    trigram_match g_rows = static_cast<trigram_match>(m->ws_each_rows.p);
    uint32_t* g_counts = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(m->ws_each_rows.p) + row_bytes);
    if (!N.rn && launch_scope_gather_strings(N.d_packed, N.d_offsets, D.d_idx, D.d_goff, uint32_t(ng), D.d_gpk, stream) < 0)
      return -1;
    for (size_t g = 0; g < P.group_scope.size(); ++g) {
      const size_t k0 = P.group_start[g], cnt = P.group_start[g + 1] - k0;
      const ScopeMasksOf sm = masks_of(P.group_scope[g]);
      RefNeedles rg{};
      if (N.rn) {
        if (launch_scope_gather_refs(*N.rn, D.d_idx + k0, uint32_t(cnt), D.gq + k0, D.gn + k0, D.gw + k0, stream) < 0)
          return -1;
        rg = RefNeedles{N.rn->codes, D.gq + k0, D.gn + k0, D.gw + k0, uint32_t(cnt), N.rn->code_slots};
      }
      if (run_find(m, N.rn ? nullptr : D.d_gpk, N.rn ? 0 : size_t(goff[ng]), N.rn ? nullptr : D.d_goff + k0, cnt, limit,
                   g_rows + k0 * limit, g_counts + k0, nullptr, maybe_long, maybe_mid, stream, N.rn ? &rg : nullptr,
                   sm.ptr()) < 0)
        return -1;
      NameScope name_scope(&names);                      // (what that run noted in last_kernels, in launch order)
      for (size_t b = 0, e; b < m->last_kernels.size(); b = e + 1) {
        e = m->last_kernels.find('+', b);
        if (e == std::string::npos) e = m->last_kernels.size();
        note_launch(m->last_kernels.substr(b, e - b).c_str());
      }
    }
    if (launch_scope_scatter(g_rows, g_counts, D.d_idx, uint32_t(ng), limit, d_results, d_counts, stream) < 0) return -1;
  }
  m->last_kernels = names;
  return 0;
}

}  // namespace

extern "C" {

int blurrily_storage_find_batch_each_in_device(trigram_map m, const blurrily_scope* scopes, size_t n_scopes,
                                               const uint32_t* d_which, const char* d_packed, size_t packed_bytes,
                                               const uint64_t* d_offsets, size_t n, uint16_t limit,
                                               trigram_match d_results, uint32_t* d_counts, void* stream) {
  (void)packed_bytes;
  if (each_check(m, scopes, n_scopes) < 0) return -1;
  if (n && (!d_which || !d_offsets || !d_counts || (limit && !d_results))) { errno = EINVAL; return -1; }
  if (n > kMaxBatchNeedles) { errno = EINVAL; return -1; }
  DeviceScope scope(m->dev.device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (map_ready(m, st) < 0) return -1;
  if (n == 0) return 0;
  std::vector<uint32_t> which(n);                        // (read back to group the needles: the call waits for it)
  BLURRILY_HIP_TRY(hipMemcpyAsync(which.data(), d_which, n * 4, hipMemcpyDeviceToHost, st));
  BLURRILY_HIP_TRY(hipStreamSynchronize(st));
  if (each_check_which(which.data(), n, n_scopes) < 0) return -1;
  EachPlan P;
  if (each_plan(m, scopes, n_scopes, which.data(), n, limit, st, &P) < 0) return -1;
  EachNeedles N;
  N.d_packed = d_packed; N.d_offsets = d_offsets;
  return each_run(m, P, N, n, limit, d_results, d_counts, true, true, st);
}

int blurrily_storage_find_batch_each_in(trigram_map m, const blurrily_scope* scopes, size_t n_scopes,
                                        const uint32_t* which, const char* packed, const uint64_t* offsets, size_t n,
                                        uint16_t limit, trigram_match results, uint32_t* counts) {
  if (each_check(m, scopes, n_scopes) < 0) return -1;
  if (n && (!which || !packed || !offsets || !counts || (limit && !results))) { errno = EINVAL; return -1; }
  if (n > kMaxBatchNeedles) { errno = EINVAL; return -1; }
  if (each_check_which(which, n, n_scopes) < 0) return -1;
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  if (n == 0) return 0;
  EachPlan P;
  if (each_plan(m, scopes, n_scopes, which, n, limit, stream, &P) < 0) return -1;
  const size_t max_len = longest_needle(packed, offsets, n);
  const BatchBlocks B(n, size_t(offsets[n]), limit, false);
  // (the page carries the scope table and the order behind the needles)
  const size_t o_tab = align_up(B.in_bytes, 256), o_ord = o_tab + align_up(P.table.size() * sizeof(ScopeDirect) + 8, 256);
  const size_t page_in = o_ord + P.order.size() * sizeof(uint2);
  // a small batch served directly alone: needles, scope table and order read, rows written, in mapped pinned memory --
  // one launch, no copies
  if (P.idx.empty() && !P.order.empty() && page_in <= kScopePageBytes && B.out_bytes <= kScopePageBytes) {
    if (scope_page(m) < 0) return -1;
    unsigned char* h_in = m->h_scope;
    const BatchBlocks::Out h_out = B.out(m->h_scope + kScopePageBytes);
    B.fill_in(h_in, packed, offsets);
    std::memcpy(h_in + o_tab, P.table.data(), P.table.size() * sizeof(ScopeDirect));
    std::memcpy(h_in + o_ord, P.order.data(), P.order.size() * sizeof(uint2));
    unsigned char* d_in = m->d_scope;
    const BatchBlocks::Out out = B.out(m->d_scope + kScopePageBytes);
    if (P.any_empty) std::memset(h_out.counts, 0, B.cnt_bytes);
    EachNeedles N;
    N.d_packed = B.in(d_in).packed; N.d_offsets = B.in(d_in).offsets;
    NameScope name_scope(&m->last_kernels);
    m->last_kernels.clear();
    if (each_launch_direct(P, N, reinterpret_cast<const ScopeDirect*>(d_in + o_tab),
                           reinterpret_cast<const uint2*>(d_in + o_ord), limit, out.rows, out.counts, stream) < 0)
      return -1;
    BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
    B.take_out(h_out, counts, nullptr, results);
    return 0;
  }
  if (m->ws_io_in.reserve(B.in_bytes, stream) < 0 || m->ws_io_out.reserve(B.out_bytes, stream) < 0) return -1;
  unsigned char* d_in = static_cast<unsigned char*>(m->ws_io_in.p);
  const BatchBlocks::Out out = B.out(static_cast<unsigned char*>(m->ws_io_out.p));
  if (B.copy_in(d_in, packed, offsets, stream) < 0) return -1;
  EachNeedles N;
  N.d_packed = B.in(d_in).packed; N.d_offsets = B.in(d_in).offsets;
  N.h_offsets = offsets;
  if (each_run(m, P, N, n, limit, out.rows, out.counts, max_len > 126, max_len > 63, stream) < 0) return -1;
  return B.copy_out(out.counts, nullptr, out.rows, counts, nullptr, results, stream);
}

int blurrily_storage_find_references_each_in(trigram_map m, const blurrily_scope* scopes, size_t n_scopes,
                                             const uint32_t* which, const uint32_t* references, size_t n,
                                             uint16_t limit, trigram_match results, uint32_t* counts,
                                             uint32_t* nb_trigrams) {
  if (each_check(m, scopes, n_scopes) < 0) return -1;
  if (n && (!which || !references || !counts || (limit && !results))) { errno = EINVAL; return -1; }
  if (n > kMaxBatchNeedles) { errno = EINVAL; return -1; }
  if (each_check_which(which, n, n_scopes) < 0) return -1;
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  if (n == 0) return 0;
  EachPlan P;
  if (each_plan(m, scopes, n_scopes, which, n, limit, stream, &P) < 0) return -1;
  const BatchBlocks B(n, 0, limit, false);               // (the references go in alone; out: [counts | rows])
  if (m->ws_io_in.reserve(n * sizeof(uint32_t), stream) < 0 || m->ws_io_out.reserve(B.out_bytes, stream) < 0) return -1;
  const BatchBlocks::Out out = B.out(static_cast<unsigned char*>(m->ws_io_out.p));
  BLURRILY_HIP_TRY(hipMemcpyAsync(m->ws_io_in.p, references, n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  RefExtract x;                                          // (after every scope's preparation: both use ws_refs)
  if (refs_extract(m, static_cast<const uint32_t*>(m->ws_io_in.p), n, stream, &x) < 0) return -1;
  EachNeedles N;
  N.rn = &x.needles; N.V = NeedleView{x.needles.codes, x.needles.qoff, x.needles.ntri};
  if (each_run(m, P, N, n, limit, out.rows, out.counts, true, true, stream) < 0) return -1;
  return B.copy_out(out.counts, x.needles.ntri, out.rows, counts, nb_trigrams, results, stream);   // (the counts of trigrams: the extraction's own)
}

}  // extern "C"
