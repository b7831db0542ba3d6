// scope_internal.h -- the scope object and what scope.hip (its preparation, the scope-per-needle plan, the plain entries),
// scope_similar.hip and scope_above.hip (the scoped similarity and threshold finds) share; no one else includes it.
#pragma once
#include "map_internal.h"
#include "scope_similar.h"

// A scope keeps its references sorted and distinct.  Its device state is made at the first scoped find and whenever
// the map has changed since (base_builds, log_version): the members are looked up and extracted as by reference
// (refs_extract), a mask per image excludes every rank but the members held now, and -- for scopes the direct strategy
// may serve -- the held members' codes, weights and references in (weight, reference) order are copied into the
// scope's own buffers (ws_refs is every later by-reference call's).
struct blurrily_scope_t {
  trigram_map           map = nullptr;
  std::vector<uint32_t> refs;           // sorted, distinct
  bool         ready = false;
  bool         mask_ready = false;       // (a scope prepared with others, by a scope-per-needle call, has no masks yet)
  uint64_t     built_base = 0, built_log = 0;
  uint32_t     n_held = 0;               // members held at the last preparation
  blurrily::detail::DeviceBuffer d_refs, d_mask[2];        // masks: base image, delta image (pending puts)
  bool         has_delta = false;
  // direct form (n_direct members: m_off [n_direct + 1] | m_ref | m_weight | m_codes)
  bool         direct = false;
  uint32_t     n_direct = 0;
  uint64_t     direct_codes = 0;
  blurrily::detail::DeviceBuffer d_direct;
  const uint32_t *m_off = nullptr, *m_ref = nullptr, *m_weight = nullptr;
  const uint16_t* m_codes = nullptr;
  __attribute__((visibility("hidden"))) ~blurrily_scope_t() = default;   // (its buffers go with it; not a dynamic symbol)
};

namespace blurrily {
namespace detail __attribute__((visibility("hidden"))) {

inline int scope_check(trigram_map m, blurrily_scope sc) {
  if (!m || !sc || sc->map != m) { errno = EINVAL; return -1; }
  return 0;
}
inline int each_check(trigram_map m, const blurrily_scope* scopes, size_t n_scopes) {
  if (!m || (n_scopes && !scopes)) { errno = EINVAL; return -1; }
  for (size_t j = 0; j < n_scopes; ++j)
    if (!scopes[j] || scopes[j]->map != m) { errno = EINVAL; return -1; }
  return 0;
}
inline int each_check_which(const uint32_t* which, size_t n, size_t n_scopes) {
  for (size_t i = 0; i < n; ++i)
    if (which[i] != BLURRILY_NO_SCOPE && which[i] >= n_scopes) { errno = EINVAL; return -1; }
  return 0;
}
// The scope's device state for the map as it is now (the image brought up to date and tombstones applied first): the
// direct form of this one scope, if it is stale, and its masks.
int scope_prepare(trigram_map m, blurrily_scope sc, hipStream_t stream);
// Which strategy serves a scoped find of `limit` (the scope prepared): the direct one declines limits above its pool and
// scopes without a direct form (above kScopeMaxMembers held members, or a member of more than 255 distinct trigrams);
// auto takes it for scopes of at most "scope_direct_max" member codes.
bool scope_takes_direct(const trigram_map_t* m, const blurrily_scope_t* sc, uint16_t limit);

// A prepared scope as the launches take it: a sweep's masks (ptr(): null for the NO_SCOPE group's), the direct form.
struct ScopeMasksOf : ScopeMasks {
  bool scoped;
  const ScopeMasks* ptr() const { return scoped ? this : nullptr; }
};
inline ScopeMasksOf masks_of(const blurrily_scope_t* sc) {
  return {ScopeMasks{sc ? static_cast<const uint32_t*>(sc->d_mask[0].p) : nullptr,
                     sc && sc->has_delta ? static_cast<const uint32_t*>(sc->d_mask[1].p) : nullptr}, sc != nullptr};
}
inline ScopeDirect direct_of(const blurrily_scope_t* sc) {
  return ScopeDirect{sc->m_off, sc->m_codes, sc->m_ref, sc->m_weight, sc->n_direct, 0u};
}

// Which launch serves each needle of a call.
struct EachPlan {
  std::vector<ScopeDirect>    table;         // the direct scopes' forms
  std::vector<uint2>          order;         // the direct needles {needle, table slot}: largest scopes first
  uint32_t                    max_members = 0;
  std::vector<uint32_t>       idx;           // the swept groups' needles, group after group
  std::vector<size_t>         group_start;   // [groups + 1]
  std::vector<blurrily_scope> group_scope;   // nullptr: the NO_SCOPE group
  bool                        any_empty = false;   // needles of a scope without rows (no held member, limit 0)
};
// Group the needles and prepare what serves them: the stale scopes together, then the masks of the scopes the mask
// serves.  (Every extraction of the call happens here, before the by-reference needles take ws_refs.)
int each_plan(trigram_map m, const blurrily_scope* scopes, size_t n_scopes, const uint32_t* which, size_t n,
              uint16_t limit, hipStream_t stream, EachPlan* P);

// The needles of a call: strings on the device (d_offsets set; h_offsets: the caller's offsets on the host, or nullptr:
// read back if the plain each-in sweeps a group) and / or code lists (V: references always; strings too where the
// similarity or threshold each-in sweeps a group).  rn: the plain each-in's references as run_find takes them.  into():
// the five leading fields of ScopeEachArgs / ScopeSimilarArgs / ScopeAboveArgs, the strings where the call has them.
struct EachNeedles {
  const char*       d_packed = nullptr;
  const uint64_t    *d_offsets = nullptr, *h_offsets = nullptr;
  NeedleView        V{};
  const RefNeedles* rn = nullptr;
  template <class Args> void into(Args& a) const {
    if (d_offsets) { a.packed = d_packed; a.offsets = d_offsets; }
    else { a.codes = V.codes; a.qoff = V.qoff; a.ntri = V.ntri; }
  }
};
// n host strings copied into `buf` as a host batch's in block, where a direct launch reads them ...
inline int stage_direct_strings(const char* packed, const uint64_t* offsets, size_t n, DeviceBuffer& buf,
                                hipStream_t stream, EachNeedles* N) {
  const BatchBlocks B(n, size_t(offsets[n]), 0, false);
  if (buf.reserve(B.in_bytes, stream) < 0) return -1;
  unsigned char* d_in = static_cast<unsigned char*>(buf.p);
  N->d_packed = B.in(d_in).packed; N->d_offsets = B.in(d_in).offsets;
  return B.copy_in(d_in, packed, offsets, stream);
}
// ... and a planned call's: tokenised into `swept` where a group is swept (the strings in front of the codes), copied
// into `direct` where the direct launch alone reads them, neither where nothing serves any needle (*N stays empty).
inline int stage_each_strings(trigram_map m, const EachPlan& P, const char* packed, const uint64_t* offsets, size_t n,
                              DeviceBuffer& swept, DeviceBuffer& direct, hipStream_t stream, EachNeedles* N) {
  if (P.idx.empty()) return P.order.empty() ? 0 : stage_direct_strings(packed, offsets, n, direct, stream, N);
  if (stage_string_needles(m, packed, offsets, n, swept, stream, &N->V) < 0) return -1;
  const BatchBlocks::In in = BatchBlocks(n, size_t(offsets[n]), 0, false).in(static_cast<unsigned char*>(swept.p));
  N->d_packed = in.packed; N->d_offsets = in.offsets;
  return 0;
}

// A call's plan on the device, in m->ws_each: table | order | idx | (goff), uploaded from m->h_each in one copy, then the
// device's own: (gpk) | gq | gn | (gw), the swept groups' gathered descriptors, n_desc entries each.  goff (the compacted
// strings' offsets, with gpk_bytes for the strings) and the weights are the plain each-in's.
struct EachOnDevice {
  const ScopeDirect* d_table;
  const uint2*       d_order;
  const uint32_t*    d_idx;
  const uint64_t*    d_goff;
  char*              d_gpk;
  uint64_t*          gq;
  uint32_t           *gn, *gw;
  int upload(trigram_map m, const EachPlan& P, const std::vector<uint64_t>* goff, size_t gpk_bytes, size_t n_desc,
             bool weights, hipStream_t stream);
};
// Group g of a plan as the similarity and threshold sweeps take it: its first needle in P.idx and its count, its
// scope's masks, and its needles' descriptors, gathered (one launch) behind the plan.
struct SweptGroup {
  size_t       k0, cnt;
  ScopeMasksOf masks;
  NeedleView   V;
  int gather(const EachPlan& P, const EachOnDevice& D, const NeedleView& all, size_t g, hipStream_t stream) {
    k0 = P.group_start[g]; cnt = P.group_start[g + 1] - k0;
    masks = masks_of(P.group_scope[g]);
    V = NeedleView{all.codes, D.gq + k0, D.gn + k0};
    return launch_scope_similar_gather(all.qoff, all.ntri, D.d_idx + k0, uint32_t(cnt), D.gq + k0, D.gn + k0, stream);
  }
};

}  // namespace detail
}  // namespace blurrily
