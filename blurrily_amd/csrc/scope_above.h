// scope_above.h -- launch interface of the scoped threshold find's direct strategy (scope_above_kernels.hip; DESIGN.md
// section 27): every member of a scope's direct form (find_kernels.h: ScopeDirect) with at least the needle's bar of
// matches, in the threshold find's order, scored member by member.  T, the bar and the order are the threshold find's
// (above.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/blurrily_storage.h"
#include "find_kernels.h"

namespace blurrily {

// One workgroup per needle.  Workgroup b is job j = first + b: needle order[j].x with scope scopes[order[j].y]'s direct
// form -- or, with order == nullptr, needle j with `one`.
//   Count launch (seg == nullptr): counts[j] = the needle's rows.
//   Emit launch: the rows, in result order, at rows + seg[b] .. -- counts[j] of them, what the count launch found
//   (jobs without rows end at once).
struct ScopeAboveArgs {
  const char*        packed;       // the needles as strings (codes == nullptr) ...
  const uint64_t*    offsets;
  const uint16_t*    codes;        // ... or as extracted references (needle q's ntri[q] codes at codes + qoff[q] + q)
  const uint64_t*    qoff;
  const uint32_t*    ntri;
  const uint2*       order;        // [jobs] {needle, scope table slot}, or nullptr
  const ScopeDirect* scopes;
  ScopeDirect        one;
  uint32_t           first;        // the launch's first job
  uint32_t           n;            // workgroups
  uint32_t           max_members;  // the largest scope's members: a byte each of dynamic LDS
  uint32_t           min_matches;
  uint32_t           min_permille;
  uint32_t*          counts;       // [jobs]
  const uint32_t*    seg;          // [n] where each workgroup's rows start, or nullptr: count
  trigram_match_t*   rows;
};
int launch_scope_above(const ScopeAboveArgs& a, hipStream_t stream);

}  // namespace blurrily
