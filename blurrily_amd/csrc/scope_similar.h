// scope_similar.h -- launch interface of the scoped similarity find's direct strategy (scope_similar_kernels.hip;
// DESIGN.md section 24): a needle's best `limit` rows by trigram Jaccard similarity among the members of a scope's
// direct form (find_kernels.h: ScopeDirect), scored member by member.  T, R, m, the row test and the order are the
// similarity find's (similar.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/blurrily_storage.h"
#include "find_kernels.h"

namespace blurrily {

// One workgroup per needle.  Workgroup b serves needle order[b].x with scope scopes[order[b].y]'s direct form -- or,
// with order == nullptr, needle b with `one` -- and writes its rows, best first, at rows + b * limit (row_ntri
// likewise, when given) and their number at counts[b]: the host puts an each-in call's rows back in the caller's order.
struct ScopeSimilarArgs {
  const char*        packed;       // the needles as strings (codes == nullptr) ...
  const uint64_t*    offsets;
  const uint16_t*    codes;        // ... or as extracted references (needle q's ntri[q] codes at codes + qoff[q] + q)
  const uint64_t*    qoff;
  const uint32_t*    ntri;
  const uint2*       order;        // [n] {needle, scope table slot}, or nullptr
  const ScopeDirect* scopes;
  ScopeDirect        one;
  uint32_t           n;            // workgroups
  uint32_t           max_members;  // the largest scope's members: a byte each of dynamic LDS
  uint32_t           limit;        // 1 .. kScopeMaxKeep
  uint32_t           min_permille;
  trigram_match_t*   rows;         // [n * limit]
  uint32_t*          row_ntri;     // [n * limit], or nullptr
  uint32_t*          counts;       // [n]
};
int launch_scope_similar(const ScopeSimilarArgs& a, hipStream_t stream);

// The needles of a group the sweep serves, compacted: descriptor k is needle idx[k]'s (codes + gq[k] + k: its codes,
// left where they are; qoff[q] + q >= k always, since idx ascends within a group).
int launch_scope_similar_gather(const uint64_t* qoff, const uint32_t* ntri, const uint32_t* idx, uint32_t n,
                                uint64_t* gq, uint32_t* gn, hipStream_t stream);

}  // namespace blurrily
