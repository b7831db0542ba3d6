// cluster_host.h -- what the clustering entries' translation units share on the host side (cluster.hip,
// cluster_levels.hip, cluster_centres.hip, cluster_cores.hip, cluster_extend.hip): a call's launch chunk, its device scratch and the node numbering.
#pragma once
#include <algorithm>
#include <vector>

#include "map_internal.h"

namespace blurrily {
namespace detail __attribute__((visibility("hidden"))) {

constexpr size_t kClusterChunkNeedles = size_t(1) << 20;   // needles per sweep launch (nothing else bounds a chunk)

// device scratch of one call, freed on the way out
struct ClusterScratch {
  DeviceBuffer refs, inv, node_of_pos, parent, labels, totals;
  ~ClusterScratch() { for (DeviceBuffer* b : {&refs, &inv, &node_of_pos, &parent, &labels, &totals}) b->release(); }
};

// The caller's references ascending without repeats (the node numbering), and each element's number.  A list that is
// strictly ascending already is its own numbering: inv stays empty.
inline void number_nodes(const uint32_t* references, size_t n, std::vector<uint32_t>& uniq, std::vector<uint32_t>& inv) {
  bool ascending = true;
  for (size_t i = 1; i < n && ascending; ++i) ascending = references[i - 1] < references[i];
  if (ascending) { uniq.assign(references, references + n); return; }
  std::vector<uint64_t> keyed(n);
  for (size_t i = 0; i < n; ++i) keyed[i] = (uint64_t(references[i]) << 32) | i;
  std::sort(keyed.begin(), keyed.end());
  inv.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t ref = uint32_t(keyed[i] >> 32);
    if (uniq.empty() || uniq.back() != ref) uniq.push_back(ref);
    inv[uint32_t(keyed[i])] = uint32_t(uniq.size() - 1);
  }
}

}  // namespace detail
}  // namespace blurrily
