// cluster_within.hip -- blurrily_storage_cluster_within (include/blurrily_storage.h):
// blurrily_storage_cluster's components within caller-given blocks, one call for all blocks.  The call sequence is
// ClusterCall's (cluster_host.h) over a numbering made here, before a GPU is asked for, because the numbering is where a
// reference listed under two keys shows.  On top of it: each number's key on the device, and the plan -- the numbers
// sorted by (key, number), every block given to one of two kernels (cluster_within_kernels.hip): the direct kernel's
// tiles for a block of at most kClusterWithinDirectMax listed members, the sweep's needle list for a larger one.  Both
// unite in the one forest; the node tables and the labels are cluster_kernels.hip's kernels as they are.
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

namespace {

// The listed members of a block up to which "scope_strategy" 0 scores the block directly.  Direct work grows with the
// square of a block, the sweep's with the map: on configs[2]'s haystack at 700 per mille, one block of 10^5 consecutive
// references takes the direct kernel 16 ms against the sweep's 170 ms, one of 10^6 1.96 s against 1.72 s
// (profiles/cluster_within_geonames.json).  This is the largest size measured at which direct was no slower.
// "scope_strategy" 1 sweeps every block, 2 scores every block directly.
constexpr size_t kClusterWithinDirectMax = 100000;

}  // namespace

extern "C" int blurrily_storage_cluster_within(trigram_map m, const uint32_t* references, const uint32_t* blocks, size_t n,
                                               uint32_t min_permille, uint32_t* labels, uint32_t* n_clusters,
                                               uint64_t* n_edges) {
  if (!m || min_permille > 1000 || (n && (!references || !blocks || !labels)) || n > kMaxBatchNeedles) {
    errno = EINVAL;
    return -1;
  }
  std::vector<uint32_t> uniq, inv, key_of;
  if (n && !number_nodes_keyed(references, blocks, n, uniq, inv, key_of)) {
    errno = EINVAL;                                           // a reference listed under two keys
    return -1;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  if (n_clusters) *n_clusters = 0;
  if (n_edges) *n_edges = 0;
  if (n == 0) return 0;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  // the plan: the numbers block after block, ascending inside a block (keys that ascend with the numbers already are)
  const size_t nu = uniq.size();
  std::vector<uint32_t> order(nu);
  if (std::is_sorted(key_of.begin(), key_of.end())) {
    for (size_t u = 0; u < nu; ++u) order[u] = uint32_t(u);
  } else {
    std::vector<uint64_t> keyed(nu);
    for (size_t u = 0; u < nu; ++u) keyed[u] = (uint64_t(key_of[u]) << 32) | u;
    std::sort(keyed.begin(), keyed.end());
    for (size_t u = 0; u < nu; ++u) order[u] = uint32_t(keyed[u]);
  }
  std::vector<ClusterWithinTile> tiles;
  std::vector<uint32_t> swept;
  for (size_t b = 0; b < nu;) {
    size_t e = b + 1;
    while (e < nu && key_of[order[e]] == key_of[order[b]]) ++e;
    const bool direct = m->scope_strategy == 2 || (m->scope_strategy == 0 && e - b <= kClusterWithinDirectMax);
    if (!direct) {
      swept.insert(swept.end(), order.begin() + b, order.begin() + e);
    } else if (e - b > 1) {                                   // (a block of one has no pair to score)
      for (size_t f = b; f < e; f += kClusterWithinTile)
        tiles.push_back({uint32_t(b), uint32_t(f), uint32_t(std::min<size_t>(kClusterWithinTile, e - f))});
    }
    b = e;
  }
  // the tiles that pass over the most members first: the longest workgroups do not start last
  // (equal ones in the plan's order)
  if (tiles.size() > 0x7FFFFFFFull) { errno = EINVAL; return -1; }
  {
    std::vector<uint64_t> by_scan(tiles.size());
    for (size_t t = 0; t < tiles.size(); ++t)
      by_scan[t] = (uint64_t(~(tiles[t].first + tiles[t].count - tiles[t].begin)) << 32) | t;
    std::sort(by_scan.begin(), by_scan.end());
    std::vector<ClusterWithinTile> sorted(tiles.size());
    for (size_t t = 0; t < tiles.size(); ++t) sorted[t] = tiles[uint32_t(by_scan[t])];
    tiles.swap(sorted);
  }

  ClusterCall c(m, stream);
  if (c.begin(std::move(uniq), std::move(inv), n, 1, sizeof(ClusterTotals)) < 0) return -1;
  ClusterTotals* d_totals = static_cast<ClusterTotals*>(c.d_totals);
  uint32_t *d_block_of = nullptr, *d_order = nullptr, *d_swept = nullptr;
  ClusterWithinTile* d_tiles = nullptr;
  if (c.more(d_tiles, tiles.size() * sizeof(ClusterWithinTile)) < 0 || c.more(d_swept, swept.size() * 4) < 0 ||
      (!tiles.empty() && c.more(d_order, nu * 4) < 0) || (!swept.empty() && c.more(d_block_of, nu * 4) < 0))
    return -1;
  if (d_tiles) {
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(ClusterWithinTile), hipMemcpyHostToDevice, stream));
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_order, order.data(), nu * 4, hipMemcpyHostToDevice, stream));
  }
  if (d_swept) {
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_swept, swept.data(), swept.size() * 4, hipMemcpyHostToDevice, stream));
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_block_of, key_of.data(), nu * 4, hipMemcpyHostToDevice, stream));
  }

  // the large blocks over the images (windows_per_workgroup by their members' number, not the numbering's) ...
  if (c.sweep(swept.size(), min_permille, d_totals, [&](const ClusterSweepArgs& a) {
        return launch_cluster_within_sweep({a, d_swept, d_block_of}, stream);
      }) < 0)
    return -1;
  // ... and the small ones from the extraction's codes, into the same forest
  ClusterWithinArgs wa{d_tiles, d_order, uint32_t(tiles.size()), uint32_t(nu), c.x.needles.codes, c.x.needles.qoff,
                       c.x.needles.ntri, uint32_t(nu), min_permille, c.d_parent, d_totals};
  if (launch_cluster_within(wa, stream) < 0) return -1;

  if (launch_cluster_label(c.label_args(), stream) < 0) return -1;
  ClusterTotals totals{};
  if (c.read_totals(&totals) < 0 || c.wait(&totals) < 0) return -1;   // (the labels are copied out only on success)
  BLURRILY_HIP_TRY(hipMemcpyAsync(labels, c.d_labels, n * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  if (n_clusters) *n_clusters = totals.clusters;
  if (n_edges) *n_edges = totals.edges;
  return 0;
}
