// cluster_tree.hip -- blurrily_storage_cluster_tree (include/blurrily_storage.h): the maximum
// spanning forest of blurrily_storage_cluster's edges with heights in whole per mille -- the single-linkage dendrogram --
// by Boruvka rounds on the device.  The call sequence is ClusterCall's (cluster_host.h) with one forest; a round is one
// sweep over every image and chunk (cluster_tree_kernels.hip's, which chooses the best edge leaving each component),
// the merge, the flatten and four bytes read back: the merges so far.  A round that adds none was the last.
#include <algorithm>
#include <vector>

#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

static_assert(kTreeMaxNodes == BLURRILY_CLUSTER_TREE_MAX, "the header's cap is the key's");
static_assert(sizeof(ClusterTreeMerge) == sizeof(blurrily_cluster_merge_t) && sizeof(ClusterTreeMerge) == 12,
              "the kernels' record is the header's");

extern "C" int blurrily_storage_cluster_tree(trigram_map m, const uint32_t* references, size_t n, uint32_t min_permille,
                                             uint32_t* labels, blurrily_cluster_merge_t* merges, uint32_t* n_merges,
                                             uint32_t* n_clusters, uint64_t* n_edges) {
  if (!m || min_permille > 1000 || (n && (!references || !labels || !merges)) || n > kTreeMaxNodes) {
    errno = EINVAL;
    return -1;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  if (n_merges) *n_merges = 0;
  if (n_clusters) *n_clusters = 0;
  if (n_edges) *n_edges = 0;
  if (n == 0) return 0;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  ClusterCall c(m, stream);
  if (c.begin(references, n, 1, sizeof(ClusterTotals)) < 0) return -1;
  ClusterTotals* d_totals = static_cast<ClusterTotals*>(c.d_totals);
  const size_t nu = c.nu;
  ClusterTreeRoundArgs r{};
  uint32_t* d_counters = nullptr;                             // [0]: the merges so far
  if (c.more(r.best, nu * 8, true) < 0 || c.more(r.comp, nu * 4) < 0 || c.more(r.closed, nu, true) < 0 ||
      c.more(r.merges, nu * sizeof(ClusterTreeMerge)) < 0 || c.more(d_counters, 16, true) < 0)
    return -1;
  r.parent = c.d_parent; r.refs = c.d_refs; r.n_nodes = uint32_t(nu); r.n_merges = d_counters; r.totals = d_totals;
  if (launch_cluster_tree_flatten(r, stream) < 0) return -1;  // (every number its own component)

  uint32_t found = 0;
  bool done = false;
  for (uint32_t round = 1; round <= kTreeMaxRounds && !done; ++round) {
    auto launch = [&](const ClusterSweepArgs& a) {
      return launch_cluster_tree_sweep(ClusterTreeSweepArgs{a, r.comp, r.closed, r.best, round}, stream);
    };
    if (c.sweep(nu, min_permille, d_totals, launch) < 0) return -1;
    if (launch_cluster_tree_merge(r, stream) < 0 || launch_cluster_tree_flatten(r, stream) < 0) return -1;
    uint32_t now = 0;
    BLURRILY_HIP_TRY(hipMemcpyAsync(&now, d_counters, 4, hipMemcpyDeviceToHost, stream));
    BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
    done = now == found;
    found = now;
  }
  if (!done || found >= nu) { errno = EIO; return -1; }       // (the round bound ran out; a forest has fewer edges than nodes)

  if (launch_cluster_label(c.label_args(), stream) < 0) return -1;
  ClusterTotals totals{};
  if (c.read_totals(&totals) < 0) return -1;
  std::vector<ClusterTreeMerge> got(found);
  if (found)
    BLURRILY_HIP_TRY(hipMemcpyAsync(got.data(), r.merges, found * sizeof(ClusterTreeMerge), hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipMemcpyAsync(labels, c.d_labels, n * 4, hipMemcpyDeviceToHost, stream));
  if (c.wait(&totals) < 0) return -1;
  sort_tree_records(got);
  for (uint32_t i = 0; i < found; ++i) merges[i] = {got[i].a, got[i].b, got[i].permille};
  if (n_merges) *n_merges = found;
  if (n_clusters) *n_clusters = totals.clusters;
  if (n_edges) *n_edges = totals.edges;
  return 0;
}
