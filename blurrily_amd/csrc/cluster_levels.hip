// cluster_levels.hip -- blurrily_storage_cluster_levels (include/blurrily_storage.h): the
// clusters of blurrily_storage_cluster at up to kClusterMaxLevels floors from one sweep at the lowest of them.  The
// call sequence is ClusterCall's (cluster_host.h), with a forest, a row of labels and a ClusterTotals per level; the
// sweep is cluster_levels_kernels.hip's, the node tables and the labels are cluster_kernels.hip's kernels once per level.
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

static_assert(kClusterMaxLevels == BLURRILY_CLUSTER_MAX_LEVELS, "the header's cap is the kernels'");

extern "C" int blurrily_storage_cluster_levels(trigram_map m, const uint32_t* references, size_t n,
                                               const uint32_t* floors, uint32_t n_floors, uint32_t* labels,
                                               uint32_t* n_clusters, uint64_t* n_edges) {
  bool valid = m && floors && n_floors >= 1 && n_floors <= kClusterMaxLevels && !(n && (!references || !labels)) &&
               n <= kMaxBatchNeedles;
  for (uint32_t k = 0; valid && k < n_floors; ++k) valid = floors[k] <= 1000 && (k == 0 || floors[k - 1] < floors[k]);
  if (!valid) {
    errno = EINVAL;
    return -1;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  for (uint32_t k = 0; k < n_floors; ++k) {
    if (n_clusters) n_clusters[k] = 0;
    if (n_edges) n_edges[k] = 0;
  }
  if (n == 0) return 0;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  ClusterCall c(m, stream);                                    // a forest, a row of labels and a ClusterTotals per level
  if (c.begin(references, n, n_floors, n_floors * sizeof(ClusterTotals)) < 0) return -1;
  ClusterTotals* d_totals = static_cast<ClusterTotals*>(c.d_totals);
  auto launch = [&](const ClusterSweepArgs& a) {
    ClusterLevelsSweepArgs A{a, n_floors, {}};
    std::copy(floors, floors + n_floors, A.floors);
    return launch_cluster_levels_sweep(A, stream);
  };
  if (c.sweep(c.nu, floors[0], d_totals, launch) < 0) return -1;
  for (uint32_t k = 0; k < n_floors; ++k)
    if (launch_cluster_label(c.label_args(k), stream) < 0) return -1;
  ClusterTotals totals[kClusterMaxLevels] = {};
  if (c.read_totals(totals) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(labels, c.d_labels, n_floors * n * 4, hipMemcpyDeviceToHost, stream));
  if (c.wait(totals) < 0) return -1;
  for (uint32_t k = 0; k < n_floors; ++k) {
    if (n_clusters) n_clusters[k] = totals[k].clusters;
    if (n_edges) n_edges[k] = totals[k].edges;
  }
  return 0;
}
