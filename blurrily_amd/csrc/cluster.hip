// cluster.hip -- blurrily_storage_cluster (include/blurrily_storage.h): single-linkage clusters
// of stored references under a floor of trigram Jaccard similarity, one label per reference.  The call sequence is
// ClusterCall's (cluster_host.h), with one forest and nothing of its own; the kernels are cluster_kernels.hip's.
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

extern "C" int blurrily_storage_cluster(trigram_map m, const uint32_t* references, size_t n, uint32_t min_permille,
                                        uint32_t* labels, uint32_t* n_clusters, uint64_t* n_edges) {
  if (!m || min_permille > 1000 || (n && (!references || !labels)) || n > kMaxBatchNeedles) {
    errno = EINVAL;
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

  ClusterCall c(m, stream);
  if (c.begin(references, n, 1, sizeof(ClusterTotals)) < 0) return -1;
  ClusterTotals* d_totals = static_cast<ClusterTotals*>(c.d_totals);
  if (c.sweep(c.nu, min_permille, d_totals, [&](const ClusterSweepArgs& a) { return launch_cluster_sweep(a, stream); }) < 0)
    return -1;
  if (launch_cluster_label(c.label_args(), stream) < 0) return -1;
  ClusterTotals totals{};
  if (c.read_totals(&totals) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(labels, c.d_labels, n * 4, hipMemcpyDeviceToHost, stream));
  if (c.wait(&totals) < 0) return -1;
  if (n_clusters) *n_clusters = totals.clusters;
  if (n_edges) *n_edges = totals.edges;
  return 0;
}
