// cluster_within.hip -- blurrily_storage_cluster_within (include/blurrily_storage.h):
// blurrily_storage_cluster's components within caller-given blocks, one call for all blocks.  The call sequence is
// ClusterCall's (cluster_host.h) over a numbering made here, before a GPU is asked for, because the numbering is where a
// reference listed under two keys shows.  On top of it, from ClusterCall::begin_blocked, which the other blocked
// entries share: each number's key on the device, and the plan (cluster_plan.h's plan_within_blocks) -- the numbers
// sorted by (key, number), every block given to one of two kernels (cluster_within_kernels.hip): the direct kernel's
// tiles for a block of at most kClusterWithinDirectMax listed members, the sweep's needle list for a larger one.  Both
// unite in the one forest; the node tables and the labels are cluster_kernels.hip's kernels as they are.
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

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

  // the plan: the numbers block after block, every block the direct kernel's or the sweep's
  ClusterCall c(m, stream);
  if (c.begin_blocked(std::move(uniq), std::move(inv), key_of, n) < 0) return -1;
  ClusterTotals* d_totals = static_cast<ClusterTotals*>(c.d_totals);

  // the large blocks over the images (windows_per_workgroup by their members' number, not the numbering's) ...
  if (c.sweep(c.plan.swept.size(), min_permille, d_totals, [&](const ClusterSweepArgs& a) {
        return launch_cluster_within_sweep({a, c.d_swept, c.d_block_of}, stream);
      }) < 0)
    return -1;
  // ... and the small ones from the extraction's codes, into the same forest
  if (launch_cluster_within(c.within_args(min_permille, c.d_parent, d_totals), stream) < 0) return -1;

  if (launch_cluster_label(c.label_args(), stream) < 0) return -1;
  ClusterTotals totals{};
  if (c.read_totals(&totals) < 0 || c.wait(&totals) < 0) return -1;   // (the labels are copied out only on success)
  BLURRILY_HIP_TRY(hipMemcpyAsync(labels, c.d_labels, n * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  if (n_clusters) *n_clusters = totals.clusters;
  if (n_edges) *n_edges = totals.edges;
  return 0;
}
