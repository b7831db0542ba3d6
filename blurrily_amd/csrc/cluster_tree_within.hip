// cluster_tree_within.hip -- blurrily_storage_cluster_tree_within (include/blurrily_storage.h): the
// cluster tree within caller-given blocks, one call for all blocks.  Both halves are shared: the numbering made before a
// GPU is asked for (cluster_plan.h: number_nodes_keyed) and the blocked beginning with its plan are
// blurrily_storage_cluster_within's (cluster_host.h: ClusterCall::begin_blocked), the rounds
// blurrily_storage_cluster_tree's (TreeRounds).  What a round offers is the sweep of the large blocks' needles over
// every image and chunk, then the direct kernel over the small blocks' tiles into the same best[]
// (cluster_tree_within_kernels.hip: both choose the best edge leaving each component, under the block key).
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

static_assert(sizeof(ClusterTreeMerge) == sizeof(blurrily_cluster_merge_t), "the kernels' record is the header's");

extern "C" int blurrily_storage_cluster_tree_within(trigram_map m, const uint32_t* references, const uint32_t* blocks,
                                                    size_t n, uint32_t min_permille, uint32_t* labels,
                                                    blurrily_cluster_merge_t* merges, uint32_t* n_merges,
                                                    uint32_t* n_clusters, uint64_t* n_edges) {
  if (!m || min_permille > 1000 || (n && (!references || !blocks || !labels || !merges)) || n > kTreeMaxNodes) {
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
  if (n_merges) *n_merges = 0;
  if (n_clusters) *n_clusters = 0;
  if (n_edges) *n_edges = 0;
  if (n == 0) return 0;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  // the plan: the numbers block after block, every block the direct kernel's or the sweep's
  ClusterCall c(m, stream);
  if (c.begin_blocked(std::move(uniq), std::move(inv), key_of, n) < 0) return -1;
  ClusterTotals* d_totals = static_cast<ClusterTotals*>(c.d_totals);
  TreeRounds t;
  if (t.begin(c, d_totals) < 0) return -1;
  const ClusterTreeRoundArgs& r = t.r;

  const ClusterWithinArgs wa = c.within_args(min_permille, c.d_parent, d_totals);
  const auto offer = [&](uint32_t round) {
    // the large blocks over the images (windows_per_workgroup by their members' number, not the numbering's) ...
    const auto launch = [&](const ClusterSweepArgs& a) {
      return launch_cluster_tree_within_sweep(
          {ClusterTreeSweepArgs{a, r.comp, r.closed, r.best, round}, c.d_swept, c.d_block_of}, stream);
    };
    if (c.sweep(c.plan.swept.size(), min_permille, d_totals, launch) < 0) return -1;
    // ... and the small ones from the extraction's codes, into the same best[]
    return launch_cluster_tree_within({wa, r.comp, r.closed, r.best, round}, stream);
  };
  if (t.run(offer) < 0) return -1;

  if (launch_cluster_label(c.label_args(), stream) < 0) return -1;
  ClusterTotals totals{};
  if (c.read_totals(&totals) < 0 || t.read_records() < 0) return -1;
  if (c.wait(&totals) < 0) return -1;                         // (the labels and records are copied out only on success)
  BLURRILY_HIP_TRY(hipMemcpyAsync(labels, c.d_labels, n * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  t.deliver(merges);
  if (n_merges) *n_merges = t.found;
  if (n_clusters) *n_clusters = totals.clusters;
  if (n_edges) *n_edges = totals.edges;
  return 0;
}
