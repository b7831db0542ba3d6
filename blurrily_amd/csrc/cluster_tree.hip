// cluster_tree.hip -- blurrily_storage_cluster_tree (include/blurrily_storage.h): the maximum
// spanning forest of blurrily_storage_cluster's edges with heights in whole per mille -- the single-linkage dendrogram --
// by Boruvka rounds on the device.  The call sequence is ClusterCall's (cluster_host.h) with one forest, the rounds are
// TreeRounds' (the same header: the merge, the flatten and four bytes read back per round, the merges so far; a round
// that adds none was the last), and what a round offers is one sweep over every image and chunk
// (cluster_tree_kernels.hip's, which chooses the best edge leaving each component).
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
  TreeRounds t;
  if (t.begin(c, d_totals) < 0) return -1;
  const ClusterTreeRoundArgs& r = t.r;
  const auto offer = [&](uint32_t round) {
    return c.sweep(c.nu, min_permille, d_totals, [&](const ClusterSweepArgs& a) {
      return launch_cluster_tree_sweep(ClusterTreeSweepArgs{a, r.comp, r.closed, r.best, round}, stream);
    });
  };
  if (t.run(offer) < 0) return -1;

  if (launch_cluster_label(c.label_args(), stream) < 0) return -1;
  ClusterTotals totals{};
  if (c.read_totals(&totals) < 0 || t.read_records() < 0) return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(labels, c.d_labels, n * 4, hipMemcpyDeviceToHost, stream));
  if (c.wait(&totals) < 0) return -1;
  t.deliver(merges);
  if (n_merges) *n_merges = t.found;
  if (n_clusters) *n_clusters = totals.clusters;
  if (n_edges) *n_edges = totals.edges;
  return 0;
}
