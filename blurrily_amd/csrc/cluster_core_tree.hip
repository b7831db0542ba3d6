// cluster_core_tree.hip -- blurrily_storage_cluster_core_tree (include/blurrily_storage.h): the
// dendrogram of blurrily_storage_cluster_cores' cores at every floor from one call.  The call sequence is ClusterCall's
// (cluster_host.h) with one forest.  First the core heights, by histogram refinement: a sweep over every image and
// chunk and a settle per step, max(1, ceil(log_kCoreBuckets(1001 - min_permille))) steps, none with min_degree == 0.
// Then the cluster tree's rounds (TreeRounds, cluster_host.h) with cluster_core_tree_kernels.hip's sweep for a round's
// offer in place of the tree's.
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

static_assert(kNoCore == BLURRILY_NO_CORE, "the header's word for no core height is the kernels'");
static_assert(sizeof(ClusterTreeMerge) == sizeof(blurrily_cluster_merge_t), "the kernels' record is the header's");

extern "C" int blurrily_storage_cluster_core_tree(trigram_map m, const uint32_t* references, size_t n,
                                                  uint32_t min_permille, uint32_t min_degree, uint32_t* labels,
                                                  uint32_t* core_permille, blurrily_cluster_merge_t* merges,
                                                  uint32_t* n_merges, uint32_t* n_clusters, uint64_t* n_edges,
                                                  uint64_t* n_core_edges) {
  if (!m || min_permille > 1000 || (n && (!references || !labels || !core_permille || !merges)) || n > kTreeMaxNodes) {
    errno = EINVAL;
    return -1;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  if (n_merges) *n_merges = 0;
  if (n_clusters) *n_clusters = 0;
  if (n_edges) *n_edges = 0;
  if (n_core_edges) *n_core_edges = 0;
  if (n == 0) return 0;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  ClusterCall c(m, stream);
  if (c.begin(references, n, 1, sizeof(ClusterCoresTotals)) < 0) return -1;
  ClusterCoresTotals* d_totals = static_cast<ClusterCoresTotals*>(c.d_totals);
  const size_t nu = c.nu;

  // the core heights: a bracket's lower end and the count above it per number, kCoreBuckets counters each
  uint32_t *d_core = nullptr, *d_above = nullptr, *d_hist = nullptr;
  if (c.more(d_core, nu * 4) < 0 || c.more(d_above, nu * 4) < 0) return -1;
  if (min_degree && c.more(d_hist, nu * kCoreBuckets * 4, true) < 0) return -1;
  ClusterCoreHeightSettleArgs settle{d_core, d_above, d_hist, c.x.needles.ntri, uint32_t(nu), min_permille, min_degree,
                                     0, 0, d_totals};
  if (launch_cluster_core_height_settle(settle, stream) < 0) return -1;
  const auto pass = [&](uint32_t span, uint32_t width, bool first) {
    return c.sweep(nu, min_permille, nullptr, [&](const ClusterSweepArgs& a) {
      return launch_cluster_core_height_sweep({a, d_core, d_hist, span, width, first, d_totals}, stream);
    });
  };
  if (min_degree && core_height_passes(settle, stream, pass) < 0) return -1;

  // the forest: the cluster tree's rounds over the edges between two numbers with a core height
  TreeRounds t;
  if (t.begin(c, &d_totals->t) < 0) return -1;
  const ClusterTreeRoundArgs& r = t.r;
  const auto offer = [&](uint32_t round) {
    return c.sweep(nu, min_permille, nullptr, [&](const ClusterSweepArgs& a) {
      return launch_cluster_core_tree_sweep({ClusterTreeSweepArgs{a, r.comp, r.closed, r.best, round}, d_core,
                                             min_degree == 0u, d_totals}, stream);
    });
  };
  if (t.run(offer) < 0) return -1;

  // a number without a core height was hooked by nothing: its label is its own reference
  if (launch_cluster_label(c.label_args(), stream) < 0) return -1;
  ClusterCoresTotals totals{};
  std::vector<uint32_t> core(nu);
  if (c.read_totals(&totals) < 0 || t.read_records() < 0) return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(core.data(), d_core, nu * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipMemcpyAsync(labels, c.d_labels, n * 4, hipMemcpyDeviceToHost, stream));
  if (c.wait(&totals.t) < 0) return -1;
  t.deliver(merges);
  for (size_t i = 0; i < n; ++i) core_permille[i] = core[c.inv.empty() ? i : c.inv[i]];
  const size_t cores = size_t(std::count_if(core.begin(), core.end(), [](uint32_t h) { return h != kNoCore; }));
  if (n_merges) *n_merges = t.found;
  if (n_clusters) *n_clusters = uint32_t(cores - t.found);    // (a forest: its components are its nodes minus its edges)
  if (n_edges) *n_edges = totals.t.edges;
  if (n_core_edges) *n_core_edges = totals.core_edges;
  return 0;
}
