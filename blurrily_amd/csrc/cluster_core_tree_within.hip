// cluster_core_tree_within.hip -- blurrily_storage_cluster_core_tree_within (include/blurrily_storage.h; DESIGN.md
// section 44): the cluster core tree within caller-given blocks, one call for all blocks.  Every half is shared: the
// numbering made before a GPU is asked for (cluster_plan.h: number_nodes_keyed) and the blocked beginning with its
// plan are blurrily_storage_cluster_within's (cluster_host.h: ClusterCall::begin_blocked), the bracket loop
// blurrily_storage_cluster_core_tree's (core_height_passes), the rounds blurrily_storage_cluster_tree's (TreeRounds).
// What a height pass and a round do to the edges is this entry's own: the sweep of the large blocks' needles over every
// image and chunk, then the direct kernel over the small blocks' tiles, into the same hist[] or best[]
// (cluster_core_tree_within_kernels.hip).
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

static_assert(kNoCore == BLURRILY_NO_CORE, "the header's word for no core height is the kernels'");
static_assert(sizeof(ClusterTreeMerge) == sizeof(blurrily_cluster_merge_t), "the kernels' record is the header's");

extern "C" int blurrily_storage_cluster_core_tree_within(trigram_map m, const uint32_t* references,
                                                         const uint32_t* blocks, size_t n, uint32_t min_permille,
                                                         uint32_t min_degree, uint32_t* labels, uint32_t* core_permille,
                                                         blurrily_cluster_merge_t* merges, uint32_t* n_merges,
                                                         uint32_t* n_clusters, uint64_t* n_edges,
                                                         uint64_t* n_core_edges) {
  if (!m || min_permille > 1000 || (n && (!references || !blocks || !labels || !core_permille || !merges)) ||
      n > kTreeMaxNodes) {
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
  if (n_core_edges) *n_core_edges = 0;
  if (n == 0) return 0;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  // the plan: the numbers block after block, every block the direct kernel's or the sweep's
  ClusterCall c(m, stream);
  if (c.begin_blocked(std::move(uniq), std::move(inv), key_of, n, sizeof(ClusterCoresTotals)) < 0) return -1;
  ClusterCoresTotals* d_totals = static_cast<ClusterCoresTotals*>(c.d_totals);
  const size_t nu = c.nu;
  const size_t n_swept = c.plan.swept.size();

  // the core heights: a bracket's lower end and the count above it per number, kCoreBuckets counters each
  uint32_t *d_core = nullptr, *d_above = nullptr, *d_hist = nullptr;
  if (c.more(d_core, nu * 4) < 0 || c.more(d_above, nu * 4) < 0) return -1;
  if (min_degree && c.more(d_hist, nu * kCoreBuckets * 4, true) < 0) return -1;
  ClusterCoreHeightSettleArgs settle{d_core, d_above, d_hist, c.x.needles.ntri, uint32_t(nu), min_permille, min_degree,
                                     0, 0, d_totals};
  if (launch_cluster_core_height_settle(settle, stream) < 0) return -1;
  const ClusterWithinArgs wa = c.within_args(min_permille, nullptr, nullptr);
  // one pass over every block's edges: the large blocks over the images, then the small ones from the extraction's
  // codes, into the same counters
  const auto pass = [&](uint32_t span, uint32_t width, bool first) {
    if (c.sweep(n_swept, min_permille, nullptr, [&](const ClusterSweepArgs& a) {
          return launch_cluster_core_tree_within_sweep({a, c.d_swept, c.d_block_of, d_core, d_hist, span, width, first,
                                                        nullptr, nullptr, nullptr, 0, d_totals}, false, stream);
        }) < 0)
      return -1;
    return launch_cluster_core_tree_within({wa, d_core, d_hist, span, width, first, nullptr, nullptr, nullptr, 0, d_totals},
                                           false, stream);
  };
  if (min_degree && core_height_passes(settle, stream, pass) < 0) return -1;

  // the forest: the cluster tree's rounds over the within-block edges between two numbers with a core height
  TreeRounds t;
  if (t.begin(c, &d_totals->t) < 0) return -1;
  const ClusterTreeRoundArgs& r = t.r;
  const uint32_t count_edges = min_degree == 0u;              // (no height pass ran: round 1 counts every edge)
  const auto offer = [&](uint32_t round) {
    if (c.sweep(n_swept, min_permille, nullptr, [&](const ClusterSweepArgs& a) {
          return launch_cluster_core_tree_within_sweep({a, c.d_swept, c.d_block_of, d_core, nullptr, 0, 0, count_edges,
                                                        r.comp, r.closed, r.best, round, d_totals}, true, stream);
        }) < 0)
      return -1;
    return launch_cluster_core_tree_within({wa, d_core, nullptr, 0, 0, count_edges, r.comp, r.closed, r.best, round,
                                            d_totals}, true, stream);
  };
  if (t.run(offer) < 0) return -1;

  // a number without a core height was hooked by nothing: its label is its own reference
  if (launch_cluster_label(c.label_args(), stream) < 0) return -1;
  ClusterCoresTotals totals{};
  std::vector<uint32_t> core(nu), got_labels(n);
  if (c.read_totals(&totals) < 0 || t.read_records() < 0) return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(core.data(), d_core, nu * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipMemcpyAsync(got_labels.data(), c.d_labels, n * 4, hipMemcpyDeviceToHost, stream));
  if (c.wait(&totals.t) < 0) return -1;                       // (the outputs are written only on success)
  std::copy(got_labels.begin(), got_labels.end(), labels);
  t.deliver(merges);
  for (size_t i = 0; i < n; ++i) core_permille[i] = core[c.inv.empty() ? i : c.inv[i]];
  const size_t cores = size_t(std::count_if(core.begin(), core.end(), [](uint32_t h) { return h != kNoCore; }));
  if (n_merges) *n_merges = t.found;
  if (n_clusters) *n_clusters = uint32_t(cores - t.found);    // (a forest: its components are its nodes minus its edges)
  if (n_edges) *n_edges = totals.t.edges;
  if (n_core_edges) *n_core_edges = totals.core_edges;
  return 0;
}
