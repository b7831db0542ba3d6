// cluster_tree_within.hip -- blurrily_storage_cluster_tree_within (include/blurrily_storage.h): the
// cluster tree within caller-given blocks, one call for all blocks.  Both halves are other entries': the numbering made
// before a GPU is asked for and the block plan are blurrily_storage_cluster_within's (cluster_host.h: number_nodes_keyed,
// plan_within_blocks), the rounds' buffers, the round loop, the four bytes read back per round and the record order are
// blurrily_storage_cluster_tree's.  A round is the sweep of the large blocks' needles over every image and chunk, the
// direct kernel over the small blocks' tiles into the same best[] (cluster_tree_within_kernels.hip: both choose the best
// edge leaving each component, under the block key), then cluster_tree_kernels.hip's merge and flatten as they are.
#include <algorithm>
#include <vector>

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
  const size_t nu = uniq.size();
  ClusterWithinPlan plan;
  if (plan_within_blocks(key_of, m->scope_strategy, plan) < 0) return -1;

  ClusterCall c(m, stream);
  if (c.begin(std::move(uniq), std::move(inv), n, 1, sizeof(ClusterTotals)) < 0) return -1;
  ClusterTotals* d_totals = static_cast<ClusterTotals*>(c.d_totals);
  if (c.upload(plan, key_of) < 0) return -1;

  // the rounds' buffers (cluster_tree.hip's)
  ClusterTreeRoundArgs r{};
  uint32_t* d_counters = nullptr;                             // [0]: the merges so far
  if (c.more(r.best, nu * 8, true) < 0 || c.more(r.comp, nu * 4) < 0 || c.more(r.closed, nu, true) < 0 ||
      c.more(r.merges, nu * sizeof(ClusterTreeMerge)) < 0 || c.more(d_counters, 16, true) < 0)
    return -1;
  r.parent = c.d_parent; r.refs = c.d_refs; r.n_nodes = uint32_t(nu); r.n_merges = d_counters; r.totals = d_totals;
  if (launch_cluster_tree_flatten(r, stream) < 0) return -1;  // (every number its own component)

  const ClusterWithinArgs wa{plan.d_tiles, plan.d_order, uint32_t(plan.tiles.size()), uint32_t(nu), c.x.needles.codes,
                             c.x.needles.qoff, c.x.needles.ntri, uint32_t(nu), min_permille, c.d_parent, d_totals};
  uint32_t found = 0;
  bool done = false;
  for (uint32_t round = 1; round <= kTreeMaxRounds && !done; ++round) {
    // the large blocks over the images (windows_per_workgroup by their members' number, not the numbering's) ...
    auto launch = [&](const ClusterSweepArgs& a) {
      return launch_cluster_tree_within_sweep(
          {ClusterTreeSweepArgs{a, r.comp, r.closed, r.best, round}, plan.d_swept, plan.d_block_of}, stream);
    };
    if (c.sweep(plan.swept.size(), min_permille, d_totals, launch) < 0) return -1;
    // ... and the small ones from the extraction's codes, into the same best[]
    if (launch_cluster_tree_within({wa, r.comp, r.closed, r.best, round}, stream) < 0) return -1;
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
  if (c.wait(&totals) < 0) return -1;                         // (the labels and records are copied out only on success)
  BLURRILY_HIP_TRY(hipMemcpyAsync(labels, c.d_labels, n * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  sort_tree_records(got);
  for (uint32_t i = 0; i < found; ++i) merges[i] = {got[i].a, got[i].b, got[i].permille};
  if (n_merges) *n_merges = found;
  if (n_clusters) *n_clusters = totals.clusters;
  if (n_edges) *n_edges = totals.edges;
  return 0;
}
