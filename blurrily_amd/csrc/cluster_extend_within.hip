// cluster_extend_within.hip -- blurrily_storage_cluster_extend_within (include/blurrily_storage.h):
// blurrily_storage_cluster_extend inside caller-given blocks -- the clusters of old and new references together, from
// the labels the caller holds for the old ones, where a seed and an edge also need both ends under one block key.  The
// call sequence is ClusterCall's (cluster_host.h) over old ++ new, as cluster_extend.hip's, with the numbering made
// here, before a GPU is asked for, because the numbering is where a reference listed under two keys shows, as in
// cluster_within.hip.  On the device on top of it: a bit per number for "new" (mark_new), the old labels, every
// number's key, and the plan (cluster_plan.h's plan_extend_within_blocks) -- every block that has a new number given to
// the direct kernel's tiles or to the sweep's needle list, a block without one to neither.  The seeds, the sweep and
// the direct kernel are cluster_extend_within_kernels.hip's, the node tables and the labels cluster_kernels.hip's
// kernels as they are.
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

extern "C" int blurrily_storage_cluster_extend_within(trigram_map m, const uint32_t* old_refs, const uint32_t* old_blocks,
                                                      const uint32_t* old_labels, size_t n_old, const uint32_t* new_refs,
                                                      const uint32_t* new_blocks, size_t n_new, uint32_t min_permille,
                                                      uint32_t* labels_old, uint32_t* labels_new, uint32_t* n_clusters,
                                                      uint64_t* n_edges) {
  if (!m || min_permille > 1000 || (n_old && (!old_refs || !old_blocks || !old_labels || !labels_old)) ||
      (n_new && (!new_refs || !new_blocks || !labels_new)) || n_old > kMaxBatchNeedles ||
      n_new > kMaxBatchNeedles - n_old) {
    errno = EINVAL;
    return -1;
  }
  const size_t n = n_old + n_new;
  // the numbering over old ++ new with the keys alongside, which numbers are new, and the plan
  std::vector<uint32_t> uniq, inv, key_of, is_new, new_nodes;
  ClusterExtendWithinPlan plan;
  if (n) {
    std::vector<uint32_t> all(n), keys(n);
    std::copy(old_refs, old_refs + n_old, all.begin());
    std::copy(new_refs, new_refs + n_new, all.begin() + n_old);
    std::copy(old_blocks, old_blocks + n_old, keys.begin());
    std::copy(new_blocks, new_blocks + n_new, keys.begin() + n_old);
    if (!number_nodes_keyed(all.data(), keys.data(), n, uniq, inv, key_of)) {
      errno = EINVAL;                                         // a reference listed under two keys
      return -1;
    }
    mark_new(inv, n_old, n_new, uniq.size(), is_new, new_nodes);
    if (plan_extend_within_blocks(key_of, is_new, m->scope_strategy, plan) < 0) return -1;
  }
  if (n == 0) {                                               // nothing listed: no GPU is asked for
    if (n_clusters) *n_clusters = 0;
    if (n_edges) *n_edges = 0;
    return 0;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  ClusterCall c(m, stream);
  if (c.begin(std::move(uniq), std::move(inv), n, 1, sizeof(ClusterTotals)) < 0) return -1;
  const size_t nu = c.nu;
  ClusterTotals* d_totals = static_cast<ClusterTotals*>(c.d_totals);
  const size_t n_tiles = plan.tiles.size(), n_swept = plan.swept.size(), n_new_order = plan.new_order.size();
  uint32_t *d_is_new, *d_old_labels, *d_block_of, *d_order, *d_new_order, *d_swept;
  ClusterExtendWithinTile* d_tiles;
  if (c.more(d_is_new, is_new.size() * 4) < 0 || c.more(d_old_labels, n_old * 4) < 0 || c.more(d_block_of, nu * 4) < 0 ||
      c.more(d_tiles, n_tiles * sizeof(ClusterExtendWithinTile)) < 0 || c.more(d_order, n_tiles ? nu * 4 : 0) < 0 ||
      c.more(d_new_order, n_tiles ? n_new_order * 4 : 0) < 0 || c.more(d_swept, n_swept * 4) < 0)
    return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(d_is_new, is_new.data(), is_new.size() * 4, hipMemcpyHostToDevice, stream));
  BLURRILY_HIP_TRY(hipMemcpyAsync(d_block_of, key_of.data(), nu * 4, hipMemcpyHostToDevice, stream));
  if (n_old) BLURRILY_HIP_TRY(hipMemcpyAsync(d_old_labels, old_labels, n_old * 4, hipMemcpyHostToDevice, stream));
  if (n_tiles) {
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_tiles, plan.tiles.data(), n_tiles * sizeof(ClusterExtendWithinTile),
                                    hipMemcpyHostToDevice, stream));
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_order, plan.order.data(), nu * 4, hipMemcpyHostToDevice, stream));
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_new_order, plan.new_order.data(), n_new_order * 4, hipMemcpyHostToDevice, stream));
  }
  if (n_swept) BLURRILY_HIP_TRY(hipMemcpyAsync(d_swept, plan.swept.data(), n_swept * 4, hipMemcpyHostToDevice, stream));

  // the seeds: what the caller's labels say of the old-old edges inside a key (the old elements come first in inv)
  ClusterExtendWithinSeedArgs sa{{d_old_labels, c.d_inv, c.d_refs, c.x.needles.ntri, d_is_new, uint32_t(n_old),
                                  uint32_t(nu), c.d_parent, d_totals},
                                 d_block_of};
  if (launch_cluster_extend_within_seed(sa, stream) < 0) return -1;

  // the swept blocks' new numbers over every window of both images (windows_per_workgroup by their number) ...
  if (c.sweep(n_swept, min_permille, d_totals, [&](const ClusterSweepArgs& a) {
        return launch_cluster_extend_within_sweep({a, d_swept, d_is_new, d_block_of}, stream);
      }) < 0)
    return -1;
  // ... and the other blocks' from the extraction's codes, into the same forest
  ClusterExtendWithinArgs wa{d_tiles, d_order, d_new_order, uint32_t(n_tiles), uint32_t(nu), uint32_t(n_new_order),
                             c.x.needles.codes, c.x.needles.qoff, c.x.needles.ntri, d_is_new, uint32_t(nu), min_permille,
                             c.d_parent, d_totals};
  if (launch_cluster_extend_within(wa, stream) < 0) return -1;

  if (launch_cluster_label(c.label_args(), stream) < 0) return -1;
  ClusterTotals totals{};
  if (c.read_totals(&totals) < 0 || c.wait(&totals) < 0) return -1;   // (the labels are copied out only on success)
  if (n_old) BLURRILY_HIP_TRY(hipMemcpyAsync(labels_old, c.d_labels, n_old * 4, hipMemcpyDeviceToHost, stream));
  if (n_new) BLURRILY_HIP_TRY(hipMemcpyAsync(labels_new, c.d_labels + n_old, n_new * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  if (n_clusters) *n_clusters = totals.clusters;
  if (n_edges) *n_edges = totals.edges;
  return 0;
}
