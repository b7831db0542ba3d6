// cluster_edges.hip -- blurrily_storage_cluster_edges and blurrily_storage_cluster_edges_within (include/
// blurrily_storage.h): the edges of blurrily_storage_cluster's graph, or of
// blurrily_storage_cluster_within's, each once, as {a, b, permille} records in the cluster tree's order.  The call
// sequence is ClusterCall's (cluster_host.h) -- for the blocked form over a numbering made here, before a GPU is asked
// for, and with cluster_within's plan (ClusterCall::begin_blocked) -- with one forest, which nothing reads (the node
// tables are filled per forest), and with ClusterTotals::edges as the call's cursor: every sweep launch of the call
// appends through it (cluster_edges_kernels.hip), and what it holds after the last one is the edge count, in every
// mode.  An emitting call then sorts the keys (segsort.h, one segment) and turns them into records; a count-only call,
// or one whose count does not fit, launches neither (ClusterCall::deliver_edges, which cluster_edges_extend.hip ends
// with too).
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

static_assert(sizeof(ClusterTreeMerge) == sizeof(blurrily_cluster_merge_t), "the kernels' record is the header's");
static_assert(kTreeMaxNodes == BLURRILY_CLUSTER_TREE_MAX, "the key holds both ends in kTreeNumberBits each");

namespace {

// Both entries behind their checks: key_of empty for the unblocked form (uniq and inv are then made by begin()).
int cluster_edges_run(trigram_map m, const uint32_t* references, size_t n, bool blocked, std::vector<uint32_t>& uniq,
                      std::vector<uint32_t>& inv, const std::vector<uint32_t>& key_of, uint32_t min_permille,
                      blurrily_cluster_merge_t* edges, uint64_t capacity, uint64_t* n_edges) {
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  *n_edges = 0;
  if (n == 0) return 0;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  ClusterCall c(m, stream);
  if ((blocked ? c.begin_blocked(std::move(uniq), std::move(inv), key_of, n)
               : c.begin(references, n, 1, sizeof(ClusterTotals))) < 0)
    return -1;
  ClusterTotals* d_totals = static_cast<ClusterTotals*>(c.d_totals);

  // the room: what the caller can take, as far as the option allows (count only: none)
  ClusterEdgesOut out{&d_totals->edges, nullptr, edges ? std::min<uint64_t>(capacity, m->cluster_edges_max) : 0u};
  if (c.more(out.keys, out.room * sizeof(ClusterEdgeKey)) < 0) return -1;

  if (!blocked) {
    if (c.sweep(c.nu, min_permille, d_totals, [&](const ClusterSweepArgs& a) {
          return launch_cluster_edges_sweep({a, nullptr, nullptr, out}, stream);
        }) < 0)
      return -1;
  } else {
    // the large blocks over the images, the small ones from the extraction's codes, through the one cursor
    if (c.sweep(c.plan.swept.size(), min_permille, d_totals, [&](const ClusterSweepArgs& a) {
          return launch_cluster_edges_sweep({a, c.d_swept, c.d_block_of, out}, stream);
        }) < 0)
      return -1;
    if (launch_cluster_edges_within({c.within_args(min_permille, nullptr, nullptr), out}, stream) < 0) return -1;
  }
  return c.deliver_edges(out, edges, capacity, n_edges);      // (the count, ERANGE or EOVERFLOW, the sort, the records)
}

}  // namespace

extern "C" int blurrily_storage_cluster_edges(trigram_map m, const uint32_t* references, size_t n, uint32_t min_permille,
                                              blurrily_cluster_merge_t* edges, uint64_t capacity, uint64_t* n_edges) {
  if (!m || min_permille > 1000 || (n && !references) || !n_edges || n > kTreeMaxNodes) {
    errno = EINVAL;
    return -1;
  }
  std::vector<uint32_t> uniq, inv, key_of;
  return cluster_edges_run(m, references, n, false, uniq, inv, key_of, min_permille, edges, capacity, n_edges);
}

extern "C" int blurrily_storage_cluster_edges_within(trigram_map m, const uint32_t* references, const uint32_t* blocks,
                                                     size_t n, uint32_t min_permille, blurrily_cluster_merge_t* edges,
                                                     uint64_t capacity, uint64_t* n_edges) {
  if (!m || min_permille > 1000 || (n && (!references || !blocks)) || !n_edges || n > kTreeMaxNodes) {
    errno = EINVAL;
    return -1;
  }
  std::vector<uint32_t> uniq, inv, key_of;
  if (n && !number_nodes_keyed(references, blocks, n, uniq, inv, key_of)) {
    errno = EINVAL;                                           // a reference listed under two keys
    return -1;
  }
  return cluster_edges_run(m, references, n, true, uniq, inv, key_of, min_permille, edges, capacity, n_edges);
}
