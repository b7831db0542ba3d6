// cluster_edges.hip -- blurrily_storage_cluster_edges and blurrily_storage_cluster_edges_within (include/
// blurrily_storage.h): the edges of blurrily_storage_cluster's graph, or of
// blurrily_storage_cluster_within's, each once, as {a, b, permille} records in the cluster tree's order.  The call
// sequence is ClusterCall's (cluster_host.h) -- for the blocked form over a numbering made here, before a GPU is asked
// for, and with cluster_within's plan (ClusterCall::begin_blocked) -- with one forest, which nothing reads (the node
// tables are filled per forest), and with ClusterTotals::edges as the call's cursor: every sweep launch of the call
// appends through it (cluster_edges_kernels.hip), and what it holds after the last one is the edge count, in every
// mode.  An emitting call then sorts the keys (segsort.h, one segment) and turns them into records; a count-only call,
// or one whose count does not fit, launches neither.
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
  ClusterTotals totals{};
  if (c.read_totals(&totals) < 0 || c.wait(&totals) < 0) return -1;
  const uint64_t E = totals.edges;
  *n_edges = E;
  if (!edges) return 0;                                       // count only
  if (capacity < E) { errno = ERANGE; return -1; }
  if (E > out.room) { errno = EOVERFLOW; return -1; }          // (the option's bound: not every key was stored)
  if (E == 0) return 0;

  const ClusterEdgeKey* sorted = out.keys;
  DeviceBuffer tables;
  if (E >= 2) {
    ClusterEdgeKey* d_sorted = nullptr;
    if (c.more(d_sorted, E * sizeof(ClusterEdgeKey)) < 0) return -1;
    const uint32_t off[2] = {0u, uint32_t(E)};                // (E <= room <= 2^31)
    if (segmented_sort(out.keys, d_sorted, off, 1, 2, false, tables, stream) < 0) return -1;
    sorted = d_sorted;
  }
  ClusterTreeMerge* d_rows = nullptr;
  if (c.more(d_rows, E * sizeof(ClusterTreeMerge)) < 0) return -1;
  if (launch_cluster_edges_rows({sorted, c.d_refs, uint32_t(E), uint32_t(c.nu), d_rows}, stream) < 0) return -1;
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));             // (the records are copied out only on success)
  BLURRILY_HIP_TRY(hipMemcpyAsync(edges, d_rows, E * sizeof(ClusterTreeMerge), hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  return 0;
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
