// cluster_edges_extend.hip -- blurrily_storage_cluster_edges_extend and blurrily_storage_cluster_edges_between (include/
// blurrily_storage.h): the edges of blurrily_storage_cluster's graph over two lists that have a new
// end (the second list's), or exactly one end in each list, each once, as blurrily_storage_cluster_edges' records in its
// order.  The call sequence is ClusterCall's (cluster_host.h) over the concatenation first ++ second with one forest,
// which nothing reads, as cluster_extend.hip's is; the bit per number for the second list is mark_new's (cluster_plan.h),
// the side that sweeps choose_between_side's (the new numbers, for the extending entry), the sweep
// cluster_edges_extend_kernels.hip's, over the sweeping side's numbers alone, and the ending -- the count, ERANGE or
// EOVERFLOW, the sort, the records -- cluster_edges.hip's (ClusterCall::deliver_edges).
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

static_assert(sizeof(ClusterTreeMerge) == sizeof(blurrily_cluster_merge_t), "the kernels' record is the header's");
static_assert(kTreeMaxNodes == BLURRILY_CLUSTER_TREE_MAX, "the key holds both ends in kTreeNumberBits each");

namespace {

// Both entries behind their checks.  first: old or left, second: new or right.
int cluster_edges_extend_run(trigram_map m, const uint32_t* first, size_t n_first, const uint32_t* second, size_t n_second,
                             bool between, uint32_t min_permille, blurrily_cluster_merge_t* edges, uint64_t capacity,
                             uint64_t* n_edges) {
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  *n_edges = 0;
  if (n_second == 0 || (between && n_first == 0)) return 0;   // no new end; or a side with nothing on it
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  // the beginning over first ++ second, which numbers the second list names, and which side sweeps
  const size_t n = n_first + n_second;
  ClusterCall c(m, stream);
  {
    std::vector<uint32_t> all(n);
    std::copy(first, first + n_first, all.begin());
    std::copy(second, second + n_second, all.begin() + n_first);
    if (c.begin(all.data(), n, 1, sizeof(ClusterTotals)) < 0) return -1;
  }
  std::vector<uint32_t> side, needles, left_nodes;
  mark_new(c.inv, n_first, n_second, c.nu, side, needles);
  if (between && !choose_between_side(side, needles.size(), c.nu, left_nodes)) needles.swap(left_nodes);
  const size_t nn = needles.size();

  ClusterTotals* d_totals = static_cast<ClusterTotals*>(c.d_totals);
  uint32_t *d_side = nullptr, *d_needles = nullptr;
  if (c.more(d_side, side.size() * 4) < 0 || c.more(d_needles, nn * 4) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(d_side, side.data(), side.size() * 4, hipMemcpyHostToDevice, stream));
  if (nn) BLURRILY_HIP_TRY(hipMemcpyAsync(d_needles, needles.data(), nn * 4, hipMemcpyHostToDevice, stream));

  // the room: what the caller can take, as far as the option allows (count only: none)
  ClusterEdgesOut out{&d_totals->edges, nullptr, edges ? std::min<uint64_t>(capacity, m->cluster_edges_max) : 0u};
  if (c.more(out.keys, out.room * sizeof(ClusterEdgeKey)) < 0) return -1;

  // the sweeping side over every window of both images (windows_per_workgroup by its number, not the numbering's)
  if (c.sweep(nn, min_permille, d_totals, [&](const ClusterSweepArgs& a) {
        return launch_cluster_edges_extend_sweep({a, d_needles, d_side, between ? 1u : 0u, out}, stream);
      }) < 0)
    return -1;
  return c.deliver_edges(out, edges, capacity, n_edges);
}

bool bad_arguments(trigram_map m, const uint32_t* first, size_t n_first, const uint32_t* second, size_t n_second,
                   uint32_t min_permille, const uint64_t* n_edges) {
  return !m || min_permille > 1000 || (n_first && !first) || (n_second && !second) || !n_edges ||
         n_first > kTreeMaxNodes || n_second > kTreeMaxNodes - n_first;
}

}  // namespace

extern "C" int blurrily_storage_cluster_edges_extend(trigram_map m, const uint32_t* old_refs, size_t n_old,
                                                     const uint32_t* new_refs, size_t n_new, uint32_t min_permille,
                                                     blurrily_cluster_merge_t* edges, uint64_t capacity,
                                                     uint64_t* n_edges) {
  if (bad_arguments(m, old_refs, n_old, new_refs, n_new, min_permille, n_edges)) {
    errno = EINVAL;
    return -1;
  }
  return cluster_edges_extend_run(m, old_refs, n_old, new_refs, n_new, false, min_permille, edges, capacity, n_edges);
}

extern "C" int blurrily_storage_cluster_edges_between(trigram_map m, const uint32_t* left_refs, size_t n_left,
                                                      const uint32_t* right_refs, size_t n_right, uint32_t min_permille,
                                                      blurrily_cluster_merge_t* edges, uint64_t capacity,
                                                      uint64_t* n_edges) {
  if (bad_arguments(m, left_refs, n_left, right_refs, n_right, min_permille, n_edges)) {
    errno = EINVAL;
    return -1;
  }
  return cluster_edges_extend_run(m, left_refs, n_left, right_refs, n_right, true, min_permille, edges, capacity, n_edges);
}
