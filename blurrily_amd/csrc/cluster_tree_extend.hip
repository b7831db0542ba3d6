// cluster_tree_extend.hip -- blurrily_storage_cluster_tree_extend (include/blurrily_storage.h): the
// cluster tree of old and new references together, from the records the caller holds for the old ones.  The call
// sequence is ClusterCall's (cluster_host.h) over the concatenation old ++ new with one forest; the bit per number for
// "new" and the list of the new numbers are mark_new's (cluster_plan.h), as cluster_extend.hip's are, the rounds
// TreeRounds' (cluster_host.h).  The old records are uploaded once and resolved to keys in a launch in front of the
// rounds; what a round offers is the new nodes' sweeps over every image and chunk, then the records' offer.  No old
// reference is ever a needle.
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

static_assert(sizeof(ClusterTreeMerge) == sizeof(blurrily_cluster_merge_t), "the kernels' record is the header's");

extern "C" int blurrily_storage_cluster_tree_extend(trigram_map m, const uint32_t* old_refs, size_t n_old,
                                                    const blurrily_cluster_merge_t* old_merges, size_t n_old_merges,
                                                    const uint32_t* new_refs, size_t n_new, uint32_t min_permille,
                                                    uint32_t* labels_old, uint32_t* labels_new,
                                                    blurrily_cluster_merge_t* merges, uint32_t* n_merges,
                                                    uint32_t* n_clusters, uint64_t* n_edges) {
  if (!m || min_permille > 1000 || (n_old && (!old_refs || !labels_old)) || (n_new && (!new_refs || !labels_new)) ||
      (n_old_merges && !old_merges) || n_old > kTreeMaxNodes || n_new > kTreeMaxNodes - n_old ||
      ((n_old || n_new) && !merges) || n_old_merges > n_old) {
    errno = EINVAL;
    return -1;
  }
  for (size_t i = 0; i < n_old_merges; ++i)
    if (old_merges[i].a >= old_merges[i].b || old_merges[i].permille > 1000) { errno = EINVAL; return -1; }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  if (n_merges) *n_merges = 0;
  if (n_clusters) *n_clusters = 0;
  if (n_edges) *n_edges = 0;
  const size_t n = n_old + n_new;
  if (n == 0) return 0;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  // the beginning over old ++ new, and which numbers are new
  ClusterCall c(m, stream);
  {
    std::vector<uint32_t> all(n);
    std::copy(old_refs, old_refs + n_old, all.begin());
    std::copy(new_refs, new_refs + n_new, all.begin() + n_old);
    if (c.begin(all.data(), n, 1, sizeof(ClusterTotals)) < 0) return -1;
  }
  const size_t nu = c.nu;
  std::vector<uint32_t> is_new, new_nodes;
  mark_new(c.inv, n_old, n_new, nu, is_new, new_nodes);
  const size_t nn = new_nodes.size();

  ClusterTotals* d_totals = static_cast<ClusterTotals*>(c.d_totals);
  uint32_t *d_is_new, *d_new_nodes;
  ClusterTreeMerge* d_records = nullptr;
  unsigned long long* d_keys = nullptr;
  if (c.more(d_is_new, is_new.size() * 4) < 0 || c.more(d_new_nodes, nn * 4) < 0 ||
      c.more(d_records, n_old_merges * sizeof(ClusterTreeMerge)) < 0 || c.more(d_keys, n_old_merges * 8) < 0)
    return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(d_is_new, is_new.data(), is_new.size() * 4, hipMemcpyHostToDevice, stream));
  if (nn) BLURRILY_HIP_TRY(hipMemcpyAsync(d_new_nodes, new_nodes.data(), nn * 4, hipMemcpyHostToDevice, stream));
  if (n_old_merges)
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_records, old_merges, n_old_merges * sizeof(ClusterTreeMerge), hipMemcpyHostToDevice, stream));

  TreeRounds t;
  if (t.begin(c, d_totals) < 0) return -1;
  const ClusterTreeRoundArgs& r = t.r;

  // the old records as keys: which of them are candidates at all
  const ClusterTreeExtendRecordsArgs ra{d_records, uint32_t(n_old_merges), c.d_refs, c.x.needles.ntri, d_is_new, uint32_t(nu),
                                        min_permille, d_keys, r.comp, r.best};
  if (launch_cluster_tree_extend_resolve(ra, stream) < 0) return -1;

  // a round's offer: the new nodes over every window of both images (windows_per_workgroup by their number, not the
  // numbering's), then the old records
  const auto offer = [&](uint32_t round) {
    const auto launch = [&](const ClusterSweepArgs& a) {
      return launch_cluster_tree_extend_sweep({ClusterTreeSweepArgs{a, r.comp, r.closed, r.best, round}, d_new_nodes, d_is_new},
                                              stream);
    };
    return c.sweep(nn, min_permille, d_totals, launch) < 0 ? -1 : launch_cluster_tree_extend_offer(ra, stream);
  };
  if (t.run(offer) < 0) return -1;

  if (launch_cluster_label(c.label_args(), stream) < 0) return -1;
  ClusterTotals totals{};
  if (c.read_totals(&totals) < 0 || t.read_records() < 0) return -1;
  if (c.wait(&totals) < 0) return -1;                         // (the labels and records are copied out only on success)
  if (n_old) BLURRILY_HIP_TRY(hipMemcpyAsync(labels_old, c.d_labels, n_old * 4, hipMemcpyDeviceToHost, stream));
  if (n_new) BLURRILY_HIP_TRY(hipMemcpyAsync(labels_new, c.d_labels + n_old, n_new * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  t.deliver(merges);
  if (n_merges) *n_merges = t.found;
  if (n_clusters) *n_clusters = totals.clusters;
  if (n_edges) *n_edges = totals.edges;
  return 0;
}
