// cluster_extend.hip -- blurrily_storage_cluster_extend (include/blurrily_storage.h): the clusters
// of old and new references together, from the labels the caller holds for the old ones.  The call sequence is
// ClusterCall's (cluster_host.h) over the concatenation old ++ new, with two things more on the device -- a bit per
// number for "new" and the list of the new numbers (mark_new, cluster_plan.h) -- a seed launch in front of the sweeps,
// and the sweeps over the new numbers alone.  The seeds and the sweep are cluster_extend_kernels.hip's, the node tables
// and the labels cluster_kernels.hip's kernels as they are.
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

extern "C" int blurrily_storage_cluster_extend(trigram_map m, const uint32_t* old_refs, const uint32_t* old_labels,
                                               size_t n_old, const uint32_t* new_refs, size_t n_new,
                                               uint32_t min_permille, uint32_t* labels_old, uint32_t* labels_new,
                                               uint32_t* n_clusters, uint64_t* n_edges) {
  if (!m || min_permille > 1000 || (n_old && (!old_refs || !old_labels || !labels_old)) ||
      (n_new && (!new_refs || !labels_new)) || n_old > kMaxBatchNeedles || n_new > kMaxBatchNeedles - n_old) {
    errno = EINVAL;
    return -1;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  if (n_clusters) *n_clusters = 0;
  if (n_edges) *n_edges = 0;
  const size_t n = n_old + n_new;
  if (n == 0) return 0;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  // the beginning over old ++ new (1 .. n then n + 1 .. n + k ascends strictly: no sort), and which numbers are new
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
  uint32_t *d_is_new, *d_old_labels, *d_new_nodes;
  if (c.more(d_is_new, is_new.size() * 4) < 0 || c.more(d_old_labels, n_old * 4) < 0 || c.more(d_new_nodes, nn * 4) < 0)
    return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(d_is_new, is_new.data(), is_new.size() * 4, hipMemcpyHostToDevice, stream));
  if (n_old) BLURRILY_HIP_TRY(hipMemcpyAsync(d_old_labels, old_labels, n_old * 4, hipMemcpyHostToDevice, stream));
  if (nn) BLURRILY_HIP_TRY(hipMemcpyAsync(d_new_nodes, new_nodes.data(), nn * 4, hipMemcpyHostToDevice, stream));

  // the seeds: what the caller's labels say of the old-old edges (the old elements come first in inv)
  ClusterExtendSeedArgs sa{d_old_labels, c.d_inv, c.d_refs, c.x.needles.ntri, d_is_new, uint32_t(n_old), uint32_t(nu),
                           c.d_parent, d_totals};
  if (launch_cluster_extend_seed(sa, stream) < 0) return -1;

  // the new nodes over every window of both images (windows_per_workgroup by their number, not the numbering's)
  if (c.sweep(nn, min_permille, d_totals, [&](const ClusterSweepArgs& a) {
        return launch_cluster_extend_sweep({a, d_new_nodes, d_is_new}, stream);
      }) < 0)
    return -1;

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
