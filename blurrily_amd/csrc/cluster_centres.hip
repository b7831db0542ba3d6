// cluster_centres.hip -- blurrily_storage_cluster_centres (include/blurrily_storage.h): the
// clusters of blurrily_storage_cluster with each node's degree, each component's centre and whether a node shares an
// edge with its centre.  The call sequence is ClusterCall's (cluster_host.h), with four more words per number on the
// device and, when the caller asks for `attached`, a second sweep; the sweeps and the centres are
// cluster_centres_kernels.hip's, the node tables and the labels cluster_kernels.hip's kernels as they are.
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

extern "C" int blurrily_storage_cluster_centres(trigram_map m, const uint32_t* references, size_t n,
                                                uint32_t min_permille, uint32_t* labels, uint32_t* degrees,
                                                uint32_t* centres, uint8_t* attached, uint32_t* n_clusters,
                                                uint64_t* n_edges) {
  if (!m || min_permille > 1000 || (n && (!references || !labels)) || n > kMaxBatchNeedles) {
    errno = EINVAL;
    return -1;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  if (n_clusters) *n_clusters = 0;
  if (n_edges) *n_edges = 0;
  if (n == 0) return 0;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  ClusterCall c(m, stream);
  if (c.begin(references, n, 1, sizeof(ClusterTotals)) < 0) return -1;
  const size_t nu = c.nu;
  ClusterTotals* d_totals = static_cast<ClusterTotals*>(c.d_totals);
  // four more things per number (degree, the 64-bit word the centres are chosen in, centre, attached), two per element
  uint32_t *d_degree, *d_centre_of, *d_attached, *d_degrees, *d_centres;
  unsigned long long* d_best;
  if (c.more(d_degree, nu * 4, true) < 0 || c.more(d_best, nu * 8, true) < 0 || c.more(d_centre_of, nu * 4) < 0 ||
      c.more(d_attached, nu * 4) < 0 || c.more(d_degrees, n * 4) < 0 || c.more(d_centres, n * 4) < 0)
    return -1;

  // one sweep over every image and chunk: the unions and the degrees, or (mark) the nodes attached to their centres
  auto sweeps = [&](bool mark) {
    return c.sweep(nu, min_permille, d_totals, [&](const ClusterSweepArgs& a) {
      return launch_cluster_centres_sweep({a, d_degree, d_centre_of, d_attached}, mark, stream);
    });
  };
  if (sweeps(false) < 0) return -1;
  const ClusterLabelArgs la = c.label_args();
  if (launch_cluster_label(la, stream) < 0) return -1;
  ClusterCentresArgs ca{la.parent, la.ntri, la.refs, la.inv, d_degree, la.n_nodes, la.n, d_best, d_centre_of, d_attached,
                        d_centres, d_degrees, d_totals};
  if (launch_cluster_centres(ca, stream) < 0) return -1;
  if (attached && sweeps(true) < 0) return -1;                 // (nobody asked: the second sweep is not run)

  ClusterTotals totals{};
  std::vector<uint32_t> att(attached ? nu : 0);                // the device's words per number; bytes per element below
  if (c.read_totals(&totals) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(labels, c.d_labels, n * 4, hipMemcpyDeviceToHost, stream));
  if (degrees) BLURRILY_HIP_TRY(hipMemcpyAsync(degrees, d_degrees, n * 4, hipMemcpyDeviceToHost, stream));
  if (centres) BLURRILY_HIP_TRY(hipMemcpyAsync(centres, d_centres, n * 4, hipMemcpyDeviceToHost, stream));
  if (attached) BLURRILY_HIP_TRY(hipMemcpyAsync(att.data(), d_attached, nu * 4, hipMemcpyDeviceToHost, stream));
  if (c.wait(&totals) < 0) return -1;
  if (attached)
    for (size_t i = 0; i < n; ++i) attached[i] = uint8_t(att[c.inv.empty() ? i : c.inv[i]]);
  if (n_clusters) *n_clusters = totals.clusters;
  if (n_edges) *n_edges = totals.edges;
  return 0;
}
