// cluster_cores.hip -- blurrily_storage_cluster_cores (include/blurrily_storage.h): density-based
// clusters over the edges of blurrily_storage_cluster -- cores, borders and noise.  The call sequence is ClusterCall's
// (cluster_host.h), with two more words per number on the device and always two sweeps: the degrees first, then, when
// they are final, the unions of the edges between cores and the borders' anchors.  The sweeps and the labels are
// cluster_cores_kernels.hip's, the node tables cluster_kernels.hip's kernel as it is.
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

extern "C" int blurrily_storage_cluster_cores(trigram_map m, const uint32_t* references, size_t n,
                                              uint32_t min_permille, uint32_t min_degree, uint32_t* labels,
                                              uint32_t* degrees, uint8_t* kinds, uint32_t* n_clusters,
                                              uint64_t* n_edges, uint64_t* n_core_edges) {
  if (!m || min_permille > 1000 || (n && (!references || !labels)) || n > kMaxBatchNeedles) {
    errno = EINVAL;
    return -1;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  if (n_clusters) *n_clusters = 0;
  if (n_edges) *n_edges = 0;
  if (n_core_edges) *n_core_edges = 0;
  if (n == 0) return 0;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  ClusterCall c(m, stream);
  if (c.begin(references, n, 1, sizeof(ClusterCoresTotals)) < 0) return -1;
  const size_t nu = c.nu;
  ClusterCoresTotals* d_totals = static_cast<ClusterCoresTotals*>(c.d_totals);
  // a degree word and a 64-bit anchor word per number, a degree and a kind per element
  uint32_t *d_degree, *d_degrees;
  unsigned long long* d_anchor;
  uint8_t* d_kinds;
  if (c.more(d_degree, nu * 4, true) < 0 || c.more(d_anchor, nu * 8, true) < 0 || c.more(d_degrees, n * 4) < 0 ||
      c.more(d_kinds, n) < 0)
    return -1;

  // one sweep over every image and chunk: the degrees, or (unite) the unions between cores and the borders' anchors
  auto sweeps = [&](bool unite) {
    return c.sweep(nu, min_permille, nullptr, [&](const ClusterSweepArgs& a) {
      return launch_cluster_cores_sweep({a, d_degree, d_anchor, min_degree, d_totals}, unite, stream);
    });
  };
  if (sweeps(false) < 0 || sweeps(true) < 0) return -1;        // (the second reads the degrees the first has finished)

  ClusterCoresLabelArgs la{c.d_parent, c.x.needles.ntri, c.d_refs, c.d_inv, d_degree, d_anchor, uint32_t(nu), uint32_t(n),
                           min_degree, c.d_labels, d_degrees, d_kinds, d_totals};
  if (launch_cluster_cores_label(la, stream) < 0) return -1;

  ClusterCoresTotals totals{};
  if (c.read_totals(&totals) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(labels, c.d_labels, n * 4, hipMemcpyDeviceToHost, stream));
  if (degrees) BLURRILY_HIP_TRY(hipMemcpyAsync(degrees, d_degrees, n * 4, hipMemcpyDeviceToHost, stream));
  if (kinds) BLURRILY_HIP_TRY(hipMemcpyAsync(kinds, d_kinds, n, hipMemcpyDeviceToHost, stream));
  if (c.wait(&totals.t) < 0) return -1;
  if (n_clusters) *n_clusters = totals.t.clusters;
  if (n_edges) *n_edges = totals.t.edges;
  if (n_core_edges) *n_core_edges = totals.core_edges;
  return 0;
}
