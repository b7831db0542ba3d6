// cluster_cores_within.hip -- blurrily_storage_cluster_cores_within (include/blurrily_storage.h):
// blurrily_storage_cluster_cores' cores, borders and noise within caller-given blocks, one call for all blocks.  The call
// sequence is ClusterCall's (cluster_host.h) over a numbering made here, before a GPU is asked for, because the
// numbering is where a reference listed under two keys shows; the plan is begin_blocked's, as cluster_within.hip's, with
// cluster_cores.hip's two more words per number and its larger totals.  Two passes, the degrees and then, when they are
// final, the unions between cores and the borders' anchors; in each the swept blocks go first and the directly scored
// ones behind them into the same words (cluster_cores_within_kernels.hip).  The labels are cluster_cores_kernels.hip's
// kernel as it is, the node tables cluster_kernels.hip's.
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

extern "C" int blurrily_storage_cluster_cores_within(trigram_map m, const uint32_t* references, const uint32_t* blocks,
                                                     size_t n, uint32_t min_permille, uint32_t min_degree,
                                                     uint32_t* labels, uint32_t* degrees, uint8_t* kinds,
                                                     uint32_t* n_clusters, uint64_t* n_edges, uint64_t* n_core_edges) {
  if (!m || min_permille > 1000 || (n && (!references || !blocks || !labels)) || n > kMaxBatchNeedles) {
    errno = EINVAL;
    return -1;
  }
  std::vector<uint32_t> uniq, inv, key_of;
  if (n && !number_nodes_keyed(references, blocks, n, uniq, inv, key_of)) {
    errno = EINVAL;                                           // a reference listed under two keys
    return -1;
  }
  if (n == 0) {                                               // nothing listed: no GPU is asked for
    if (n_clusters) *n_clusters = 0;
    if (n_edges) *n_edges = 0;
    if (n_core_edges) *n_core_edges = 0;
    return 0;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  // the plan: the numbers block after block, every block the direct kernel's or the sweep's
  ClusterCall c(m, stream);
  if (c.begin_blocked(std::move(uniq), std::move(inv), key_of, n, sizeof(ClusterCoresTotals)) < 0) return -1;
  const size_t nu = c.nu;
  ClusterCoresTotals* d_totals = static_cast<ClusterCoresTotals*>(c.d_totals);
  // a degree word and a 64-bit anchor word per number, a degree and a kind per element
  uint32_t *d_degree, *d_degrees;
  unsigned long long* d_anchor;
  uint8_t* d_kinds;
  if (c.more(d_degree, nu * 4, true) < 0 || c.more(d_anchor, nu * 8, true) < 0 || c.more(d_degrees, n * 4) < 0 ||
      c.more(d_kinds, n) < 0)
    return -1;

  // one pass over every block: the large blocks over the images, then the small ones from the extraction's codes --
  // the degrees, or (unite) the unions between cores and the borders' anchors
  auto pass = [&](bool unite) {
    if (c.sweep(c.plan.swept.size(), min_permille, nullptr, [&](const ClusterSweepArgs& a) {
          return launch_cluster_cores_within_sweep({{a, d_degree, d_anchor, min_degree, d_totals}, c.d_swept, c.d_block_of},
                                                   unite, stream);
        }) < 0)
      return -1;
    return launch_cluster_cores_within({c.within_args(min_permille, c.d_parent, nullptr), d_degree, d_anchor, min_degree,
                                        d_totals},
                                       unite, stream);
  };
  if (pass(false) < 0 || pass(true) < 0) return -1;            // (the second reads the degrees the first has finished)

  ClusterCoresLabelArgs la{c.d_parent, c.x.needles.ntri, c.d_refs, c.d_inv, d_degree, d_anchor, uint32_t(nu), uint32_t(n),
                           min_degree, c.d_labels, d_degrees, d_kinds, d_totals};
  if (launch_cluster_cores_label(la, stream) < 0) return -1;

  ClusterCoresTotals totals{};
  if (c.read_totals(&totals) < 0 || c.wait(&totals.t) < 0) return -1;   // (the outputs are copied out only on success)
  BLURRILY_HIP_TRY(hipMemcpyAsync(labels, c.d_labels, n * 4, hipMemcpyDeviceToHost, stream));
  if (degrees) BLURRILY_HIP_TRY(hipMemcpyAsync(degrees, d_degrees, n * 4, hipMemcpyDeviceToHost, stream));
  if (kinds) BLURRILY_HIP_TRY(hipMemcpyAsync(kinds, d_kinds, n, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  if (n_clusters) *n_clusters = totals.t.clusters;
  if (n_edges) *n_edges = totals.t.edges;
  if (n_core_edges) *n_core_edges = totals.core_edges;
  return 0;
}
