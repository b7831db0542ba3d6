// cluster_cores.hip -- blurrily_storage_cluster_cores (include/blurrily_storage.h): density-based
// clusters over the edges of blurrily_storage_cluster -- cores, borders and noise.  It follows cluster_centres.hip step
// for step, with a degree word and a 64-bit anchor word per number on the device and always two sweeps: the degrees
// first, then, when they are final, the unions of the edges between cores and the borders' anchors.  The sweeps and
// the labels are cluster_cores_kernels.hip's, the node tables cluster_kernels.hip's kernel as it is.
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

namespace {

// what a call holds on the device beyond ClusterScratch, freed on the way out
struct CoresScratch {
  DeviceBuffer degree, anchor, degrees, kinds;
  ~CoresScratch() { for (DeviceBuffer* b : {&degree, &anchor, &degrees, &kinds}) b->release(); }
};

}  // namespace

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

  std::vector<uint32_t> uniq, inv;
  number_nodes(references, n, uniq, inv);
  const size_t nu = uniq.size();
  ClusterScratch S;
  CoresScratch X;
  if (S.refs.reserve(nu * 4, stream) < 0 || S.parent.reserve(nu * 4, stream) < 0 ||
      S.labels.reserve(n * 4, stream) < 0 || S.totals.reserve(sizeof(ClusterCoresTotals), stream) < 0 ||
      (!inv.empty() && S.inv.reserve(n * 4, stream) < 0) || X.degree.reserve(nu * 4, stream) < 0 ||
      X.anchor.reserve(nu * 8, stream) < 0 || X.degrees.reserve(n * 4, stream) < 0 || X.kinds.reserve(n, stream) < 0)
    return -1;
  uint32_t* d_refs = static_cast<uint32_t*>(S.refs.p);
  uint32_t* d_degree = static_cast<uint32_t*>(X.degree.p);
  unsigned long long* d_anchor = static_cast<unsigned long long*>(X.anchor.p);
  ClusterCoresTotals* d_totals = static_cast<ClusterCoresTotals*>(S.totals.p);
  BLURRILY_HIP_TRY(hipMemcpyAsync(d_refs, uniq.data(), nu * 4, hipMemcpyHostToDevice, stream));
  if (!inv.empty()) BLURRILY_HIP_TRY(hipMemcpyAsync(S.inv.p, inv.data(), n * 4, hipMemcpyHostToDevice, stream));
  BLURRILY_HIP_TRY(hipMemsetAsync(d_totals, 0, sizeof(ClusterCoresTotals), stream));
  BLURRILY_HIP_TRY(hipMemsetAsync(d_degree, 0, nu * 4, stream));
  BLURRILY_HIP_TRY(hipMemsetAsync(d_anchor, 0, nu * 8, stream));

  RefExtract x;                                                // the by-reference front end (section 11)
  if (refs_extract(m, d_refs, nu, stream, &x) < 0) return -1;
  const MapImages I = map_images(m);                           // (the images the extraction looked the references up in)
  SimilarTables call;
  SimilarTable tab[2];
  for (uint32_t i = 0; i < I.n; ++i)
    if (similar_table(I.img[i], stream, call, &tab[i]) < 0) return -1;

  // the node tables: a word per position of both images, a parent per number
  const uint64_t n_pos = (uint64_t(I.img[0]->n_windows) + (I.n > 1 ? I.img[1]->n_windows : 0u)) * kWindowRanks;
  if (n_pos > 0xFFFFFFFFull) { errno = ENOMEM; return -1; }
  if (S.node_of_pos.reserve(std::max<size_t>(n_pos * 4, 16), stream) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemsetAsync(S.node_of_pos.p, 0xFF, n_pos * 4, stream));   // (kNoNode)
  ClusterNodesArgs na{x.loc, x.needles.ntri, uint32_t(nu), static_cast<uint32_t*>(S.node_of_pos.p),
                      static_cast<uint32_t*>(S.parent.p)};
  if (launch_cluster_nodes(na, stream) < 0) return -1;

  // one sweep over every image and chunk: the degrees, or (unite) the unions between cores and the borders' anchors
  auto sweeps = [&](bool unite) -> int {
    for (uint32_t i = 0; i < I.n; ++i) {
      const DeviceIndex& ix = *I.img[i];
      for (size_t s = 0; s < nu; s += kClusterChunkNeedles) {
        const size_t nc = std::min(kClusterChunkNeedles, nu - s);
        ClusterCoresSweepArgs A{};
        ClusterSweepArgs& a = A.s;
        a.slice_se = ix.d_slice_se; a.ent = ix.d_ent; a.win_max_tri = ix.d_win_max_tri; a.win_min_tri = tab[i].win_min_tri;
        a.ntri_of_rank = tab[i].ntri_of_rank; a.n_windows = ix.n_windows; a.n_refs = ix.n_refs; a.dense_min8 = ix.dense_min8;
        a.per = windows_per_workgroup(m, ix, nc); a.win0 = i ? x.win0_delta : 0u;
        a.qcodes = x.needles.codes; a.qoff = x.needles.qoff; a.q_ntri = x.needles.ntri; a.loc = x.loc;
        a.q_base = uint32_t(s); a.n = uint32_t(nc); a.n_nodes = uint32_t(nu); a.min_permille = min_permille;
        a.node_of_pos = na.node_of_pos; a.parent = na.parent;
        A.degree = d_degree; A.anchor = d_anchor; A.min_degree = min_degree; A.totals = d_totals;
        if (launch_cluster_cores_sweep(A, unite, stream) < 0) return -1;
      }
    }
    return 0;
  };
  if (sweeps(false) < 0 || sweeps(true) < 0) return -1;        // (the second reads the degrees the first has finished)

  const uint32_t* d_inv = inv.empty() ? nullptr : static_cast<const uint32_t*>(S.inv.p);
  ClusterCoresLabelArgs la{na.parent, x.needles.ntri, d_refs, d_inv, d_degree, d_anchor, uint32_t(nu), uint32_t(n),
                           min_degree, static_cast<uint32_t*>(S.labels.p), static_cast<uint32_t*>(X.degrees.p),
                           static_cast<uint8_t*>(X.kinds.p), d_totals};
  if (launch_cluster_cores_label(la, stream) < 0) return -1;

  ClusterCoresTotals totals{};
  BLURRILY_HIP_TRY(hipMemcpyAsync(&totals, d_totals, sizeof totals, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipMemcpyAsync(labels, S.labels.p, n * 4, hipMemcpyDeviceToHost, stream));
  if (degrees) BLURRILY_HIP_TRY(hipMemcpyAsync(degrees, X.degrees.p, n * 4, hipMemcpyDeviceToHost, stream));
  if (kinds) BLURRILY_HIP_TRY(hipMemcpyAsync(kinds, X.kinds.p, n, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  if (totals.t.error) { errno = EIO; return -1; }
  if (n_clusters) *n_clusters = totals.t.clusters;
  if (n_edges) *n_edges = totals.t.edges;
  if (n_core_edges) *n_core_edges = totals.core_edges;
  return 0;
}
