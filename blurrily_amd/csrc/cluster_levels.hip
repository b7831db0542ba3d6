// cluster_levels.hip -- blurrily_storage_cluster_levels (include/blurrily_storage.h): the
// clusters of blurrily_storage_cluster at up to kClusterMaxLevels floors from one sweep at the lowest of them.  It
// follows cluster.hip step for step, with a forest, a row of labels and a ClusterTotals per level; the sweep is
// cluster_levels_kernels.hip's, the node tables and the labels are cluster_kernels.hip's kernels once per level.
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

static_assert(kClusterMaxLevels == BLURRILY_CLUSTER_MAX_LEVELS, "the header's cap is the kernels'");

extern "C" int blurrily_storage_cluster_levels(trigram_map m, const uint32_t* references, size_t n,
                                               const uint32_t* floors, uint32_t n_floors, uint32_t* labels,
                                               uint32_t* n_clusters, uint64_t* n_edges) {
  bool valid = m && floors && n_floors >= 1 && n_floors <= kClusterMaxLevels && !(n && (!references || !labels)) &&
               n <= kMaxBatchNeedles;
  for (uint32_t k = 0; valid && k < n_floors; ++k) valid = floors[k] <= 1000 && (k == 0 || floors[k - 1] < floors[k]);
  if (!valid) {
    errno = EINVAL;
    return -1;
  }
  DeviceScope scope(m->dev.device);
  hipStream_t stream = nullptr;
  if (map_ready(m, stream) < 0) return -1;
  for (uint32_t k = 0; k < n_floors; ++k) {
    if (n_clusters) n_clusters[k] = 0;
    if (n_edges) n_edges[k] = 0;
  }
  if (n == 0) return 0;
  NameScope names(&m->last_kernels);
  m->last_kernels.clear();

  std::vector<uint32_t> uniq, inv;
  number_nodes(references, n, uniq, inv);
  const size_t nu = uniq.size();
  ClusterScratch S;
  if (S.refs.reserve(nu * 4, stream) < 0 || S.parent.reserve(n_floors * nu * 4, stream) < 0 ||
      S.labels.reserve(n_floors * n * 4, stream) < 0 || S.totals.reserve(n_floors * sizeof(ClusterTotals), stream) < 0 ||
      (!inv.empty() && S.inv.reserve(n * 4, stream) < 0))
    return -1;
  uint32_t* d_refs = static_cast<uint32_t*>(S.refs.p);
  uint32_t* d_parent = static_cast<uint32_t*>(S.parent.p);     // forest k: words [k * nu, k * nu + nu)
  uint32_t* d_labels = static_cast<uint32_t*>(S.labels.p);     // level k: words [k * n, k * n + n), as the caller's
  ClusterTotals* d_totals = static_cast<ClusterTotals*>(S.totals.p);
  BLURRILY_HIP_TRY(hipMemcpyAsync(d_refs, uniq.data(), nu * 4, hipMemcpyHostToDevice, stream));
  if (!inv.empty()) BLURRILY_HIP_TRY(hipMemcpyAsync(S.inv.p, inv.data(), n * 4, hipMemcpyHostToDevice, stream));
  BLURRILY_HIP_TRY(hipMemsetAsync(d_totals, 0, n_floors * sizeof(ClusterTotals), stream));

  RefExtract x;                                                // the by-reference front end (section 11)
  if (refs_extract(m, d_refs, nu, stream, &x) < 0) return -1;
  const MapImages I = map_images(m);                           // (the images the extraction looked the references up in)
  SimilarTables call;
  SimilarTable tab[2];
  for (uint32_t i = 0; i < I.n; ++i)
    if (similar_table(I.img[i], stream, call, &tab[i]) < 0) return -1;

  // the node tables: a word per position of both images, a parent per number and level
  const uint64_t n_pos = (uint64_t(I.img[0]->n_windows) + (I.n > 1 ? I.img[1]->n_windows : 0u)) * kWindowRanks;
  if (n_pos > 0xFFFFFFFFull) { errno = ENOMEM; return -1; }
  if (S.node_of_pos.reserve(std::max<size_t>(n_pos * 4, 16), stream) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemsetAsync(S.node_of_pos.p, 0xFF, n_pos * 4, stream));   // (kNoNode)
  uint32_t* d_node_of_pos = static_cast<uint32_t*>(S.node_of_pos.p);
  for (uint32_t k = 0; k < n_floors; ++k) {                    // (every level writes the same node words)
    ClusterNodesArgs na{x.loc, x.needles.ntri, uint32_t(nu), d_node_of_pos, d_parent + k * nu};
    if (launch_cluster_nodes(na, stream) < 0) return -1;
  }

  for (uint32_t i = 0; i < I.n; ++i) {
    const DeviceIndex& ix = *I.img[i];
    for (size_t s = 0; s < nu; s += kClusterChunkNeedles) {
      const size_t nc = std::min(kClusterChunkNeedles, nu - s);
      ClusterLevelsSweepArgs A{};
      ClusterSweepArgs& a = A.s;
      a.slice_se = ix.d_slice_se; a.ent = ix.d_ent; a.win_max_tri = ix.d_win_max_tri; a.win_min_tri = tab[i].win_min_tri;
      a.ntri_of_rank = tab[i].ntri_of_rank; a.n_windows = ix.n_windows; a.n_refs = ix.n_refs; a.dense_min8 = ix.dense_min8;
      a.per = windows_per_workgroup(m, ix, nc); a.win0 = i ? x.win0_delta : 0u;
      a.qcodes = x.needles.codes; a.qoff = x.needles.qoff; a.q_ntri = x.needles.ntri; a.loc = x.loc;
      a.q_base = uint32_t(s); a.n = uint32_t(nc); a.n_nodes = uint32_t(nu); a.min_permille = floors[0];
      a.node_of_pos = d_node_of_pos; a.parent = d_parent; a.totals = d_totals;
      A.n_floors = n_floors;
      std::copy(floors, floors + n_floors, A.floors);
      if (launch_cluster_levels_sweep(A, stream) < 0) return -1;
    }
  }

  for (uint32_t k = 0; k < n_floors; ++k) {
    ClusterLabelArgs la{d_parent + k * nu, x.needles.ntri, d_refs, inv.empty() ? nullptr : static_cast<const uint32_t*>(S.inv.p),
                        uint32_t(nu), uint32_t(n), d_labels + k * n, d_totals + k};
    if (launch_cluster_label(la, stream) < 0) return -1;
  }
  ClusterTotals totals[kClusterMaxLevels] = {};
  BLURRILY_HIP_TRY(hipMemcpyAsync(totals, d_totals, n_floors * sizeof(ClusterTotals), hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipMemcpyAsync(labels, d_labels, n_floors * n * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  for (uint32_t k = 0; k < n_floors; ++k)
    if (totals[k].error) { errno = EIO; return -1; }
  for (uint32_t k = 0; k < n_floors; ++k) {
    if (n_clusters) n_clusters[k] = totals[k].clusters;
    if (n_edges) n_edges[k] = totals[k].edges;
  }
  return 0;
}
