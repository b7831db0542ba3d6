// cluster_extend.hip -- blurrily_storage_cluster_extend (include/blurrily_storage.h): the clusters
// of old and new references together, from the labels the caller holds for the old ones.  It follows cluster.hip step
// for step over the concatenation old ++ new, with two things more on the device -- a bit per number for "new" and the
// list of the new numbers -- a seed launch in front of the sweeps, and the sweeps over the new numbers alone.  The
// seeds and the sweep are cluster_extend_kernels.hip's, the node tables and the labels cluster_kernels.hip's kernels
// as they are.
#include "map_internal.h"
#include "cluster.h"
#include "cluster_host.h"

using namespace blurrily;
using namespace blurrily::detail;

namespace {

// what a call holds on the device beyond ClusterScratch, freed on the way out
struct ExtendScratch {
  DeviceBuffer old_labels, is_new, new_nodes;
  ~ExtendScratch() { for (DeviceBuffer* b : {&old_labels, &is_new, &new_nodes}) b->release(); }
};

}  // namespace

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

  // the numbering over old ++ new (1 .. n then n + 1 .. n + k ascends strictly: no sort), and which numbers are new
  std::vector<uint32_t> uniq, inv;
  {
    std::vector<uint32_t> all(n);
    std::copy(old_refs, old_refs + n_old, all.begin());
    std::copy(new_refs, new_refs + n_new, all.begin() + n_old);
    number_nodes(all.data(), n, uniq, inv);
  }
  const size_t nu = uniq.size();
  std::vector<uint32_t> is_new((nu + 31) / 32, 0u), new_nodes(inv.empty() ? n_new : 0);
  if (inv.empty()) {
    for (size_t j = 0; j < n_new; ++j) new_nodes[j] = uint32_t(n_old + j);
    for (uint32_t u : new_nodes) is_new[u >> 5] |= 1u << (u & 31u);
  } else {
    for (size_t j = 0; j < n_new; ++j) is_new[inv[n_old + j] >> 5] |= 1u << (inv[n_old + j] & 31u);
    for (size_t u = 0; u < nu; ++u)
      if ((is_new[u >> 5] >> (u & 31u)) & 1u) new_nodes.push_back(uint32_t(u));
  }
  const size_t nn = new_nodes.size();

  ClusterScratch S;
  ExtendScratch X;
  if (S.refs.reserve(nu * 4, stream) < 0 || S.parent.reserve(nu * 4, stream) < 0 ||
      S.labels.reserve(n * 4, stream) < 0 || S.totals.reserve(sizeof(ClusterTotals), stream) < 0 ||
      (!inv.empty() && S.inv.reserve(n * 4, stream) < 0) || X.is_new.reserve(is_new.size() * 4, stream) < 0 ||
      (n_old && X.old_labels.reserve(n_old * 4, stream) < 0) || (nn && X.new_nodes.reserve(nn * 4, stream) < 0))
    return -1;
  uint32_t* d_refs = static_cast<uint32_t*>(S.refs.p);
  const uint32_t* d_inv = inv.empty() ? nullptr : static_cast<const uint32_t*>(S.inv.p);
  const uint32_t* d_is_new = static_cast<const uint32_t*>(X.is_new.p);
  ClusterTotals* d_totals = static_cast<ClusterTotals*>(S.totals.p);
  BLURRILY_HIP_TRY(hipMemcpyAsync(d_refs, uniq.data(), nu * 4, hipMemcpyHostToDevice, stream));
  if (!inv.empty()) BLURRILY_HIP_TRY(hipMemcpyAsync(S.inv.p, inv.data(), n * 4, hipMemcpyHostToDevice, stream));
  BLURRILY_HIP_TRY(hipMemcpyAsync(X.is_new.p, is_new.data(), is_new.size() * 4, hipMemcpyHostToDevice, stream));
  if (n_old) BLURRILY_HIP_TRY(hipMemcpyAsync(X.old_labels.p, old_labels, n_old * 4, hipMemcpyHostToDevice, stream));
  if (nn) BLURRILY_HIP_TRY(hipMemcpyAsync(X.new_nodes.p, new_nodes.data(), nn * 4, hipMemcpyHostToDevice, stream));
  BLURRILY_HIP_TRY(hipMemsetAsync(d_totals, 0, sizeof(ClusterTotals), stream));

  RefExtract x;                                                // the by-reference front end (section 11), over every node
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

  // the seeds: what the caller's labels say of the old-old edges (the old elements come first in inv)
  ClusterExtendSeedArgs sa{static_cast<const uint32_t*>(X.old_labels.p), d_inv, d_refs, x.needles.ntri, d_is_new,
                           uint32_t(n_old), uint32_t(nu), na.parent, d_totals};
  if (launch_cluster_extend_seed(sa, stream) < 0) return -1;

  // the new nodes over every window of both images
  for (uint32_t i = 0; i < I.n; ++i) {
    const DeviceIndex& ix = *I.img[i];
    for (size_t s = 0; s < nn; s += kClusterChunkNeedles) {
      const size_t nc = std::min(kClusterChunkNeedles, nn - s);
      ClusterExtendSweepArgs A{};
      ClusterSweepArgs& a = A.s;
      a.slice_se = ix.d_slice_se; a.ent = ix.d_ent; a.win_max_tri = ix.d_win_max_tri; a.win_min_tri = tab[i].win_min_tri;
      a.ntri_of_rank = tab[i].ntri_of_rank; a.n_windows = ix.n_windows; a.n_refs = ix.n_refs; a.dense_min8 = ix.dense_min8;
      a.per = windows_per_workgroup(m, ix, nc); a.win0 = i ? x.win0_delta : 0u;
      a.qcodes = x.needles.codes; a.qoff = x.needles.qoff; a.q_ntri = x.needles.ntri; a.loc = x.loc;
      a.q_base = uint32_t(s); a.n = uint32_t(nc); a.n_nodes = uint32_t(nu); a.min_permille = min_permille;
      a.node_of_pos = na.node_of_pos; a.parent = na.parent; a.totals = d_totals;
      A.new_nodes = static_cast<const uint32_t*>(X.new_nodes.p); A.is_new = d_is_new;
      if (launch_cluster_extend_sweep(A, stream) < 0) return -1;
    }
  }

  ClusterLabelArgs la{na.parent, x.needles.ntri, d_refs, d_inv, uint32_t(nu), uint32_t(n),
                      static_cast<uint32_t*>(S.labels.p), d_totals};
  if (launch_cluster_label(la, stream) < 0) return -1;
  ClusterTotals totals{};
  BLURRILY_HIP_TRY(hipMemcpyAsync(&totals, d_totals, sizeof totals, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  if (totals.error) { errno = EIO; return -1; }                // (the labels are copied out only on success)
  const uint32_t* d_labels = static_cast<const uint32_t*>(S.labels.p);
  if (n_old) BLURRILY_HIP_TRY(hipMemcpyAsync(labels_old, d_labels, n_old * 4, hipMemcpyDeviceToHost, stream));
  if (n_new) BLURRILY_HIP_TRY(hipMemcpyAsync(labels_new, d_labels + n_old, n_new * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  if (n_clusters) *n_clusters = totals.clusters;
  if (n_edges) *n_edges = totals.edges;
  return 0;
}
