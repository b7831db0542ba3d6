// cluster_host.hip -- ClusterCall and TreeRounds (cluster_host.h; DESIGN.md sections 25 and 40): what the clustering
// entries do alike, once.
#include "cluster_host.h"

namespace blurrily {
namespace detail {

int ClusterCall::begin_blocked(std::vector<uint32_t>&& numbering, std::vector<uint32_t>&& element_number,
                               const std::vector<uint32_t>& key_of, size_t n_listed, size_t n_totals_bytes) {
  if (plan_within_blocks(key_of, m->scope_strategy, plan) < 0 ||
      begin(std::move(numbering), std::move(element_number), n_listed, 1, n_totals_bytes) < 0)
    return -1;
  const std::vector<ClusterWithinTile>& tiles = plan.tiles;
  if (more(d_tiles, tiles.size() * sizeof(ClusterWithinTile)) < 0 || more(d_swept, plan.swept.size() * 4) < 0 ||
      (!tiles.empty() && more(d_order, nu * 4) < 0) || (!plan.swept.empty() && more(d_block_of, nu * 4) < 0))
    return -1;
  if (d_tiles) {
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(ClusterWithinTile), hipMemcpyHostToDevice, stream));
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_order, plan.order.data(), nu * 4, hipMemcpyHostToDevice, stream));
  }
  if (d_swept) {
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_swept, plan.swept.data(), plan.swept.size() * 4, hipMemcpyHostToDevice, stream));
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_block_of, key_of.data(), nu * 4, hipMemcpyHostToDevice, stream));
  }
  return 0;
}

ClusterWithinArgs ClusterCall::within_args(uint32_t min_permille, uint32_t* parent, ClusterTotals* totals) const {
  return {d_tiles, d_order, uint32_t(plan.tiles.size()), uint32_t(nu), x.needles.codes, x.needles.qoff, x.needles.ntri,
          uint32_t(nu), min_permille, parent, totals};
}

ClusterCall::~ClusterCall() {
  for (void* p : buffers) (void)hipFree(p);
}

int ClusterCall::alloc(void** p, size_t bytes, bool zeroed) {
  if (bytes == 0) return 0;
  BLURRILY_HIP_TRY(hipMalloc(p, bytes));
  buffers.push_back(*p);
  if (zeroed) BLURRILY_HIP_TRY(hipMemsetAsync(*p, 0, bytes, stream));
  return 0;
}

int ClusterCall::begin(const uint32_t* references, size_t n_listed, uint32_t n_forests, size_t n_totals_bytes) {
  std::vector<uint32_t> numbering, element_number;
  number_nodes(references, n_listed, numbering, element_number);
  return begin(std::move(numbering), std::move(element_number), n_listed, n_forests, n_totals_bytes);
}

int ClusterCall::begin(std::vector<uint32_t>&& numbering, std::vector<uint32_t>&& element_number, size_t n_listed,
                       uint32_t n_forests, size_t n_totals_bytes) {
  n = n_listed; forests = n_forests; totals_bytes = n_totals_bytes;
  uniq = std::move(numbering);
  inv = std::move(element_number);
  nu = uniq.size();
  uint32_t* up_inv = nullptr;
  if (more(d_refs, nu * 4) < 0 || more(d_parent, forests * nu * 4) < 0 || more(d_labels, forests * n * 4) < 0 ||
      more(d_totals, totals_bytes) < 0 || more(up_inv, inv.size() * 4) < 0)
    return -1;
  d_inv = up_inv;
  BLURRILY_HIP_TRY(hipMemcpyAsync(d_refs, uniq.data(), nu * 4, hipMemcpyHostToDevice, stream));
  if (up_inv) BLURRILY_HIP_TRY(hipMemcpyAsync(up_inv, inv.data(), n * 4, hipMemcpyHostToDevice, stream));
  BLURRILY_HIP_TRY(hipMemsetAsync(d_totals, 0, totals_bytes, stream));

  if (refs_extract(m, d_refs, nu, stream, &x) < 0) return -1;
  images = map_images(m);
  for (uint32_t i = 0; i < images.n; ++i)
    if (similar_table(images.img[i], stream, tables, &tab[i]) < 0) return -1;

  // the node tables: a word per position of both images, a parent per number and forest
  const uint64_t n_pos = (uint64_t(images.img[0]->n_windows) + (images.n > 1 ? images.img[1]->n_windows : 0u)) * kWindowRanks;
  if (n_pos > 0xFFFFFFFFull) { errno = ENOMEM; return -1; }
  if (more(d_node_of_pos, std::max<size_t>(n_pos * 4, 16)) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemsetAsync(d_node_of_pos, 0xFF, n_pos * 4, stream));   // (kNoNode)
  for (uint32_t k = 0; k < forests; ++k) {                   // (every forest writes the same node words)
    ClusterNodesArgs na{x.loc, x.needles.ntri, uint32_t(nu), d_node_of_pos, d_parent + k * nu};
    if (launch_cluster_nodes(na, stream) < 0) return -1;
  }
  return 0;
}

ClusterLabelArgs ClusterCall::label_args(uint32_t k) const {
  return {d_parent + k * nu, x.needles.ntri, d_refs, d_inv, uint32_t(nu), uint32_t(n), d_labels + k * n,
          static_cast<ClusterTotals*>(d_totals) + k};
}

int ClusterCall::read_totals(void* host) {
  BLURRILY_HIP_TRY(hipMemcpyAsync(host, d_totals, totals_bytes, hipMemcpyDeviceToHost, stream));
  return 0;
}

int ClusterCall::wait(const ClusterTotals* t) {
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  for (uint32_t k = 0; k < forests; ++k)
    if (t[k].error) { errno = EIO; return -1; }
  return 0;
}

int ClusterCall::deliver_edges(const ClusterEdgesOut& out, blurrily_cluster_merge_t* edges, uint64_t capacity,
                               uint64_t* n_edges) {
  ClusterTotals totals{};
  if (read_totals(&totals) < 0 || wait(&totals) < 0) return -1;
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
    if (more(d_sorted, E * sizeof(ClusterEdgeKey)) < 0) return -1;
    const uint32_t off[2] = {0u, uint32_t(E)};                // (E <= room <= 2^31)
    if (segmented_sort(out.keys, d_sorted, off, 1, 2, false, tables, stream) < 0) return -1;
    sorted = d_sorted;
  }
  ClusterTreeMerge* d_rows = nullptr;
  if (more(d_rows, E * sizeof(ClusterTreeMerge)) < 0) return -1;
  if (launch_cluster_edges_rows({sorted, d_refs, uint32_t(E), uint32_t(nu), d_rows}, stream) < 0) return -1;
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));             // (the records are copied out only on success)
  BLURRILY_HIP_TRY(hipMemcpyAsync(edges, d_rows, E * sizeof(ClusterTreeMerge), hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

int TreeRounds::begin(ClusterCall& c, ClusterTotals* d_totals) {
  const size_t nu = c.nu;
  stream = c.stream;
  if (c.more(r.best, nu * 8, true) < 0 || c.more(r.comp, nu * 4) < 0 || c.more(r.closed, nu, true) < 0 ||
      c.more(r.merges, nu * sizeof(ClusterTreeMerge)) < 0 || c.more(r.n_merges, 16, true) < 0)
    return -1;
  r.parent = c.d_parent; r.refs = c.d_refs; r.n_nodes = uint32_t(nu); r.totals = d_totals;
  return launch_cluster_tree_flatten(r, stream);
}

int TreeRounds::merge_and_count(uint32_t& now) {
  if (launch_cluster_tree_merge(r, stream) < 0 || launch_cluster_tree_flatten(r, stream) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(&now, r.n_merges, 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

int TreeRounds::read_records() {
  got = std::vector<ClusterTreeMerge>(found);
  if (found)
    BLURRILY_HIP_TRY(hipMemcpyAsync(got.data(), r.merges, found * sizeof(ClusterTreeMerge), hipMemcpyDeviceToHost, stream));
  return 0;
}

void TreeRounds::deliver(blurrily_cluster_merge_t* merges) {
  sort_tree_records(got);
  for (uint32_t i = 0; i < found; ++i) merges[i] = {got[i].a, got[i].b, got[i].permille};
}

}  // namespace detail
}  // namespace blurrily
