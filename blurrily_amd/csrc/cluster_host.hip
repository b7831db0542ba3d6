// cluster_host.hip -- ClusterCall (cluster_host.h): what the clustering entries do alike, once.
#include "cluster_host.h"

namespace blurrily {
namespace detail {

int plan_within_blocks(const std::vector<uint32_t>& key_of, uint32_t scope_strategy, ClusterWithinPlan& plan) {
  // the numbers block after block, ascending inside a block (keys that ascend with the numbers already are)
  const size_t nu = key_of.size();
  std::vector<uint32_t>& order = plan.order;
  order.resize(nu);
  if (std::is_sorted(key_of.begin(), key_of.end())) {
    for (size_t u = 0; u < nu; ++u) order[u] = uint32_t(u);
  } else {
    std::vector<uint64_t> keyed(nu);
    for (size_t u = 0; u < nu; ++u) keyed[u] = (uint64_t(key_of[u]) << 32) | u;
    std::sort(keyed.begin(), keyed.end());
    for (size_t u = 0; u < nu; ++u) order[u] = uint32_t(keyed[u]);
  }
  std::vector<ClusterWithinTile>& tiles = plan.tiles;
  for (size_t b = 0; b < nu;) {
    size_t e = b + 1;
    while (e < nu && key_of[order[e]] == key_of[order[b]]) ++e;
    const bool direct = scope_strategy == 2 || (scope_strategy == 0 && e - b <= kClusterWithinDirectMax);
    if (!direct) {
      plan.swept.insert(plan.swept.end(), order.begin() + b, order.begin() + e);
    } else if (e - b > 1) {                                   // (a block of one has no pair to score)
      for (size_t f = b; f < e; f += kClusterWithinTile)
        tiles.push_back({uint32_t(b), uint32_t(f), uint32_t(std::min<size_t>(kClusterWithinTile, e - f))});
    }
    b = e;
  }
  // the tiles that pass over the most members first: the longest workgroups do not start last
  // (equal ones in the plan's order)
  if (tiles.size() > 0x7FFFFFFFull) { errno = EINVAL; return -1; }
  std::vector<uint64_t> by_scan(tiles.size());
  for (size_t t = 0; t < tiles.size(); ++t)
    by_scan[t] = (uint64_t(~(tiles[t].first + tiles[t].count - tiles[t].begin)) << 32) | t;
  std::sort(by_scan.begin(), by_scan.end());
  std::vector<ClusterWithinTile> sorted(tiles.size());
  for (size_t t = 0; t < tiles.size(); ++t) sorted[t] = tiles[uint32_t(by_scan[t])];
  tiles.swap(sorted);
  return 0;
}

int ClusterCall::upload(ClusterWithinPlan& plan, const std::vector<uint32_t>& key_of) {
  const std::vector<ClusterWithinTile>& tiles = plan.tiles;
  if (more(plan.d_tiles, tiles.size() * sizeof(ClusterWithinTile)) < 0 || more(plan.d_swept, plan.swept.size() * 4) < 0 ||
      (!tiles.empty() && more(plan.d_order, nu * 4) < 0) || (!plan.swept.empty() && more(plan.d_block_of, nu * 4) < 0))
    return -1;
  if (plan.d_tiles) {
    BLURRILY_HIP_TRY(hipMemcpyAsync(plan.d_tiles, tiles.data(), tiles.size() * sizeof(ClusterWithinTile), hipMemcpyHostToDevice, stream));
    BLURRILY_HIP_TRY(hipMemcpyAsync(plan.d_order, plan.order.data(), nu * 4, hipMemcpyHostToDevice, stream));
  }
  if (plan.d_swept) {
    BLURRILY_HIP_TRY(hipMemcpyAsync(plan.d_swept, plan.swept.data(), plan.swept.size() * 4, hipMemcpyHostToDevice, stream));
    BLURRILY_HIP_TRY(hipMemcpyAsync(plan.d_block_of, key_of.data(), nu * 4, hipMemcpyHostToDevice, stream));
  }
  return 0;
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

}  // namespace detail
}  // namespace blurrily
