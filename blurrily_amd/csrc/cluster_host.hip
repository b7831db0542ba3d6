// cluster_host.hip -- ClusterCall (cluster_host.h): what the clustering entries do alike, once.
#include "cluster_host.h"

namespace blurrily {
namespace detail {

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
