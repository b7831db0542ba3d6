// map_log.hip -- the mutation log between the host index and the device images (DESIGN.md "Mutation and device sync"):
// what the base image does not hold yet, the delta image of pending puts, the tombstones.
#include "map_internal.h"

using namespace blurrily;
using namespace blurrily::detail;

namespace {

// deletes since the last find: set their bits in the tombstone bitmap, in stream order with the find
__global__ void apply_tombstones_kernel(uint32_t* __restrict__ tomb, const uint32_t* __restrict__ ranks, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicOr(&tomb[ranks[i] >> 5], 1u << (ranks[i] & 31));
}

}  // namespace

namespace blurrily {
namespace detail {

size_t log_budget(const trigram_map m) { return std::max<size_t>(4096, m->dev.n_refs / 64); }

static void clear_log(trigram_map m) {
  m->pending.clear();
  m->n_tomb = 0;
  m->tomb_queue.clear();
  m->log_overflow = false;
  ++m->log_version;
  m->delta_version = m->log_version;
  if (m->delta.device >= 0) device_index_free(&m->delta);
  delete m->delta_host;
  m->delta_host = nullptr;
}

// (a replica's side map holds clones of the images; the log they were cloned at is the primary's)
const trigram_map_t* log_of(const trigram_map_t* m) { return m->mirror_of ? m->mirror_of : m; }
bool log_empty(const trigram_map_t* m) { const trigram_map_t* l = log_of(m); return l->pending.empty() && l->n_tomb == 0 && !l->log_overflow; }

// Bring the device side up to date with the host index.  Small logs are served by a delta
// image (built from the pending puts only) plus tombstones on the base image; a log past
// 1/64 of the base (or 4096 mutations) triggers a full rebuild.
int ensure_device(trigram_map m) {
  const bool have_base = m->dev.device >= 0;
  if (!have_base || m->log_overflow || m->pending.size() + m->n_tomb > log_budget(m)) {
    if (device_index_build(*m->host, &m->dev, m->sweep.build_opt) < 0) return -1;
    ++m->base_builds;
    forget_choices(m);                                 // a new image: measure again
    clear_log(m);
    if (m->n_cus == 0) {
      hipDeviceProp_t prop;
      BLURRILY_HIP_TRY(hipGetDeviceProperties(&prop, m->dev.device));
      m->n_cus = prop.multiProcessorCount;
    }
    return 0;
  }
  if (log_empty(m) || m->delta_version == m->log_version) return 0;
  // The delta host index is kept in step by log_put / log_delete; its device image is rebuilt only
  // when the set of pending puts changed (a delete of a base reference is a tombstone, no rebuild).
  if (m->delta_image_version != m->delta_puts_version) {
    if (m->pending.empty()) {
      if (m->delta.device >= 0) device_index_free(&m->delta);
    } else if (device_index_build(*m->delta_host, &m->delta, m->sweep.build_opt) < 0) {
      return -1;
    }
    m->delta_image_version = m->delta_puts_version;
  }
  // whole-map bucket sizes (nb_entries of the base run)
  std::vector<uint32_t> totals(kNumCodes);
  for (uint32_t t = 0; t < kNumCodes; ++t) totals[t] = m->host->bucket(t).used;
  if (m->d_code_total_now.alloc(kNumCodes) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemcpy(m->d_code_total_now, totals.data(), kNumCodes * sizeof(uint32_t), hipMemcpyHostToDevice));
  m->delta_version = m->log_version;
  return 0;
}

// Host side of put/delete after the base image exists: log what the image is missing.
void log_put(trigram_map m, const char* needle, size_t len, uint32_t ref, uint32_t weight) {
  if (m->dev.device < 0 || m->log_overflow) return;    // no image yet / rebuild pending: nothing to track
  if (m->pending.size() >= log_budget(m)) {            // bulk import: stop logging, rebuild at the next find
    m->pending.clear();
    m->log_overflow = true;
    return;
  }
  if (!m->delta_host) m->delta_host = new HostIndex();
  if (m->delta_host->put(needle, len, ref, weight) < 0) {   // (out of memory) the delta image would miss it:
    m->pending.clear();                                     // fold everything into a rebuilt base instead
    m->log_overflow = true;
    return;
  }
  m->pending[ref] = PendingPut{std::string(needle, len), weight};
  ++m->delta_puts_version;
  ++m->log_version;
}

int log_delete(trigram_map m, uint32_t ref) {
  if (m->dev.device < 0 || m->log_overflow) return 0;
  ++m->log_version;
  if (m->pending.erase(ref)) {                         // never reached the base image
    if (m->delta_host) m->delta_host->del(ref);
    ++m->delta_puts_version;
    return 0;
  }
  const int64_t rk = device_index_rank_of(m->dev, ref);
  if (rk < 0) return 0;
  // the tombstone bit is set by the next find, on that find's stream (apply_tombstones): no
  // synchronous round trip per delete, and ordered with whatever stream the caller finds on
  m->tomb_queue.push_back(uint32_t(rk));
  ++m->n_tomb;
  return 0;
}

// Upload the queued tombstone ranks and set their bits, ordered before the find on `stream`.
int apply_tombstones(trigram_map m, hipStream_t stream) {
  if (m->tomb_queue.empty()) return 0;
  const size_t n = m->tomb_queue.size();
  if (m->ws_tomb.reserve(n * sizeof(uint32_t), stream) < 0) return -1;
  // Deletes are rare on this path: a synchronous copy (the queue may be cleared when it returns, whatever the
  // runtime does with a pageable source), the kernel on the find's stream, and a wait for it -- so that the bits
  // are set for every stream and for device_info / debug reads, not only for finds on this one.
  BLURRILY_HIP_TRY(hipMemcpy(m->ws_tomb.p, m->tomb_queue.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(apply_tombstones_kernel, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, stream, m->dev.d_tomb,
                     static_cast<const uint32_t*>(m->ws_tomb.p), uint32_t(n));
  BLURRILY_HIP_TRY(hipGetLastError());
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  m->tomb_queue.clear();
  return 0;
}

MapImages map_images(trigram_map m) {
  const bool with_delta = !log_of(m)->pending.empty() && m->delta.device >= 0;
  return MapImages{with_delta ? 2u : 1u, {&m->dev, &m->delta}, {log_of(m)->n_tomb ? m->dev.d_tomb : nullptr, nullptr}};
}

int map_ready(trigram_map m, hipStream_t stream) {
  if (m->host->dirty_buckets()) m->host->sort_dirty_buckets();
  if (ensure_device(m) < 0) return -1;
  return apply_tombstones(m, stream);
}

}  // namespace detail
}  // namespace blurrily
