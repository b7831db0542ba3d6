// c_abi.hip -- extern "C" entry points of libblurrily_hip.so
// (include/blurrily_storage.h).  Part 1 mirrors ext/blurrily/storage.h:36-117.
#include "map_internal.h"

using namespace blurrily;
using namespace blurrily::detail;

// where note_launch() writes: the `last_kernels` of the map whose batch is being enqueued on this thread (NameScope)
namespace blurrily {
namespace detail {
std::string*& launch_names() {
  thread_local std::string* t_launch_names = nullptr;
  return t_launch_names;
}
}  // namespace detail
}  // namespace blurrily
namespace blurrily {
void note_launch(const char* kernel_name) {
  std::string* s = detail::launch_names();
  if (!s) return;
  // distinct names, launch order (a window-major batch launches wsweep_kernel once per window)
  const std::string name(kernel_name);
  size_t at = 0;
  while (at <= s->size()) {
    const size_t end = s->find('+', at);
    const std::string have = s->substr(at, end == std::string::npos ? std::string::npos : end - at);
    if (have == name) return;
    if (end == std::string::npos) break;
    at = end + 1;
  }
  if (!s->empty()) *s += '+';
  *s += name;
}
}

extern "C" {

int blurrily_storage_new(trigram_map* haystack) {
  trigram_map m = new (std::nothrow) trigram_map_t();
  if (!m) { errno = ENOMEM; return -1; }
  m->host = new (std::nothrow) HostIndex();
  if (!m->host) { delete m; errno = ENOMEM; return -1; }
  *haystack = m;
  return 0;
}

int blurrily_storage_load(trigram_map* haystack, const char* path) {
  HostIndex* ix = HostIndex::load(path);
  if (!ix) return -1;                                   // errno set by load()
  trigram_map m = new (std::nothrow) trigram_map_t();
  if (!m) { delete ix; errno = ENOMEM; return -1; }
  m->host = ix;
  *haystack = m;
  return 0;
}

int blurrily_storage_close(trigram_map* haystack) {
  trigram_map m = *haystack;
  if (m) {
    DeviceScope scope(m->dev.device);
    for (Replica& r : m->replicas) free_replica(r);
    m->replicas.clear();
    if (m->dev.device >= 0) {
      (void)hipDeviceSynchronize();
      device_index_free(&m->dev);
    }
    if (m->delta.device >= 0) device_index_free(&m->delta);
    delete m->delta_host;
    delete m->host;
    delete m;                                            // (what its finds hold on the device and of the runtime goes with it)
  }
  *haystack = nullptr;
  return 0;
}

void blurrily_storage_mark(trigram_map) {}

int blurrily_storage_save(trigram_map haystack, const char* path) { return haystack->host->save(path); }

int blurrily_storage_put(trigram_map haystack, const char* needle, uint32_t reference, uint32_t weight) {
  const size_t len = std::strlen(needle);
  const int added = haystack->host->put(needle, len, reference, weight);
  if (added > 0) log_put(haystack, needle, len, reference, weight);
  return added;
}

long blurrily_storage_put_many(trigram_map haystack, const char* packed, const uint64_t* offsets,
                               const uint32_t* references, const uint32_t* weights, size_t n) {
  // A bulk import -- no device image to keep in step, or more strings than the mutation log takes:
  // the image is rebuilt at the next find anyway -- goes through the parallel host path.
  const bool tracked = haystack->dev.device >= 0 && !haystack->log_overflow;
  if (n >= 65536 && (!tracked || n > log_budget(haystack))) {
    const long added = haystack->host->put_many(packed, offsets, references, weights, n);
    if (tracked && added > 0) { haystack->pending.clear(); haystack->log_overflow = true; }
    return added;
  }
  long total = 0;
  for (size_t i = 0; i < n; ++i) {
    const char* s = packed + offsets[i];
    const size_t len = needle_len(s, size_t(offsets[i + 1] - offsets[i]));
    const int added = haystack->host->put(s, len, references[i], weights ? weights[i] : 0u);
    if (added > 0) log_put(haystack, s, len, references[i], weights ? weights[i] : 0u);
    total += added;
  }
  return total;
}

int blurrily_storage_delete(trigram_map haystack, uint32_t reference) {
  const int removed = haystack->host->del(reference);
  if (removed > 0 && log_delete(haystack, reference) < 0) return -1;
  return removed;
}

int blurrily_storage_stats(trigram_map haystack, trigram_stat_t* stats) {
  stats->references = haystack->host->total_refs();
  stats->trigrams   = haystack->host->total_trigrams();
  return 0;
}

int blurrily_storage_sync_device(trigram_map haystack) {
  DeviceScope scope(haystack->dev.device);
  haystack->host->sort_dirty_buckets();
  return ensure_device(haystack);
}

int blurrily_storage_find_batch_device(trigram_map m, const char* d_packed, size_t packed_bytes,
                                       const uint64_t* d_offsets, size_t n, uint16_t limit,
                                       trigram_match d_results, uint32_t* d_counts,
                                       uint32_t* d_nb_entries, void* stream) {
  // The needles are not visible to the host here, so every dirty bucket is
  // sorted (the reference sorts only the needle's own, storage.c:516; results
  // are identical, see DESIGN.md "Mutation and device sync").
  DeviceScope scope(m->dev.device);
  if (m->host->dirty_buckets()) m->host->sort_dirty_buckets();
  if (ensure_device(m) < 0) return -1;
  if (wants_multi(m, n))
    return run_find_multi(m, d_packed, packed_bytes, d_offsets, n, limit, d_results, d_counts, d_nb_entries,
                          static_cast<hipStream_t>(stream));
  return run_find(m, d_packed, packed_bytes, d_offsets, n, limit, d_results, d_counts, d_nb_entries, true,
                  true, static_cast<hipStream_t>(stream));
}

int blurrily_storage_find_batch(trigram_map m, const char* packed, const uint64_t* offsets, size_t n,
                                uint16_t limit, trigram_match results, uint32_t* counts) {
  return find_batch_host(m, packed, offsets, n, limit, results, counts, false, nullptr);
}

int blurrily_storage_find_batch_raw(trigram_map m, const char* packed, const uint64_t* offsets, size_t n,
                                    uint16_t limit, trigram_match results, uint32_t* counts,
                                    uint32_t* non_ascii) {
  return find_batch_host(m, packed, offsets, n, limit, results, counts, true, non_ascii);
}

int blurrily_normalize_batch_device(const char* d_packed, const uint64_t* d_offsets, size_t n, char* d_out,
                                    uint32_t* d_non_ascii, void* stream) {
  if (n > 0xFFFFFFFFull) { errno = EINVAL; return -1; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {   // no CPU fallback, here neither
    std::fprintf(stderr, "blurrily_hip: no usable HIP device\n");
    errno = ENODEV;
    return -1;
  }
  return launch_normalise(d_packed, d_offsets, uint32_t(n), d_out, d_non_ascii, static_cast<hipStream_t>(stream));
}

int blurrily_storage_find(trigram_map haystack, const char* needle, uint16_t limit, trigram_match results) {
  {
    const size_t len = std::strlen(needle);
    uint32_t n_rows = 0;
    const int one = find_few(haystack, &needle, &len, 1, limit, results, &n_rows);
    if (one != kOneNotTaken) return one < 0 ? one : int(n_rows);
  }
  const uint64_t offsets[2] = {0, std::strlen(needle)};
  uint32_t count = 0;
  // the device writes `limit` rows per needle; go through a scratch so a short
  // caller buffer is never over-written beyond `limit` rows (it is exactly limit rows)
  if (blurrily_storage_find_batch(haystack, needle, offsets, 1, limit, results, &count) < 0) return -1;
  return int(count);
}

int blurrily_tokeniser_parse_string(const char* input, uint16_t* output) {
  return tokenise(input, std::strlen(input), output);
}

int blurrily_storage_device_info(trigram_map m, blurrily_device_info_t* info) {
  info->device_ordinal = m->dev.device;
  info->n_refs = m->dev.n_refs;
  info->n_windows = m->dev.n_windows;
  info->window_bits = kWindowBits;
  info->n_entries = m->dev.n_entries;
  info->device_bytes = m->dev.device_bytes;
  info->last_find_kernel_ms = m->last_find_ms;
  info->last_tokenise_kernel_ms = m->last_tok_ms;
  info->n_pending = uint32_t(m->pending.size());
  info->n_tombstones = uint32_t(m->n_tomb);
  info->base_builds = m->base_builds;
  info->mean_hit_slice = m->dev.mean_hit_slice;
  info->n_bitmaps = m->dev.n_bitmaps;
  info->reserved_ = 0;
  info->dense_share = m->dev.dense_share;
  info->ws_gain = m->dev.ws_gain;
  // what the replicas sit on: physical devices by PCI bus id
  info->n_replicas = uint32_t(m->replicas.size());
  info->peer_access_mask = 0; info->same_device_mask = 0;
  std::memset(info->pci_bus_id, 0, sizeof info->pci_bus_id);
  std::vector<std::string> seen;
  auto bus_of = [](int dev) { char b[32] = {0}; if (dev < 0 || hipDeviceGetPCIBusId(b, sizeof b, dev) != hipSuccess) b[0] = 0; return std::string(b); };
  if (m->dev.device >= 0) {
    const std::string mine = bus_of(m->dev.device);
    std::snprintf(info->pci_bus_id, sizeof info->pci_bus_id, "%s", mine.c_str());
    seen.push_back(mine.empty() ? "dev" + std::to_string(m->dev.device) : mine);
  }
  for (size_t k = 0; k < m->replicas.size(); ++k) {
    const Replica& r = m->replicas[k];
    if (k < 32) { info->peer_access_mask |= uint32_t(r.peer_access) << k; info->same_device_mask |= uint32_t(r.same_device) << k; }
    std::string b = bus_of(r.device);
    if (b.empty()) b = "dev" + std::to_string(r.device);
    if (std::find(seen.begin(), seen.end(), b) == seen.end()) seen.push_back(b);
  }
  info->distinct_devices = uint32_t(seen.size());
  return 0;
}

size_t blurrily_storage_device_info_sized(trigram_map m, void* info, size_t info_size) {
  blurrily_device_info_t full;
  std::memset(&full, 0, sizeof full);
  (void)blurrily_storage_device_info(m, &full);
  std::memcpy(info, &full, std::min(info_size, sizeof full));
  return sizeof full;
}

int blurrily_storage_tune(trigram_map m, const char* packed, const uint64_t* offsets, size_t n_given, size_t n,
                          uint16_t limit) {
  if (!packed || !offsets || n_given == 0 || n == 0) { errno = EINVAL; return -1; }
  // n needles, the given ones over and over: one host-buffer batch in one piece, whose class is then measured by the
  // find itself if it has not been (run_find_on); the rows are thrown away
  std::vector<uint64_t> off(n + 1);
  std::vector<char> buf;
  off[0] = 0;
  for (size_t i = 0; i < n; ++i) {
    const size_t g = i % n_given;
    buf.insert(buf.end(), packed + offsets[g], packed + offsets[g + 1]);
    off[i + 1] = buf.size();
  }
  if (buf.empty()) buf.push_back(0);
  std::vector<trigram_match_t> rows(n * size_t(limit) + 1);
  std::vector<uint32_t> counts(n);
  const uint32_t chunk = m->host_chunk;
  m->host_chunk = 0;
  const int rc = blurrily_storage_find_batch(m, buf.data(), off.data(), n, limit, rows.data(), counts.data());
  m->host_chunk = chunk;
  return rc;
}

void blurrily_storage_set_timing(trigram_map m, int enabled) { m->timing = enabled != 0; }

void blurrily_storage_set_stats(trigram_map m, int enabled) { m->collect_stats = enabled != 0; }

// debugging aid (tools/ws_probe.py): all counter slots, phase clocks of the window-major sweep included
int blurrily_debug_find_stats16(trigram_map m, uint64_t* out16) {
  std::memset(out16, 0, kStatAllSlots * 8);
  if (!m->d_stats) return 0;
  DeviceScope scope(m->dev.device);
  BLURRILY_HIP_TRY(hipDeviceSynchronize());
  BLURRILY_HIP_TRY(hipMemcpy(out16, m->d_stats, kStatAllSlots * 8, hipMemcpyDeviceToHost));
  return 0;
}

int blurrily_storage_find_stats(trigram_map m, uint64_t* out8) {
  std::memset(out8, 0, kStatSlots * 8);
  if (!m->d_stats) return 0;
  DeviceScope scope(m->dev.device);
  BLURRILY_HIP_TRY(hipDeviceSynchronize());
  BLURRILY_HIP_TRY(hipMemcpy(out8, m->d_stats, kStatSlots * 8, hipMemcpyDeviceToHost));
  return 0;
}

size_t blurrily_storage_last_kernels(trigram_map m, char* out, size_t cap) {
  const std::string& s = m->last_kernels;
  if (out && cap) {
    const size_t k = std::min(s.size(), cap - 1);
    std::memcpy(out, s.data(), k);
    out[k] = '\0';
  }
  return s.size();
}

int blurrily_storage_find_path_flags(trigram_map m, uint32_t* out, size_t n) {
  if (!m->ws_flags.p || n > m->n_flags) { errno = EINVAL; return -1; }
  DeviceScope scope(m->dev.device);
  BLURRILY_HIP_TRY(hipDeviceSynchronize());
  BLURRILY_HIP_TRY(hipMemcpy(out, m->ws_flags.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

// debugging aid (tools/phase_profile.py): per-workgroup phase clocks of the last find launched while
// blurrily_storage_set_stats was on
int blurrily_debug_phase_clocks(trigram_map m, unsigned long long* out, size_t n_workgroups) {
  if (!m->d_phase || n_workgroups > kPhaseWorkgroups) { errno = EINVAL; return -1; }
  DeviceScope scope(m->dev.device);
  BLURRILY_HIP_TRY(hipDeviceSynchronize());
  BLURRILY_HIP_TRY(hipMemcpy(out, m->d_phase, n_workgroups * 16 * 8, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
