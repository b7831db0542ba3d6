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
    for (hipEvent_t e : {m->ev_ready, m->ev_t0, m->ev_t1}) if (e) (void)hipEventDestroy(e);
    if (m->dev.device >= 0) {
      (void)hipDeviceSynchronize();
      device_index_free(&m->dev);
    }
    if (m->delta.device >= 0) device_index_free(&m->delta);
    delete m->delta_host;
    if (m->d_code_total_now) (void)hipFree(m->d_code_total_now);
    if (m->d_stats) (void)hipFree(m->d_stats);
    if (m->d_phase) (void)hipFree(m->d_phase);
    m->ws_base_rows.release(); m->ws_base_counts.release(); m->ws_delta_rows.release(); m->ws_delta_counts.release();
    for (auto& e : m->ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : m->tune_ev) if (e) (void)hipEventDestroy(e);
    for (auto& w : m->watch_ev) for (auto& e : w) if (e) (void)hipEventDestroy(e);
    m->ws_codes.release(); m->ws_small.release(); m->ws_parts.release(); m->ws_io_in.release();
    m->ws_io_out.release(); m->ws_tomb.release(); m->ws_flags.release(); m->ws_refs.release();
    m->ws_each.release(); m->ws_each_rows.release();
    if (m->h_stage) (void)hipHostFree(m->h_stage);
    if (m->h_scope) (void)hipHostFree(m->h_scope);
    if (m->one.stream) { (void)hipStreamSynchronize(m->one.stream); (void)hipStreamDestroy(m->one.stream); }
    if (m->one.h_out) (void)hipHostFree(m->one.h_out);
    m->one.d_parts.release();
    for (int i = 0; i < 2; ++i) {
      if (m->pipe.h_in[i]) (void)hipHostFree(m->pipe.h_in[i]);
      if (m->pipe.h_out[i]) (void)hipHostFree(m->pipe.h_out[i]);
      m->pipe.d_in[i].release(); m->pipe.d_out[i].release();
      for (hipEvent_t e : {m->pipe.ev_in[i], m->pipe.ev_run[i], m->pipe.ev_out[i]}) if (e) (void)hipEventDestroy(e);
    }
    for (hipStream_t s : {m->pipe.s_in, m->pipe.s_run, m->pipe.s_out}) if (s) (void)hipStreamDestroy(s);
    delete m->host;
    delete m;
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

// Tunables: one table, so that set and get cannot drift apart.  A map's options are plain fields read by its
// next find (calls on one map are serial, as in the reference: no lock); the process-wide ones are atomics.
namespace {
struct OptionSlot { const char* key; long long lo, hi; };
constexpr OptionSlot kMapOptions[] = {
    {"wsweep", 0, 1}, {"ws_cmin", 1, 64}, {"ws_min_windows", 0, 1 << 20}, {"ws_min_needles", 0, 1ll << 32},
    {"ws_min_slice", 0, 1ll << 31}, {"dense_min", 64, 65536}, {"host_chunk", 0, 1ll << 30},
    {"ws_autotune", 0, 1}, {"ws_static_slice", 0, 1ll << 31}, {"ws_choice", 0, 0},
    {"nm_cmin", 0, 64}, {"nm_dense", 64, 65536}, {"last_sweep", 0, 0}, {"devices", 1, 64},
    {"nm_min_windows", 0, 1 << 20}, {"tuned_class", 0, 0}, {"tuned_nm_us", 0, 0}, {"tuned_ws_us", 0, 0},
    {"tuned_leave_us", 0, 0}, {"small_sweep", 0, 1}, {"small_min_needles", 0, 1ll << 32},
    {"one_launch", 0, 1}, {"one_taken", 0, 0}, {"one_windows_per_wg", 0, 1 << 20},
    {"retunes", 0, 0}, {"tune_inject", 0, 3}, {"mid_workgroups", 64, 1 << 16}, {"few_max", 1, kMidMaxNeedles}, {"mid_max", 0, kMidMaxNeedles},
    {"latency_tasks", 0, 16}, {"scope_strategy", 0, 2}, {"scope_direct_max", 0, 1ll << 40}};
constexpr OptionSlot kProcessOptions[] = {{"host_threads", 0, 256}, {"build_trace", 0, 1}};
int find_option(const OptionSlot* tab, size_t n, const char* key) {
  for (size_t i = 0; i < n; ++i) if (std::strcmp(tab[i].key, key) == 0) return int(i);
  return -1;
}
#define FIND_OPTION(tab, key) find_option(tab, sizeof(tab) / sizeof(tab[0]), key)
}  // namespace

int blurrily_storage_set_option(trigram_map m, const char* key, long long value) {
  if (!key) { errno = EINVAL; return -1; }
  if (!m) {
    const int i = FIND_OPTION(kProcessOptions, key);
    if (i < 0 || value < kProcessOptions[i].lo || value > kProcessOptions[i].hi) { errno = EINVAL; return -1; }
    if (i == 0) set_host_threads(unsigned(value)); else set_build_trace(value != 0);
    return 0;
  }
  const int i = FIND_OPTION(kMapOptions, key);
  if (i < 0 || value < kMapOptions[i].lo || value > kMapOptions[i].hi) { errno = EINVAL; return -1; }
  switch (i) {
    case 0: m->build_opt.ws_enabled = value != 0; break;
    case 1: m->ws_cmin = uint32_t(value); break;
    case 2: m->build_opt.ws_min_windows = uint32_t(value); break;
    case 3: m->ws_min_needles = uint32_t(std::min<long long>(value, 0xFFFFFFFFll)); break;
    case 4: m->build_opt.ws_min_slice = uint32_t(value); break;
    case 5:                                        // which slices have bitmaps: the image is rebuilt by the next find
      if (m->build_opt.dense_min != uint32_t(value) && m->dev.device >= 0) m->log_overflow = true;
      m->build_opt.dense_min = uint32_t(value);
      break;
    case 6: m->host_chunk = uint32_t(value); break;
    case 7: m->ws_autotune = value != 0; break;
    case 8: m->ws_static_slice = uint32_t(value); break;
    case 9: break;                                       // (value 0 only: forget what was measured)
    case 10: m->nm_cmin = uint32_t(value); break;
    case 11: m->nm_dense = uint32_t(value); break;
    case 12: m->last_sweep = 0; return 0;                // (value 0 only; nothing to measure again)
    case 13:                                             // (replicas are made by the next large batch; dropped at once)
      m->n_devices = uint32_t(value);
      while (m->replicas.size() + 1 > m->n_devices) { free_replica(m->replicas.back()); m->replicas.pop_back(); }
      return 0;
    case 14: m->nm_min_windows = uint32_t(value); break;
    case 15: case 16: case 17: case 18: return 0;        // (read-only: what the last measurement saw)
    case 19: m->small_sweep = value != 0; break;
    case 20: m->small_min_needles = uint32_t(std::min<long long>(value, 0xFFFFFFFFll)); break;
    case 21: m->one.enabled = value != 0; return 0;      // (the single find's own launch; nothing to measure again)
    case 22: return 0;                                   // (read-only)
    case 23: m->one.min_per = uint32_t(value); return 0;
    case 24: return 0;                                   // (read-only)
    case 25: m->tune_inject = int(value); return 0;      // (tests: the next measurement's bad sample)
    case 26: m->one.mid_workgroups = uint32_t(value); return 0;
    case 27: m->one.few_max = uint32_t(value); return 0;
    case 28: m->one.mid_max = uint32_t(value); return 0;
    case 29: m->latency_tasks = uint32_t(value); return 0;
    case 30: m->scope_strategy = uint32_t(value); return 0;   // (scoped finds only: nothing to measure again)
    case 31: m->scope_direct_max = uint64_t(value); return 0;
  }
  if (i != 6) std::fill(std::begin(m->ws_choice), std::end(m->ws_choice), 0);   // the sweep's choice is measured again
  return 0;
}

int blurrily_storage_get_option(trigram_map m, const char* key, long long* value) {
  if (!key || !value) { errno = EINVAL; return -1; }
  if (!m) {
    const int i = FIND_OPTION(kProcessOptions, key);
    if (i < 0) { errno = EINVAL; return -1; }
    *value = i == 0 ? (long long)host_threads() : (long long)build_trace();
    return 0;
  }
  switch (FIND_OPTION(kMapOptions, key)) {
    case 0: *value = m->build_opt.ws_enabled; return 0;
    case 1: *value = m->ws_cmin; return 0;
    case 2: *value = m->build_opt.ws_min_windows; return 0;
    case 3: *value = m->ws_min_needles; return 0;
    case 4: *value = m->build_opt.ws_min_slice; return 0;
    case 5: *value = m->build_opt.dense_min; return 0;
    case 6: *value = m->host_chunk; return 0;
    case 7: *value = m->ws_autotune; return 0;
    case 8: *value = m->ws_static_slice; return 0;
    case 9: {                                            // what was measured so far: class c's choice in bits 2c+1:2c
      long long v = 0;                                   // (1 needle-major, 2 window-major, 3 needle-major with slices left out)
      for (int c = 0; c < 8; ++c) v |= (long long)(m->ws_choice[c]) << (2 * c);
      *value = v;
      return 0;
    }
    case 10: *value = m->nm_cmin; return 0;
    case 11: *value = m->nm_dense; return 0;
    case 12: *value = m->last_sweep; return 0;
    case 13: *value = m->n_devices; return 0;
    case 14: *value = m->nm_min_windows; return 0;
    case 15: *value = m->last_tuned; return 0;             // -1: nothing measured yet
    case 16: case 17: case 18:                             // microseconds of the sweep in that measurement (0: it could not run)
      *value = m->last_tuned < 0 ? 0 : (long long)(1000.0 * m->ws_tuned_ms[m->last_tuned][FIND_OPTION(kMapOptions, key) - 16]);
      return 0;
    case 19: *value = m->small_sweep; return 0;
    case 20: *value = m->small_min_needles; return 0;
    case 21: *value = m->one.enabled; return 0;
    case 22: *value = (long long)m->one.taken; return 0;
    case 23: *value = m->one.min_per; return 0;
    case 24: *value = (long long)m->retunes; return 0;
    case 25: *value = m->tune_inject; return 0;
    case 26: *value = m->one.mid_workgroups; return 0;
    case 27: *value = m->one.few_max; return 0;
    case 28: *value = m->one.mid_max; return 0;
    case 29: *value = m->latency_tasks; return 0;
    case 30: *value = m->scope_strategy; return 0;
    case 31: *value = (long long)m->scope_direct_max; return 0;
    default: errno = EINVAL; return -1;
  }
}

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
