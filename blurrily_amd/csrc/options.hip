// options.hip -- blurrily_storage_set_option / blurrily_storage_get_option (include/blurrily_storage.h): one table per
// scope -- a map's tunables, the process's -- and one row per option, holding everything about it: its key and range,
// how it is read, how it is written, and whether writing it has the sweep's measured choices forgotten.  The entries
// look a key up, check the range and call; nothing depends on where a row stands.  A map's options are plain fields
// read by its next find (calls on one map are serial, as in the reference: no lock); the process-wide ones are atomics.
#include "map_internal.h"

using namespace blurrily;
using namespace blurrily::detail;

namespace {

struct Option {
  const char* key;
  long long lo, hi;
  long long (*get)(const trigram_map_t*);
  void (*set)(trigram_map_t*, long long);      // none: read-only (its range is [0, 0]: 0 is taken and changes nothing)
  bool forgets;                                // a set has every class of batch measured again (forget_choices)
};

// a row's read and write for a plain field of the map; the same with a value of up to 2^32 stored as 2^32 - 1 at most
#define READS(field) [](const trigram_map_t* m) -> long long { return (long long)(m->field); }
#define PLAIN(field) READS(field), [](trigram_map_t* m, long long v) { m->field = decltype(m->field)(v); }
#define UP_TO_U32(field) READS(field), [](trigram_map_t* m, long long v) { m->field = uint32_t(std::min(v, 0xFFFFFFFFll)); }

// microseconds of a sweep in the last measurement (0: it could not run, or nothing was measured yet)
long long tuned_us(const trigram_map_t* m, int sweep) {
  return m->last_tuned < 0 ? 0 : (long long)(1000.0 * m->cls[m->last_tuned].tuned_ms[sweep]);
}

const Option kMapOptions[] = {
    {"wsweep", 0, 1, PLAIN(sweep.build_opt.ws_enabled), true},
    {"ws_cmin", 1, 64, PLAIN(sweep.ws_cmin), true},
    {"ws_min_windows", 0, 1 << 20, PLAIN(sweep.build_opt.ws_min_windows), true},
    {"ws_min_needles", 0, 1ll << 32, UP_TO_U32(sweep.ws_min_needles), true},
    {"ws_min_slice", 0, 1ll << 31, PLAIN(sweep.build_opt.ws_min_slice), true},
    {"dense_min", 64, 65536, READS(sweep.build_opt.dense_min),
     [](trigram_map_t* m, long long v) {       // which slices have bitmaps: the image is rebuilt by the next find
       if (m->sweep.build_opt.dense_min != uint32_t(v) && m->dev.device >= 0) m->log_overflow = true;
       m->sweep.build_opt.dense_min = uint32_t(v);
     }, true},
    {"host_chunk", 0, 1ll << 30, PLAIN(host_chunk), false},
    {"ws_autotune", 0, 1, PLAIN(sweep.ws_autotune), true},
    {"ws_static_slice", 0, 1ll << 31, PLAIN(sweep.ws_static_slice), true},
    {"ws_choice", 0, 0,                        // what was measured so far: class c's choice in bits 2c+1:2c (1 needle-major,
     [](const trigram_map_t* m) -> long long { //  2 window-major, 3 needle-major with slices left out); set to 0: forget it
       long long v = 0;
       for (int c = 0; c < 8; ++c) v |= (long long)(m->cls[c].choice) << (2 * c);
       return v;
     }, nullptr, true},
    {"nm_cmin", 0, 64, PLAIN(sweep.nm_cmin), true},
    {"nm_dense", 64, 65536, PLAIN(sweep.nm_dense), true},
    {"last_sweep", 0, 0, PLAIN(last_sweep), false},         // (set to 0: reset)
    {"devices", 1, 64, READS(n_devices),
     [](trigram_map_t* m, long long v) {       // (replicas are made by the next large batch; dropped at once)
       m->n_devices = uint32_t(v);
       while (m->replicas.size() + 1 > m->n_devices) { free_replica(m->replicas.back()); m->replicas.pop_back(); }
     }, false},
    {"nm_min_windows", 0, 1 << 20, PLAIN(sweep.nm_min_windows), true},
    {"tuned_class", 0, 0, READS(last_tuned), nullptr, false},   // -1: nothing measured yet
    {"tuned_nm_us", 0, 0, [](const trigram_map_t* m) { return tuned_us(m, 0); }, nullptr, false},
    {"tuned_ws_us", 0, 0, [](const trigram_map_t* m) { return tuned_us(m, 1); }, nullptr, false},
    {"tuned_leave_us", 0, 0, [](const trigram_map_t* m) { return tuned_us(m, 2); }, nullptr, false},
    {"small_sweep", 0, 1, PLAIN(sweep.small_sweep), true},
    {"small_min_needles", 0, 1ll << 32, UP_TO_U32(sweep.small_min_needles), true},
    {"one_launch", 0, 1, PLAIN(one.enabled), false},        // (the single find's own launch; nothing to measure again)
    {"one_taken", 0, 0, READS(one.taken), nullptr, false},
    {"one_windows_per_wg", 0, 1 << 20, PLAIN(one.min_per), false},
    {"retunes", 0, 0, READS(retunes), nullptr, false},
    {"tune_inject", 0, 3, PLAIN(tune_inject), false},       // (tests: the next measurement's bad sample)
    {"mid_workgroups", 64, 1 << 16, PLAIN(one.mid_workgroups), false},
    {"few_max", 1, kMidMaxNeedles, PLAIN(one.few_max), false},
    {"mid_max", 0, kMidMaxNeedles, PLAIN(one.mid_max), false},
    {"latency_tasks", 0, 16, PLAIN(latency_tasks), false},
    {"scope_strategy", 0, 2, PLAIN(scope_strategy), false}, // (scoped finds only: nothing to measure again)
    {"scope_direct_max", 0, 1ll << 40, PLAIN(scope_direct_max), false},
    {"cluster_edges_max", 1, 1ll << 31, PLAIN(cluster_edges_max), false}};   // (records one cluster_edges call may emit)

#undef UP_TO_U32
#undef PLAIN
#undef READS

const Option kProcessOptions[] = {
    {"host_threads", 0, 256, [](const trigram_map_t*) -> long long { return host_threads(); },
     [](trigram_map_t*, long long v) { set_host_threads(unsigned(v)); }, false},
    {"build_trace", 0, 1, [](const trigram_map_t*) -> long long { return build_trace(); },
     [](trigram_map_t*, long long v) { set_build_trace(v != 0); }, false}};

// the row of `key` among a map's options, or (no map) the process's; none: EINVAL
const Option* find_option(const trigram_map_t* m, const char* key) {
  const Option* tab = m ? kMapOptions : kProcessOptions;
  const size_t n = m ? std::size(kMapOptions) : std::size(kProcessOptions);
  for (size_t i = 0; key && i < n; ++i)
    if (std::strcmp(tab[i].key, key) == 0) return &tab[i];
  errno = EINVAL;
  return nullptr;
}

}  // namespace

extern "C" {

int blurrily_storage_set_option(trigram_map m, const char* key, long long value) {
  const Option* o = find_option(m, key);
  if (!o) return -1;
  if (value < o->lo || value > o->hi) { errno = EINVAL; return -1; }
  if (o->set) o->set(m, value);
  if (o->forgets) forget_choices(m);           // the sweep's choice is measured again
  return 0;
}

int blurrily_storage_get_option(trigram_map m, const char* key, long long* value) {
  const Option* o = value ? find_option(m, key) : nullptr;
  if (!o) { errno = EINVAL; return -1; }
  *value = o->get(m);
  return 0;
}

}  // extern "C"
