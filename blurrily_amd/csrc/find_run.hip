// find_run.hip -- the batch search's launch logic: the launch sequences that serve a batch of device-resident needles on
// one image and the step that chooses among them (run_find_on; its arithmetic: find_choice.h), and the map as it is now --
// base image, tombstones, delta image -- searched and merged (run_find).
#include "map_internal.h"

using namespace blurrily;
using namespace blurrily::detail;

namespace blurrily {
namespace detail {

// the timed build of the kernels, or (while request counters are collected) the counted one
struct FindBuild {
  int (*find)(const FindArgs&, bool, uint32_t, hipStream_t);
  int (*find_small)(const FindArgs&, uint32_t, hipStream_t);
  int (*wsweep)(const FindArgs&, uint32_t, uint32_t, uint32_t, bool, hipStream_t);
  int (*finalize_rows)(const FindArgs&, uint32_t, hipStream_t);
};
static const FindBuild kTimedBuild{launch_find, launch_find_small, launch_wsweep, launch_finalize_rows};
static const FindBuild kCountedBuild{counted::launch_find, counted::launch_find_small, counted::launch_wsweep,
                                     counted::launch_finalize_rows};

// One run_find_on call, as its launch sequences see it.  They share ONE FindArgs: a sequence sets what its launches
// read and leaves short_only, own_only, ranges and the part / over fields zero for the next; nm_cmin is run_sweep's.
struct FindCall {
  trigram_map m;
  const DeviceIndex& ix;
  hipStream_t stream;
  size_t n;
  uint32_t limit;
  size_t wgs;                                          // resident byte-counter workgroups
  bool maybe_mid;
  bool cb = false;                                     // the counted build serves the call
  FindArgs a{};
  // ws_small (lay_out): scalars [0]=big_count [1]=mid_count [2]=over_count [3..]=queues, then the per-needle arrays
  uint32_t *scalars = nullptr, *q_ntri = nullptr, *q_nb = nullptr, *big_list = nullptr, *mid_list = nullptr,
           *q_start = nullptr, *over_list = nullptr;
  unsigned long long* floor = nullptr;
  uint32_t queue_slot = 3;

  bool is_base() const { return &ix == &m->dev; }      // (the delta image of pending puts is searched the same way)
  const FindBuild& build() const { return cb ? kCountedBuild : kTimedBuild; }
  uint32_t grid() const { return uint32_t(std::min<size_t>(n, wgs)); }

  // scratch: scalars | per-needle arrays | (limits above 256) a floor per needle
  int lay_out(uint32_t* d_nb) {
    const size_t per_n = align_up(n * sizeof(uint32_t), 256);
    const bool multi_pass = limit > 256;             // long needles keep 256 rows per pass, short ones 1024
    if (m->ws_small.reserve(per_n * 6 + (multi_pass ? align_up(n * 8, 256) : 0) + 256, stream) < 0) return -1;
    unsigned char* sp = static_cast<unsigned char*>(m->ws_small.p);
    auto take = [&sp](size_t bytes) { uint32_t* p = reinterpret_cast<uint32_t*>(sp); sp += bytes; return p; };
    scalars = take(256); q_ntri = take(per_n);
    uint32_t* q_nb_ws = take(per_n);
    big_list = take(per_n); mid_list = take(per_n); q_start = take(per_n);
    over_list = take(per_n);                           // (small-haystack sweep: needles of 16..64 trigrams)
    floor = multi_pass ? reinterpret_cast<unsigned long long*>(sp) : nullptr;
    q_nb = d_nb ? d_nb : q_nb_ws;
    return 0;
  }
  // every launch gets its own zeroed queue word (scalars[3..63]); recycled in stream order
  int next_queue() {
    if (queue_slot >= 64) {
      if (hipMemsetAsync(scalars + 3, 0, 244, stream) != hipSuccess) { errno = EIO; return -1; }
      queue_slot = 3;
    }
    a.queue = scalars + queue_slot++;
    return 0;
  }
  int find(bool long_needles, uint32_t grid) {         // the find kernel, on a queue word of its own
    return next_queue() < 0 ? -1 : build().find(a, long_needles, grid, stream);
  }
  // what a sequence's first launch works on: the whole batch (n_work needles, or latency mode's tasks), rows
  // [base, base + keep) of each
  void whole_batch(size_t n_work, uint32_t base, uint32_t keep) {
    a.work_list = nullptr; a.n_work_dev = nullptr; a.n_work = uint32_t(n_work);
    a.pass_base = base; a.keep = keep; a.pool_cap = find_pool_cap(keep);
  }
  // 65..127 distinct trigrams -- the tokeniser's mid list --: needle-major, whole needle per workgroup, all windows
  int mid_tail() {
    if (!maybe_mid) return 0;
    a.work_list = mid_list; a.n_work_dev = scalars + 1; a.n_work = 0;
    return find(false, grid());
  }
};

// Latency mode: a batch too small to fill the GPU cuts every needle's windows into ranges
// swept by different workgroups, then merges the per-range candidates (single pass only).
static int run_ranges(FindCall& c, uint32_t ranges) {
  FindArgs& a = c.a;
  const size_t tasks = c.n * ranges;
  const size_t key_bytes = align_up(tasks * c.limit * 8, 256);
  if (c.m->ws_parts.reserve(key_bytes + align_up(tasks * 4, 256), c.stream) < 0) return -1;
  c.whole_batch(tasks, 0, c.limit);
  a.ranges = ranges;
  a.part_keys = static_cast<unsigned long long*>(c.m->ws_parts.p);
  a.part_count = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(c.m->ws_parts.p) + key_bytes);
  // (every task writes its part_count, also the ones the byte-counter kernel skips)
  a.short_only = 1;
  if (c.find(false, uint32_t(std::min<size_t>(tasks, c.wgs))) < 0) return -1;
  uint32_t merge_cap = 1024;
  while (merge_cap < ranges * c.limit) merge_cap <<= 1;
  a.pool_cap = merge_cap;
  if (launch_merge_parts(a, uint32_t(c.n), c.stream) < 0) return -1;
  a.ranges = 0; a.part_keys = nullptr; a.part_count = nullptr; a.short_only = 0;
  a.pool_cap = find_pool_cap(a.keep);
  return c.mid_tail();
}

// needles with <= 127 distinct trigrams, needle-major: byte counters, up to 1024 rows per pass
static int run_nm(FindCall& c) {
  for (uint32_t base = 0; base < c.limit; base += 1024) {
    c.whole_batch(c.n, base, std::min<uint32_t>(1024, c.limit - base));
    c.a.short_only = 1;                                // needles with <= 64 distinct trigrams
    if (c.find(false, c.grid()) < 0) return -1;
    c.a.short_only = 0;
    if (c.mid_tail() < 0) return -1;
  }
  return 0;
}

// Large batches over many windows: the window-major sweep (find_kernels.hip, wsweep_kernel).
// Phase 1 -- the needle-major kernel over the window pair of every needle's own length class --
// seeds the needles' states; one launch per window follows; keys become rows at the end.
static int run_ws(FindCall& c) {
  FindArgs& a = c.a;
  c.whole_batch(c.n, 0, c.limit);
  a.cmin = c.m->sweep.ws_cmin;
  // Phase 1: the needle-major kernel over the window pair of every needle's own length class seeds the
  // states (a needle's best matches live there, so its threshold is tight before the other windows are
  // visited).  (Seeding through wsweep_kernel's own robust path instead -- own_pass launches -- was
  // measured: configs[2] 321 -> 355 ms per 300 k needles, configs[4] 82 -> 129 ms: without a threshold
  // the 4-wave task floods its pool again and again where the 16-wave kernel bisects once.  Phase 1 over the
  // ONE window of the length class, in byte counters, the sibling window left to the window-major launches:
  // configs[4] 69.0 -> 71.8 ms per 100 k needles, Geonames scale 266 -> 275 ms per 300 k, round 3.)
  a.short_only = 1; a.own_only = 1;
  if (c.find(false, c.grid()) < 0) return -1;
  a.own_only = 0;
  for (uint32_t w = 0; w < c.ix.n_windows; ++w)
    if (c.next_queue() < 0 || c.build().wsweep(a, w, uint32_t(c.n), uint32_t(c.m->n_cus), false, c.stream) < 0) return -1;
  if (c.build().finalize_rows(a, uint32_t(c.n), c.stream) < 0) return -1;
  a.short_only = 0;
  return c.mid_tail();
}

// An image of a few windows, a large batch, a limit of at most 64: the small-haystack sweep (find_small_kernel) --
// four waves and one window's 4-bit counters per needle, four needles' chains per CU instead of two -- for the
// needles of at most 15 trigrams; the ones it lists (16..64) follow through the byte-counter kernel.
static int run_small(FindCall& c) {
  FindArgs& a = c.a;
  c.whole_batch(c.n, 0, c.limit);
  a.over_list = c.over_list; a.over_count = c.scalars + 2;
  if (c.next_queue() < 0 || c.build().find_small(a, uint32_t(c.m->n_cus), c.stream) < 0) return -1;
  a.work_list = c.over_list; a.n_work_dev = c.scalars + 2; a.n_work = 0;
  a.over_list = nullptr; a.over_count = nullptr;
  a.short_only = 1;
  if (c.find(false, c.grid()) < 0) return -1;
  a.short_only = 0;
  return c.mid_tail();
}

// longer needles: 16-bit counters, one workgroup per CU, 256 rows per pass
static int run_long(FindCall& c) {
  FindArgs& a = c.a;
  for (uint32_t base = 0; base < c.limit; base += 256) {
    a.work_list = c.big_list; a.n_work_dev = c.scalars; a.n_work = 0;
    a.pass_base = base; a.keep = std::min<uint32_t>(256, c.limit - base);
    a.pool_cap = 1024;
    if (c.find(true, uint32_t(std::min<size_t>(c.n, size_t(c.m->n_cus)))) < 0) return -1;
  }
  return 0;
}

static int run_sweep(FindCall& c, int which) {
  c.a.nm_cmin = which == kSweepLeave ? c.m->sweep.nm_cmin : 0u;
  const int rc = which == kSweepWindows ? run_ws(c) : which == kSweepSmall ? run_small(c) : run_nm(c);
  c.a.nm_cmin = 0;                                     // (latency mode and the long-needle launches leave nothing out)
  return rc;
}

// what the class's last batch took, if it has finished (never waited for): slow against the measurement?
static void watch_read(trigram_map m, int cls) {
  if (!m->cls[cls].watch_pending || hipEventQuery(m->watch_ev[cls][1]) != hipSuccess) return;
  float ms = 0.f;
  m->cls[cls].watch_pending = false;
  if (hipEventElapsedTime(&ms, m->watch_ev[cls][0], m->watch_ev[cls][1]) == hipSuccess)
    watch_verdict(ms, &m->cls[cls], &m->retunes);      // (choice 0: measured again, by this call)
}

// the brackets of a watched batch: two events around the chosen sweep, read by watch_read at the class's next batch
static int watch_begin(FindCall& c, int cls) {
  if (c.m->watch_ev[cls].make() < 0) return -1;
  BLURRILY_HIP_TRY(hipEventRecord(c.m->watch_ev[cls][0], c.stream));
  return 0;
}
static int watch_end(FindCall& c, int cls) {
  BLURRILY_HIP_TRY(hipEventRecord(c.m->watch_ev[cls][1], c.stream));
  c.m->cls[cls].watch_pending = true;
  c.m->cls[cls].watch_n = c.n;
  return 0;
}

// The measurement of a class, by its first batch (which waits for it): the runs of measure_order, an event between
// each, the better time of a sweep's two runs counting; the batch's rows are the last run's, the plain sweep's
static int measure_sweeps(FindCall& c, int cls, bool ws_possible, bool leave_possible) {
  trigram_map m = c.m;
  if (m->tune_ev.make() < 0) return -1;
  int order[6];
  measure_order(ws_possible, leave_possible, order);
  float ms_of[4] = {0.f, 0.f, 0.f, 0.f};               // by sweep: [1] plain, [2] window-major, [3] slices left out
  BLURRILY_HIP_TRY(hipEventRecord(m->tune_ev[0], c.stream));
  for (int k = 0; k < 6; ++k) {
    if (order[k] && run_sweep(c, order[k]) < 0) return -1;
    BLURRILY_HIP_TRY(hipEventRecord(m->tune_ev[k + 1], c.stream));
  }
  BLURRILY_HIP_TRY(hipEventSynchronize(m->tune_ev[6]));
  for (int k = 0; k < 6; ++k) {
    if (!order[k]) continue;
    float ms = 0.f;
    BLURRILY_HIP_TRY(hipEventElapsedTime(&ms, m->tune_ev[k], m->tune_ev[k + 1]));
    ms_of[order[k]] = ms_of[order[k]] == 0.f ? ms : std::min(ms_of[order[k]], ms);
  }
  float best = 0.f;
  ClassChoice& cc = m->cls[cls];
  cc.choice = pick_sweep(ms_of, &m->tune_inject, ws_possible, leave_possible, &best);
  std::copy(ms_of + 1, ms_of + 4, cc.tuned_ms);
  cc.tuned_us_per_needle = 1000.f * best / float(c.n);
  cc.tuned_n = c.n;
  cc.watch_pending = false;
  m->last_tuned = cls;
  return kSweepPlain;                                  // (the rows in place are the plain run's; all give the same)
}

// WHICH sweep serves the short needles of a batch that latency mode does not take (returned: the one that did).  An
// image of a few windows has the small-haystack sweep (4).  Otherwise three can: the needle-major sweep as it was through round 3
// (1: every posting of every needle trigram counted), the needle-major sweep that leaves the largest dense
// slices out of a step's count and settles candidates through bitmaps (3: "nm_cmin" > 0, limits up to 64), and
// the window-major sweep (2: an image whose mean_hit_slice reaches "ws_min_slice", batches from "ws_min_needles"
// on, limits up to 128).  No statistic of the image predicts the winner across kinds of haystack and of needles
// (at the same mean_hit_slice one family of haystacks wins 1.4x with the window-major sweep
// where another loses 0.7x; leaving slices out wins 14 % on a haystack four times Geonames scale, 3 % at
// Geonames scale, and LOSES 9 % there on needles without a close match), so the choice is MEASURED: the first
// batch of a class -- limit up to / above 32, by batch size 129.. / 16 384.. / 65 536.. / 262 144.. -- on an image runs
// every sweep it can take (they give the same rows; that one call waits for them), the plain sweep twice -- the
// first run of all meets cold caches -- and the fastest serves the class until the image is rebuilt or an option
// changes; a sweep other than the plain one has to win by 1.5 % (window-major: 5 %, it pays a launch per window).
// With "ws_autotune" 0, for smaller batches, and while request counters are collected on an unmeasured class, the
// static rules apply: window-major by the measured table's mean_hit_slice rule, slices left out from 256 windows.
static int serve_short_needles(FindCall& c, size_t code_slots, bool scoped) {
  trigram_map m = c.m;
  const DeviceIndex& ix = c.ix;
  if (m->sweep.small_sweep && ix.n_windows <= kSmallMaxWindows && c.limit <= kSmallMaxKeep && c.n >= m->sweep.small_min_needles)
    return run_sweep(c, kSweepSmall) < 0 ? -1 : kSweepSmall;
  const bool leave_possible = m->sweep.nm_cmin != 0 && c.limit <= 1024 && find_can_leave(c.limit) && ix.n_bitmaps != 0;
  const bool ws_possible = c.limit <= kWsMaxKeep && c.n >= m->sweep.ws_min_needles && ix.n_bitmaps != 0 &&
                           m->sweep.build_opt.ws_can_run(ix.n_windows, ix.mean_hit_slice) && code_slots < 0xFFFFFFFFull;
  // (a chunk of a host-buffer batch belongs to the class of the WHOLE batch: class_hint)
  const size_t n_cls = std::max(c.n, m->class_hint);
  const int cls = batch_class(n_cls, c.limit);
  const bool tunable = m->sweep.ws_autotune && c.is_base() && n_cls >= 129 && (leave_possible || ws_possible);
  // (counters must describe ONE sweep: a counted call neither measures nor watches the class; nor does a scoped call)
  const bool own = tunable && !c.cb && !scoped;
  if (own) watch_read(m, cls);
  holdoff_tick(&m->cls[cls].holdoff, scoped);
  const int held = m->cls[cls].choice;
  int choice;
  if (tunable && held != 0 && (held != kSweepWindows || ws_possible) && (held != kSweepLeave || leave_possible))
    choice = held;
  else if (!own)
    choice = static_sweep(n_cls, c.limit, ws_possible, leave_possible, ix.mean_hit_slice, m->sweep.ws_static_slice,
                          ix.n_windows, m->sweep.nm_min_windows);
  else
    return measure_sweeps(c, cls, ws_possible, leave_possible);
  const bool watch = own && m->cls[cls].tuned_us_per_needle > 0.f;     // (own: the choice is the measured one)
  if (watch && watch_begin(c, cls) < 0) return -1;
  if (run_sweep(c, choice) < 0) return -1;
  if (watch && watch_end(c, cls) < 0) return -1;
  return choice;
}

// tokenise_kernel, or (rn) ref_needles_kernel in its place: the needles' codes, counts and lists
static int launch_front_end(FindCall& c, const uint32_t* d_code_total, const char* d_packed, const uint64_t* d_offsets,
                            const RefNeedles* rn) {
  if (rn)
    return launch_ref_needles(*rn, d_code_total, c.ix.d_start_win, c.q_ntri, c.q_nb, c.q_start, c.big_list, c.scalars,
                              c.mid_list, c.scalars + 1, c.stream);
  TokeniseArgs t{d_packed, d_offsets, uint32_t(c.n), d_code_total, static_cast<uint16_t*>(c.m->ws_codes.p),
                 c.q_ntri, c.q_nb, c.big_list, c.scalars, c.mid_list, c.scalars + 1, c.ix.d_start_win, c.q_start,
                 c.maybe_mid ? 0u : 63u};              // host-buffer batches know their longest needle
  return launch_tokenise(t, c.stream);
}

// what every launch of the call reads: the image, the needles, the rows; and the counted build's own arrays
static int fill_args(FindCall& c, const uint64_t* d_offsets, const RefNeedles* rn, const uint32_t* d_tomb,
                     trigram_match d_results, uint32_t* d_counts) {
  trigram_map m = c.m;
  const DeviceIndex& ix = c.ix;
  FindArgs& a = c.a;
  image_args(ix, &a);
  a.offsets = rn ? rn->qoff : d_offsets; a.qcodes = rn ? rn->codes : static_cast<const uint16_t*>(m->ws_codes.p);
  a.q_ntri = c.q_ntri; a.q_nb = c.q_nb; a.q_start = c.q_start;
  a.results = d_results; a.counts = d_counts; a.limit = c.limit;
  a.floor = c.floor;
  a.tomb = d_tomb;
  a.nm_dense = std::max((m->sweep.nm_dense + 7u) & ~7u, ix.dense_min8);
  a.nm_cmin = 0;                                     // (set per sweep: run_sweep)
  a.stats = m->collect_stats ? m->d_stats.h : nullptr;
  c.cb = a.stats != nullptr;
#ifdef BLURRILY_TRACE
  const bool clocks = true;                          // (trace build: time stamps of a few needles' steps, timed kernels)
#else
  const bool clocks = c.cb;                          // wave 0's phase clocks per workgroup (counted build only)
#endif
  if (clocks) {
    if (m->d_phase.alloc(kPhaseWords) < 0) return -1;
    BLURRILY_HIP_TRY(hipMemsetAsync(m->d_phase, 0, kPhaseBytes, c.stream));
    a.phase_clocks = m->d_phase;
  }
  if (c.cb) a.path_flags = static_cast<uint32_t*>(m->ws_flags.p);   // (sized and zeroed by run_find)
  return 0;
}

// Enqueue tokenise + find for n device-resident needles -- or, with `rn`, find for n references whose trigrams
// launch_refs_extract has left on the device (d_packed / d_offsets unused): ref_needles_kernel in tokenise_kernel's place,
// every launch after it the same.  `scoped`: d_tomb is a scope's mask (run_find); the call neither measures nor watches
// a class's choice of sweep -- it takes the measured one, or the static rule -- so that unscoped batches never depend
// on scoped ones.
static int run_find_on(trigram_map m, const DeviceIndex& ix, const uint32_t* d_code_total, const uint32_t* d_tomb,
                const char* d_packed, size_t packed_bytes, const uint64_t* d_offsets, size_t n, uint16_t limit,
                trigram_match d_results, uint32_t* d_counts, uint32_t* d_nb, bool maybe_long, bool maybe_mid,
                hipStream_t stream, const RefNeedles* rn = nullptr, bool scoped = false) {
  if (n == 0) return 0;
  if (n > kMaxBatchNeedles) { errno = EINVAL; return -1; }
  FindCall c{m, ix, stream, n, limit, size_t(m->n_cus) * find_wgs_per_cu(), maybe_mid};
  if (c.is_base()) m->last_sweep = 0;
  NameScope name_scope(c.is_base() ? &m->last_kernels : nullptr);    // the launches below note their kernels' names in the map
  if (c.is_base()) m->last_kernels.clear();

  // scratch: codes | per-needle arrays | scalars
  const size_t code_slots = rn ? size_t(rn->code_slots) : packed_bytes + n;
  if (!rn && m->ws_codes.reserve(align_up(code_slots * sizeof(uint16_t), 256), stream) < 0) return -1;
  if (c.lay_out(d_nb) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemsetAsync(c.scalars, 0, 256, stream));

  if (m->timing) BLURRILY_HIP_TRY(hipEventRecord(m->ev[0], stream));
  if (launch_front_end(c, d_code_total, d_packed, d_offsets, rn) < 0) return -1;
  if (m->timing) {
    BLURRILY_HIP_TRY(hipEventRecord(m->ev[1], stream));
    BLURRILY_HIP_TRY(hipEventRecord(m->ev[2], stream));
  }
  if (fill_args(c, d_offsets, rn, d_tomb, d_results, d_counts) < 0) return -1;

  if (limit == 0) {
    BLURRILY_HIP_TRY(hipMemsetAsync(d_counts, 0, n * sizeof(uint32_t), stream));
  } else {
    const uint32_t ranges = latency_ranges(n, limit, ix.n_windows, c.wgs, m->latency_tasks);
    if (ranges > 1) {
      if (run_ranges(c, ranges) < 0) return -1;
    } else {
      const int served = serve_short_needles(c, code_slots, scoped);
      if (served < 0) return -1;
      if (c.is_base()) m->last_sweep = served;
    }
    if (maybe_long && run_long(c) < 0) return -1;
  }
  if (m->timing) {
    BLURRILY_HIP_TRY(hipEventRecord(m->ev[3], stream));
    BLURRILY_HIP_TRY(hipEventSynchronize(m->ev[3]));
    float ms = 0.f;
    BLURRILY_HIP_TRY(hipEventElapsedTime(&ms, m->ev[0], m->ev[1])); m->last_tok_ms = ms;
    BLURRILY_HIP_TRY(hipEventElapsedTime(&ms, m->ev[2], m->ev[3])); m->last_find_ms = ms;
  }
  return 0;
}

// Enqueue tokenise + find for n device-resident needles on the map's current contents.
// (rn: the needles are references, extracted once: both images are searched with the same codes)
// (sm: a scoped find's masks, in the tombstone bitmap's place: they exclude the deleted ranks too)
int run_find(trigram_map m, const char* d_packed, size_t packed_bytes, const uint64_t* d_offsets, size_t n,
             uint16_t limit, trigram_match d_results, uint32_t* d_counts, uint32_t* d_nb, bool maybe_long,
             bool maybe_mid, hipStream_t stream, const RefNeedles* rn, const ScopeMasks* sm) {
  if (m->timing && m->ev.make() < 0) return -1;        // (every timed run_find_on goes through here: its events, at first use)
  if (m->collect_stats) {
    if (m->d_stats.alloc(kStatAllSlots) < 0) return -1;
    BLURRILY_HIP_TRY(hipMemsetAsync(m->d_stats, 0, kStatAllSlots * 8, stream));
    if (m->ws_flags.reserve(std::max<size_t>(n, 1) * sizeof(uint32_t), stream) < 0) return -1;
    BLURRILY_HIP_TRY(hipMemsetAsync(m->ws_flags.p, 0, std::max<size_t>(n, 1) * sizeof(uint32_t), stream));
    m->n_flags = n;
  }
  if (apply_tombstones(m, stream) < 0) return -1;
  if (log_empty(m))
    return run_find_on(m, m->dev, m->dev.d_code_total, sm ? sm->base : nullptr, d_packed, packed_bytes, d_offsets, n,
                       limit, d_results, d_counts, d_nb, maybe_long, maybe_mid, stream, rn, sm != nullptr);
  // base image (minus tombstones) and delta image hold disjoint references: find on both, merge
  const size_t row_bytes = std::max<size_t>(n * size_t(limit) * sizeof(trigram_match_t), 16);
  if (m->ws_base_rows.reserve(row_bytes, stream) < 0 || m->ws_base_counts.reserve(n * 4, stream) < 0 ||
      m->ws_delta_rows.reserve(row_bytes, stream) < 0 || m->ws_delta_counts.reserve(n * 4, stream) < 0)
    return -1;
  trigram_match base_rows = static_cast<trigram_match>(m->ws_base_rows.p);
  uint32_t* base_counts = static_cast<uint32_t*>(m->ws_base_counts.p);
  trigram_match delta_rows = static_cast<trigram_match>(m->ws_delta_rows.p);
  uint32_t* delta_counts = static_cast<uint32_t*>(m->ws_delta_counts.p);
  const uint32_t* base_tomb = sm ? sm->base : log_of(m)->n_tomb ? m->dev.d_tomb : nullptr;
  if (run_find_on(m, m->dev, m->d_code_total_now, base_tomb, d_packed, packed_bytes, d_offsets, n, limit, base_rows,
                  base_counts, d_nb, maybe_long, maybe_mid, stream, rn, sm != nullptr) < 0)
    return -1;
  if (log_of(m)->pending.empty()) {
    BLURRILY_HIP_TRY(hipMemsetAsync(delta_counts, 0, n * 4, stream));
  } else if (run_find_on(m, m->delta, m->delta.d_code_total, sm ? sm->delta : nullptr, d_packed, packed_bytes, d_offsets,
                         n, limit, delta_rows, delta_counts, nullptr, maybe_long, maybe_mid, stream, rn,
                         sm != nullptr) < 0) {
    return -1;
  }
  return launch_merge_rows(base_rows, base_counts, delta_rows, delta_counts, uint32_t(n), limit, d_results,
                           d_counts, stream);
}

// The string front end of the threshold and similarity finds: host strings up, tokenised as a batch's are.  (run_find_on's
// own set-up above does not call it: its needles are on the device already, its arrays live in the map's ws_codes /
// ws_small in another order, and its launch passes the batch's longest-needle hint where this one passes 0.)
int stage_string_needles(trigram_map m, const char* packed, const uint64_t* offsets, size_t n, DeviceBuffer& buf,
                         hipStream_t stream, NeedleView* out) {
  const size_t packed_bytes = size_t(offsets[n]);
  const BatchBlocks B(n, packed_bytes, 0, false);             // the needles as a host batch's in block, then the tokeniser's arrays
  const size_t per_n = align_up(n * 4, 256), o_codes = align_up(B.in_bytes, 256);
  const size_t o_ntri = o_codes + align_up((packed_bytes + n) * 2, 256);
  const size_t bytes = o_ntri + 6 * per_n + 256;
  if (buf.reserve(bytes, stream) < 0) return -1;
  unsigned char* b = static_cast<unsigned char*>(buf.p);
  const uint64_t* d_offsets = B.in(b).offsets;
  char* d_packed = B.in(b).packed;
  uint16_t* d_codes = reinterpret_cast<uint16_t*>(b + o_codes);
  uint32_t* q = reinterpret_cast<uint32_t*>(b + o_ntri);      // ntri | nb | big | mid | start | (spare) | scalars
  uint32_t* scalars = reinterpret_cast<uint32_t*>(b + o_ntri + 6 * per_n);
  if (B.copy_in(b, packed, offsets, stream) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemsetAsync(scalars, 0, 256, stream));
  const size_t w = per_n / 4;
  TokeniseArgs t{d_packed, d_offsets, uint32_t(n), m->dev.d_code_total, d_codes, q, q + w, q + 2 * w, scalars,
                 q + 3 * w, scalars + 1, m->dev.d_start_win, q + 4 * w, 0u};
  note_launch("tokenise_kernel");
  if (launch_tokenise(t, stream) < 0) return -1;
  *out = NeedleView{d_codes, d_offsets, q};
  return 0;
}

}  // namespace detail
}  // namespace blurrily
