// find_run.hip -- the batch search's launch logic: which sweeps serve a batch of device-resident needles on one image
// (run_find_on), and the map as it is now -- base image, tombstones, delta image -- searched and merged (run_find).
#include "map_internal.h"

using namespace blurrily;
using namespace blurrily::detail;

namespace blurrily {
namespace detail {

// the timed build of the kernels, or (while request counters are collected) the counted one
// Latency mode: the ranges a needle's windows are cut into when n needles are too few to fill `wgs` resident workgroups
// (1: whole needles).  Tasks aimed at: ONE per workgroup up to sixty needles -- every task starts at once, none
// queues behind another's learning sweep --, two beyond (round 6, tools/experiments/r6_run_mid5.sh, host clock at Geonames
// scale, one / two / three / four tasks per workgroup: 32 needles 131 / 179 / 197 / 228 us, 56: 188 / 226 / 244 / 268,
// 64: 216 / 209 / 239 / 274, 128: 319 / 261 / 285 / 302; through round 5 two, and four from a hundred needles on); from
// seven needles per SIXTEEN workgroups on (225 needles on this chip) whole needles win: up to a needle per workgroup their
// time is the slowest needle's, 368 us at Geonames scale whatever the batch, and ranges take 243 us at 129 needles, 298 at
// 160, 310 at 192, 356 at 224, 385 at 256 (round 6: tools/experiments/r6_lat256.py; through round 5 the crossover sat at one
// needle per four workgroups, through round 4 at one per workgroup: the ranged sweep paid a whole learning sweep per task
// and ended with its dearest tasks).
uint32_t latency_ranges(size_t n, uint32_t limit, uint32_t n_windows, size_t wgs, uint32_t tasks_per_wg) {
  if (limit == 0 || limit > 1024 || n * 16 > wgs * 7 || n_windows <= 2) return 1;
  const size_t target_tasks = (tasks_per_wg ? tasks_per_wg : n <= 60 ? 1 : 2) * wgs;      // (option "latency_tasks": 0 = this rule)
  uint32_t ranges = uint32_t(std::min<size_t>((n_windows + 1) / 2, target_tasks / n));   // ranges are whole window pairs
  return std::max<uint32_t>(1u, std::min<uint32_t>(ranges, std::max<uint32_t>(1u, 4096u / limit)));      // (the merge's pool)
}

static int do_launch_find(bool counted_build, const FindArgs& a, bool long_needles, uint32_t grid, hipStream_t stream) {
  return counted_build ? counted::launch_find(a, long_needles, grid, stream) : launch_find(a, long_needles, grid, stream);
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
  const bool is_base = &ix == &m->dev;                 // (the delta image of pending puts is searched the same way)
  if (is_base) m->last_sweep = 0;
  NameScope name_scope(is_base ? &m->last_kernels : nullptr);    // the launches below note their kernels' names in the map
  if (is_base) m->last_kernels.clear();

  // scratch: codes | per-needle arrays | scalars
  const size_t code_slots = rn ? size_t(rn->code_slots) : packed_bytes + n;
  if (!rn && m->ws_codes.reserve(align_up(code_slots * sizeof(uint16_t), 256), stream) < 0) return -1;
  const size_t per_n = align_up(n * sizeof(uint32_t), 256);
  const bool multi_pass = limit > 256;             // long needles keep 256 rows per pass, short ones 1024
  const size_t small_bytes = per_n * 6 + (multi_pass ? align_up(n * 8, 256) : 0) + 256;
  if (m->ws_small.reserve(small_bytes, stream) < 0) return -1;
  unsigned char* sp = static_cast<unsigned char*>(m->ws_small.p);
  uint32_t* scalars  = reinterpret_cast<uint32_t*>(sp);            sp += 256;   // [0]=big_count [1]=mid_count [2]=over_count [3..]=queues
  uint32_t* q_ntri   = reinterpret_cast<uint32_t*>(sp);            sp += per_n;
  uint32_t* q_nb_ws  = reinterpret_cast<uint32_t*>(sp);            sp += per_n;
  uint32_t* big_list = reinterpret_cast<uint32_t*>(sp);            sp += per_n;
  uint32_t* mid_list = reinterpret_cast<uint32_t*>(sp);            sp += per_n;
  uint32_t* q_start  = reinterpret_cast<uint32_t*>(sp);            sp += per_n;
  uint32_t* over_list = reinterpret_cast<uint32_t*>(sp);           sp += per_n;   // (small-haystack sweep: needles of 16..64 trigrams)
  unsigned long long* floor = nullptr;
  if (multi_pass) floor = reinterpret_cast<unsigned long long*>(sp);
  uint32_t* q_nb = d_nb ? d_nb : q_nb_ws;
  BLURRILY_HIP_TRY(hipMemsetAsync(scalars, 0, 256, stream));

  if (m->timing) BLURRILY_HIP_TRY(hipEventRecord(m->ev[0], stream));
  if (rn) {
    if (launch_ref_needles(*rn, d_code_total, ix.d_start_win, q_ntri, q_nb, q_start, big_list, scalars, mid_list,
                           scalars + 1, stream) < 0)
      return -1;
  } else {
    TokeniseArgs t{d_packed, d_offsets, uint32_t(n), d_code_total, static_cast<uint16_t*>(m->ws_codes.p),
                   q_ntri, q_nb, big_list, scalars, mid_list, scalars + 1, ix.d_start_win, q_start,
                   maybe_mid ? 0u : 63u};                // host-buffer batches know their longest needle
    if (launch_tokenise(t, stream) < 0) return -1;
  }
  if (m->timing) {
    BLURRILY_HIP_TRY(hipEventRecord(m->ev[1], stream));
    BLURRILY_HIP_TRY(hipEventRecord(m->ev[2], stream));
  }

  FindArgs a{};
  a.slice_se = ix.d_slice_se; a.ent = ix.d_ent; a.ref_of_rank = ix.d_ref_of_rank;
  a.weight_of_rank = ix.d_weight_of_rank; a.n_refs = ix.n_refs; a.n_windows = ix.n_windows;
  a.offsets = rn ? rn->qoff : d_offsets; a.qcodes = rn ? rn->codes : static_cast<const uint16_t*>(m->ws_codes.p);
  a.q_ntri = q_ntri; a.q_nb = q_nb; a.q_start = q_start; a.win_max_tri = ix.d_win_max_tri; a.nib_windows = ix.nib_windows; a.results = d_results; a.counts = d_counts; a.limit = limit;
  a.floor = floor;
  a.tomb = d_tomb;
  a.dense_min8 = ix.dense_min8;
  a.nm_dense = std::max((m->nm_dense + 7u) & ~7u, ix.dense_min8);
  a.nm_cmin = 0;                                     // (set per launch sequence: see "WHICH sweep" below)
  a.stats = m->collect_stats ? m->d_stats : nullptr;
  const bool cb = a.stats != nullptr;
  if (cb) {                                          // wave 0's phase clocks per workgroup (counted build only)
    if (!m->d_phase) BLURRILY_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m->d_phase), kPhaseBytes));
    BLURRILY_HIP_TRY(hipMemsetAsync(m->d_phase, 0, kPhaseBytes, stream));
    a.phase_clocks = m->d_phase;
    a.path_flags = static_cast<uint32_t*>(m->ws_flags.p);   // (sized and zeroed by run_find)
  }
#ifdef BLURRILY_TRACE
  if (!cb) {                                         // (trace build: time stamps of a few needles' steps, timed kernels)
    if (!m->d_phase) BLURRILY_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m->d_phase), kPhaseBytes));
    BLURRILY_HIP_TRY(hipMemsetAsync(m->d_phase, 0, kPhaseBytes, stream));
    a.phase_clocks = m->d_phase;
  }
#endif
  // every launch gets its own zeroed queue word (scalars[3..63]); recycled in stream order
  uint32_t queue_slot = 3;
  auto next_queue = [&]() -> uint32_t* {
    if (queue_slot >= 64) {
      if (hipMemsetAsync(scalars + 3, 0, 244, stream) != hipSuccess) return nullptr;
      queue_slot = 3;
    }
    return scalars + queue_slot++;
  };

  if (limit == 0) {
    BLURRILY_HIP_TRY(hipMemsetAsync(d_counts, 0, n * sizeof(uint32_t), stream));
  } else {
    // Latency mode: a batch too small to fill the GPU cuts every needle's windows into ranges
    // swept by different workgroups, then merges the per-range candidates (single pass only).
    const size_t wgs = size_t(m->n_cus) * find_wgs_per_cu();
    const uint32_t ranges = latency_ranges(n, limit, ix.n_windows, wgs, m->latency_tasks);
    if (ranges > 1) {
      const size_t tasks = n * ranges;
      const size_t key_bytes = align_up(tasks * limit * 8, 256);
      if (m->ws_parts.reserve(key_bytes + align_up(tasks * 4, 256), stream) < 0) return -1;
      a.work_list = nullptr; a.n_work_dev = nullptr; a.n_work = uint32_t(tasks);
      a.ranges = ranges;
      a.part_keys = static_cast<unsigned long long*>(m->ws_parts.p);
      a.part_count = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(m->ws_parts.p) + key_bytes);
      a.pass_base = 0; a.keep = limit; a.pool_cap = find_pool_cap(limit);
      if (!(a.queue = next_queue())) { errno = EIO; return -1; }
      // (every task writes its part_count, also the ones the byte-counter kernel skips)
      a.short_only = 1;
      if (do_launch_find(cb, a, false, uint32_t(std::min<size_t>(tasks, wgs)), stream) < 0) return -1;
      uint32_t merge_cap = 1024;
      while (merge_cap < ranges * limit) merge_cap <<= 1;
      a.pool_cap = merge_cap;
      if (launch_merge_parts(a, uint32_t(n), stream) < 0) return -1;
      a.ranges = 0; a.part_keys = nullptr; a.part_count = nullptr; a.short_only = 0;
      if (maybe_mid) {                               // 65..127 distinct trigrams: whole needle per workgroup
        a.work_list = mid_list; a.n_work_dev = scalars + 1; a.n_work = 0;
        a.pool_cap = find_pool_cap(a.keep);
        if (!(a.queue = next_queue())) { errno = EIO; return -1; }
        if (do_launch_find(cb, a, false, uint32_t(std::min<size_t>(n, wgs)), stream) < 0) return -1;
      }
    }
    // Large batches over many windows: the window-major sweep (find_kernels.hip, wsweep_kernel).
    // Phase 1 -- the needle-major kernel over the window pair of every needle's own length class --
    // seeds the needles' states; one launch per window follows; keys become rows at the end.
    auto run_ws = [&]() -> int {
      a.work_list = nullptr; a.n_work_dev = nullptr; a.n_work = uint32_t(n);
      a.pass_base = 0; a.keep = limit; a.pool_cap = find_pool_cap(limit);
      a.cmin = m->ws_cmin;
      // Phase 1: the needle-major kernel over the window pair of every needle's own length class seeds the
      // states (a needle's best matches live there, so its threshold is tight before the other windows are
      // visited).  (Seeding through wsweep_kernel's own robust path instead -- own_pass launches -- was
      // measured: configs[2] 321 -> 355 ms per 300 k needles, configs[4] 82 -> 129 ms: without a threshold
      // the 4-wave task floods its pool again and again where the 16-wave kernel bisects once.  Phase 1 over the
      // ONE window of the length class, in byte counters, the sibling window left to the window-major launches:
      // configs[4] 69.0 -> 71.8 ms per 100 k needles, Geonames scale 266 -> 275 ms per 300 k, round 3.)
      if (!(a.queue = next_queue())) { errno = EIO; return -1; }
      a.short_only = 1; a.own_only = 1;
      if (do_launch_find(cb, a, false, uint32_t(std::min<size_t>(n, wgs)), stream) < 0) return -1;
      a.own_only = 0;
      for (uint32_t w = 0; w < ix.n_windows; ++w) {
        if (!(a.queue = next_queue())) { errno = EIO; return -1; }
        if ((cb ? counted::launch_wsweep(a, w, uint32_t(n), uint32_t(m->n_cus), false, stream)
                : launch_wsweep(a, w, uint32_t(n), uint32_t(m->n_cus), false, stream)) < 0) return -1;
      }
      if ((cb ? counted::launch_finalize_rows(a, uint32_t(n), stream) : launch_finalize_rows(a, uint32_t(n), stream)) < 0) return -1;
      a.short_only = 0;
      if (maybe_mid) {                               // 65..127 distinct trigrams: needle-major, all windows
        a.work_list = mid_list; a.n_work_dev = scalars + 1; a.n_work = 0;
        if (!(a.queue = next_queue())) { errno = EIO; return -1; }
        if (do_launch_find(cb, a, false, uint32_t(std::min<size_t>(n, wgs)), stream) < 0) return -1;
      }
      return 0;
    };
    // needles with <= 127 distinct trigrams, needle-major: byte counters, up to 1024 rows per pass
    auto run_nm = [&]() -> int {
      for (uint32_t base = 0; base < limit; base += 1024) {
        a.work_list = nullptr; a.n_work_dev = nullptr; a.n_work = uint32_t(n);
        a.pass_base = base; a.keep = std::min<uint32_t>(1024, limit - base);
        a.pool_cap = find_pool_cap(a.keep);
        if (!(a.queue = next_queue())) { errno = EIO; return -1; }
        const uint32_t grid = uint32_t(std::min<size_t>(n, wgs));
        a.short_only = 1;                              // needles with <= 64 distinct trigrams
        if (do_launch_find(cb, a, false, grid, stream) < 0) return -1;
        a.short_only = 0;
        if (maybe_mid) {                               // 65..127: the tokeniser's mid list
          a.work_list = mid_list; a.n_work_dev = scalars + 1; a.n_work = 0;
          if (!(a.queue = next_queue())) { errno = EIO; return -1; }
          if (do_launch_find(cb, a, false, uint32_t(std::min<size_t>(n, wgs)), stream) < 0) return -1;
        }
      }
      return 0;
    };
    // An image of a few windows, a large batch, a limit of at most 64: the small-haystack sweep (find_small_kernel) --
    // four waves and one window's 4-bit counters per needle, four needles' chains per CU instead of two -- for the
    // needles of at most 15 trigrams; the ones it lists (16..64) follow through the byte-counter kernel.
    auto run_small = [&]() -> int {
      a.work_list = nullptr; a.n_work_dev = nullptr; a.n_work = uint32_t(n);
      a.pass_base = 0; a.keep = limit; a.pool_cap = find_pool_cap(limit);
      a.over_list = over_list; a.over_count = scalars + 2;
      if (!(a.queue = next_queue())) { errno = EIO; return -1; }
      if ((cb ? counted::launch_find_small(a, uint32_t(m->n_cus), stream) : launch_find_small(a, uint32_t(m->n_cus), stream)) < 0) return -1;
      a.work_list = over_list; a.n_work_dev = scalars + 2; a.n_work = 0;
      a.over_list = nullptr; a.over_count = nullptr;
      if (!(a.queue = next_queue())) { errno = EIO; return -1; }
      a.short_only = 1;
      if (do_launch_find(cb, a, false, uint32_t(std::min<size_t>(n, wgs)), stream) < 0) return -1;
      a.short_only = 0;
      if (maybe_mid) {                                 // 65..127: the tokeniser's mid list
        a.work_list = mid_list; a.n_work_dev = scalars + 1; a.n_work = 0;
        if (!(a.queue = next_queue())) { errno = EIO; return -1; }
        if (do_launch_find(cb, a, false, uint32_t(std::min<size_t>(n, wgs)), stream) < 0) return -1;
      }
      return 0;
    };
    // WHICH sweep serves the batch's short needles.  Three can: the needle-major sweep as it was through round 3
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
    const uint32_t cmin_opt = m->nm_cmin;
    const bool leave_possible = ranges <= 1 && cmin_opt != 0 && limit <= 1024 && find_can_leave(limit) && ix.n_bitmaps != 0;
    const bool ws_possible = ranges <= 1 && limit <= kWsMaxKeep && n >= m->ws_min_needles && ix.n_bitmaps != 0 &&
                             m->build_opt.ws_can_run(ix.n_windows, ix.mean_hit_slice) && code_slots < 0xFFFFFFFFull;
    auto run_sweep = [&](int which) -> int {           // 1 plain, 2 window-major, 3 slices left out, 4 small haystack
      a.nm_cmin = which == 3 ? cmin_opt : 0u;
      return which == 2 ? run_ws() : which == 4 ? run_small() : run_nm();
    };
    int choice = 1;
    a.nm_cmin = 0;                                     // (latency mode and the long-needle launches leave nothing out)
    const bool small_possible = ranges <= 1 && m->small_sweep && ix.n_windows <= kSmallMaxWindows && limit <= kSmallMaxKeep &&
                                n >= m->small_min_needles;
    if (small_possible) {
      if (run_sweep(4) < 0) return -1;
      if (is_base) m->last_sweep = 4;
    } else if (ranges <= 1) {
      // (a chunk of a host-buffer batch belongs to the class of the WHOLE batch: class_hint)
      const size_t n_cls = std::max(n, m->class_hint);
      const double slice_factor = (n_cls < 65536 ? (limit > 32 ? 4.0 : 1.7) : (limit > 32 ? 1.7 : 1.0));
      const int static_choice = ws_possible && ix.mean_hit_slice >= slice_factor * double(m->ws_static_slice) ? 2
                                : leave_possible && ix.n_windows >= m->nm_min_windows ? 3 : 1;
      // (classes 6 and 7: batches of 129 .. 16 383 needles -- a server's coalesced FINDs; at Geonames scale leaving slices
      // out wins there as it does on large batches: 0.9 -> 0.8 ms for 1 024 needles, 2.6 -> 2.1 for 4 096, 6.4 -> 5.4 for
      // 12 000, which the static rule -- from 256 windows on -- gave away through round 5's first half)
      const int cls = n_cls < 16384 ? (limit > 32 ? 7 : 6) : (limit > 32 ? 3 : 0) + (n_cls < 65536 ? 0 : n_cls < 262144 ? 1 : 2);
      const bool tunable = m->ws_autotune && is_base && n_cls >= 129 && (leave_possible || ws_possible);
      // what the class's last batch took, if it has finished (never waited for): slow against the measurement?
      if (tunable && !cb && !scoped && m->watch_pending[cls] && hipEventQuery(m->watch_ev[cls][1]) == hipSuccess) {
        float ms = 0.f;
        m->watch_pending[cls] = false;
        // (only a batch of about the size the class was measured at is held against that figure: classes 6 / 7 span 129 ..
        // 16 383 needles, and a small batch's fixed costs -- 1.4 us a needle at 256 against 0.5 at 4 096 -- are not a slow sweep)
        const bool comparable = m->tuned_n[cls] != 0 && m->watch_n[cls] * 2 >= m->tuned_n[cls] && m->watch_n[cls] <= m->tuned_n[cls] * 2;
        if (hipEventElapsedTime(&ms, m->watch_ev[cls][0], m->watch_ev[cls][1]) == hipSuccess && m->watch_n[cls] && comparable &&
            m->tuned_us_per_needle[cls] > 0.f && m->ws_choice[cls] != 0) {
          const float us = 1000.f * ms / float(m->watch_n[cls]);
          // (TWO batches in a row: a single slow one -- seen on a shared box, 2.3 x inside bench.py's three timed steps --
          // would put a measurement of every sweep, twice, into a batch that had nothing wrong)
          if (us <= 1.10f * m->tuned_us_per_needle[cls]) {
            m->watch_strikes[cls] = 0;
          } else if (++m->watch_strikes[cls] >= 2 && m->retune_holdoff[cls] == 0) {
            m->ws_choice[cls] = 0;                     // measured again, below
            m->retune_holdoff[cls] = 16;
            m->watch_strikes[cls] = 0;
            ++m->retunes;
          }
        }
      }
      if (m->retune_holdoff[cls] && !scoped) --m->retune_holdoff[cls];
      if (!tunable) {
        choice = static_choice;
      } else if (m->ws_choice[cls] != 0 && (m->ws_choice[cls] != 2 || ws_possible) && (m->ws_choice[cls] != 3 || leave_possible)) {
        choice = m->ws_choice[cls];
      } else if (cb || scoped) {
        choice = static_choice;                        // (counters must describe ONE sweep: an unmeasured class is not measured here;
                                                       // nor by a scoped call)
      } else {
        if (!m->tune_ev[0]) {
          hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
          for (auto& e : ev)
            if (hipEventCreate(&e) != hipSuccess) {
              for (auto& d : ev) if (d) (void)hipEventDestroy(d);
              errno = EIO;
              return -1;
            }
          for (int i = 0; i < 7; ++i) m->tune_ev[i] = ev[i];
        }
        // every sweep the class can take, TWICE, the better run counting (the first run of all meets cold caches; one
        // sample per sweep with a 1.5 % margin -- rounds 3 and 4 -- sat inside run-to-run noise); the plain sweep goes last,
        // so that the rows in place are its
        const int order[6] = {1, leave_possible ? 3 : 0, ws_possible ? 2 : 0, leave_possible ? 3 : 0, ws_possible ? 2 : 0, 1};
        float ms_of[4] = {0.f, 0.f, 0.f, 0.f};         // by sweep: [1] plain, [2] window-major, [3] slices left out
        BLURRILY_HIP_TRY(hipEventRecord(m->tune_ev[0], stream));
        for (int k = 0; k < 6; ++k) {
          if (order[k] && run_sweep(order[k]) < 0) return -1;
          BLURRILY_HIP_TRY(hipEventRecord(m->tune_ev[k + 1], stream));
        }
        BLURRILY_HIP_TRY(hipEventSynchronize(m->tune_ev[6]));
        for (int k = 0; k < 6; ++k) {
          if (!order[k]) continue;
          float ms = 0.f;
          BLURRILY_HIP_TRY(hipEventElapsedTime(&ms, m->tune_ev[k], m->tune_ev[k + 1]));
          ms_of[order[k]] = ms_of[order[k]] == 0.f ? ms : std::min(ms_of[order[k]], ms);
        }
        if (m->tune_inject >= 1 && m->tune_inject <= 3) { ms_of[m->tune_inject] *= 0.5f; m->tune_inject = 0; }   // (tests)
        choice = 1;
        float best = ms_of[1];
        if (leave_possible && ms_of[3] < 0.97f * ms_of[1]) { choice = 3; best = ms_of[3]; }
        if (ws_possible && ms_of[2] < 0.95f * ms_of[1] && ms_of[2] < best) { choice = 2; best = ms_of[2]; }
        m->ws_choice[cls] = choice;
        m->ws_tuned_ms[cls][0] = ms_of[1]; m->ws_tuned_ms[cls][1] = ms_of[2]; m->ws_tuned_ms[cls][2] = ms_of[3];
        m->tuned_us_per_needle[cls] = 1000.f * best / float(n);
        m->tuned_n[cls] = n;
        m->watch_pending[cls] = false;
        m->last_tuned = cls;
        m->last_sweep = 1;                             // (the rows in place are the plain run's; all give the same)
        a.nm_cmin = 0;
        goto short_needles_done;
      }
      const bool watch = tunable && !cb && !scoped && m->ws_choice[cls] == choice && m->tuned_us_per_needle[cls] > 0.f;
      if (watch) {
        if (!m->watch_ev[cls][1]) {                    // (both events or none: a half-made pair would be recorded into)
          hipEvent_t e0 = nullptr, e1 = nullptr;
          if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
            if (e0) (void)hipEventDestroy(e0);
            errno = EIO;
            return -1;
          }
          m->watch_ev[cls][0] = e0; m->watch_ev[cls][1] = e1;
        }
        BLURRILY_HIP_TRY(hipEventRecord(m->watch_ev[cls][0], stream));
      }
      if (run_sweep(choice) < 0) return -1;
      if (watch) {
        BLURRILY_HIP_TRY(hipEventRecord(m->watch_ev[cls][1], stream));
        m->watch_pending[cls] = true;
        m->watch_n[cls] = n;
      }
      if (is_base) m->last_sweep = choice;
      a.nm_cmin = 0;
    }
  short_needles_done:
    // longer needles: 16-bit counters, one workgroup per CU, 256 rows per pass
    if (maybe_long) {
      for (uint32_t base = 0; base < limit; base += 256) {
        a.work_list = big_list; a.n_work_dev = scalars; a.n_work = 0;
        a.pass_base = base; a.keep = std::min<uint32_t>(256, limit - base);
        a.pool_cap = 1024;
        if (!(a.queue = next_queue())) { errno = EIO; return -1; }
        const uint32_t grid = uint32_t(std::min<size_t>(n, size_t(m->n_cus)));
        if (do_launch_find(cb, a, true, grid, stream) < 0) return -1;
      }
    }
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
  if (m->timing && !m->ev[0])                          // (every timed run_find_on goes through here: its events, at first use)
    for (auto& e : m->ev) BLURRILY_HIP_TRY(hipEventCreate(&e));
  if (m->collect_stats) {
    if (!m->d_stats) BLURRILY_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m->d_stats), kStatAllSlots * 8));
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
