// find_choice.h -- the batch search's decisions as plain arithmetic (find_run.hip's run_find_on acts on them): the ranges
// of latency mode, the class of a batch, the static rule for the short needles' sweep, the pick among measured sweeps,
// the verdict on a watched batch; and find_few's (host_batch.hip): its ranges, the merge's pool, the shared launch's shape.
// No HIP and no map here: tests/cpp/find_choice_check.cpp compiles it alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace blurrily {
namespace detail __attribute__((visibility("hidden"))) {

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
inline uint32_t latency_ranges(size_t n, uint32_t limit, uint32_t n_windows, size_t wgs, uint32_t tasks_per_wg) {
  if (limit == 0 || limit > 1024 || n * 16 > wgs * 7 || n_windows <= 2) return 1;
  const size_t target_tasks = (tasks_per_wg ? tasks_per_wg : n <= 60 ? 1 : 2) * wgs;      // (option "latency_tasks": 0 = this rule)
  uint32_t ranges = uint32_t(std::min<size_t>((n_windows + 1) / 2, target_tasks / n));   // ranges are whole window pairs
  return std::max<uint32_t>(1u, std::min<uint32_t>(ranges, std::max<uint32_t>(1u, 4096u / limit)));      // (the merge's pool)
}

// The ranges of a find_few call of n_rows needles with a posting (host_batch.hip): 1 -- the shared launch,
// find_one_kernel -- unless few_max < n_rows <= mid_max; there latency mode's, lowered until its tasks fit the lists
// the call's buffers hold (find_few_layout.h: FewLists::max_lists).  With tasks_per_wg 0 the bound never binds: the rule
// aims at no more than two tasks per resident workgroup, 2 432 tasks on 1 216 workgroups against 4 608 lists; option
// "latency_tasks" at 8 .. 16 is what reaches it.
inline uint32_t few_ranges(size_t n_rows, uint32_t few_max, uint32_t mid_max, uint32_t limit, uint32_t n_windows, size_t wgs,
                           uint32_t tasks_per_wg, size_t max_lists) {
  if (n_rows <= few_max || n_rows > mid_max) return 1;
  const uint32_t ranges = latency_ranges(n_rows, limit, n_windows, wgs, tasks_per_wg);
  return uint32_t(std::min<size_t>(ranges, std::max<size_t>(1, max_lists / n_rows)));
}

// The pool of the merge behind latency mode's ranges: the power of two at or above ranges * limit, from 1 024.
inline uint32_t merge_pool_cap(uint32_t ranges, uint32_t limit) {
  uint32_t cap = 1024;
  while (cap < ranges * limit) cap <<= 1;
  return cap;
}

// The shared launch's shape (find_one_kernel): windows per workgroup and workgroups per needle.  One window per workgroup
// while that fills at most max_grid of them, whole window pairs beyond; more than eight needles: about mid_workgroups
// (a thousand) workgroups in all -- two rounds of what the chip holds --, i.e. several window pairs a workgroup (its
// later steps arrive with its own threshold: one_select's cheap way); at least min_per (a test's way to the
// several-steps-per-workgroup path on a small image).  Then as many more as keep a launch's lists, grid * n_rows, within
// max_lists: the first three rules do that by themselves up to sixteen needles and at the default mid_workgroups --
// the option may be set to 65 536, and a tunable changes a launch's shape, never whether the call succeeds.
struct OneGrid { uint32_t per, grid; };
inline OneGrid one_grid(uint32_t n_windows, uint32_t n_rows, uint32_t mid_workgroups, uint32_t min_per, uint32_t max_grid,
                        size_t max_lists) {
  const auto whole_pairs = [](uint32_t per) { return per + (per > 1 ? per & 1u : 0u); };
  uint32_t per = 1;
  if (n_windows > max_grid) per = whole_pairs((n_windows + max_grid - 1) / max_grid);
  if (n_rows > 8) {                                       // (from nine needles on: measured, tools/mid_probe.py)
    const uint32_t rows_wgs = std::max<uint32_t>(2u, mid_workgroups / n_rows);     // workgroups per needle
    per = std::max(per, whole_pairs((n_windows + rows_wgs - 1) / rows_wgs));
  }
  per = std::max(per, min_per);
  const uint32_t rows_max = uint32_t(std::max<size_t>(1, max_lists / std::max<uint32_t>(n_rows, 1u)));   // workgroups per needle the lists hold
  per = std::max(per, whole_pairs((n_windows + rows_max - 1) / rows_max));
  return OneGrid{per, (n_windows + per - 1) / per};
}

// The sweeps that can serve a batch's short needles (trigram_map_t::last_sweep, ws_choice).
enum : int { kSweepPlain = 1, kSweepWindows = 2, kSweepLeave = 3, kSweepSmall = 4 };

// The class a batch's choice of sweep is measured and kept under: limit up to / above 32, by batch size.
// (classes 6 and 7: batches of 129 .. 16 383 needles -- a server's coalesced FINDs; at Geonames scale leaving slices
// out wins there as it does on large batches: 0.9 -> 0.8 ms for 1 024 needles, 2.6 -> 2.1 for 4 096, 6.4 -> 5.4 for
// 12 000, which the static rule -- from 256 windows on -- gave away through round 5's first half)
inline int batch_class(size_t n_cls, uint32_t limit) {
  return n_cls < 16384 ? (limit > 32 ? 7 : 6) : (limit > 32 ? 3 : 0) + (n_cls < 65536 ? 0 : n_cls < 262144 ? 1 : 2);
}

// The static rule ("ws_autotune" 0, batches under 129 needles, a counted or scoped call on an unmeasured class):
// window-major by the measured table's mean_hit_slice rule, slices left out from nm_min_windows windows on.
inline int static_sweep(size_t n_cls, uint32_t limit, bool ws_possible, bool leave_possible, double mean_hit_slice,
                        uint32_t ws_static_slice, uint32_t n_windows, uint32_t nm_min_windows) {
  const double slice_factor = (n_cls < 65536 ? (limit > 32 ? 4.0 : 1.7) : (limit > 32 ? 1.7 : 1.0));
  return ws_possible && mean_hit_slice >= slice_factor * double(ws_static_slice) ? kSweepWindows
         : leave_possible && n_windows >= nm_min_windows ? kSweepLeave : kSweepPlain;
}

// The runs of a class's measurement (0: none): every sweep the class can take, TWICE, the better run counting (the first
// run of all meets cold caches; one sample per sweep with a 1.5 % margin -- rounds 3 and 4 -- sat inside run-to-run
// noise); the plain sweep goes last, so that the rows in place are its
inline void measure_order(bool ws_possible, bool leave_possible, int order[6]) {
  const int ws = ws_possible ? kSweepWindows : 0, leave = leave_possible ? kSweepLeave : 0;
  const int runs[6] = {kSweepPlain, leave, ws, leave, ws, kSweepPlain};
  std::copy(runs, runs + 6, order);
}

// The pick among a measurement's times (ms_of by sweep: [1] plain, [2] window-major, [3] slices left out): a sweep other
// than the plain one has to win by 3 % (window-major: 5 %, it pays a launch per window).  *best_ms: the picked sweep's.
// (tests: *tune_inject names a sweep that is seen at HALF its time, once)
inline int pick_sweep(float ms_of[4], int* tune_inject, bool ws_possible, bool leave_possible, float* best_ms) {
  if (*tune_inject >= 1 && *tune_inject <= 3) { ms_of[*tune_inject] *= 0.5f; *tune_inject = 0; }
  int choice = kSweepPlain;
  float best = ms_of[1];
  if (leave_possible && ms_of[3] < 0.97f * ms_of[1]) { choice = kSweepLeave; best = ms_of[3]; }
  if (ws_possible && ms_of[2] < 0.95f * ms_of[1] && ms_of[2] < best) { choice = kSweepWindows; best = ms_of[2]; }
  *best_ms = best;
  return choice;
}

// (only a batch of about the size the class was measured at is held against that figure: classes 6 / 7 span 129 ..
// 16 383 needles, and a small batch's fixed costs -- 1.4 us a needle at 256 against 0.5 at 4 096 -- are not a slow sweep)
inline bool watch_comparable(size_t watch_n, size_t tuned_n) {
  return tuned_n != 0 && watch_n * 2 >= tuned_n && watch_n <= tuned_n * 2;
}

// What a map keeps per class of batch (batch_class): the measured choice and what the measurement saw, and the watch
// on it -- the chosen sweep's later batches of the class are bracketed by two events (the map's: read at the class's
// next batch, never waited for).  Forgetting the choice (a set option, a new image) leaves everything else in place.
struct ClassChoice {
  int      choice = 0;                  // 0 not measured yet, or the kSweep* that serves the class
  float    tuned_ms[3] = {0.f, 0.f, 0.f};   // what the measurement saw: needle-major, window-major, slices left out
  size_t   tuned_n = 0;                 // the batch size it was measured at (the watch compares like with like)
  float    tuned_us_per_needle = 0.f;   // of the sweep that was chosen
  bool     watch_pending = false;       // a bracketed batch is under way or unread
  size_t   watch_n = 0;                 // ... of this many needles
  uint32_t strikes = 0;                 // consecutive batches of the class seen slow (one is noise: another tenant, a clock step)
  uint32_t holdoff = 0;                 // batches of the class until it may be measured again
};

// The verdict on a class's watched batch that took `ms` for c->watch_n needles, against tuned_us_per_needle at tuned_n:
// over 10 % slower is a strike, and the second in a row, outside the hold-off, has the class measured again (choice 0).
// (TWO batches in a row: a single slow one -- seen on a shared box, 2.3 x inside bench.py's three timed steps --
// would put a measurement of every sweep, twice, into a batch that had nothing wrong)
inline void watch_verdict(float ms, ClassChoice* c, uint64_t* retunes) {
  if (!c->watch_n || !watch_comparable(c->watch_n, c->tuned_n) || !(c->tuned_us_per_needle > 0.f) || c->choice == 0) return;
  const float us = 1000.f * ms / float(c->watch_n);
  if (us <= 1.10f * c->tuned_us_per_needle) {
    c->strikes = 0;
  } else if (++c->strikes >= 2 && c->holdoff == 0) {
    c->choice = 0;
    c->holdoff = 16;
    c->strikes = 0;
    ++*retunes;
  }
}
// ... at most once in sixteen batches: the hold-off runs down with every unscoped batch of the class that latency mode
// and the small-haystack sweep do not take, watched or not
inline void holdoff_tick(uint32_t* holdoff, bool scoped) {
  if (*holdoff && !scoped) --*holdoff;
}

}  // namespace detail
}  // namespace blurrily
