// find_choice_check.cpp -- the decisions of run_find_on and find_few (blurrily_amd/csrc/find_choice.h) against expectations
// written down by hand from the expressions they were taken out of.  Stand-alone: tests/test_find_choice.py builds and runs it,
// once plainly and once under the address and undefined-behaviour sanitizers.
#include "find_choice.h"

#include <cstdio>

using namespace blurrily::detail;

static int failures = 0;
#define EXPECT(cond) \
  do { if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static void the_class() {
  EXPECT(batch_class(129, 32) == 6 && batch_class(129, 33) == 7);
  EXPECT(batch_class(16383, 32) == 6 && batch_class(16384, 32) == 0);
  EXPECT(batch_class(65535, 32) == 0 && batch_class(65536, 32) == 1);
  EXPECT(batch_class(262143, 32) == 1 && batch_class(262144, 32) == 2);
  EXPECT(batch_class(16383, 33) == 7 && batch_class(16384, 33) == 3);
  EXPECT(batch_class(65535, 33) == 3 && batch_class(65536, 33) == 4);
  EXPECT(batch_class(262143, 33) == 4 && batch_class(262144, 33) == 5);
  EXPECT(batch_class(1, 1) == 6 && batch_class(size_t(1) << 32, 1024) == 5);
}

static void the_latency_ranges() {
  const struct { size_t n; uint32_t limit, n_windows, tasks_per_wg, ranges; } rows[] = {
      {32, 10, 100, 0, 16}, {60, 10, 100, 0, 8},  {61, 10, 100, 0, 16}, {224, 10, 100, 0, 4},
      {225, 10, 100, 0, 1}, {32, 1024, 100, 0, 4}, {32, 1025, 100, 0, 1}, {32, 0, 100, 0, 1},
      {32, 10, 3, 0, 2},    {32, 10, 2, 0, 1},    {32, 10, 100, 4, 50}};
  for (const auto& r : rows) {
    const uint32_t got = latency_ranges(r.n, r.limit, r.n_windows, 512, r.tasks_per_wg);
    if (got != r.ranges) std::printf("latency_ranges(%zu, %u, %u, 512, %u) = %u, not %u\n", r.n, r.limit, r.n_windows,
                                     r.tasks_per_wg, got, r.ranges);
    EXPECT(got == r.ranges);
  }
}

// find_few's ranges: the shared launch outside few_max < n_rows <= mid_max, latency_ranges inside, lowered to 4 608 lists
static void the_ranges_of_a_few() {
  const size_t rows[] = {2, 24, 25, 60, 61, 128}, wgs[] = {608, 1216};
  const uint32_t limits[] = {1, 10, 120}, windows[] = {2, 3, 5, 129, 515};
  for (size_t n : rows)
    for (uint32_t limit : limits)
      for (uint32_t w : windows)
        for (size_t g : wgs) {
          // "latency_tasks" 0: the product always fits, the rule's own value; the defaults' gate (24, 128) and none (1, 128)
          const uint32_t rule = latency_ranges(n, limit, w, g, 0);
          EXPECT(n * rule <= 4608);
          EXPECT(few_ranges(n, 24, 128, limit, w, g, 0, 4608) == (n > 24 ? rule : 1u));
          EXPECT(few_ranges(n, 1, 128, limit, w, g, 0, 4608) == rule);
          EXPECT(few_ranges(n, 1, uint32_t(n) - 1, limit, w, g, 0, 4608) == 1);      // beyond mid_max
          if (w < 129) continue;
          for (uint32_t tasks : {8u, 16u}) {                // the option that reaches the bound
            const uint32_t free_ = latency_ranges(n, limit, w, g, tasks), got = few_ranges(n, 1, 128, limit, w, g, tasks, 4608);
            EXPECT(got >= 1 && n * got <= 4608);
            if (n * free_ <= 4608) EXPECT(got == free_);
            else EXPECT(n * got >= 4608 - n + 1);           // no more taken than it must
          }
        }
  // by hand: 25 needles on 608 workgroups 608 / 25 = 24 ranges, 128 needles two tasks a workgroup, 1 216 / 128 = 9;
  // sixteen tasks a workgroup: 9 728 / 128 = 76 ranges, 9 728 tasks, lowered to 4 608 / 128 = 36; 25 needles at limit 1
  // on 1 216 workgroups: 258 window pairs each, 6 450 tasks, lowered to 4 608 / 25 = 184
  EXPECT(few_ranges(25, 24, 128, 10, 515, 608, 0, 4608) == 24);
  EXPECT(few_ranges(128, 24, 128, 10, 515, 608, 0, 4608) == 9);
  EXPECT(latency_ranges(128, 10, 515, 608, 16) == 76 && few_ranges(128, 24, 128, 10, 515, 608, 16, 4608) == 36);
  EXPECT(latency_ranges(25, 1, 515, 1216, 16) == 258 && few_ranges(25, 24, 128, 1, 515, 1216, 16, 4608) == 184);
}

static void the_merges_pool() {
  EXPECT(merge_pool_cap(1, 1) == 1024 && merge_pool_cap(8, 128) == 1024);      // ranges * limit 1 024
  EXPECT(merge_pool_cap(41, 25) == 2048);                                      // 1 025
  EXPECT(merge_pool_cap(2047, 1) == 2048 && merge_pool_cap(64, 64) == 4096 && merge_pool_cap(4097, 1) == 8192);
}

// the shared launch's {windows per workgroup, workgroups per needle}: the three rules' figures at 288 workgroups and 4 608
// lists, where the lists' bound never binds; then where option "mid_workgroups" makes it bind
static void the_shape_of_the_shared_launch() {
  const uint32_t windows[7] = {1, 2, 129, 288, 289, 577, 1200}, rows[6] = {1, 8, 9, 16, 17, 128};
  const uint32_t mid_workgroups[3] = {64, 256, 1024}, min_per[2] = {0, 2};
  static const OneGrid want[2][3][7][6] = {{
    // min_per 0, mid_workgroups 64
    {
     {{1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}},   // 1 window
     {{1, 2}, {1, 2}, {1, 2}, {1, 2}, {1, 2}, {1, 2}},   // 2 windows
     {{1, 129}, {1, 129}, {20, 7}, {34, 4}, {44, 3}, {66, 2}},   // 129 windows
     {{1, 288}, {1, 288}, {42, 7}, {72, 4}, {96, 3}, {144, 2}},   // 288 windows
     {{2, 145}, {2, 145}, {42, 7}, {74, 4}, {98, 3}, {146, 2}},   // 289 windows
     {{4, 145}, {4, 145}, {84, 7}, {146, 4}, {194, 3}, {290, 2}},   // 577 windows
     {{6, 200}, {6, 200}, {172, 7}, {300, 4}, {400, 3}, {600, 2}},   // 1200 windows
    },
    // min_per 0, mid_workgroups 256
    {
     {{1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}},
     {{1, 2}, {1, 2}, {1, 2}, {1, 2}, {1, 2}, {1, 2}},
     {{1, 129}, {1, 129}, {6, 22}, {10, 13}, {10, 13}, {66, 2}},
     {{1, 288}, {1, 288}, {12, 24}, {18, 16}, {20, 15}, {144, 2}},
     {{2, 145}, {2, 145}, {12, 25}, {20, 15}, {20, 15}, {146, 2}},
     {{4, 145}, {4, 145}, {22, 27}, {38, 16}, {40, 15}, {290, 2}},
     {{6, 200}, {6, 200}, {44, 28}, {76, 16}, {80, 15}, {600, 2}},
    },
    // min_per 0, mid_workgroups 1024
    {
     {{1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}},
     {{1, 2}, {1, 2}, {1, 2}, {1, 2}, {1, 2}, {1, 2}},
     {{1, 129}, {1, 129}, {2, 65}, {4, 33}, {4, 33}, {18, 8}},
     {{1, 288}, {1, 288}, {4, 72}, {6, 48}, {6, 48}, {36, 8}},
     {{2, 145}, {2, 145}, {4, 73}, {6, 49}, {6, 49}, {38, 8}},
     {{4, 145}, {4, 145}, {6, 97}, {10, 58}, {10, 58}, {74, 8}},
     {{6, 200}, {6, 200}, {12, 100}, {20, 60}, {20, 60}, {150, 8}},
    }}, {
    // min_per 2, mid_workgroups 64
    {
     {{2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}},
     {{2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}},
     {{2, 65}, {2, 65}, {20, 7}, {34, 4}, {44, 3}, {66, 2}},
     {{2, 144}, {2, 144}, {42, 7}, {72, 4}, {96, 3}, {144, 2}},
     {{2, 145}, {2, 145}, {42, 7}, {74, 4}, {98, 3}, {146, 2}},
     {{4, 145}, {4, 145}, {84, 7}, {146, 4}, {194, 3}, {290, 2}},
     {{6, 200}, {6, 200}, {172, 7}, {300, 4}, {400, 3}, {600, 2}},
    },
    // min_per 2, mid_workgroups 256
    {
     {{2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}},
     {{2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}},
     {{2, 65}, {2, 65}, {6, 22}, {10, 13}, {10, 13}, {66, 2}},
     {{2, 144}, {2, 144}, {12, 24}, {18, 16}, {20, 15}, {144, 2}},
     {{2, 145}, {2, 145}, {12, 25}, {20, 15}, {20, 15}, {146, 2}},
     {{4, 145}, {4, 145}, {22, 27}, {38, 16}, {40, 15}, {290, 2}},
     {{6, 200}, {6, 200}, {44, 28}, {76, 16}, {80, 15}, {600, 2}},
    },
    // min_per 2, mid_workgroups 1024
    {
     {{2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}},
     {{2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}},
     {{2, 65}, {2, 65}, {2, 65}, {4, 33}, {4, 33}, {18, 8}},
     {{2, 144}, {2, 144}, {4, 72}, {6, 48}, {6, 48}, {36, 8}},
     {{2, 145}, {2, 145}, {4, 73}, {6, 49}, {6, 49}, {38, 8}},
     {{4, 145}, {4, 145}, {6, 97}, {10, 58}, {10, 58}, {74, 8}},
     {{6, 200}, {6, 200}, {12, 100}, {20, 60}, {20, 60}, {150, 8}},
    }}};
  for (int p = 0; p < 2; ++p)
    for (int m = 0; m < 3; ++m)
      for (int w = 0; w < 7; ++w)
        for (int r = 0; r < 6; ++r) {
          const OneGrid got = one_grid(windows[w], rows[r], mid_workgroups[m], min_per[p], 288, 4608), &exp = want[p][m][w][r];
          if (got.per != exp.per || got.grid != exp.grid)
            std::printf("one_grid(%u, %u, %u, %u) = {%u, %u}, not {%u, %u}\n", windows[w], rows[r], mid_workgroups[m], min_per[p],
                        got.per, got.grid, exp.per, exp.grid);
          EXPECT(got.per == exp.per && got.grid == exp.grid);
        }
  // "mid_workgroups" 8 192, 40 needles, 130 windows: the three rules give a window per workgroup, 130 * 40 = 5 200 lists;
  // 4 608 / 40 = 115 workgroups per needle fit, so a window pair each: 65 * 40 = 2 600
  const OneGrid g = one_grid(130, 40, 8192, 0, 288, 4608);
  EXPECT(g.per == 2 && g.grid == 65 && g.grid * 40 <= 4608);
  // ... at its largest, on 288 windows and 128 needles: 36 workgroups per needle fit, eight windows each
  const OneGrid h = one_grid(288, 128, 65536, 0, 288, 4608);
  EXPECT(h.per == 8 && h.grid == 36 && h.grid * 128 == 4608);
  // ... and in whole window pairs: 100 windows over 36 workgroups are three each, so four
  const OneGrid k = one_grid(100, 128, 65536, 0, 288, 4608);
  EXPECT(k.per == 4 && k.grid == 25);
}

static void the_static_rule() {
  // {needles, limit, the least mean_hit_slice that takes the window-major sweep at ws_static_slice 2200}
  const struct { size_t n; uint32_t limit; double from; } rows[] = {
      {129, 32, 3740}, {65535, 32, 3740}, {129, 33, 8800}, {65535, 33, 8800},
      {65536, 32, 2200}, {262144, 32, 2200}, {65536, 33, 3740}, {262144, 33, 3740}};
  const uint32_t nm_min_windows = 256;
  for (const auto& r : rows) {
    EXPECT(static_sweep(r.n, r.limit, true, true, r.from, 2200, 300, nm_min_windows) == 2);
    EXPECT(static_sweep(r.n, r.limit, true, true, r.from - 1, 2200, 256, nm_min_windows) == 3);
    EXPECT(static_sweep(r.n, r.limit, true, true, r.from - 1, 2200, 255, nm_min_windows) == 1);
    // the window-major sweep cannot run: slices left out or plain, by the windows alone
    EXPECT(static_sweep(r.n, r.limit, false, true, r.from, 2200, 256, nm_min_windows) == 3);
    EXPECT(static_sweep(r.n, r.limit, false, true, r.from, 2200, 255, nm_min_windows) == 1);
    // slices cannot be left out: window-major or plain
    EXPECT(static_sweep(r.n, r.limit, true, false, r.from, 2200, 300, nm_min_windows) == 2);
    EXPECT(static_sweep(r.n, r.limit, true, false, r.from - 1, 2200, 300, nm_min_windows) == 1);
    EXPECT(static_sweep(r.n, r.limit, false, false, r.from, 2200, 300, nm_min_windows) == 1);
  }
}

static int pick(float leave_ms, float ws_ms, bool ws_possible, bool leave_possible, float* best, int inject = 0) {
  float ms_of[4] = {0.f, 100.f, ws_ms, leave_ms};
  const int choice = pick_sweep(ms_of, &inject, ws_possible, leave_possible, best);
  EXPECT(inject == 0);
  return choice;
}

static void the_pick() {
  float best = 0.f;
  EXPECT(pick(96.9f, 0.f, false, true, &best) == 3 && best == 96.9f);
  EXPECT(pick(97.1f, 0.f, false, true, &best) == 1 && best == 100.f);
  EXPECT(pick(0.f, 94.9f, true, false, &best) == 2 && best == 94.9f);
  EXPECT(pick(0.f, 95.1f, true, false, &best) == 1 && best == 100.f);
  EXPECT(pick(96.9f, 95.1f, true, true, &best) == 3);            // (window-major is measured against PLAIN's 0.95)
  EXPECT(pick(93.f, 94.f, true, true, &best) == 3 && best == 93.f);
  EXPECT(pick(93.f, 92.f, true, true, &best) == 2 && best == 92.f);
  EXPECT(pick(50.f, 50.f, false, false, &best) == 1 && best == 100.f);   // a sweep that cannot run is never picked
  // the injected bad sample: the named sweep at half its time, once
  EXPECT(pick(93.f, 92.f, true, true, &best, 1) == 1 && best == 50.f);
  EXPECT(pick(97.1f, 0.f, false, true, &best, 3) == 3 && best == 48.55f);
  EXPECT(pick(93.f, 190.f, true, true, &best, 2) == 3 && best == 93.f);  // (190 / 2 = 95: not under 0.95 of plain)
  float ms_of[4] = {0.f, 100.f, 80.f, 60.f};
  int inject = 4;                                                // out of range: nothing halved, the value stays
  EXPECT(pick_sweep(ms_of, &inject, true, true, &best) == 3 && inject == 4 && ms_of[1] == 100.f);
  inject = 2;                                                    // the halved figure is what the caller records
  EXPECT(pick_sweep(ms_of, &inject, true, true, &best) == 2 && ms_of[2] == 40.f && best == 40.f);
}

static void the_order_of_a_measurement() {
  const struct { bool ws, leave; int order[6]; } rows[] = {{true, true, {1, 3, 2, 3, 2, 1}}, {false, true, {1, 3, 0, 3, 0, 1}},
                                                           {true, false, {1, 0, 2, 0, 2, 1}}};
  for (const auto& r : rows) {
    int order[6] = {9, 9, 9, 9, 9, 9};
    measure_order(r.ws, r.leave, order);
    for (int k = 0; k < 6; ++k) EXPECT(order[k] == r.order[k]);
    EXPECT(order[0] == 1 && order[5] == 1);                      // the plain sweep twice, and last: the rows in place are its
  }
}

namespace {
struct Watched : ClassChoice {                                 // one class's state, as trigram_map_t keeps it
  Watched() { choice = 3; }
  uint64_t retunes = 0;
  // a watched batch of n needles at us_per_needle, the class measured at 10 us per needle over 4 096
  void batch(float us_per_needle, size_t n = 4096, size_t tuned_at = 4096, float tuned_us = 10.f) {
    watch_n = n; tuned_n = tuned_at; tuned_us_per_needle = tuned_us;
    watch_verdict(us_per_needle * float(n) / 1000.f, this, &retunes);
  }
  bool is(int c, uint32_t s, uint32_t h, uint64_t r) const { return choice == c && strikes == s && holdoff == h && retunes == r; }
};
}  // namespace

static void the_watch() {
  EXPECT(watch_comparable(2048, 4096) && watch_comparable(8192, 4096));
  EXPECT(!watch_comparable(2047, 4096) && !watch_comparable(8193, 4096));
  EXPECT(watch_comparable(2048, 4097) == false && watch_comparable(2049, 4097));   // (half of an odd size: 2 n >= tuned)
  EXPECT(!watch_comparable(4096, 0) && !watch_comparable(0, 4096));
  {
    Watched w;                                                   // 1.10 of the tuned figure exactly: not slow
    w.strikes = 1;
    w.batch(11.f, 1000, 1000);
    EXPECT(w.is(3, 0, 0, 0));
    w.batch(11.1f, 1000, 1000);
    EXPECT(w.is(3, 1, 0, 0));
  }
  {
    Watched w;                                                   // one slow batch: a strike, nothing else; a good one clears it
    w.batch(20.f);
    EXPECT(w.is(3, 1, 0, 0));
    w.batch(10.f);
    EXPECT(w.is(3, 0, 0, 0));
    w.batch(20.f);
    EXPECT(w.is(3, 1, 0, 0));
    w.batch(20.f);                                               // the second in a row: measured again, hold-off 16
    EXPECT(w.is(0, 0, 16, 1));
    w.batch(20.f);                                               // (an unmeasured class: nothing to hold a batch against)
    EXPECT(w.is(0, 0, 16, 1));
  }
  {
    Watched w;                                                   // during the hold-off: strikes count, nothing is unmeasured
    w.holdoff = 5;
    w.batch(20.f);
    EXPECT(w.is(3, 1, 5, 0));
    w.batch(20.f);
    EXPECT(w.is(3, 2, 5, 0));
    w.holdoff = 0;                                               // ... and the next slow batch after it does
    w.batch(20.f);
    EXPECT(w.is(0, 0, 16, 1));
  }
  {
    Watched w;                                                   // batches that are not held against the figure
    w.batch(20.f, 2047);
    w.batch(20.f, 8193);
    w.batch(20.f, 4096, 0);
    w.batch(20.f, 4096, 4096, 0.f);
    w.batch(20.f, 0);
    EXPECT(w.is(3, 0, 0, 0));
    w.batch(20.f, 2048);
    w.batch(20.f, 8192);
    EXPECT(w.is(0, 0, 16, 1));
  }
  {
    Watched w;                                                   // the hold-off runs down with unscoped batches only, and stops at 0
    w.batch(20.f);
    w.batch(20.f);
    EXPECT(w.is(0, 0, 16, 1));
    w.choice = 1;                                                // (measured again)
    for (int k = 0; k < 3; ++k) holdoff_tick(&w.holdoff, true);
    EXPECT(w.holdoff == 16);
    for (int k = 0; k < 15; ++k) holdoff_tick(&w.holdoff, false);
    w.batch(20.f);
    w.batch(20.f);
    EXPECT(w.is(1, 2, 1, 1));                                    // one batch short of the sixteen: still held
    for (int k = 0; k < 2; ++k) holdoff_tick(&w.holdoff, false);
    EXPECT(w.holdoff == 0);
    w.batch(20.f);
    EXPECT(w.is(0, 0, 16, 2));
  }
}

int main() {
  the_class();
  the_order_of_a_measurement();
  the_latency_ranges();
  the_ranges_of_a_few();
  the_merges_pool();
  the_shape_of_the_shared_launch();
  the_static_rule();
  the_pick();
  the_watch();
  std::printf("find_choice: %d expectations failed\n", failures);
  return failures ? 1 : 0;
}
