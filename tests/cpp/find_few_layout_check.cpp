// find_few_layout_check.cpp -- the pinned page and the device lists of find_few (blurrily_amd/csrc/find_few_layout.h) at
// the kernels' limits, 120 rows kept / 288 workgroups / 16 needles as arguments / 128 needles, against figures written
// down by hand from the constants host_batch.hip held; and the merge of a needle's two lists of rows.  Stand-alone:
// tests/test_find_choice.py builds and runs it, once plainly and once under the address and undefined-behaviour sanitizers.
#include "find_few_layout.h"

#include <cstdio>
#include <vector>

using namespace blurrily::detail;

static int failures = 0;
#define EXPECT(cond) \
  do { if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// rows 128 * 120 * 12 = 184 320 | words 128 * 8 (+ 64) | codes 128 * 64 * 2 = 16 384 | T, postings, start windows 512 each |
// offsets, from a multiple of 8, 129 * 8 = 1 032 (+ 64)
static void the_page() {
  constexpr FewPage P(120, 128);
  static_assert(sizeof(trigram_match_t) == 12, "a packed row");
  EXPECT(P.row_bytes == 1440 && P.words_at == 184320 && P.codes_at == 185408 && P.t_at == 201792);
  EXPECT(P.nb_at == 202304 && P.start_at == 202816 && P.offsets_at == 203328 && P.bytes == 204424);
  EXPECT(P.offsets_at % 8 == 0 && P.bytes % 8 == 0);         // (the second image's offsets are aligned too)
  std::vector<unsigned char> mem(2 * P.bytes);
  unsigned char* base = mem.data();
  EXPECT(P.image(base, 0) == base && P.image(base, 1) == base + 204424);
  unsigned char* page = P.image(base, 1);
  const auto at = [&](const void* p) { return size_t(static_cast<const unsigned char*>(p) - page); };
  EXPECT(at(P.rows(page)) == 0 && at(P.rows(page, 1)) == 1440 && at(P.rows(page, 127) + 120) == P.words_at);
  EXPECT(at(P.words(page)) == 184320 && at(P.words(page) + 2 * 128) + 64 == P.codes_at);
  EXPECT(at(P.codes(page)) == 185408 && at(P.codes(page) + 128 * 64) == P.t_at);
  EXPECT(at(P.T(page)) == 201792 && at(P.T(page) + 128) == P.nb_at);
  EXPECT(at(P.nb(page)) == 202304 && at(P.nb(page) + 128) == P.start_at);
  EXPECT(at(P.start(page)) == 202816 && at(P.start(page) + 128) == P.offsets_at);
  EXPECT(at(P.offsets(page)) == 203328 && at(P.offsets(page) + 129) + 64 == P.bytes);
  // every word of both pages can be written
  for (int which = 0; which < 2; ++which) {
    unsigned char* p = P.image(base, which);
    P.rows(p, 127)[119].weight = 1; P.words(p)[255] = 2; P.codes(p)[128 * 64 - 1] = 3; P.T(p)[127] = 4;
    P.nb(p)[127] = 5; P.start(p)[127] = 6; P.offsets(p)[128] = 7;
  }
}

// keys 4 608 * 120 * 8 = 4 423 680 | flags 4 608 * 4 = 18 432 | tickets 512 | queue 4 -- 4 442 628 bytes so far, all there
// was -- | latency mode's counts 18 432
static void the_lists() {
  constexpr FewLists L(120, 288, 16, 128);
  EXPECT(L.max_lists == 4608);
  EXPECT(L.flags_at == 4423680 && L.tickets_at == 4442112 && L.queue_at == 4442624 && L.mid_counts_at == 4442628);
  EXPECT(L.bytes == 4461060 && L.bytes == 4442628 + L.max_lists * 4);
  std::vector<unsigned char> mem(2 * L.bytes);                // what find_few reserves
  unsigned char* base = mem.data();
  EXPECT(L.image(base, 0) == base && L.image(base, 1) == base + 4461060);
  for (int which = 0; which < 2; ++which) {
    unsigned char* lists = L.image(base, which);
    const auto at = [&](const void* p) { return size_t(static_cast<const unsigned char*>(p) - lists); };
    // {first byte, byte behind the last} of keys, flags, tickets, queue, latency mode's counts
    const size_t region[5][2] = {{at(L.keys(lists)), at(L.keys(lists) + 4608 * 120)}, {at(L.flags(lists)), at(L.flags(lists) + 4608)},
                                 {at(L.tickets(lists)), at(L.tickets(lists) + 128)}, {at(L.queue(lists)), at(L.queue(lists) + 1)},
                                 {at(L.mid_counts(lists)), at(L.mid_counts(lists) + 4608)}};
    EXPECT(region[0][0] == 0 && region[1][0] == 4423680 && region[2][0] == 4442112 && region[3][0] == 4442624 && region[4][0] == 4442628);
    for (int a = 0; a < 5; ++a) {
      EXPECT(region[a][0] < region[a][1] && region[a][1] <= L.bytes);
      for (int b = a + 1; b < 5; ++b) EXPECT(region[a][1] <= region[b][0] || region[b][1] <= region[a][0]);
    }
    // latency mode's counts lie clear of the flags: no count word is a flag word
    EXPECT(region[4][0] >= region[1][1] || region[4][1] <= region[1][0]);
    if (which == 0) {                                         // every region's last word can be written
      L.keys(lists)[4608 * 120 - 1] = 1; L.flags(lists)[4607] = 2; L.tickets(lists)[127] = 3; *L.queue(lists) = 4; L.mid_counts(lists)[4607] = 5;
    }
  }
  // As it always was, and recorded here rather than changed: an image's lists are 4 bytes short of a multiple of 8, so the
  // delta image's 64-bit keys sit on 4-byte boundaries.  The device reads and writes them so; the host never does.
  EXPECT(L.bytes % 8 == 4 && 4442628 % 8 == 4);
}

static bool same(const trigram_match_t* got, const trigram_match_t* want, uint32_t n) {
  for (uint32_t k = 0; k < n; ++k)
    if (got[k].reference != want[k].reference || got[k].matches != want[k].matches || got[k].weight != want[k].weight) return false;
  return true;
}

// rows are {reference, matches, weight}; order: matches descending, weight ascending, reference ascending
static void the_merge() {
  const trigram_match_t a[] = {{7, 9, 1}, {3, 8, 2}, {9, 8, 2}, {5, 8, 4}, {1, 2, 1}};
  const trigram_match_t b[] = {{2, 9, 3}, {4, 8, 2}, {6, 8, 3}, {8, 1, 1}};
  trigram_match_t out[16];
  const trigram_match_t guard = {99, 99, 99};
  for (auto& r : out) r = guard;
  // ties on matches (9: weight 1 before 3; 8: weights 2, 2, 2, 3, 4) and on matches and weight (8 / 2: references 3, 4, 9)
  const trigram_match_t all[] = {{7, 9, 1}, {2, 9, 3}, {3, 8, 2}, {4, 8, 2}, {9, 8, 2}, {6, 8, 3}, {5, 8, 4}, {1, 2, 1}, {8, 1, 1}};
  EXPECT(merge_rows(a, 5, b, 4, 16, out) == 9 && same(out, all, 9) && same(out + 9, &guard, 1));   // a limit above both together
  EXPECT(merge_rows(b, 4, a, 5, 16, out) == 9 && same(out, all, 9));                              // either way round
  for (auto& r : out) r = guard;
  EXPECT(merge_rows(a, 5, b, 4, 3, out) == 3 && same(out, all, 3) && same(out + 3, &guard, 1));    // a limit below either list
  EXPECT(merge_rows(a, 5, b, 4, 1, out) == 1 && same(out, all, 1));
  // one list empty
  EXPECT(merge_rows(a, 5, b, 0, 16, out) == 5 && same(out, a, 5));
  EXPECT(merge_rows(a, 0, b, 4, 16, out) == 4 && same(out, b, 4));
  EXPECT(merge_rows(a, 0, b, 0, 16, out) == 0);
  // counts above the limit are cut to it: the rows behind the limit are not there to be read
  const trigram_match_t a2[] = {{7, 9, 1}, {3, 8, 2}}, b2[] = {{2, 9, 3}, {4, 1, 2}};
  const trigram_match_t cut[] = {{7, 9, 1}, {2, 9, 3}};
  for (auto& r : out) r = guard;
  EXPECT(merge_rows(a2, 4000000000u, b2, 121, 2, out) == 2 && same(out, cut, 2) && same(out + 2, &guard, 1));
  const trigram_match_t cut_b[] = {{7, 9, 1}, {3, 8, 2}};
  EXPECT(merge_rows(a2, 500, b2, 0, 2, out) == 2 && same(out, cut_b, 2));
}

int main() {
  the_page();
  the_lists();
  the_merge();
  std::printf("find_few_layout: %d expectations failed\n", failures);
  return failures ? 1 : 0;
}
