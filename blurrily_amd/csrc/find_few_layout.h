// find_few_layout.h -- the two regions find_few (host_batch.hip) shares with its kernels, each laid out ONCE, and the merge
// of a needle's two lists of rows.  No HIP and no map here, and the kernels' limits (find_kernels.h: kOneMaxKeep,
// kOneMaxGrid, kOneMaxNeedles, kMidMaxNeedles) come in as arguments: tests/cpp/find_few_layout_check.cpp compiles it alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/blurrily_storage.h"

namespace blurrily {
namespace detail __attribute__((visibility("hidden"))) {

// The pinned page of ONE image (trigram_map_t::One::h_out as the host addresses it, d_out as the device does; the delta
// image's page follows the base image's): what the kernels write for the host to poll, and what the host stages for the
// kernels to read over the link.
//   rows [mid_needles][max_keep] | words [mid_needles][2] {count, sequence word} | 64 | codes [mid_needles][64] |
//   T [mid_needles] | postings [mid_needles] | start window [mid_needles] | code offsets [mid_needles + 1] | 64
// (the last three: latency mode's needle arrays -- what the batch path's tokeniser would have left on the device)
struct FewPage {
  size_t row_bytes, words_at, codes_at, t_at, nb_at, start_at, offsets_at, bytes;
  constexpr FewPage(size_t max_keep, size_t mid_needles)
      : row_bytes(max_keep * sizeof(trigram_match_t)), words_at(mid_needles * row_bytes),
        codes_at(words_at + mid_needles * 2 * sizeof(uint32_t) + 64),
        t_at(codes_at + mid_needles * 64 * sizeof(uint16_t)), nb_at(t_at + mid_needles * sizeof(uint32_t)),
        start_at(nb_at + mid_needles * sizeof(uint32_t)),
        offsets_at((start_at + mid_needles * sizeof(uint32_t) + 7) & ~size_t(7)),
        bytes(offsets_at + (mid_needles + 1) * sizeof(uint64_t) + 64) {}
  // image `which`'s page behind `base` (0: the base image, 1: the delta image), and the arrays of a page
  unsigned char*   image(unsigned char* base, int which) const { return base + size_t(which) * bytes; }
  trigram_match_t* rows(unsigned char* page, size_t r = 0) const { return reinterpret_cast<trigram_match_t*>(page + r * row_bytes); }
  uint32_t*        words(unsigned char* page) const { return reinterpret_cast<uint32_t*>(page + words_at); }
  uint16_t*        codes(unsigned char* page) const { return reinterpret_cast<uint16_t*>(page + codes_at); }
  uint32_t*        T(unsigned char* page) const { return reinterpret_cast<uint32_t*>(page + t_at); }
  uint32_t*        nb(unsigned char* page) const { return reinterpret_cast<uint32_t*>(page + nb_at); }
  uint32_t*        start(unsigned char* page) const { return reinterpret_cast<uint32_t*>(page + start_at); }
  uint64_t*        offsets(unsigned char* page) const { return reinterpret_cast<uint64_t*>(page + offsets_at); }
};

// The device lists of ONE image (trigram_map_t::One::d_parts; the delta image's follow the base image's), reserved and
// zeroed once.  max_lists: the lists a launch may leave -- up to max_needles rows of max_grid workgroups, or more rows of
// fewer, or latency mode's tasks (find_choice.h keeps both within it: one_grid, few_ranges).
//   keys [max_lists][max_keep] | flags [max_lists] | tickets [mid_needles] | queue [1] | mid counts [max_lists]
//   flags       INVARIANT: they hold any value but the `seq` of the launch that waits on them.  Only find_one_kernel
//               writes them (a workgroup sets its own to the launch's seq), and a seq is used once: nothing else
//               may point into them -- latency mode's counts, 0 .. limit per task, have the words behind the queue.
//   tickets     zero between launches: the workgroup that takes a row's last ticket hands it back
//   queue       latency mode's task counter, zero between launches: the merge hands it back
//   mid counts  latency mode's rows per task (FindArgs::part_count); its keys share `keys`
// (bytes is 4 modulo 8 at the kernels' limits, so the delta image's keys start off an 8-byte boundary, as they always have)
struct FewLists {
  size_t max_lists, flags_at, tickets_at, queue_at, mid_counts_at, bytes;
  constexpr FewLists(size_t max_keep, size_t max_grid, size_t max_needles, size_t mid_needles)
      : max_lists(max_needles * max_grid), flags_at(max_lists * max_keep * sizeof(unsigned long long)),
        tickets_at(flags_at + max_lists * sizeof(uint32_t)), queue_at(tickets_at + mid_needles * sizeof(uint32_t)),
        mid_counts_at(queue_at + sizeof(uint32_t)), bytes(mid_counts_at + max_lists * sizeof(uint32_t)) {}
  unsigned char*      image(unsigned char* base, int which) const { return base + size_t(which) * bytes; }
  unsigned long long* keys(unsigned char* lists) const { return reinterpret_cast<unsigned long long*>(lists); }
  uint32_t*           flags(unsigned char* lists) const { return reinterpret_cast<uint32_t*>(lists + flags_at); }
  uint32_t*           tickets(unsigned char* lists) const { return reinterpret_cast<uint32_t*>(lists + tickets_at); }
  uint32_t*           queue(unsigned char* lists) const { return reinterpret_cast<uint32_t*>(lists + queue_at); }
  uint32_t*           mid_counts(unsigned char* lists) const { return reinterpret_cast<uint32_t*>(lists + mid_counts_at); }
};

// A needle's rows from the two images (disjoint references), merged into at most `limit` rows at `out`; returns how many.
// got_a / got_b: the counts the kernels left, cut to `limit` here.  Result order: matches descending, weight ascending,
// reference ascending (storage.c:129-138, :566).
inline uint32_t merge_rows(const trigram_match_t* a_rows, uint32_t got_a, const trigram_match_t* b_rows, uint32_t got_b,
                           uint32_t limit, trigram_match_t* out) {
  const uint32_t na = got_a < limit ? got_a : limit, nb = got_b < limit ? got_b : limit;
  uint32_t ia = 0, ib = 0, k = 0;
  while (k < limit && (ia < na || ib < nb)) {
    bool take_a;
    if (ia >= na) take_a = false;
    else if (ib >= nb) take_a = true;
    else {
      const trigram_match_t x = a_rows[ia], y = b_rows[ib];
      take_a = x.matches != y.matches ? x.matches > y.matches : x.weight != y.weight ? x.weight < y.weight : x.reference < y.reference;
    }
    out[k++] = take_a ? a_rows[ia++] : b_rows[ib++];
  }
  return k;
}

}  // namespace detail
}  // namespace blurrily
