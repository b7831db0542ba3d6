// cluster_plan_check.cpp -- the clustering entries' host arithmetic (blurrily_amd/csrc/cluster_plan.h: the node
// numbering, the block plan, the new numbers of an extending call, the order of a tree's records) against expectations
// worked out by hand from the contracts in that header's comments, on lists small enough to check by reading.
// Stand-alone: tests/test_find_choice.py builds and runs it, once plainly and once under the address and
// undefined-behaviour sanitizers.
#include "cluster_plan.h"

#include <cstdio>
#include <vector>

using namespace blurrily;
using namespace blurrily::detail;

static int failures = 0;
#define EXPECT(cond) \
  do { if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using U32s = std::vector<uint32_t>;

static_assert(sizeof(ClusterWithinTile) == 12 && sizeof(ClusterTreeMerge) == 12, "three words each, as the kernels read them");
static_assert(kClusterWithinTile == 16, "the tile sizes below");
static_assert(kTreeMaxRounds >= 29, "28 halvings serve 2^27 numbers, and one round finds nothing");

static bool same_tile(const ClusterWithinTile& t, uint32_t begin, uint32_t first, uint32_t count) {
  return t.begin == begin && t.first == first && t.count == count;
}

static void the_numbering() {
  const uint32_t none[1] = {0};
  U32s uniq, inv;
  number_nodes(none, 0, uniq, inv);                          // an empty list
  EXPECT(uniq.empty() && inv.empty());

  const uint32_t ascending[3] = {2, 4, 7};                    // its own numbering
  number_nodes(ascending, 3, uniq, inv);
  EXPECT(uniq == U32s({2, 4, 7}) && inv.empty());

  const uint32_t shuffled[5] = {5, 3, 5, 9, 3};
  uniq.clear();
  number_nodes(shuffled, 5, uniq, inv);
  EXPECT(uniq == U32s({3, 5, 9}) && inv == U32s({1, 0, 1, 2, 0}));

  const uint32_t twice[4] = {1, 2, 2, 3};                     // equal neighbours do not ascend strictly: sorted
  uniq.clear(); inv.clear();
  number_nodes(twice, 4, uniq, inv);
  EXPECT(uniq == U32s({1, 2, 3}) && inv == U32s({0, 1, 1, 2}));
}

static void the_numbering_with_keys() {
  const uint32_t none[1] = {0};
  U32s uniq, inv, key_of;
  EXPECT(number_nodes_keyed(none, none, 0, uniq, inv, key_of));
  EXPECT(uniq.empty() && inv.empty() && key_of.empty());

  const uint32_t ascending[3] = {2, 4, 7}, k_ascending[3] = {9, 8, 9};
  EXPECT(number_nodes_keyed(ascending, k_ascending, 3, uniq, inv, key_of));
  EXPECT(uniq == U32s({2, 4, 7}) && inv.empty() && key_of == U32s({9, 8, 9}));

  // 5 and 3 twice each, under one key each: accepted, and key_of lines up with uniq (3 -> 1, 5 -> 7, 9 -> 2)
  const uint32_t shuffled[5] = {5, 3, 5, 9, 3}, k_one[5] = {7, 1, 7, 2, 1};
  uniq.clear(); key_of.clear();
  EXPECT(number_nodes_keyed(shuffled, k_one, 5, uniq, inv, key_of));
  EXPECT(uniq == U32s({3, 5, 9}) && inv == U32s({1, 0, 1, 2, 0}) && key_of == U32s({1, 7, 2}));

  const uint32_t k_two[5] = {7, 1, 8, 2, 1};                  // 5 under 7 and under 8
  uniq.clear(); inv.clear(); key_of.clear();
  EXPECT(!number_nodes_keyed(shuffled, k_two, 5, uniq, inv, key_of));

  const uint32_t twice[4] = {1, 2, 2, 3}, k_twice[4] = {4, 5, 5, 6};
  uniq.clear(); inv.clear(); key_of.clear();
  EXPECT(number_nodes_keyed(twice, k_twice, 4, uniq, inv, key_of));
  EXPECT(uniq == U32s({1, 2, 3}) && inv == U32s({0, 1, 1, 2}) && key_of == U32s({4, 5, 6}));
}

static void the_block_plan() {
  {  // keys that ascend with the numbers: blocks {0, 1} and {2, 3, 4}, the longer block's tile first
    ClusterWithinPlan p;
    EXPECT(plan_within_blocks({1, 1, 2, 2, 2}, 0, p) == 0);
    EXPECT(p.order == U32s({0, 1, 2, 3, 4}) && p.swept.empty() && p.tiles.size() == 2);
    EXPECT(same_tile(p.tiles[0], 2, 2, 3) && same_tile(p.tiles[1], 0, 0, 2));
  }
  // shuffled keys: key 3 holds numbers 1 and 3, key 5 number 4, key 7 numbers 0 and 2
  const U32s shuffled = {7, 3, 7, 3, 5};
  for (uint32_t strategy : {0u, 2u}) {
    ClusterWithinPlan p;
    EXPECT(plan_within_blocks(shuffled, strategy, p) == 0);
    EXPECT(p.order == U32s({1, 3, 4, 0, 2}) && p.swept.empty());
    // the block of one (place 2) has no tile; the two tiles pass over 2 members each: the plan's order
    EXPECT(p.tiles.size() == 2 && same_tile(p.tiles[0], 0, 0, 2) && same_tile(p.tiles[1], 3, 3, 2));
  }
  {  // every block swept, the block of one too
    ClusterWithinPlan p;
    EXPECT(plan_within_blocks(shuffled, 1, p) == 0);
    EXPECT(p.order == U32s({1, 3, 4, 0, 2}) && p.tiles.empty() && p.swept == U32s({1, 3, 4, 0, 2}));
  }
  // blocks of 16, 17 and 33 members at places 0, 16 and 33: 1, 2 and 3 tiles of 16 / 16 + 1 / 16 + 16 + 1 places
  U32s keys;
  keys.insert(keys.end(), 16, 0u);
  keys.insert(keys.end(), 17, 1u);
  keys.insert(keys.end(), 33, 2u);
  for (uint32_t strategy : {0u, 2u}) {
    ClusterWithinPlan p;
    EXPECT(plan_within_blocks(keys, strategy, p) == 0);
    EXPECT(p.order.size() == 66 && p.swept.empty() && p.tiles.size() == 6);
    for (uint32_t u = 0; u < p.order.size(); ++u) EXPECT(p.order[u] == u);
    if (p.tiles.size() != 6) continue;
    // a tile passes over first + count - begin members: 33, 32, 17, then 16 three times in the plan's order
    EXPECT(same_tile(p.tiles[0], 33, 65, 1) && same_tile(p.tiles[1], 33, 49, 16) && same_tile(p.tiles[2], 16, 32, 1));
    EXPECT(same_tile(p.tiles[3], 0, 0, 16) && same_tile(p.tiles[4], 16, 16, 16) && same_tile(p.tiles[5], 33, 33, 16));
  }
  {
    ClusterWithinPlan p;
    EXPECT(plan_within_blocks(keys, 1, p) == 0);
    EXPECT(p.tiles.empty() && p.swept == p.order && p.swept.size() == 66);
  }
}

static void the_new_numbers() {
  U32s is_new, new_nodes;
  mark_new({}, 3, 2, 5, is_new, new_nodes);                   // element i is number i: the new ones are 3 and 4
  EXPECT(is_new == U32s({0x18u}) && new_nodes == U32s({3, 4}));

  // old {10, 20, 30}, new {20, 5}: the numbering is {5, 10, 20, 30}, and 20, which an old element holds too, is marked
  // new with 5.  That is what both extending entries do today, written down from their code as it is.
  const uint32_t all[5] = {10, 20, 30, 20, 5};
  U32s uniq, inv;
  number_nodes(all, 5, uniq, inv);
  EXPECT(uniq == U32s({5, 10, 20, 30}) && inv == U32s({1, 2, 3, 2, 0}));
  mark_new(inv, 3, 2, uniq.size(), is_new, new_nodes);
  EXPECT(is_new == U32s({0x5u}) && new_nodes == U32s({0, 2}));

  // the last number new, at the words' edge
  mark_new({}, 30, 1, 31, is_new, new_nodes);
  EXPECT(is_new == U32s({0x40000000u}) && new_nodes == U32s({30}));
  mark_new({}, 31, 1, 32, is_new, new_nodes);
  EXPECT(is_new == U32s({0x80000000u}) && new_nodes == U32s({31}));
  mark_new({}, 32, 1, 33, is_new, new_nodes);
  EXPECT(is_new == U32s({0u, 1u}) && new_nodes == U32s({32}));
  mark_new({}, 0, 33, 33, is_new, new_nodes);                 // ... and every number
  EXPECT(is_new == U32s({0xFFFFFFFFu, 1u}) && new_nodes.size() == 33 && new_nodes.front() == 0 && new_nodes.back() == 32);
}

static void the_record_order() {
  std::vector<ClusterTreeMerge> r = {{1, 5, 700}, {1, 4, 700}, {0, 9, 700}, {2, 3, 900}, {7, 8, 100}};
  sort_tree_records(r);
  const uint32_t want[5][3] = {{2, 3, 900}, {0, 9, 700}, {1, 4, 700}, {1, 5, 700}, {7, 8, 100}};
  for (int i = 0; i < 5; ++i) EXPECT(r[i].a == want[i][0] && r[i].b == want[i][1] && r[i].permille == want[i][2]);
}

int main() {
  the_numbering();
  the_numbering_with_keys();
  the_block_plan();
  the_new_numbers();
  the_record_order();
  std::printf("cluster_plan: %d expectations failed\n", failures);
  return failures != 0;
}
