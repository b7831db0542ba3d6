// cluster_extend_within_plan_check.cpp -- the block plan of blurrily_storage_cluster_extend_within (blurrily_amd/csrc/
// cluster_plan.h: plan_extend_within_blocks over number_nodes_keyed's keys and mark_new's bitmap) against expectations
// worked out by hand from the contract in that header's comment: the numbers block after block, the new ones in the
// same order, tiles of up to 16 new numbers over the whole block for a block scored directly, the new numbers as
// needles for a block that is swept, nothing for a block without a new number or of one member, the tiles that pass
// over the most members first.  Stand-alone: tests/test_cluster_extend_within_abi.py builds and runs it, once plainly
// and once under the address and undefined-behaviour sanitizers.
#include "cluster_plan.h"

#include <cstdio>
#include <map>
#include <vector>

using namespace blurrily;
using namespace blurrily::detail;

static int failures = 0;
#define EXPECT(cond) \
  do { if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using U32s = std::vector<uint32_t>;

static U32s bits_of(const U32s& numbers, size_t nu) {
  U32s bits((nu + 31) / 32, 0u);
  for (uint32_t u : numbers) bits[u >> 5] |= 1u << (u & 31u);
  return bits;
}
static bool is_set(const U32s& bits, uint32_t u) { return (bits[u >> 5] >> (u & 31u)) & 1u; }

// What every plan must satisfy, whatever the strategy: `order` is the numbers by (key, number), new_order the new ones
// of it, no tile crosses a block or names a number that is not new, a tile's [begin, end) is its block, the tiles come
// by members passed over descending, and every new number of a block of two or more is in exactly one tile or once in
// the needle list -- by block, never both.
static void check_invariants(const U32s& key_of, const U32s& is_new, const ClusterExtendWithinPlan& p) {
  const size_t nu = key_of.size();
  EXPECT(p.order.size() == nu);
  for (size_t i = 1; i < p.order.size(); ++i) {
    const uint32_t x = p.order[i - 1], y = p.order[i];
    EXPECT(key_of[x] < key_of[y] || (key_of[x] == key_of[y] && x < y));
  }
  U32s want_new;
  for (uint32_t u : p.order)
    if (is_set(is_new, u)) want_new.push_back(u);
  EXPECT(p.new_order == want_new);
  std::map<uint32_t, size_t> size_of;                          // members by key
  for (uint32_t k : key_of) ++size_of[k];
  std::vector<int> in_tile(nu, 0), in_swept(nu, 0);
  std::map<uint32_t, int> served;                              // by key: 1 tiles, 2 needles
  for (size_t t = 0; t < p.tiles.size(); ++t) {
    const ClusterExtendWithinTile& tile = p.tiles[t];
    EXPECT(tile.begin < tile.end && tile.end <= nu);
    EXPECT(tile.count >= 1 && tile.count <= kClusterWithinTile && tile.first + tile.count <= p.new_order.size());
    if (tile.end > nu || tile.first + tile.count > p.new_order.size()) continue;
    const uint32_t key = key_of[p.order[tile.begin]];
    EXPECT(tile.end - tile.begin == size_of[key]);             // the whole block: no more, no less
    EXPECT(tile.begin == 0 || key_of[p.order[tile.begin - 1]] != key);
    EXPECT(key_of[p.order[tile.end - 1]] == key);
    for (uint32_t i = 0; i < tile.count; ++i) {
      const uint32_t u = p.new_order[tile.first + i];
      EXPECT(key_of[u] == key && is_set(is_new, u));
      ++in_tile[u];
    }
    served[key] |= 1;
    if (t) EXPECT(p.tiles[t - 1].end - p.tiles[t - 1].begin >= tile.end - tile.begin);
  }
  for (uint32_t u : p.swept) {
    EXPECT(u < nu && is_set(is_new, u));
    if (u < nu) { ++in_swept[u]; served[key_of[u]] |= 2; }
  }
  for (auto& kv : served) EXPECT(kv.second == 1 || kv.second == 2);   // a block is one kernel's as a whole
  for (uint32_t u = 0; u < nu; ++u) {
    const bool pairs = is_set(is_new, u) && size_of[key_of[u]] >= 2;
    EXPECT(in_tile[u] + in_swept[u] == (pairs ? 1 : 0));
  }
}

static ClusterExtendWithinPlan plan_of(const U32s& key_of, const U32s& is_new, uint32_t strategy) {
  ClusterExtendWithinPlan p;
  EXPECT(plan_extend_within_blocks(key_of, is_new, strategy, p) == 0);
  check_invariants(key_of, is_new, p);
  return p;
}

int main() {
  // six blocks whose keys are in no order, three old members each and 0, 1, 15, 16, 17 and 33 new ones, the numbers
  // dealt round the blocks so that every block's members lie anywhere among the numbers
  const uint32_t keys[6] = {50, 7, 90, 3, 20, 60}, news[6] = {0, 1, 15, 16, 17, 33};
  U32s key_of, new_numbers;
  for (uint32_t round = 0; round < 36; ++round)
    for (uint32_t b = 0; b < 6; ++b)
      if (round < 3 + news[b]) {
        if (round >= 3) new_numbers.push_back(uint32_t(key_of.size()));
        key_of.push_back(keys[b]);
      }
  const size_t nu = key_of.size();
  EXPECT(nu == 18 + 82 && new_numbers.size() == 82);
  const U32s is_new = bits_of(new_numbers, nu);

  ClusterExtendWithinPlan p = plan_of(key_of, is_new, 2);
  EXPECT(p.swept.empty() && p.new_order.size() == 82);
  // ceil(new / 16) tiles a block: 0, 1, 1, 1, 2, 3; the block without a new number (key 50) has none
  EXPECT(p.tiles.size() == 8);
  // by members passed over: key 60 (36 members, 3 tiles of 16, 16, 1), 20 (20: 16, 1), 3 (19: 16), 90 (18: 15), 7 (4: 1)
  const uint32_t want_key[8] = {60, 60, 60, 20, 20, 3, 90, 7}, want_count[8] = {16, 16, 1, 16, 1, 16, 15, 1};
  const uint32_t want_size[8] = {36, 36, 36, 20, 20, 19, 18, 4};
  for (size_t t = 0; t < 8 && t < p.tiles.size(); ++t) {
    EXPECT(key_of[p.order[p.tiles[t].begin]] == want_key[t]);
    EXPECT(p.tiles[t].count == want_count[t] && p.tiles[t].end - p.tiles[t].begin == want_size[t]);
    if (t && want_key[t] == want_key[t - 1]) EXPECT(p.tiles[t].first == p.tiles[t - 1].first + p.tiles[t - 1].count);
  }
  // the blocks by key are 3, 7, 20, 50, 60, 90: their places in `order`
  EXPECT(p.tiles[5].begin == 0 && p.tiles[5].end == 19 && p.tiles[7].begin == 19 && p.tiles[7].end == 23);
  EXPECT(p.tiles[3].begin == 23 && p.tiles[3].end == 43 && p.tiles[0].begin == 46 && p.tiles[0].end == 82);
  EXPECT(p.tiles[6].begin == 82 && p.tiles[6].end == 100);
  // ... and in new_order: 16 of key 3, 1 of 7, 17 of 20, none of 50, 33 of 60, 15 of 90
  EXPECT(p.tiles[5].first == 0 && p.tiles[7].first == 16 && p.tiles[3].first == 17 && p.tiles[0].first == 34);
  EXPECT(p.tiles[6].first == 67);

  // every such block swept: the needles are the new numbers in the plan's order, no tile
  ClusterExtendWithinPlan s = plan_of(key_of, is_new, 1);
  EXPECT(s.tiles.empty() && s.swept == s.new_order && s.order == p.order && s.new_order == p.new_order);
  // auto: all of them are far below the cap
  ClusterExtendWithinPlan z = plan_of(key_of, is_new, 0);
  EXPECT(z.swept.empty() && z.tiles.size() == 8);

  // a block of new numbers only (key 4: numbers 1, 3, 5), a block of one new number (key 9: number 2) and one of one
  // old number (key 2: number 0), an old pair without a new number (key 6: numbers 4, 6)
  {
    const U32s k = {2, 4, 9, 4, 6, 4, 6}, nw = bits_of({1, 2, 3, 5}, 7);
    ClusterExtendWithinPlan q = plan_of(k, nw, 2);
    EXPECT(q.order == U32s({0, 1, 3, 5, 4, 6, 2}) && q.new_order == U32s({1, 3, 5, 2}));
    EXPECT(q.tiles.size() == 1 && q.tiles[0].begin == 1 && q.tiles[0].end == 4 && q.tiles[0].first == 0 &&
           q.tiles[0].count == 3);
    EXPECT(q.swept.empty());
    q = plan_of(k, nw, 1);
    EXPECT(q.tiles.empty() && q.swept == U32s({1, 3, 5}));     // (the block of one has no pair: no needle either)
    // nothing new anywhere: nothing to launch under any strategy
    for (uint32_t strategy = 0; strategy < 3; ++strategy) {
      q = plan_of(k, bits_of({}, 7), strategy);
      EXPECT(q.tiles.empty() && q.swept.empty() && q.new_order.empty() && q.order.size() == 7);
    }
    // nothing at all
    q = plan_of({}, {}, 0);
    EXPECT(q.order.empty() && q.new_order.empty() && q.tiles.empty() && q.swept.empty());
  }

  // a number both lists name is new: old {10, 20, 30} under keys {1, 1, 2}, new {20, 40} under {1, 2}
  {
    const U32s refs = {10, 20, 30, 20, 40}, ks = {1, 1, 2, 1, 2};
    U32s uniq, inv, key, nw, new_nodes;
    EXPECT(number_nodes_keyed(refs.data(), ks.data(), refs.size(), uniq, inv, key));
    EXPECT(uniq == U32s({10, 20, 30, 40}) && key == U32s({1, 1, 2, 2}));
    mark_new(inv, 3, 2, uniq.size(), nw, new_nodes);
    EXPECT(new_nodes == U32s({1, 3}) && nw == U32s({0x0Au}));
    ClusterExtendWithinPlan q = plan_of(key, nw, 0);
    EXPECT(q.new_order == U32s({1, 3}) && q.tiles.size() == 2);
    EXPECT(q.tiles[0].begin == 0 && q.tiles[0].end == 2 && q.tiles[0].first == 0 && q.tiles[0].count == 1);
    EXPECT(q.tiles[1].begin == 2 && q.tiles[1].end == 4 && q.tiles[1].first == 1 && q.tiles[1].count == 1);
    // ... and under two keys across the lists it is no numbering at all
    const U32s two = {1, 1, 2, 7, 2};
    U32s u2, i2, k2;
    EXPECT(!number_nodes_keyed(refs.data(), two.data(), refs.size(), u2, i2, k2));
  }

  // around the cap: a block of exactly kClusterExtendWithinDirectMax listed members, old and new together, is scored
  // directly by auto, one of a member more is swept; 1 and 2 do not ask
  {
    const size_t cap = kClusterExtendWithinDirectMax;
    U32s k(2 * cap + 1);
    for (size_t u = 0; u < k.size(); ++u) k[u] = u < cap ? 8u : 5u;   // key 8: cap members, key 5: cap + 1
    const U32s nw = bits_of({3, 4, uint32_t(cap - 1), uint32_t(cap), uint32_t(2 * cap)}, k.size());
    ClusterExtendWithinPlan q = plan_of(k, nw, 0);
    EXPECT(q.swept == U32s({uint32_t(cap), uint32_t(2 * cap)}));
    EXPECT(q.tiles.size() == 1 && q.tiles[0].count == 3 && q.tiles[0].begin == cap + 1 && q.tiles[0].end == 2 * cap + 1 &&
           q.tiles[0].first == 2);
    q = plan_of(k, nw, 1);
    EXPECT(q.tiles.empty() && q.swept.size() == 5);
    q = plan_of(k, nw, 2);
    EXPECT(q.swept.empty() && q.tiles.size() == 2 && q.tiles[0].end - q.tiles[0].begin == cap + 1 &&
           q.tiles[1].end - q.tiles[1].begin == cap);
  }

  std::printf("cluster_extend_within_plan: %d expectations failed\n", failures);
  return failures != 0;
}
