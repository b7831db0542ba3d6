// cluster_edges_extend_plan_check.cpp -- which side of blurrily_storage_cluster_edges_between sweeps (blurrily_amd/csrc/
// cluster_plan.h: choose_between_side over mark_new's bitmap) against expectations worked out by hand from the contract
// in that header's comment: the side with fewer numbers, a tie the right, a number both lists name on the right only.
// Stand-alone: tests/test_cluster_edges_extend_abi.py builds and runs it, once plainly and once under the address and
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

// left ++ right numbered, marked and chosen as cluster_edges_extend.hip does: (the right sweeps, the needles)
struct Choice {
  bool right;
  U32s needles, is_right;
  size_t nu;
};
static Choice choose(const U32s& left, const U32s& right) {
  U32s all(left), uniq, inv, right_nodes, left_nodes;
  all.insert(all.end(), right.begin(), right.end());
  number_nodes(all.data(), all.size(), uniq, inv);
  Choice c{};
  c.nu = uniq.size();
  mark_new(inv, left.size(), right.size(), c.nu, c.is_right, right_nodes);
  c.right = choose_between_side(c.is_right, right_nodes.size(), c.nu, left_nodes);
  EXPECT(!c.right || left_nodes.empty());
  c.needles = c.right ? right_nodes : left_nodes;
  return c;
}

int main() {
  // the fewer side sweeps, whichever way round: numbers of {10, 20, 30, 40, 50} are 0 .. 4
  Choice c = choose({10, 20, 30}, {40, 50});
  EXPECT(c.right && c.needles == U32s({3, 4}) && c.nu == 5 && c.is_right == U32s({0x18u}));
  c = choose({40, 50}, {10, 20, 30});
  EXPECT(!c.right && c.needles == U32s({3, 4}) && c.is_right == U32s({0x07u}));
  c = choose({50, 10}, {40, 30, 20});                          // shuffled lists: numbers ascend with the references
  EXPECT(!c.right && c.needles == U32s({0, 4}) && c.is_right == U32s({0x0Eu}));

  // a tie: the right
  c = choose({10, 20}, {30, 40});
  EXPECT(c.right && c.needles == U32s({2, 3}));
  c = choose({30, 40}, {10, 20});
  EXPECT(c.right && c.needles == U32s({0, 1}));

  // repeats count once: three distinct on the left against two on the right listed five times
  c = choose({10, 20, 30}, {40, 50, 40, 50, 40});
  EXPECT(c.right && c.needles == U32s({3, 4}) && c.nu == 5);
  c = choose({40, 50, 40, 50, 40}, {10, 20, 30});
  EXPECT(!c.right && c.needles == U32s({3, 4}));

  // one side empty: it sweeps, with no needle; both empty
  c = choose({}, {10, 20});
  EXPECT(!c.right && c.needles.empty() && c.nu == 2 && c.is_right == U32s({0x03u}));
  c = choose({10, 20}, {});
  EXPECT(c.right && c.needles.empty() && c.is_right == U32s({0u}));
  c = choose({}, {});
  EXPECT(c.right && c.needles.empty() && c.nu == 0 && c.is_right.empty());

  // an overlap is counted on the right: {10, 20, 30} against {20, 30, 40} is 1 left, 3 right, so the left sweeps
  c = choose({10, 20, 30}, {20, 30, 40});
  EXPECT(!c.right && c.needles == U32s({0}) && c.nu == 4 && c.is_right == U32s({0x0Eu}));
  // ... {10, 20, 30, 40} against {30, 40}: 2 and 2, a tie, the right
  c = choose({10, 20, 30, 40}, {30, 40});
  EXPECT(c.right && c.needles == U32s({2, 3}));
  // ... a left list wholly named by the right: nothing on the left
  c = choose({20, 30}, {10, 20, 30});
  EXPECT(!c.right && c.needles.empty() && c.is_right == U32s({0x07u}));

  // more than one bitmap word: 40 on the left, 33 .. on the right
  U32s left, right;
  for (uint32_t r = 0; r < 40; ++r) left.push_back(100 + r);
  for (uint32_t r = 0; r < 33; ++r) right.push_back(200 + r);
  c = choose(left, right);
  EXPECT(c.right && c.needles.size() == 33 && c.needles.front() == 40 && c.needles.back() == 72);
  EXPECT(c.is_right == U32s({0u, 0xFFFFFF00u, 0x000001FFu}));
  c = choose(right, left);
  EXPECT(!c.right && c.needles.size() == 33 && c.needles.front() == 40 && c.needles.back() == 72);
  EXPECT(c.is_right == U32s({0xFFFFFFFFu, 0x000000FFu, 0u}));

  std::printf("cluster_edges_extend_plan: %d expectations failed\n", failures);
  return failures != 0;
}
