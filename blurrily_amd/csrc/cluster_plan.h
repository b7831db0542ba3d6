// cluster_plan.h -- the clustering entries' host arithmetic that needs no GPU: the node
// numbering, the block plan of the blocked entries, which numbers an extending call adds, and the cluster tree's round
// bound and record order, with the two records they work on.  Plain C++: cluster.h includes it for the records,
// cluster_host.h for the rest, and tests/cpp/cluster_plan_check.cpp includes it alone.
#pragma once
#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace blurrily {

// A tile of the blocked entries' direct kernel (cluster.h: ClusterWithinArgs).
constexpr uint32_t kClusterWithinTile = 16;
struct ClusterWithinTile {
  uint32_t begin;                // the block's first place in `order`
  uint32_t first;                // the tile's first place
  uint32_t count;                // its places: 1 .. kClusterWithinTile, all of one block
};

// A tile of the extending blocked entry's direct kernel (cluster.h: ClusterExtendWithinArgs).
struct ClusterExtendWithinTile {
  uint32_t begin, end;           // the block's places in `order`: [begin, end)
  uint32_t first;                // the tile's first place in `new_order`
  uint32_t count;                // its places there: 1 .. kClusterWithinTile, all NEW numbers of that block
};

// One chosen edge, as the caller gets it (blurrily_cluster_merge_t of include/blurrily_storage.h).
struct ClusterTreeMerge { uint32_t a, b, permille; };

namespace detail __attribute__((visibility("hidden"))) {

// The caller's references ascending without repeats (the node numbering), and each element's number.  A list that is
// strictly ascending already is its own numbering: inv stays empty.
inline void number_nodes(const uint32_t* references, size_t n, std::vector<uint32_t>& uniq, std::vector<uint32_t>& inv) {
  bool ascending = true;
  for (size_t i = 1; i < n && ascending; ++i) ascending = references[i - 1] < references[i];
  if (ascending) { uniq.assign(references, references + n); return; }
  std::vector<uint64_t> keyed(n);
  for (size_t i = 0; i < n; ++i) keyed[i] = (uint64_t(references[i]) << 32) | i;
  std::sort(keyed.begin(), keyed.end());
  inv.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t ref = uint32_t(keyed[i] >> 32);
    if (uniq.empty() || uniq.back() != ref) uniq.push_back(ref);
    inv[uint32_t(keyed[i])] = uint32_t(uniq.size() - 1);
  }
}

// The same numbering for references that carry a key each (blurrily_storage_cluster_within's blocks): key_of[u] is number
// u's.  False, with nothing to rely on in the outputs: a reference is listed more than once under different keys.  A
// strictly ascending list names every reference once, so it cannot be, and is its own numbering as above.
inline bool number_nodes_keyed(const uint32_t* references, const uint32_t* keys, size_t n, std::vector<uint32_t>& uniq,
                               std::vector<uint32_t>& inv, std::vector<uint32_t>& key_of) {
  bool ascending = true;
  for (size_t i = 1; i < n && ascending; ++i) ascending = references[i - 1] < references[i];
  if (ascending) { uniq.assign(references, references + n); key_of.assign(keys, keys + n); return true; }
  std::vector<uint64_t> keyed(n);
  for (size_t i = 0; i < n; ++i) keyed[i] = (uint64_t(references[i]) << 32) | i;
  std::sort(keyed.begin(), keyed.end());
  inv.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t ref = uint32_t(keyed[i] >> 32), key = keys[uint32_t(keyed[i])];
    if (uniq.empty() || uniq.back() != ref) { uniq.push_back(ref); key_of.push_back(key); }
    else if (key_of.back() != key) return false;
    inv[uint32_t(keyed[i])] = uint32_t(uniq.size() - 1);
  }
  return true;
}

// The listed members of a block up to which "scope_strategy" 0 scores the block directly.  Direct work grows with the
// square of a block, the sweep's with the map: on configs[2]'s haystack at 700 per mille, one block of 10^5 consecutive
// references takes the direct kernel 16 ms against the sweep's 170 ms, one of 10^6 1.96 s against 1.72 s
// (profiles/cluster_within_geonames.json).  This is the largest size measured at which direct was no slower.
// "scope_strategy" 1 sweeps every block, 2 scores every block directly.
// The tree within blocks takes the same cap: its rounds multiply both kernels' work alike, so there is no reason to
// expect another crossover -- but nobody has measured the crossover for the tree, only one block of 10^5 under either
// kernel: 31 ms direct against 275 ms swept (profiles/cluster_tree_within_geonames.json).
constexpr size_t kClusterWithinDirectMax = 100000;

// The block plan of the blocked entries, from each number's key: `order`, the numbers block
// after block, ascending inside a block; every block given to one of the two kernels -- the direct kernel's tiles of up
// to kClusterWithinTile places for a block of at most kClusterWithinDirectMax listed members ("scope_strategy" 2: for
// any block; a block of one has no pair to score and gets no tile), the sweep's needle list for a larger one
// ("scope_strategy" 1: for every block); the tiles that pass over the most members first, so that the longest
// workgroups do not start last (equal ones in the plan's order).
struct ClusterWithinPlan {
  std::vector<uint32_t>          order;
  std::vector<ClusterWithinTile> tiles;
  std::vector<uint32_t>          swept;
};
// -1 with EINVAL: more tiles than a launch takes.
inline int plan_within_blocks(const std::vector<uint32_t>& key_of, uint32_t scope_strategy, ClusterWithinPlan& plan) {
  // the numbers block after block, ascending inside a block (keys that ascend with the numbers already are)
  const size_t nu = key_of.size();
  std::vector<uint32_t>& order = plan.order;
  order.resize(nu);
  if (std::is_sorted(key_of.begin(), key_of.end())) {
    for (size_t u = 0; u < nu; ++u) order[u] = uint32_t(u);
  } else {
    std::vector<uint64_t> keyed(nu);
    for (size_t u = 0; u < nu; ++u) keyed[u] = (uint64_t(key_of[u]) << 32) | u;
    std::sort(keyed.begin(), keyed.end());
    for (size_t u = 0; u < nu; ++u) order[u] = uint32_t(keyed[u]);
  }
  std::vector<ClusterWithinTile>& tiles = plan.tiles;
  for (size_t b = 0; b < nu;) {
    size_t e = b + 1;
    while (e < nu && key_of[order[e]] == key_of[order[b]]) ++e;
    const bool direct = scope_strategy == 2 || (scope_strategy == 0 && e - b <= kClusterWithinDirectMax);
    if (!direct) {
      plan.swept.insert(plan.swept.end(), order.begin() + b, order.begin() + e);
    } else if (e - b > 1) {                                   // (a block of one has no pair to score)
      for (size_t f = b; f < e; f += kClusterWithinTile)
        tiles.push_back({uint32_t(b), uint32_t(f), uint32_t(std::min<size_t>(kClusterWithinTile, e - f))});
    }
    b = e;
  }
  // the tiles that pass over the most members first: the longest workgroups do not start last
  // (equal ones in the plan's order)
  if (tiles.size() > 0x7FFFFFFFull) { errno = EINVAL; return -1; }
  std::vector<uint64_t> by_scan(tiles.size());
  for (size_t t = 0; t < tiles.size(); ++t)
    by_scan[t] = (uint64_t(~(tiles[t].first + tiles[t].count - tiles[t].begin)) << 32) | t;
  std::sort(by_scan.begin(), by_scan.end());
  std::vector<ClusterWithinTile> sorted(tiles.size());
  for (size_t t = 0; t < tiles.size(); ++t) sorted[t] = tiles[uint32_t(by_scan[t])];
  tiles.swap(sorted);
  return 0;
}

// Which numbers an extending call adds to the n_old elements it is given labels or records for: elements
// [n_old, n_old + n_new) of the numbered list are the new ones (inv, nu: number_nodes' over old ++ new).  is_new is a bit
// per number (bit u & 31 of word u >> 5), new_nodes the numbers whose bit is set, ascending.  A number that an old and
// a new element share is new.
inline void mark_new(const std::vector<uint32_t>& inv, size_t n_old, size_t n_new, size_t nu,
                     std::vector<uint32_t>& is_new, std::vector<uint32_t>& new_nodes) {
  is_new = std::vector<uint32_t>((nu + 31) / 32, 0u);
  new_nodes.clear();
  if (inv.empty()) {                                          // (element i is number i)
    for (size_t j = 0; j < n_new; ++j) new_nodes.push_back(uint32_t(n_old + j));
    for (uint32_t u : new_nodes) is_new[u >> 5] |= 1u << (u & 31u);
  } else {
    for (size_t j = 0; j < n_new; ++j) is_new[inv[n_old + j] >> 5] |= 1u << (inv[n_old + j] & 31u);
    for (size_t u = 0; u < nu; ++u)
      if ((is_new[u >> 5] >> (u & 31u)) & 1u) new_nodes.push_back(uint32_t(u));
  }
}

// The listed members of a block, old and new together, up to which "scope_strategy" 0 lets
// blurrily_storage_cluster_extend_within score the block directly.  Per needle the direct kernel here reads the whole
// block, where cluster_within's reads half of it on average, but only the new numbers are needles, so its work grows
// with new x block, not with the square of the block -- and with few new numbers it launches few workgroups.  Measured
// for this entry on one MI355X (profiles/cluster_extend_within_geonames.json: configs[2]'s haystack at 700 per mille,
// one block with 10^3 new rows, medians of five calls): at 10^5 listed members direct takes 5.61 ms against the
// sweep's 18.4 ms, at 10^6 53.8 ms against 27.4 ms.  This is the largest measured size at which direct was no slower;
// it happens to equal kClusterWithinDirectMax, but it is this entry's own measurement, and nothing between the two
// sizes was measured.
constexpr size_t kClusterExtendWithinDirectMax = 100000;

// The block plan of blurrily_storage_cluster_extend_within, from each number's key and mark_new's
// bit per number: `order` as plan_within_blocks makes it, `new_order` the NEW numbers in the same order, and every block
// that has a new number given to one of two kernels -- the direct kernel's tiles of up to kClusterWithinTile places of
// new_order for a block of at most kClusterExtendWithinDirectMax listed members ("scope_strategy" 2: for any block), the
// sweep's needle list, the block's new numbers, for a larger one ("scope_strategy" 1: for every block).  A block without
// a new number gets neither: its seeds are all there is to it.  Nor does a block of one, which has no pair to score.
// The tiles that pass over the most members first (equal ones in the plan's order).
struct ClusterExtendWithinPlan {
  std::vector<uint32_t>                order, new_order;
  std::vector<ClusterExtendWithinTile> tiles;
  std::vector<uint32_t>                swept;
};
// -1 with EINVAL: more tiles than a launch takes.
inline int plan_extend_within_blocks(const std::vector<uint32_t>& key_of, const std::vector<uint32_t>& is_new,
                                     uint32_t scope_strategy, ClusterExtendWithinPlan& plan) {
  const size_t nu = key_of.size();
  std::vector<uint32_t>& order = plan.order;
  order.resize(nu);
  if (std::is_sorted(key_of.begin(), key_of.end())) {
    for (size_t u = 0; u < nu; ++u) order[u] = uint32_t(u);
  } else {
    std::vector<uint64_t> keyed(nu);
    for (size_t u = 0; u < nu; ++u) keyed[u] = (uint64_t(key_of[u]) << 32) | u;
    std::sort(keyed.begin(), keyed.end());
    for (size_t u = 0; u < nu; ++u) order[u] = uint32_t(keyed[u]);
  }
  std::vector<ClusterExtendWithinTile>& tiles = plan.tiles;
  for (size_t b = 0; b < nu;) {
    size_t e = b + 1;
    while (e < nu && key_of[order[e]] == key_of[order[b]]) ++e;
    const size_t nb = plan.new_order.size();
    for (size_t i = b; i < e; ++i)
      if ((is_new[order[i] >> 5] >> (order[i] & 31u)) & 1u) plan.new_order.push_back(order[i]);
    const size_t ne = plan.new_order.size();
    const bool direct = scope_strategy == 2 || (scope_strategy == 0 && e - b <= kClusterExtendWithinDirectMax);
    if (ne == nb || e - b < 2) {                              // (seeds only, or no pair to score)
    } else if (!direct) {
      plan.swept.insert(plan.swept.end(), plan.new_order.begin() + nb, plan.new_order.end());
    } else {
      for (size_t f = nb; f < ne; f += kClusterWithinTile)
        tiles.push_back({uint32_t(b), uint32_t(e), uint32_t(f), uint32_t(std::min<size_t>(kClusterWithinTile, ne - f))});
    }
    b = e;
  }
  if (tiles.size() > 0x7FFFFFFFull) { errno = EINVAL; return -1; }
  std::vector<uint64_t> by_scan(tiles.size());
  for (size_t t = 0; t < tiles.size(); ++t) by_scan[t] = (uint64_t(~(tiles[t].end - tiles[t].begin)) << 32) | t;
  std::sort(by_scan.begin(), by_scan.end());
  std::vector<ClusterExtendWithinTile> sorted(tiles.size());
  for (size_t t = 0; t < tiles.size(); ++t) sorted[t] = tiles[uint32_t(by_scan[t])];
  tiles.swap(sorted);
  return 0;
}

// Which side of blurrily_storage_cluster_edges_between sweeps: the edges with an end on each side
// are the same set whichever side holds the needles, and a sweep costs per needle, so the side with fewer numbers does
// (a tie: the right).  is_right and right_nodes are mark_new's over left ++ right -- a number both lists name is on the
// right only.  True: the right side sweeps (right_nodes are the needles, left_nodes is left empty).  False: the left
// side does, and left_nodes becomes its numbers, ascending.
inline bool choose_between_side(const std::vector<uint32_t>& is_right, size_t n_right_nodes, size_t nu,
                                std::vector<uint32_t>& left_nodes) {
  left_nodes.clear();
  if (n_right_nodes <= nu - n_right_nodes) return true;
  for (size_t u = 0; u < nu; ++u)
    if (!((is_right[u >> 5] >> (u & 31u)) & 1u)) left_nodes.push_back(uint32_t(u));
  return false;
}

// The cluster tree's rounds.  Every round that merges at least halves the components that still have an edge leaving
// them: 28 rounds serve 2^27 nodes, and one more finds nothing.
constexpr uint32_t kTreeMaxRounds = 40;

// The order of a tree's records: height descending, then the lower reference, then the higher.
inline void sort_tree_records(std::vector<ClusterTreeMerge>& records) {
  std::sort(records.begin(), records.end(), [](const ClusterTreeMerge& x, const ClusterTreeMerge& y) {
    if (x.permille != y.permille) return x.permille > y.permille;
    return x.a != y.a ? x.a < y.a : x.b < y.b;
  });
}

}  // namespace detail
}  // namespace blurrily
