// cluster.h -- launch interface of the clustering kernels (cluster_kernels.hip): connected
// components of the graph "J(a, b) >= min_permille / 1000" over a list of stored references, J = m / (T + R - m) as in
// similar.h.  The pairs are never written: a sweep that finds an edge joins its ends in a union-find forest in device
// memory and forgets it.
//
// Nodes are numbered by the caller's references sorted ascending without repeats (node u holds refs[u]; a reference
// the map does not hold keeps its number and is no node).  A node's POSITION is where the extraction found it:
// loc.x * kWindowRanks + loc.y, the delta image's windows numbered behind the base image's.  An edge is found from its
// end at the higher position only, so each is found once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "cluster_plan.h"
#include "device_index.h"
#include "segsort.h"

namespace blurrily {

constexpr uint32_t kNoNode = 0xFFFFFFFFu;

// What a call's launches add up and the host reads at the end.
struct ClusterTotals {
  unsigned long long edges;      // unions attempted: every edge once
  uint32_t           clusters;   // roots among the nodes
  uint32_t           error;      // non-zero: a bounded loop of the union-find ran out (the host answers EIO)
};

// node_of_pos[position] = u for every node u (kNoNode elsewhere: filled by the caller), parent[u] = u for u < n.
struct ClusterNodesArgs {
  const uint2*    loc;           // [n] where each reference was found (RefExtract::loc; x == 0xFFFFFFFF: nowhere)
  const uint32_t* ntri;          // [n] its trigrams (0: the map does not hold it)
  uint32_t        n;
  uint32_t*       node_of_pos;   // [n_pos]
  uint32_t*       parent;        // [n]
};
int launch_cluster_nodes(const ClusterNodesArgs& a, hipStream_t stream);

// One image, needles [q_base, q_base + n) of the node numbering, in the front ends' layout (needle q's T = q_ntri[q]
// codes at qcodes + qoff[q] + q).  Workgroup b sweeps windows [wr * per, wr * per + per) of needle q_base + b / tasks,
// wr = b % tasks, tasks = ceil(n_windows / per), as far as they lie in front of the needle's own position.
struct ClusterSweepArgs {
  const uint2*    slice_se;
  const uint16_t* ent;
  const uint32_t* win_max_tri;
  const uint32_t* win_min_tri;
  const uint16_t* ntri_of_rank;
  uint32_t        n_windows;
  uint32_t        n_refs;
  uint32_t        dense_min8;
  uint32_t        per;           // windows per workgroup
  uint32_t        win0;          // the image's first window in the positions' numbering
  const uint16_t* qcodes;
  const uint64_t* qoff;
  const uint32_t* q_ntri;
  const uint2*    loc;
  uint32_t        q_base;
  uint32_t        n;
  uint32_t        n_nodes;       // the numbering's size: no chain of parents is longer
  uint32_t        min_permille;
  const uint32_t* node_of_pos;
  uint32_t*       parent;
  ClusterTotals*  totals;
};
int launch_cluster_sweep(const ClusterSweepArgs& a, hipStream_t stream);

// The same sweep for several floors at once (cluster_levels_kernels.hip): floors[0 .. n_floors)
// strictly ascending, s.min_permille == floors[0].  Forest k of "J >= floors[k] / 1000" is the n_nodes words at
// s.parent + k * n_nodes, and s.totals[k] takes level k's edges (an error goes to s.totals[0]).  The node tables and
// the labels are the kernels above, once per level.
constexpr uint32_t kClusterMaxLevels = 8;
struct ClusterLevelsSweepArgs {
  ClusterSweepArgs s;
  uint32_t         n_floors;
  uint32_t         floors[kClusterMaxLevels];
};
int launch_cluster_levels_sweep(const ClusterLevelsSweepArgs& a, hipStream_t stream);

// After the last sweep: labels[i] = refs[root of inv[i]] (inv == nullptr: i itself), kNoNode for a reference that is no
// node; totals->clusters += roots.
struct ClusterLabelArgs {
  const uint32_t* parent;        // [n_nodes]
  const uint32_t* ntri;          // [n_nodes]
  const uint32_t* refs;          // [n_nodes] ascending
  const uint32_t* inv;           // [n] the caller's element i is node inv[i]
  uint32_t        n_nodes;
  uint32_t        n;
  uint32_t*       labels;        // [n]
  ClusterTotals*  totals;
};
int launch_cluster_label(const ClusterLabelArgs& a, hipStream_t stream);

// Cluster centres (cluster_centres_kernels.hip): the same sweep once more, keeping per node what
// the labels forget.  Count mode (mark == false) unites as cluster_sweep_kernel does and adds every edge to the degree
// of both its ends; mark mode, after launch_cluster_centres, sets attached[u] for every node u that shares an edge
// with its component's centre and does nothing else.
struct ClusterCentresSweepArgs {
  ClusterSweepArgs s;
  uint32_t*        degree;       // [n_nodes] zeroed by the caller; count mode adds, mark mode reads
  const uint32_t*  centre_of;    // [n_nodes] mark mode: the number of each node's centre
  uint32_t*        attached;     // [n_nodes] mark mode: 1 is stored, nothing is read
};
int launch_cluster_centres_sweep(const ClusterCentresSweepArgs& a, bool mark, hipStream_t stream);

// After the labels (parent[] final): best[root] = max over the component of degree << 32 | (0xFFFFFFFF - number), then,
// across a launch boundary, centre_of[u] and attached[u] = (u is its centre) for every number (a number that is no node:
// kNoNode and 0), and the caller's elements: centres[i] = refs[centre of inv[i]] (kNoNode for no node), degrees[i].
struct ClusterCentresArgs {
  const uint32_t*     parent;    // [n_nodes]
  const uint32_t*     ntri;      // [n_nodes]
  const uint32_t*     refs;      // [n_nodes] ascending
  const uint32_t*     inv;       // [n] (nullptr: element i is node i)
  const uint32_t*     degree;    // [n_nodes]
  uint32_t            n_nodes;
  uint32_t            n;
  unsigned long long* best;      // [n_nodes] zeroed by the caller
  uint32_t*           centre_of; // [n_nodes]
  uint32_t*           attached;  // [n_nodes]
  uint32_t*           centres;   // [n]
  uint32_t*           degrees;   // [n]
  ClusterTotals*      totals;
};
int launch_cluster_centres(const ClusterCentresArgs& a, hipStream_t stream);

// Cluster cores (cluster_cores_kernels.hip): density-based clusters over the same edges.  A node
// is core when degree >= min_degree; only an edge between two cores unites.  Two sweeps: degree mode (unite == false)
// adds every edge to the degree of both its ends and to totals->t.edges and touches no parent; unite mode, across a
// launch boundary, reads the final degrees, unites the core-core edges (counted in ClusterCoresTotals::core_edges) and
// raises anchor[b] for a non-core b with a core neighbour a to degree[a] << 32 | (0xFFFFFFFF - a): the highest degree
// wins, the lowest number among equals.  0 stays in anchor[b] when no core touches b (a key has a degree >= 1 on top).
struct ClusterCoresTotals {
  ClusterTotals      t;          // edges from degree mode, clusters from the labels, error from either
  unsigned long long core_edges; // unions attempted in unite mode: every edge between two cores once
};
struct ClusterCoresSweepArgs {
  ClusterSweepArgs    s;         // (s.totals is not used: the sweep adds to `totals` below)
  uint32_t*           degree;    // [n_nodes] zeroed by the caller; degree mode adds, unite mode reads
  unsigned long long* anchor;    // [n_nodes] zeroed by the caller; unite mode raises
  uint32_t            min_degree;
  ClusterCoresTotals* totals;
};
int launch_cluster_cores_sweep(const ClusterCoresSweepArgs& a, bool unite, hipStream_t stream);

// The kinds of blurrily_storage_cluster_cores' `kinds` (BLURRILY_KIND_* of include/blurrily_storage.h).
constexpr uint8_t kKindNone = 0, kKindNoise = 1, kKindBorder = 2, kKindCore = 3;

// After the last sweep (parent[], degree[] and anchor[] final): totals->t.clusters += the cores that are their own
// root, and per element i of the caller's, for its number v = inv[i]: no node -> kNoNode, 0, kKindNone; a core ->
// refs[root of v]; anchor[v] != 0 -> refs[root of 0xFFFFFFFF - low32(anchor[v])], a border; else refs[v], noise.
struct ClusterCoresLabelArgs {
  const uint32_t*           parent;   // [n_nodes]
  const uint32_t*           ntri;     // [n_nodes]
  const uint32_t*           refs;     // [n_nodes] ascending
  const uint32_t*           inv;      // [n] (nullptr: element i is node i)
  const uint32_t*           degree;   // [n_nodes]
  const unsigned long long* anchor;   // [n_nodes]
  uint32_t                  n_nodes;
  uint32_t                  n;
  uint32_t                  min_degree;
  uint32_t*                 labels;   // [n]
  uint32_t*                 degrees;  // [n]
  uint8_t*                  kinds;    // [n]
  ClusterCoresTotals*       totals;
};
int launch_cluster_cores_label(const ClusterCoresLabelArgs& a, hipStream_t stream);

// Cluster extend (cluster_extend_kernels.hip): the forest started from labels the caller holds
// for the OLD nodes, and only the NEW nodes swept.  is_new is a bit per number (bit u & 31 of word u >> 5).
// The seeds, in a launch of their own before the sweeps: old element i (node inv[i], or i) is united with the node
// that holds old_labels[i], looked up among refs[], unless either of the two is no node or is new.
struct ClusterExtendSeedArgs {
  const uint32_t* old_labels;    // [n_old] the caller's
  const uint32_t* inv;           // [n_old] (nullptr: element i is node i)
  const uint32_t* refs;          // [n_nodes] ascending
  const uint32_t* ntri;          // [n_nodes]
  const uint32_t* is_new;        // [(n_nodes + 31) / 32]
  uint32_t        n_old;
  uint32_t        n_nodes;
  uint32_t*       parent;        // [n_nodes]
  ClusterTotals*  totals;
};
int launch_cluster_extend_seed(const ClusterExtendSeedArgs& a, hipStream_t stream);

// cluster_sweep_kernel's sweep with the new nodes as the only needles: needle b / tasks of the launch is node
// new_nodes[s.q_base + b / tasks], and it sweeps EVERY window of the image, whichever image it lives in.  A candidate
// that is the needle is skipped, an old node is united wherever it lies, a new node only from the end at the higher
// position.
struct ClusterExtendSweepArgs {
  ClusterSweepArgs s;            // (s.q_base and s.n count in new_nodes)
  const uint32_t*  new_nodes;    // the new nodes' numbers
  const uint32_t*  is_new;       // [(n_nodes + 31) / 32]
};
int launch_cluster_extend_sweep(const ClusterExtendSweepArgs& a, hipStream_t stream);

// Clusters within blocks (cluster_within_kernels.hip): an edge needs both ends under one block key,
// block_of[u] for number u.  A block is served by one of two kernels, both uniting in the one forest.
// The direct kernel reads no image: a tile is up to kClusterWithinTile consecutive places of `order` (the numbers
// sorted by (key, number)) inside one block, and its workgroup scores the tile's needles against the block's members
// in front of the tile's last place, from the extraction's codes alone.  An edge is found from its end at the higher
// place only.  (ClusterWithinTile and kClusterWithinTile: cluster_plan.h.)
struct ClusterWithinArgs {
  const ClusterWithinTile* tiles;   // [n_tiles]
  const uint32_t* order;         // [n_order] numbers, block after block, ascending inside a block
  uint32_t        n_tiles;
  uint32_t        n_order;
  const uint16_t* qcodes;        // the extraction's (number u's q_ntri[u] distinct codes at qcodes + qoff[u] + u)
  const uint64_t* qoff;
  const uint32_t* q_ntri;        // (0: the map does not hold it, no node)
  uint32_t        n_nodes;
  uint32_t        min_permille;
  uint32_t*       parent;
  ClusterTotals*  totals;
};
int launch_cluster_within(const ClusterWithinArgs& a, hipStream_t stream);

// cluster_sweep_kernel's sweep for the blocks too large to score directly: needle b / tasks of the launch is number
// needles[s.q_base + b / tasks], it sweeps the windows in front of its own position as cluster_sweep_kernel does, and a
// candidate node under another key than the needle's is passed over before it is counted.
struct ClusterWithinSweepArgs {
  ClusterSweepArgs s;            // (s.q_base and s.n count in needles)
  const uint32_t*  needles;      // the swept blocks' numbers
  const uint32_t*  block_of;     // [n_nodes] each number's key
};
int launch_cluster_within_sweep(const ClusterWithinSweepArgs& a, hipStream_t stream);

// Cluster extend within blocks (cluster_extend_within_kernels.hip): cluster extend's forest --
// seeds for the OLD nodes, only the NEW ones looked at -- where a seed and an edge also need both ends under one block
// key, block_of[u] for number u.  The seeds are cluster_extend_seed_kernel's with that one test more.
struct ClusterExtendWithinSeedArgs {
  ClusterExtendSeedArgs s;
  const uint32_t*       block_of;   // [s.n_nodes] each number's key
};
int launch_cluster_extend_within_seed(const ClusterExtendWithinSeedArgs& a, hipStream_t stream);

// The direct kernel: a tile is up to kClusterWithinTile consecutive places of `new_order` (the NEW numbers sorted by
// (key, number)), all of one block, and its workgroup scores them against every member of the block, places
// [tile.begin, tile.end) of `order`, from the extraction's codes alone.  An old member is an edge from the needle's
// side; between two new numbers the edge is the higher number's to find.  (ClusterExtendWithinTile: cluster_plan.h.)
struct ClusterExtendWithinArgs {
  const ClusterExtendWithinTile* tiles;   // [n_tiles]
  const uint32_t* order;         // [n_order] numbers, block after block, ascending inside a block
  const uint32_t* new_order;     // [n_new_order] the new numbers in that order
  uint32_t        n_tiles;
  uint32_t        n_order;
  uint32_t        n_new_order;
  const uint16_t* qcodes;        // the extraction's (number u's q_ntri[u] distinct codes at qcodes + qoff[u] + u)
  const uint64_t* qoff;
  const uint32_t* q_ntri;        // (0: the map does not hold it, no node)
  const uint32_t* is_new;        // [(n_nodes + 31) / 32]
  uint32_t        n_nodes;
  uint32_t        min_permille;
  uint32_t*       parent;
  ClusterTotals*  totals;
};
int launch_cluster_extend_within(const ClusterExtendWithinArgs& a, hipStream_t stream);

// cluster_extend_sweep_kernel's sweep for the blocks too large to score directly: needle b / tasks of the launch is
// number needles[s.q_base + b / tasks], a new number of a swept block, and a candidate node under another key than the
// needle's is passed over before it is counted.
struct ClusterExtendWithinSweepArgs {
  ClusterSweepArgs s;            // (s.q_base and s.n count in needles)
  const uint32_t*  needles;      // the swept blocks' new numbers
  const uint32_t*  is_new;       // [(n_nodes + 31) / 32]
  const uint32_t*  block_of;     // [n_nodes] each number's key
};
int launch_cluster_extend_within_sweep(const ClusterExtendWithinSweepArgs& a, hipStream_t stream);

// Cluster tree (cluster_tree_kernels.hip): the maximum spanning forest of the edges, heights in
// whole per mille, by Boruvka rounds.  A round is one sweep, which chooses instead of uniting, then across launch
// boundaries the merge and the flatten.
// An edge's key, the total order "height descending, lower number ascending, higher number ascending" as one word that
// only rises: h << 54 | (~lo & M27) << 27 | (~hi & M27), never 0 (lo < hi <= M27).  Hence at most 2^27 numbers.
constexpr uint32_t kTreeNumberBits = 27;
constexpr uint32_t kTreeNumberMask = (1u << kTreeNumberBits) - 1u;
constexpr uint32_t kTreeMaxNodes   = 1u << kTreeNumberBits;

// cluster_sweep_kernel's sweep with another ending: an edge whose ends lie in different components of comp[] (frozen
// for the launch) raises best[] of both components to its key; nothing is united.  Round 1 counts the edges into
// s.totals->edges; from round 2 on a needle whose component is closed does nothing.
struct ClusterTreeSweepArgs {
  ClusterSweepArgs    s;         // (s.parent is not used)
  const uint32_t*     comp;      // [n_nodes] each number's component: its root when the round began
  const uint8_t*      closed;    // [n_nodes] by component: no edge leaves it
  unsigned long long* best;      // [n_nodes] by component, zero when the round begins
  uint32_t            round;     // from 1
};
int launch_cluster_tree_sweep(const ClusterTreeSweepArgs& a, hipStream_t stream);

// After a round's sweeps (ClusterTreeMerge, one chosen edge as the caller gets it: cluster_plan.h).  Merge: number i with best[i] != 0 unites its edge's ends in parent[], and the thread that
// made the hook appends {refs[lo], refs[hi], h} to merges[] at (*n_merges)++; a root with best[i] == 0 is closed;
// best[i] = 0 again.  Flatten, across a launch boundary: comp[i] = root of i.
struct ClusterTreeRoundArgs {
  uint32_t*           parent;    // [n_nodes]
  const uint32_t*     refs;      // [n_nodes] ascending
  uint32_t            n_nodes;
  unsigned long long* best;      // [n_nodes]
  uint32_t*           comp;      // [n_nodes]
  uint8_t*            closed;    // [n_nodes]
  ClusterTreeMerge*   merges;    // [n_nodes] (a forest has fewer edges than nodes)
  uint32_t*           n_merges;
  ClusterTotals*      totals;
};
int launch_cluster_tree_merge(const ClusterTreeRoundArgs& a, hipStream_t stream);
int launch_cluster_tree_flatten(const ClusterTreeRoundArgs& a, hipStream_t stream);

// Cluster tree extend (cluster_tree_extend_kernels.hip): the tree of old and new nodes together
// from the records the caller holds for the old ones.  The rounds are the cluster tree's, merge and flatten as they
// are; what offers edges to best[] differs: the new nodes' sweeps, and the old records.
// cluster_tree_sweep_kernel's sweep with cluster_extend_sweep_kernel's needles: needle b / tasks of the launch is node
// new_nodes[t.s.q_base + b / tasks], it sweeps EVERY window of the image, and a candidate that is the needle, or a new
// node at a higher position, is skipped.  Round 1 counts the edges with a new end into t.s.totals->edges.
struct ClusterTreeExtendSweepArgs {
  ClusterTreeSweepArgs t;        // (t.s.q_base and t.s.n count in new_nodes; t.s.parent is not used)
  const uint32_t*      new_nodes;   // the new nodes' numbers
  const uint32_t*      is_new;   // [(n_nodes + 31) / 32]
};
int launch_cluster_tree_extend_sweep(const ClusterTreeExtendSweepArgs& a, hipStream_t stream);

// The old records, a thread each.  Resolve, once per call: keys[i] = record i's key over the numbers of its two
// references, its height as the caller gives it, or 0 when an end is not listed, not held (ntri == 0) or new, or the
// height is below min_permille.  Offer, every round between the sweeps and the merge: a record with keys[i] != 0 whose
// ends lie in different components of comp[] raises best[] of both to its key.
struct ClusterTreeExtendRecordsArgs {
  const ClusterTreeMerge* records;   // [n_records] the caller's, a < b as references
  uint32_t            n_records;
  const uint32_t*     refs;      // [n_nodes] ascending
  const uint32_t*     ntri;      // [n_nodes]
  const uint32_t*     is_new;    // [(n_nodes + 31) / 32]
  uint32_t            n_nodes;
  uint32_t            min_permille;
  unsigned long long* keys;      // [n_records]
  const uint32_t*     comp;      // [n_nodes]
  unsigned long long* best;      // [n_nodes]
};
int launch_cluster_tree_extend_resolve(const ClusterTreeExtendRecordsArgs& a, hipStream_t stream);
int launch_cluster_tree_extend_offer(const ClusterTreeExtendRecordsArgs& a, hipStream_t stream);

// Cluster core tree (cluster_core_tree_kernels.hip): the dendrogram of cluster_cores' cores at
// every floor.  core[u] is number u's core height, the min_degree-th largest height among its edges (kNoCore: no node,
// or fewer edges), and the forest is the cluster tree's over the edges between two numbers with a core height, an
// edge's height capped by both.
// The core heights come from histogram refinement: while they are sought, core[u] is the lower end of a bracket of
// `span` heights that holds u's, above[u] counts u's edges above the bracket, and a sweep sorts every edge whose height
// lies in an end's bracket into one of that end's kCoreBuckets counters, each `width` = ceil(span / kCoreBuckets)
// heights wide.  The settle picks the counter in which the count from the top reaches min_degree: the next bracket,
// `width` heights wide.  A width of 1 is the last.
constexpr uint32_t kCoreBuckets = 32;
constexpr uint32_t kNoCore      = 0xFFFFFFFFu;

// cluster_sweep_kernel's sweep once more: every edge, found from its end at the higher position, adds 1 to the counter
// of each end whose bracket holds its height.  Nothing is united, no bracket is written.  count_edges: the edges are
// added to totals->t.edges (the first sweep's).
struct ClusterCoreHeightSweepArgs {
  ClusterSweepArgs    s;         // (s.parent and s.totals are not used)
  const uint32_t*     core;      // [n_nodes] the brackets' lower ends (kNoCore: out of the running)
  uint32_t*           hist;      // [n_nodes * kCoreBuckets] zero when the sweep begins
  uint32_t            span;      // heights in a bracket
  uint32_t            width;     // heights in a counter: ceil(span / kCoreBuckets)
  uint32_t            count_edges;
  ClusterCoresTotals* totals;
};
int launch_cluster_core_height_sweep(const ClusterCoreHeightSweepArgs& a, hipStream_t stream);

// A thread per number.  pass == 0, before any sweep: core[u] = kNoCore for a number that is no node, 1000 with
// min_degree == 0 (final: no sweep follows), else min_permille, the first bracket's lower end; above[u] = 0.
// pass >= 1, after that sweep: the walk from the top counter, the new core[u] and above[u], the counters zeroed; a
// node whose edges are fewer than min_degree (pass 1 alone can tell) gets kNoCore, and a later pass that finds no
// counter sets the error word.
struct ClusterCoreHeightSettleArgs {
  uint32_t*           core;      // [n_nodes]
  uint32_t*           above;     // [n_nodes]
  uint32_t*           hist;      // [n_nodes * kCoreBuckets]
  const uint32_t*     ntri;      // [n_nodes] (0: no node)
  uint32_t            n_nodes;
  uint32_t            min_permille;
  uint32_t            min_degree;
  uint32_t            pass;
  uint32_t            width;     // of the sweep just finished
  ClusterCoresTotals* totals;
};
int launch_cluster_core_height_settle(const ClusterCoreHeightSettleArgs& a, hipStream_t stream);

// cluster_tree_sweep_kernel's sweep over the edges between numbers with a core height (core[] final), the key's height
// min(h, core[lo], core[hi]).  Round 1 counts those edges into totals->core_edges, and with count_edges (no height
// sweep ran: every edge is one of them) into totals->t.edges too.
struct ClusterCoreTreeSweepArgs {
  ClusterTreeSweepArgs t;        // (t.s.parent and t.s.totals are not used)
  const uint32_t*      core;     // [n_nodes]
  uint32_t             count_edges;
  ClusterCoresTotals*  totals;
};
int launch_cluster_core_tree_sweep(const ClusterCoreTreeSweepArgs& a, hipStream_t stream);

// Cluster tree within blocks (cluster_tree_within_kernels.hip): the cluster tree over the edges
// whose ends carry one block key.  The rounds are the cluster tree's, merge and flatten as they are; a block's edges are
// offered to best[] by one of two kernels, as cluster_within serves a block by one of two.
// cluster_within_kernel's direct form with the tree's ending: a pair that passes the floor and whose ends lie in
// different components of comp[] raises best[] of both to its key; nothing is united (w.parent is not used).  Round 1
// counts the edges into w.totals->edges; from round 2 on a needle or a member whose component is closed takes no part,
// and a tile with no needle left does nothing.
struct ClusterTreeWithinArgs {
  ClusterWithinArgs   w;
  const uint32_t*     comp;      // [n_nodes] each number's component: its root when the round began
  const uint8_t*      closed;    // [n_nodes] by component: no edge leaves it
  unsigned long long* best;      // [n_nodes] by component
  uint32_t            round;     // from 1
};
int launch_cluster_tree_within(const ClusterTreeWithinArgs& a, hipStream_t stream);

// cluster_tree_sweep_kernel's sweep with cluster_within_sweep_kernel's needles and key test: needle b / tasks of the
// launch is number needles[t.s.q_base + b / tasks], and a candidate node under another key than the needle's is passed
// over before the edge is counted and before comp[] is read.
struct ClusterTreeWithinSweepArgs {
  ClusterTreeSweepArgs t;        // (t.s.q_base and t.s.n count in needles; t.s.parent is not used)
  const uint32_t*      needles;  // the swept blocks' numbers
  const uint32_t*      block_of; // [n_nodes] each number's key
};
int launch_cluster_tree_within_sweep(const ClusterTreeWithinSweepArgs& a, hipStream_t stream);

// Cluster edges (cluster_edges_kernels.hip): the edges themselves, each once, where every other
// entry forgets them.  A sweep that finds an edge appends its key, the cluster tree's total order as one word that is
// sorted ASCENDING: (1000 - h) << 54 | lo << 27 | hi, lo < hi the two numbers (kTreeNumberBits each).  Keys are distinct:
// an edge is found once.
struct ClusterEdgeKey {
  unsigned long long k;
};
// Where a call's launches append, all of them through one cursor: a wave adds its lanes' edges to *cursor once and
// stores the keys whose slot lies below `room`.  The cursor counts on past the room, so its final value is the edge
// count whatever was stored (room == 0: nothing is, keys may be null).
struct ClusterEdgesOut {
  unsigned long long* cursor;    // [1] zero when the call begins
  ClusterEdgeKey*     keys;      // [room]
  unsigned long long  room;
};
// cluster_sweep_kernel's sweep with the append for an ending.  needles == nullptr: needle b / tasks of the launch is
// number s.q_base + b / tasks, as cluster_sweep_kernel's.  Otherwise it is needles[s.q_base + b / tasks] and a candidate
// under another key of block_of[] is passed over before the edge is counted, as cluster_within_sweep_kernel's.
struct ClusterEdgesSweepArgs {
  ClusterSweepArgs s;            // (s.parent and s.totals are not used)
  const uint32_t*  needles;      // the swept blocks' numbers, or null
  const uint32_t*  block_of;     // [n_nodes] each number's key (null with needles)
  ClusterEdgesOut  out;
};
int launch_cluster_edges_sweep(const ClusterEdgesSweepArgs& a, hipStream_t stream);
// cluster_within_kernel's direct form with the same ending (w.parent and w.totals are not used).
struct ClusterEdgesWithinArgs {
  ClusterWithinArgs w;
  ClusterEdgesOut   out;
};
int launch_cluster_edges_within(const ClusterEdgesWithinArgs& a, hipStream_t stream);

// Sorting the keys ascending, one segment (segsort.h): cluster_edges_tiles_kernel, a bitonic sort in LDS per tile, and
// the shared merge passes.
constexpr uint32_t kClusterEdgesTile = 4096;
int launch_cluster_edges_tiles(const SegTile* tiles, uint32_t n_tiles, const ClusterEdgeKey* in, ClusterEdgeKey* out,
                               hipStream_t stream);
int launch_cluster_edges_merge(const SegMergeArgs<ClusterEdgeKey>& a, hipStream_t stream);
template <>
struct SegKey<ClusterEdgeKey> {
  static constexpr uint32_t kTile = kClusterEdgesTile;
  static int tiles(const SegTile* t, uint32_t n, const ClusterEdgeKey* in, ClusterEdgeKey* out, hipStream_t s) {
    return launch_cluster_edges_tiles(t, n, in, out, s);
  }
  static int merge(const SegMergeArgs<ClusterEdgeKey>& a, hipStream_t s) { return launch_cluster_edges_merge(a, s); }
#ifdef __HIPCC__
  __device__ static bool less(ClusterEdgeKey a, ClusterEdgeKey b) { return a.k < b.k; }
#endif
};

// Key i to record i: {refs[lo], refs[hi], 1000 - (key >> 54)}.
struct ClusterEdgesRowsArgs {
  const ClusterEdgeKey* keys;    // [n_keys] sorted
  const uint32_t*       refs;    // [n_nodes] ascending
  uint32_t              n_keys;
  uint32_t              n_nodes;
  ClusterTreeMerge*     rows;    // [n_keys]
};
int launch_cluster_edges_rows(const ClusterEdgesRowsArgs& a, hipStream_t stream);

// The edges with a new end, or with an end on each side (cluster_edges_extend_kernels.hip):
// cluster_extend_sweep_kernel's range -- needle b / tasks of the launch is node needles[s.q_base + b / tasks], it sweeps
// EVERY window of the image, whichever image it lives in, and a candidate that is the needle is skipped -- with
// cluster_edges_sweep_kernel's append for an ending.  side is a bit per number (mark_new's: the new numbers, or the
// right ones); every needle of a call lies on ONE side.  A candidate on the needle's side is passed over when
// `between` is set, and otherwise when it lies at a higher position than the needle (such an edge is its higher end's).
struct ClusterEdgesExtendSweepArgs {
  ClusterSweepArgs s;            // (s.q_base and s.n count in needles; s.parent and s.totals are not used)
  const uint32_t*  needles;      // the swept side's numbers
  const uint32_t*  side;         // [(n_nodes + 31) / 32]
  uint32_t         between;      // non-zero: only edges across the sides
  ClusterEdgesOut  out;
};
int launch_cluster_edges_extend_sweep(const ClusterEdgesExtendSweepArgs& a, hipStream_t stream);

// Cluster cores within blocks (cluster_cores_within_kernels.hip): cluster cores over the edges
// whose ends carry one block key, so a degree counts those edges only.  The two passes are cluster cores' -- degree
// mode, then across a launch boundary unite mode -- and in each a block is served by one of two kernels, as
// cluster_within serves it, both adding into the one degree[], anchor[], forest and totals.
// cluster_within_kernel's direct form with cluster cores' two endings.  Degree mode adds every pair that passes to the
// degree of both its ends and to totals->t.edges and touches no parent; unite mode reads the final degrees, unites the
// pairs of two cores in w.parent (counted in totals->core_edges) and raises anchor[] of a pair's end that is no core to
// the key of the end that is one.  (w.totals is not used.)
struct ClusterCoresWithinArgs {
  ClusterWithinArgs   w;
  uint32_t*           degree;    // [n_nodes] zeroed by the caller; degree mode adds, unite mode reads
  unsigned long long* anchor;    // [n_nodes] zeroed by the caller; unite mode raises
  uint32_t            min_degree;
  ClusterCoresTotals* totals;
};
int launch_cluster_cores_within(const ClusterCoresWithinArgs& a, bool unite, hipStream_t stream);

// cluster_cores_sweep_kernel's sweep with cluster_within_sweep_kernel's needles and key test: needle b / tasks of the
// launch is number needles[c.s.q_base + b / tasks], and a candidate node under another key than the needle's is passed
// over before anything is counted or raised.
struct ClusterCoresWithinSweepArgs {
  ClusterCoresSweepArgs c;       // (c.s.q_base and c.s.n count in needles)
  const uint32_t*       needles; // the swept blocks' numbers
  const uint32_t*       block_of;   // [n_nodes] each number's key
};
int launch_cluster_cores_within_sweep(const ClusterCoresWithinSweepArgs& a, bool unite, hipStream_t stream);

// Cluster core tree within blocks (cluster_core_tree_within_kernels.hip): the cluster core tree
// over the edges whose ends carry one block key, so a core height ranks those edges only.  The height passes and the
// rounds are the core tree's -- settle, merge and flatten as they are -- and in each a block is served by one of two
// kernels, as cluster_within serves it, both adding into the one hist[], best[] and totals.  Each kernel has the core
// tree's two endings, and one record of arguments serves both: the height ending reads core, hist, span, width and
// count_edges (the first pass: the pairs that pass are added to totals->t.edges), the tree ending core, comp, closed,
// best, round and count_edges (no height pass ran: round 1 adds its edges to totals->t.edges as well as to
// totals->core_edges).
// cluster_within_kernel's direct form with those endings (w.parent and w.totals are not used).
struct ClusterCoreTreeWithinArgs {
  ClusterWithinArgs   w;
  const uint32_t*     core;      // [n_nodes] the brackets' lower ends, or (tree) the core heights; kNoCore: none
  uint32_t*           hist;      // height: [n_nodes * kCoreBuckets] zero when the pass begins
  uint32_t            span;      // height: heights in a bracket
  uint32_t            width;     // height: heights in a counter, ceil(span / kCoreBuckets)
  uint32_t            count_edges;
  const uint32_t*     comp;      // tree: [n_nodes] each number's component, its root when the round began
  const uint8_t*      closed;    // tree: [n_nodes] by component: no edge leaves it
  unsigned long long* best;      // tree: [n_nodes] by component
  uint32_t            round;     // tree: from 1
  ClusterCoresTotals* totals;
};
int launch_cluster_core_tree_within(const ClusterCoreTreeWithinArgs& a, bool tree, hipStream_t stream);

// cluster_core_tree_kernels.hip's sweep with cluster_within_sweep_kernel's needles and key test: needle b / tasks of the
// launch is number needles[s.q_base + b / tasks], and a candidate node under another key than the needle's is passed
// over before anything is counted, added or offered.
struct ClusterCoreTreeWithinSweepArgs {
  ClusterSweepArgs    s;         // (s.q_base and s.n count in needles; s.parent and s.totals are not used)
  const uint32_t*     needles;   // the swept blocks' numbers
  const uint32_t*     block_of;  // [n_nodes] each number's key
  const uint32_t*     core;      // as above, and so the rest
  uint32_t*           hist;
  uint32_t            span;
  uint32_t            width;
  uint32_t            count_edges;
  const uint32_t*     comp;
  const uint8_t*      closed;
  unsigned long long* best;
  uint32_t            round;
  ClusterCoresTotals* totals;
};
int launch_cluster_core_tree_within_sweep(const ClusterCoreTreeWithinSweepArgs& a, bool tree, hipStream_t stream);

}  // namespace blurrily
