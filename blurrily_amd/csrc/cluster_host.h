// cluster_host.h -- the host-side call sequence the clustering entries share (cluster.hip, cluster_levels.hip,
// cluster_centres.hip, cluster_cores.hip, cluster_extend.hip, cluster_within.hip, cluster_tree.hip,
// cluster_tree_extend.hip, cluster_core_tree.hip, cluster_tree_within.hip, cluster_edges.hip): the node numbering,
// the block plan of the two within entries, the cluster tree's round bound and record order, and ClusterCall, which
// owns a call's device scratch, runs what every entry does in front of its sweeps, fills the sweeps' common arguments
// per image and chunk, and reads the totals back.  The device code is each entry's own.
#pragma once
#include <algorithm>
#include <vector>

#include "cluster.h"
#include "map_internal.h"

namespace blurrily {
namespace detail __attribute__((visibility("hidden"))) {

constexpr size_t kClusterChunkNeedles = size_t(1) << 20;   // needles per sweep launch (nothing else bounds a chunk)

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

// The block plan of blurrily_storage_cluster_within and blurrily_storage_cluster_tree_within, from
// each number's key: `order`, the numbers block after block, ascending inside a block; every block given to one of the
// two kernels -- the direct kernel's tiles of up to kClusterWithinTile places for a block of at most
// kClusterWithinDirectMax listed members ("scope_strategy" 2: for any block; a block of one has no pair to score and
// gets no tile), the sweep's needle list for a larger one ("scope_strategy" 1: for every block); the tiles that pass
// over the most members first, so that the longest workgroups do not start last (equal ones in the plan's order).
struct ClusterWithinPlan {
  std::vector<uint32_t>          order;
  std::vector<ClusterWithinTile> tiles;
  std::vector<uint32_t>          swept;
  // On the device, after upload(): null where the plan has nothing for the kernel that would read it.
  ClusterWithinTile* d_tiles = nullptr;
  uint32_t *d_order = nullptr, *d_swept = nullptr, *d_block_of = nullptr;
};
// -1 with EINVAL: more tiles than a launch takes.  Needs no GPU.
int plan_within_blocks(const std::vector<uint32_t>& key_of, uint32_t scope_strategy, ClusterWithinPlan& plan);

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

// One call of a clustering entry, from the entry's checks to its return.
struct ClusterCall {
  ClusterCall(trigram_map m, hipStream_t stream) : m(m), stream(stream) {}
  ~ClusterCall();                                            // frees every buffer of the call
  ClusterCall(const ClusterCall&) = delete;
  ClusterCall& operator=(const ClusterCall&) = delete;

  // One more device buffer of the call's, one allocation each, zeroed on the stream if asked (no bytes: p = nullptr).
  template <class T>
  int more(T*& p, size_t bytes, bool zeroed = false) {
    void* v = nullptr;
    if (alloc(&v, bytes, zeroed) < 0) return -1;
    p = static_cast<T*>(v);
    return 0;
  }

  // The beginning: the numbering of `references` (n >= 1), the call's buffers -- `forests` parent arrays of nu words,
  // as many rows of n labels, totals_bytes of zeroed totals -- the uploads, the extraction, the images with their
  // per-rank tables, and the node tables: node_of_pos once, parent + k * nu per forest.
  int begin(const uint32_t* references, size_t n, uint32_t forests, size_t totals_bytes);
  // ... with a numbering the entry made itself, before it asked for a GPU (number_nodes' or number_nodes_keyed's
  // uniq and inv of n elements; both are taken over)
  int begin(std::vector<uint32_t>&& numbering, std::vector<uint32_t>&& element_number, size_t n, uint32_t forests,
            size_t totals_bytes);

  // A block plan onto the device, after begin(): the tiles with `order` if there are tiles, the swept numbers with
  // every number's key (key_of, nu of them) if a block is swept.
  int upload(ClusterWithinPlan& plan, const std::vector<uint32_t>& key_of);

  // `needles` needles (of the numbering, or of an entry's own list) over every image, in chunks: the sweep arguments
  // all entries share, handed to launch(const ClusterSweepArgs&), which adds the entry's own and launches.
  template <class Launch>
  int sweep(size_t needles, uint32_t min_permille, ClusterTotals* totals, Launch&& launch) const {
    for (uint32_t i = 0; i < images.n; ++i) {
      const DeviceIndex& ix = *images.img[i];
      for (size_t s = 0; s < needles; s += kClusterChunkNeedles) {
        const size_t nc = std::min(kClusterChunkNeedles, needles - s);
        ClusterSweepArgs a{};
        a.slice_se = ix.d_slice_se; a.ent = ix.d_ent; a.win_max_tri = ix.d_win_max_tri; a.win_min_tri = tab[i].win_min_tri;
        a.ntri_of_rank = tab[i].ntri_of_rank; a.n_windows = ix.n_windows; a.n_refs = ix.n_refs; a.dense_min8 = ix.dense_min8;
        a.per = windows_per_workgroup(m, ix, nc); a.win0 = i ? x.win0_delta : 0u;
        a.qcodes = x.needles.codes; a.qoff = x.needles.qoff; a.q_ntri = x.needles.ntri; a.loc = x.loc;
        a.q_base = uint32_t(s); a.n = uint32_t(nc); a.n_nodes = uint32_t(nu); a.min_permille = min_permille;
        a.node_of_pos = d_node_of_pos; a.parent = d_parent; a.totals = totals;
        if (launch(a) < 0) return -1;
      }
    }
    return 0;
  }

  // The ending: cluster_label_kernel's arguments for forest k (its row of labels, its ClusterTotals) ...
  ClusterLabelArgs label_args(uint32_t k = 0) const;
  // ... the totals on their way to the host, and, after whatever else the entry reads back, the wait for the stream:
  // EIO if one of the forests' totals, t[0 .. forests), reports that a bounded loop ran out.
  int read_totals(void* host);
  int wait(const ClusterTotals* t);

  trigram_map m;
  hipStream_t stream;
  size_t      n = 0, nu = 0;                                  // the caller's elements, the numbers
  std::vector<uint32_t> inv;                                 // element i's number (empty: i itself)
  RefExtract  x{};                                           // the by-reference front end's (section 11), over every number
  uint32_t*   d_refs = nullptr;                              // [nu] ascending
  const uint32_t* d_inv = nullptr;                           // [n] (nullptr: inv is empty)
  uint32_t*   d_node_of_pos = nullptr;
  uint32_t*   d_parent = nullptr;                            // forest k: words [k * nu, k * nu + nu)
  uint32_t*   d_labels = nullptr;                            // forest k: words [k * n, k * n + n), as the caller's
  void*       d_totals = nullptr;                            // totals_bytes, as the entry's kernels type them

 private:
  int alloc(void** p, size_t bytes, bool zeroed);
  uint32_t  forests = 0;
  size_t    totals_bytes = 0;
  MapImages images{};                                        // (the images the extraction looked the references up in)
  SimilarTables tables;
  SimilarTable  tab[2];
  std::vector<uint32_t> uniq;                                // the numbering's references (the upload's source: kept to the end)
  std::vector<void*> buffers;
};

}  // namespace detail
}  // namespace blurrily
