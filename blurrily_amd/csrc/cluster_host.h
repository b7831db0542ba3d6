// cluster_host.h -- the host-side call sequence the clustering entries share (cluster.hip, cluster_levels.hip,
// cluster_centres.hip, cluster_cores.hip, cluster_extend.hip, cluster_within.hip, cluster_cores_within.hip, cluster_tree.hip,
// cluster_tree_extend.hip, cluster_core_tree.hip, cluster_tree_within.hip, cluster_core_tree_within.hip, cluster_edges.hip,
// cluster_edges_extend.hip, cluster_extend_within.hip;
// DESIGN.md sections 25 and 40): ClusterCall, which owns a call's device scratch, runs what every entry does in front of its sweeps -- for the
// blocked entries the block plan too --, fills the sweeps' common arguments per image and chunk, and reads the
// totals back; TreeRounds, the Boruvka rounds of the five tree entries around the entry's own offer of edges; and
// core_height_passes, the bracket loop of the two core tree entries around the entry's own pass over the edges.  The
// arithmetic that needs no GPU (the numbering, the plan, the new numbers, the record order) is cluster_plan.h's.  The
// device code is each entry's own.
#pragma once
#include <algorithm>
#include <vector>

#include "cluster.h"
#include "cluster_plan.h"
#include "map_internal.h"

namespace blurrily {
namespace detail __attribute__((visibility("hidden"))) {

constexpr size_t kClusterChunkNeedles = size_t(1) << 20;   // needles per sweep launch (nothing else bounds a chunk)

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

  // The beginning of a blocked entry, one forest and one ClusterTotals (or the larger record an entry's kernels add
  // into, of totals_bytes): the block plan from number_nodes_keyed's key_of under the map's "scope_strategy", begin()
  // with that numbering, and the plan onto the device -- the tiles with `order` if there are tiles, the swept numbers
  // with every number's key if a block is swept.
  int begin_blocked(std::vector<uint32_t>&& numbering, std::vector<uint32_t>&& element_number,
                    const std::vector<uint32_t>& key_of, size_t n, size_t totals_bytes = sizeof(ClusterTotals));
  // ... and the direct kernel's arguments over the plan's tiles (an entry whose kernel unites nothing or counts
  // elsewhere passes null).
  ClusterWithinArgs within_args(uint32_t min_permille, uint32_t* parent, ClusterTotals* totals) const;

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
  // The ending of the entries whose sweeps append edge keys through ClusterTotals::edges (cluster_edges.hip,
  // cluster_edges_extend.hip; one forest): the totals, the count into *n_edges in every mode, ERANGE against the
  // caller's capacity or EOVERFLOW against out.room, and for an emitting call the keys sorted (segsort.h, one segment),
  // turned into records and copied to edges[] -- only on success.
  int deliver_edges(const ClusterEdgesOut& out, blurrily_cluster_merge_t* edges, uint64_t capacity, uint64_t* n_edges);

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
  ClusterWithinPlan plan;                                    // after begin_blocked(); on the device, null where the
  ClusterWithinTile* d_tiles = nullptr;                      // plan has nothing for the kernel that would read it
  uint32_t *d_order = nullptr, *d_swept = nullptr, *d_block_of = nullptr;

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

// The cluster tree's rounds for the five tree entries: the rounds' buffers, and per round the
// entry's offer to best[], the merge, the flatten and four bytes read back, the merges so far.  A round that adds none
// was the last.
struct TreeRounds {
  // The buffers on top of c's (after its begin), the merge's and the flatten's arguments -- an error word goes to
  // *d_totals -- and the first flatten: every number its own component.
  int begin(ClusterCall& c, ClusterTotals* d_totals);

  // offer(round), from 1, enqueues whatever raises best[] this round from r.comp and r.closed (< 0: it failed).
  // EIO: kTreeMaxRounds ran out, or there are not fewer records than numbers, which no forest has.
  template <class Offer>
  int run(Offer&& offer) {
    bool done = false;
    for (uint32_t round = 1; round <= kTreeMaxRounds && !done; ++round) {
      uint32_t now = 0;
      if (offer(round) < 0 || merge_and_count(now) < 0) return -1;
      done = now == found;
      found = now;
    }
    if (!done || found >= r.n_nodes) { errno = EIO; return -1; }
    return 0;
  }

  // The ending: the `found` records on their way to the host (none: nothing is enqueued), and, after the entry's wait
  // for the stream, into merges[] in sort_tree_records' order.
  int read_records();
  void deliver(blurrily_cluster_merge_t* merges);

  ClusterTreeRoundArgs r{};
  uint32_t found = 0;                                        // the merges so far

 private:
  int merge_and_count(uint32_t& now);
  hipStream_t stream = nullptr;
  std::vector<ClusterTreeMerge> got;
};

// The core heights' bracket loop for the two core tree entries, after the settle of pass 0 and
// only with min_degree != 0: per pass the next width and pass number into `settle`, the entry's one pass over the edges
// -- pass(span, width, first) enqueues whatever adds every edge to hist[] (< 0: it failed) -- and the settle, which
// reads the counters that pass has finished.  max(1, ceil(log_kCoreBuckets(1001 - min_permille))) passes: the one that
// leaves brackets one height wide is the last.
template <class Pass>
int core_height_passes(ClusterCoreHeightSettleArgs& settle, hipStream_t stream, Pass&& pass) {
  for (uint32_t span = 1001u - settle.min_permille;; span = settle.width) {
    settle.width = (span + kCoreBuckets - 1u) / kCoreBuckets;
    settle.pass += 1;
    if (pass(span, settle.width, settle.pass == 1u) < 0) return -1;
    if (launch_cluster_core_height_settle(settle, stream) < 0) return -1;
    if (settle.width == 1) return 0;                          // the brackets are one height wide
  }
}

}  // namespace detail
}  // namespace blurrily
