// map_internal.h -- the map object behind the C ABI (include/blurrily_storage.h) and what its sources share: the
// error macro, the device scratch types, and the internal functions that cross translation units.  Everything
// declared in blurrily::detail has hidden visibility: none of it is a dynamic symbol of libblurrily_hip.so.
// The map, trigram_map_t, is three things besides its images and its mutation log: the sweep's settings (SweepSettings:
// what a replica takes over from the primary, in one assignment), the measured choice per class of batch (cls[8]:
// find_choice.h's ClassChoice; forget_choices) and the device resources of its finds, every one in an owner of
// hip_owned.h -- deleting a map gives them all back, and no function names them to free them.
//   c_abi.hip        lifecycle, put / delete / save / stats, find / find_batch entries, debug entries
//   options.hip      blurrily_storage_set_option / get_option: one row per option
//   map_log.hip      the mutation log: ensure_device, apply_tombstones, map_ready, map_images
//   find_run.hip     the batch search's launch logic: run_find_on (its decisions: find_choice.h), run_find (the timing
//                    events); stage_string_needles
//   multi_device.hip replicas, run_find_multi
//   host_batch.hip   host-buffer batches: needle_len, longest_needle, BatchBlocks; the chunked pipeline,
//                    find_batch_host, find_few (its page and lists: find_few_layout.h; its decisions: find_choice.h)
//   refs.hip         by reference: refs_extract, ExtractionOnHost, stage_reference_needles, get / find_references entries
//   scope.hip        scoped find, a scope per needle; behind scope_internal.h with scope_similar.hip and scope_above.hip,
//                    the scoped similarity and threshold finds
//   above.hip, similar.hip   the threshold and similarity finds (their shared sort: segsort.h)
//   cluster.hip      connected components of the similarity self-join (similar.hip's per-rank trigram table)
#pragma once
#include "../../include/blurrily_storage.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "device_index.h"
#include "find_choice.h"
#include "find_kernels.h"
#include "hip_owned.h"
#include "hip_try.h"
#include "host_index.h"
#include "similar.h"

struct trigram_map_t;

namespace blurrily {
namespace detail __attribute__((visibility("hidden"))) {

// A map's device image lives on the HIP device that was current when it was built.  Every entry
// point that touches the image runs inside a DeviceScope: the current device is switched to the
// map's and restored on the way out, so a caller (torch, another map) may leave any device current.
struct DeviceScope {
  int  prev = -1;
  bool changed = false;
  explicit DeviceScope(int want) {
    if (want >= 0 && hipGetDevice(&prev) == hipSuccess && prev != want) changed = hipSetDevice(want) == hipSuccess;
  }
  ~DeviceScope() { if (changed) (void)hipSetDevice(prev); }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// where note_launch() (find_kernels.h) writes: the `last_kernels` of the map whose batch is being enqueued on this thread
std::string*& launch_names();
struct NameScope {                                     // the launches inside it note their kernels' names in *s
  std::string* prev;
  explicit NameScope(std::string* s) : prev(launch_names()) { launch_names() = s; }
  ~NameScope() { launch_names() = prev; }
};

}  // namespace detail
}  // namespace blurrily

// Mutations since the base device image was built (DESIGN.md "Mutation and device sync").
struct PendingPut {
  std::string needle;
  uint32_t    weight;
};

// "devices" > 1: one more copy of the map's device side, on another visible device (or, with more replicas than
// devices, on one that already has one): clones of the primary's images, a map object of its own for the scratch
// buffers, events and measured choices its finds need, a stream, and staging for its shard of a batch.
struct __attribute__((visibility("hidden"))) Replica {
  int            device = -1;
  bool           same_device = false;   // it sits on the primary's own device (more replicas than devices)
  bool           peer_access = false;   // its device and the primary's reach each other's memory directly (both ways, enabled)
  trigram_map_t* side = nullptr;        // dev / delta / d_code_total_now are the clones; host == nullptr; mirror_of = the primary
  uint64_t       base_builds = 0, delta_image_version = 0, log_version = 0;   // the primary's, as of the clones
  blurrily::detail::Stream    stream;
  blurrily::detail::Events<1> ev_done;  // (timing disabled)
  blurrily::detail::Events<2> ev_t;     // around its shard's search, in timing mode
  blurrily::detail::DeviceBuffer d_in, d_out;   // [offsets | needles] of the batch, [rows | counts | nb_entries] of its shard
};

// The tunables of the batch sweeps that a replica's finds read as the primary's do (blurrily_storage_set_option;
// defaults from the measured gate): a replica takes them over in one assignment.
struct SweepSettings {
  blurrily::IndexBuildOptions build_opt;          // ws_enabled, ws_min_windows, ws_min_slice, dense_min
  uint32_t    ws_cmin = 3;              // a left-out slice must leave at least this many counted matches
  uint32_t    nm_cmin = 3;              // the same for the needle-major sweep (0: it leaves nothing out)
  uint32_t    nm_dense = 3072;          // ... which leaves out slices of at least this many postings only (4 096 through round 5;
                                        // round 6, same rows: configs[2] 120.8 -> 119.1 ms per 300 k needles, four times the haystack 135.1 -> 129.9)
  bool        small_sweep = true;       // images of at most kSmallMaxWindows windows: find_small_kernel serves large batches at limits up to 64
  uint32_t    small_min_needles = 4096; // ... from this many needles on (below: two chains per CU are not the limit)
  uint32_t    nm_min_windows = 256;     // ... and, where the choice is not measured, on images of at least this many windows
  uint32_t    ws_min_needles = 16384;   // smaller batches: needle-major
  bool        ws_autotune = true;       // measure the choice per class of batch on first use (run_find_on)
  uint32_t    ws_static_slice = 2200;   // the static rule's mean_hit_slice (autotune off): break-even of the skewed family
};

struct trigram_map_t {
  blurrily::HostIndex*  host = nullptr;
  const trigram_map_t* mirror_of = nullptr;   // a replica's side map: the mutation log that counts is this map's
  std::vector<Replica> replicas;        // "devices" - 1 of them
  uint32_t    n_devices = 1;            // option "devices": shards of a large batch (the primary's included)
  blurrily::detail::Events<1> ev_ready; // multi-device batches: the caller's needles are in place (timing disabled)
  blurrily::detail::Events<2> ev_t;     // ... and around the primary's shard, in timing mode
  blurrily::DeviceIndex dev;                      // base image
  // log of puts/deletes the base image does not contain yet
  std::unordered_map<uint32_t, PendingPut> pending;   // by reference
  size_t      n_tomb = 0;               // base references deleted since the build
  std::vector<uint32_t> tomb_queue;     // their ranks, not yet on the device (applied by the next find, on its stream)
  blurrily::detail::DeviceBuffer ws_tomb;
  uint64_t    log_version = 0;          // bumped by every logged mutation
  uint64_t    delta_version = 0;        // log_version the delta image / code totals were built from
  uint64_t    delta_puts_version = 0;   // bumped when the set of pending puts changes (the delta image's content)
  uint64_t    delta_image_version = 0;  // delta_puts_version the delta image was built from
  bool        log_overflow = false;     // the log outgrew its budget: the next find rebuilds the base
  uint64_t    base_builds = 0;
  blurrily::HostIndex*  delta_host = nullptr;
  blurrily::DeviceIndex delta;                    // image of `pending` only
  blurrily::detail::DeviceMem<uint32_t> d_code_total_now;   // [kNumCodes] bucket sizes of the whole map (base run's nb_entries)
  blurrily::detail::DeviceBuffer ws_base_rows, ws_base_counts, ws_delta_rows, ws_delta_counts;
  SweepSettings sweep;
  // the sweep that serves each class of batch, measured by the class's first batch and WATCHED afterwards: one that ran
  // over 10 % slower per needle than what the measurement saw has the class measured again -- at most once in sixteen
  // batches (find_choice.h: ClassChoice, watch_verdict)
  blurrily::detail::ClassChoice cls[8];
  blurrily::detail::Events<2>   watch_ev[8];      // a class's watched batch: around the chosen sweep
  blurrily::detail::Events<7>   tune_ev;          // a measurement: between its runs
  int         last_tuned = -1;          // the class measured most recently ("tuned_*_us" report its figures)
  int         last_sweep = 0;           // which sweep the last large batch of short needles took (1 / 2 / 3; 0: none yet)
  uint32_t latency_tasks = 0;           // option "latency_tasks": tasks latency mode aims at per resident workgroup (0: latency_ranges' rule)
  std::string last_kernels;             // the find kernels the last batch on the base image launched, '+'-joined (blurrily_storage_last_kernels)
  size_t      class_hint = 0;           // a chunked host batch: the WHOLE batch's size decides the class, not the chunk's
  uint64_t    retunes = 0;              // classes measured again because a batch ran slow (option "retunes", read-only)
  int         tune_inject = 0;          // (tests) the next measurement sees this sweep at HALF its time: a bad sample to recover from
  int         n_cus = 0;
  bool        timing = false;
  bool        collect_stats = false;    // request counters of the find kernels (FindArgs::stats)
  blurrily::detail::DeviceMem<unsigned long long> d_stats;   // [kStatAllSlots], zeroed by every run_find while collecting
  blurrily::detail::DeviceMem<unsigned long long> d_phase;   // [kPhaseWorkgroups][16] phase clocks of the counted build's last launch
  blurrily::detail::DeviceBuffer ws_flags;                   // [n] path flags of the last find while collecting (FindArgs::path_flags)
  size_t      n_flags = 0;
  double      last_find_ms = 0.0, last_tok_ms = 0.0;
  blurrily::detail::Events<4> ev;       // timing mode: around the front end and around the find
  blurrily::detail::DeviceBuffer ws_codes, ws_small, ws_parts, ws_io_in, ws_io_out;
  blurrily::detail::DeviceBuffer ws_refs;                 // by reference: the extraction's arrays and the references' codes (refs_extract)
  // scoped find: options "scope_strategy" (0 auto, 1 mask, 2 direct) and "scope_direct_max" (the
  // scope's member codes up to which auto scores the members directly; 0: auto always takes the mask), and a pinned
  // page the device maps, for small host batches the direct strategy serves without copies.  The default sits just
  // above the largest scope measured where direct wins both batches and single finds (configs[2], 10^4 members, 140 544
  // codes: 21x the mask's needles/s, 82 against 124 us a find; at 416 379 codes it still wins batches 4.5x but single
  // finds take 193 against 122 us -- profiles/scope_geonames.json)
  uint32_t    scope_strategy = 0;
  uint64_t    scope_direct_max = 150000;
  // cluster edges: option "cluster_edges_max", the records one call may emit -- the bound on its
  // device scratch, 28 bytes a record (two rows of 8-byte keys for the sort, the 12-byte records): 7 GiB at the default
  uint64_t    cluster_edges_max = uint64_t(1) << 28;
  blurrily::detail::HostPage h_scope;   // [kScopePageBytes in | kScopePageBytes out]
  unsigned char* d_scope = nullptr;     // the same memory as the device addresses it
  // a scope per needle: the call's plan on the device (scope table, workgroup order, the groups'
  // needles, their rows) and on the host (what is uploaded; kept until the next such call)
  blurrily::detail::DeviceBuffer ws_each, ws_each_rows;
  std::vector<unsigned char> h_each;
  blurrily::detail::HostPage h_stage;   // pinned host staging: [kStageBytes in | kStageBytes out]
  // the single find's own launch (find_one): a stream, host-coherent pinned memory the kernel writes rows, count and a
  // sequence word into, the per-workgroup lists and the ticket on the device
  struct __attribute__((visibility("hidden"))) One {
    blurrily::detail::Stream   stream;
    blurrily::detail::HostPage h_out;   // per image: a page as find_few_layout.h lays it out (FewPage)
    unsigned char* d_out = nullptr;     // the same memory as the device addresses it
    blurrily::detail::DeviceBuffer   d_parts;             // per image: the lists as find_few_layout.h lays them out (FewLists)
    uint32_t       seq = 0;
    bool           enabled = true;      // option "one_launch"
    uint32_t       min_per = 0;         // option "one_windows_per_wg": at least this many windows per workgroup (0: as few as the grid allows)
    uint32_t       mid_workgroups = 1024;   // option "mid_workgroups": workgroups a launch of more than kOneMaxNeedles needles aims at
    uint32_t       few_max = 24;        // option "few_max": host-buffer batches of up to this many needles share find_one_kernel's launch
                                        // (up to kMidMaxNeedles; from about thirty needles on latency mode's ranges are faster: DESIGN.md)
    uint32_t       mid_max = blurrily::kMidMaxNeedles;   // option "mid_max": ... and up to this many take latency mode WITHOUT copies: tokenised on the
                                        // host, read from the pinned page, the merged rows written back into it (find_few)
    uint64_t       taken = 0;           // finds served this way (option "one_taken", read-only)
  } one;
  // large host-buffer batches go in chunks through a three-stream pipeline (find_batch_chunked)
  uint32_t    host_chunk = 131072;      // needles per chunk (option "host_chunk"; 0: never chunk)
  struct __attribute__((visibility("hidden"))) Pipe {
    blurrily::detail::Stream    s_in, s_run, s_out;
    blurrily::detail::Events<2> ev_in, ev_run, ev_out;   // (timing disabled) one per slot
    blurrily::detail::HostPage  h_in[2], h_out[2];       // pinned
    size_t h_in_bytes = 0, h_out_bytes = 0;
    blurrily::detail::DeviceBuffer d_in[2], d_out[2];
  } pipe;
};

namespace blurrily {
namespace detail __attribute__((visibility("hidden"))) {

constexpr size_t kPhaseWorkgroups = 8192, kPhaseWords = kPhaseWorkgroups * 16, kPhaseBytes = kPhaseWords * 8;
// The measured choices are forgotten -- every class is measured again by its next batch -- when an option that bears
// on them is set, when the base image is rebuilt, when a replica's image is cloned again.  What the watch holds
// (the figures, the strikes, the hold-off) stays.
inline void forget_choices(trigram_map_t* m) { for (ClassChoice& c : m->cls) c.choice = 0; }
constexpr uint64_t kMaxBatchNeedles = 0xFFFFFFF0ull;   // needles (or references) a call takes: the kernels count them in 32 bits

// ---- map_log.hip ------------------------------------------------------------------------------------------------------
size_t log_budget(const trigram_map m);
const trigram_map_t* log_of(const trigram_map_t* m);
bool log_empty(const trigram_map_t* m);
int  ensure_device(trigram_map m);
void log_put(trigram_map m, const char* needle, size_t len, uint32_t ref, uint32_t weight);
int  log_delete(trigram_map m, uint32_t ref);
int  apply_tombstones(trigram_map m, hipStream_t stream);
// what an entry does first: the map's pending work, then the device image (ENODEV without a usable GPU), the tombstones
int  map_ready(trigram_map m, hipStream_t stream);

// ---- find_run.hip (latency_ranges and the other decisions of run_find_on: find_choice.h) -------------------------------
// (sm: a scoped find's masks, in the tombstone bitmap's place: they exclude the deleted ranks too)
struct ScopeMasks { const uint32_t* base; const uint32_t* delta; };
int run_find(trigram_map m, const char* d_packed, size_t packed_bytes, const uint64_t* d_offsets, size_t n,
             uint16_t limit, trigram_match d_results, uint32_t* d_counts, uint32_t* d_nb, bool maybe_long,
             bool maybe_mid, hipStream_t stream, const RefNeedles* rn = nullptr, const ScopeMasks* sm = nullptr);

// ---- multi_device.hip -------------------------------------------------------------------------------------------------
void free_replica(Replica& r);
int  run_find_multi(trigram_map m, const char* d_packed, size_t packed_bytes, const uint64_t* d_offsets, size_t n,
                    uint16_t limit, trigram_match d_results, uint32_t* d_counts, uint32_t* d_nb, hipStream_t stream);
bool wants_multi(const trigram_map_t* m, size_t n);

// ---- host_batch.hip ---------------------------------------------------------------------------------------------------
constexpr int kOneNotTaken = -2;   // find_few: the finds have to go the batch's way
int find_few(trigram_map m, const char* const* s, const size_t* len, size_t n, uint16_t limit, trigram_match results,
             uint32_t* counts);
int find_batch_host(trigram_map m, const char* packed, const uint64_t* offsets, size_t n, uint16_t limit,
                    trigram_match results, uint32_t* counts, bool raw, uint32_t* non_ascii);
// A needle's length: up to its first NUL among its `cap` bytes (where the tokeniser stops).
size_t needle_len(const char* s, size_t cap);
// The longest of n packed needles, as far as the launches need to know it (> 63, > 126): the scan stops beyond 126.
size_t longest_needle(const char* packed, const uint64_t* offsets, size_t n);

// The two blocks a host-buffer batch of n needles travels in: [offsets | needles] in, [counts | (flags) | rows] out
// (flags: a raw batch's non-ASCII flags, a by-reference batch's trigram counts).  The layout is the same whatever backs
// the blocks: device scratch with pageable copies (copy_in / copy_out), or pinned or mapped host memory the caller
// copies in one piece or not at all (fill_in / take_out).  A by-reference batch, whose references go in alone, uses the
// out block only.
struct BatchBlocks {
  struct In  { const uint64_t* offsets; char* packed; };
  struct Out { uint32_t* counts; uint32_t* flags; trigram_match rows; };
  size_t off_bytes, packed_bytes, cnt_bytes, row_bytes;
  size_t o_packed, in_bytes, o_flags, o_rows, out_bytes;
  BatchBlocks(size_t n, size_t packed_bytes, uint16_t limit, bool flags);
  In  in(unsigned char* base) const;
  Out out(unsigned char* base) const;
  void fill_in(unsigned char* h_in, const char* packed, const uint64_t* offsets) const;
  int  copy_in(unsigned char* d_in, const char* packed, const uint64_t* offsets, hipStream_t stream) const;
  // counts, the flags (where the caller wants them) and the rows to the caller; copy_out synchronises the stream
  // (d_flags: the block's, or a by-reference call's trigram counts where the extraction left them)
  void take_out(const Out& h, uint32_t* counts, uint32_t* flags, trigram_match results) const;
  int  copy_out(const uint32_t* d_counts, const uint32_t* d_flags, const trigram_match_t* d_rows, uint32_t* counts,
                uint32_t* flags, trigram_match results, hipStream_t stream) const;
};

// The needles of a call as the threshold and similarity sweeps read them (the front ends' layout: tokenise_kernel,
// refs_extract): needle q's ntri[q] distinct codes at codes + qoff[q] + q.
struct NeedleView {
  const uint16_t* codes;
  const uint64_t* qoff;
  const uint32_t* ntri;
};

// The images a call searches and the deleted ranks of each: the base image, and the delta image of pending puts.
struct MapImages {
  uint32_t        n;
  DeviceIndex*    img[2];
  const uint32_t* tomb[2];
};
MapImages map_images(trigram_map m);                                                             // map_log.hip
// What every find launch reads of the image it searches.
inline void image_args(const DeviceIndex& ix, FindArgs* a) {
  a->slice_se = ix.d_slice_se; a->ent = ix.d_ent; a->ref_of_rank = ix.d_ref_of_rank;
  a->weight_of_rank = ix.d_weight_of_rank; a->n_refs = ix.n_refs; a->n_windows = ix.n_windows;
  a->win_max_tri = ix.d_win_max_tri; a->nib_windows = ix.nib_windows; a->dense_min8 = ix.dense_min8;
}
// Windows per workgroup of a sweep over nc needles: a small batch spreads each needle's windows over the GPU, a large
// one gives a needle one workgroup (at_least: a floor of the caller's).
inline uint32_t windows_per_workgroup(const trigram_map_t* m, const DeviceIndex& ix, size_t nc, uint64_t at_least = 1) {
  const uint64_t want = uint64_t(std::max(m->n_cus, 1)) * 8u;
  const uint64_t per = std::max<uint64_t>(std::max<uint64_t>(uint64_t(ix.n_windows) * nc / want, 1), at_least);
  return uint32_t(std::min<uint64_t>(per, std::max<uint32_t>(ix.n_windows, 1)));
}
// n host strings up and tokenised by the string path's own front end (find_run.hip); buf: the call's scratch for them
int stage_string_needles(trigram_map m, const char* packed, const uint64_t* offsets, size_t n, DeviceBuffer& buf,
                         hipStream_t stream, NeedleView* out);
// n host references up and extracted by the by-reference front end (refs.hip); nb_trigrams (may be null): copied back
int stage_reference_needles(trigram_map m, const uint32_t* references, size_t n, DeviceBuffer& buf, hipStream_t stream,
                            uint32_t* nb_trigrams, NeedleView* out);

// ---- refs.hip ---------------------------------------------------------------------------------------------------------
// The trigrams of n device-resident references, extracted on `stream` from the map as it is now: the base image minus its
// deleted ranks, the delta image of pending puts (kernels/refs.inc).  Each image uploads its reference table at its first
// such call.  *out describes the needles for run_find, and where the count of distinct references found and of the codes
// extracted for them sit on the device.
struct RefExtract {
  RefNeedles needles;
  const uint64_t* win_base_total;   // [1] distinct references found
  const uint64_t* slot_start;       // [n + 1]: slot_start[*win_base_total] codes in all
  const uint2*    loc;              // [n] where each reference was found (RefArgs::loc)
  uint32_t        win0_delta;       // the delta image's first window in loc's numbering (with_delta)
  bool            with_delta;
};
int refs_extract(trigram_map m, const uint32_t* d_refs, size_t n, hipStream_t stream, RefExtract* out);

// An extraction read back to the host, in the steps its readers need: the counts and weights (enqueued: the caller
// may have more to enqueue before it waits), where each reference's codes sit and how many there are in all (waits
// for the stream), the codes themselves.
struct ExtractionOnHost {
  RefExtract x;
  size_t n;
  std::vector<uint32_t> ntri, weight;
  std::vector<uint64_t> qoff;                            // (sized by read_offsets: a scope of every reference never reads them)
  std::vector<uint16_t> all;                             // every distinct reference's codes once, behind the pad of n
  uint64_t total = 0;
  bool have_offsets = false, have_codes = false;
  explicit ExtractionOnHost(size_t n_refs) : n(n_refs), ntri(n), weight(n) {}
  int enqueue_counts(const RefExtract& from, hipStream_t stream);
  int read_offsets(hipStream_t stream);
  int read_codes(hipStream_t stream);                    // (the offsets first, unless they are here already)
  // (on the device reference i's codes sit at codes + qoff[i] + i, as a needle's do; `all` starts behind the pad)
  const uint16_t* codes_of(size_t i) const { return all.data() + (qoff[i] + i - n); }
};

// ---- above.hip -------------------------------------------------------------------------------------------------------
constexpr size_t   kAboveChunkNeedles = size_t(1) << 20;   // needles per sweep launch
constexpr uint64_t kAboveChunkRows    = uint64_t(1) << 24; // rows per emit chunk (keys, sorted keys, rows: 28 B each)
// The needles [s, e) of one emit chunk: as many as the bounds allow, one at least.  row_off: the call's n + 1 offsets.
inline size_t above_chunk_end(const uint64_t* row_off, size_t n, size_t s) {
  size_t e = s + 1;
  while (e < n && e - s < kAboveChunkNeedles && row_off[e + 1] - row_off[s] <= kAboveChunkRows) ++e;
  return e;
}
// Offsets that add up each of n needles' (or jobs') rows: off[0 .. n].
template <class Rows> void rows_to_offsets(size_t n, Rows rows, uint64_t* off) {
  off[0] = 0;
  for (size_t q = 0; q < n; ++q) off[q + 1] = off[q] + rows(q);
}
// Between a threshold call's two steps: row_off from each needle's counted rows, then whether it emits: 1, or 0 (no
// results wanted: the counts were the call) or -1 (ERANGE: they do not fit the capacity; row_off stays laid out).
template <class Rows> int above_row_off(size_t n, Rows rows, const void* results, uint64_t capacity, uint64_t* row_off) {
  rows_to_offsets(n, rows, row_off);
  if (!results) return 0;
  if (capacity < row_off[n]) { errno = ERANGE; return -1; }
  return 1;
}
// device scratch of one threshold call, freed on the way out (b[8], b[9]: the scoped calls' own)
struct AboveScratch { DeviceBuffer b[10]; };
// What the count step found, kept for the emit step: per image and needle, on the device and on the host.
struct AboveCounted {
  DeviceBuffer          d_counts;      // [n_img * n]
  std::vector<uint32_t> cnt;           // the same, read back
  size_t                n = 0;
  uint32_t              n_img = 0;
  uint64_t rows(size_t q) const { return uint64_t(cnt[q]) + (n_img > 1 ? cnt[n + q] : 0u); }
};
// The threshold find in its two steps.  above_count: the rows of each of n needles over the map as it is now (waits for
// the stream).  above_emit: their rows to host memory, needle q's at results + row_off[q] (row_off: n + 1 offsets that
// add up C.rows), in chunks of needles bounded by kAboveChunkNeedles and kAboveChunkRows.  The same needles, bar and
// masks go to both.  sm: a scoped call's masks, in the tombstone bitmaps' place.
int above_count(trigram_map m, size_t n, const NeedleView& N, uint32_t min_matches, uint32_t min_permille,
                hipStream_t stream, const ScopeMasks* sm, AboveCounted* C);
int above_emit(trigram_map m, const NeedleView& N, uint32_t min_matches, uint32_t min_permille, const AboveCounted& C,
               const uint64_t* row_off, trigram_match results, hipStream_t stream, AboveScratch& S,
               const ScopeMasks* sm);

// ---- similar.hip ------------------------------------------------------------------------------------------------------
// An image's per-rank trigram counts (similar.h: SimilarTable), built at the first call that needs them and kept in a
// registry beside the image.  A call's tables: those it found kept, and those it built and keeps -- or, where the
// runtime gives no usable buffer ids, frees on the way out.
struct SimilarTableEntry {
  const DeviceIndex* ix;
  const void*        ent;
  unsigned long long ent_id;
  int                device;
  SimilarTable       t;
  size_t             bytes;
};
struct SimilarTables {
  std::vector<SimilarTableEntry> own;
  ~SimilarTables();
};
int similar_table(DeviceIndex* ix, hipStream_t stream, SimilarTables& call, SimilarTable* out);
// device scratch of one similarity call, freed on the way out (b[8], b[9]: the scoped calls' own)
struct SimilarScratch { DeviceBuffer b[10]; };
// The top-`limit` rows of n needles over the map as it is now, to host memory: results / row_ntri [n * limit],
// counts [n].  sm: a scoped call's masks, in the tombstone bitmaps' place.
int similar_run(trigram_map m, size_t n, const NeedleView& N, uint32_t limit, uint32_t min_permille,
                trigram_match results, uint32_t* counts, uint32_t* row_ntri, hipStream_t stream, SimilarScratch& S,
                const ScopeMasks* sm = nullptr);

}  // namespace detail
}  // namespace blurrily
