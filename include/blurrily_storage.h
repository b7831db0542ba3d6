/*
 * blurrily_storage.h -- C ABI of libblurrily_hip.so, the MI355X-native drop-in
 * for the trigram index behind Blurrily::Map (mezis/blurrily v1.0.2).
 *
 * Part 1 declares the nine entry points of the reference's
 * ext/blurrily/storage.h:36-117 with the same names, argument meaning and
 * error behaviour, so the reference's own Ruby glue (ext/blurrily/map_ext.c)
 * links against this library unchanged.  Part 2 adds the
 * batched / device-resident entry points the reference has no counterpart for;
 * each batched element is defined as exactly one blurrily_storage_find.
 *
 * `find` runs on the GPU (hand-written HIP kernels for gfx950).  There is no
 * CPU fallback: without a usable device every find entry point returns -1 with
 * errno = ENODEV and says so on stderr.
 */
#ifndef BLURRILY_AMD_STORAGE_H
#define BLURRILY_AMD_STORAGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- types ---- */

/* When the reference's own ext/blurrily/storage.h has been included first (a translation unit of the gem's
 * glue, ruby/ext/blurrily/map_ext_batch.c), its types are the types: this header then only RE-DECLARES the nine
 * functions -- which the compiler checks for compatibility, tests/test_header_compat.py -- and adds part 2. */
#ifndef __STORAGE_H__

struct trigram_map_t;                               /* opaque; storage.h:15-16 */
typedef struct trigram_map_t* trigram_map;

/* storage.h:18-24 -- packed 12-byte result row. */
struct __attribute__((__packed__)) trigram_match_t {
  uint32_t reference;
  uint32_t matches;
  uint32_t weight;
};
typedef struct trigram_match_t  trigram_match_t;
typedef struct trigram_match_t* trigram_match;

/* storage.h:26-30 */
typedef struct trigram_stat_t {
  uint32_t references;
  uint32_t trigrams;
} trigram_stat_t;

#endif /* __STORAGE_H__ */

/* ------------------------------------------------- part 1: reference ABI ---- */

/* storage.h:36 / storage.c:178-206.  New empty map.  0 on success, <0 + errno. */
int blurrily_storage_new(trigram_map* haystack);

/* storage.h:41 / storage.c:210-266.  Load a `.trigrams` file written by this
 * library or by the reference (same bytes).  <0 + errno on failure: ENOENT
 * etc. from open(2); EPROTO for a short file, bad magic, wrong endianness or
 * pointer size (storage.c:226-230,245-250) and for out-of-bounds bucket
 * descriptors. */
int blurrily_storage_load(trigram_map* haystack, const char* path);

/* storage.h:46 / storage.c:270-295.  Release host and device memory; sets
 * *haystack = NULL. */
int blurrily_storage_close(trigram_map* haystack);

/* storage.h:51 / storage.c:625-629.  GC mark hook of the Ruby glue.  The ref
 * set here is native (no Ruby objects) so this is a no-op. */
void blurrily_storage_mark(trigram_map haystack);

/* storage.h:58 / storage.c:299-377.  Write the map to `path` atomically
 * (temp file + rename), byte-identical to what the reference writes for the
 * same sequence of operations. */
int blurrily_storage_save(trigram_map haystack, const char* path);

/* storage.h:70 / storage.c:398-473.  Returns the number of trigrams added,
 * 0 if `reference` is already present.  weight == 0 -> strlen(needle).
 * Out of memory: -1 with errno ENOMEM and no entry added (the reference
 * asserts in smalloc, storage.c:93-98; a bucket grown before the failing
 * allocation keeps its new capacity, which a later save writes out). */
int blurrily_storage_put(trigram_map haystack, const char* needle,
                         uint32_t reference, uint32_t weight);

/* storage.h:96 / storage.c:584-612.  Returns the number of entries removed. */
int blurrily_storage_delete(trigram_map haystack, uint32_t reference);

/* storage.h:110 / storage.c:477-580.  At most `limit` rows into the
 * caller-allocated `results`, ordered by matches descending, weight ascending,
 * reference ascending.  Returns the row count, or -1 (errno ENODEV) when no
 * GPU is usable.  ONE kernel launch and no copy for a needle of at most 64
 * distinct trigrams at a limit of 1..120 (option "one_launch"; a second launch
 * over the delta image while puts are pending); otherwise one element of
 * blurrily_storage_find_batch -- which takes the same launch for up to "few_max"
 * (24; the kernel: up to 128) such needles, a row of the grid each, and still no
 * copy for up to "mid_max" (128). */
int blurrily_storage_find(trigram_map haystack, const char* needle,
                          uint16_t limit, trigram_match results);

/* storage.h:117 / storage.c:616-621. */
int blurrily_storage_stats(trigram_map haystack, trigram_stat_t* stats);

/* ------------------------------------------- part 2: batched extensions ---- */

/* Same as `n` calls of blurrily_storage_put, in order (no reference
 * counterpart; avoids one FFI crossing per string for bulk imports).
 * Needle i is the bytes packed[offsets[i] .. offsets[i+1]) cut at the first
 * NUL.  weights may be NULL (all 0).  Returns the total number of trigrams
 * added, or -1. */
long blurrily_storage_put_many(trigram_map haystack, const char* packed,
                               const uint64_t* offsets, const uint32_t* references,
                               const uint32_t* weights, size_t n);

/* n independent finds on the GPU in one launch sequence.  Host buffers in,
 * host buffers out.  results holds n*limit rows (query i owns rows
 * [i*limit, i*limit+counts[i])); counts holds n row counts.  Returns 0, or -1
 * with errno (ENODEV: no GPU). */
int blurrily_storage_find_batch(trigram_map haystack, const char* packed,
                                const uint64_t* offsets, size_t n, uint16_t limit,
                                trigram_match results, uint32_t* counts);

/* Device-resident variant: every pointer is a device pointer on the map's GPU;
 * work is enqueued on `stream` (a hipStream_t; NULL = default stream) and the
 * call returns without waiting for it -- with these exceptions, each of which
 * blocks the calling thread until the work enqueued so far on `stream` is done:
 *   - the first call after a mutation builds / refreshes the device image
 *     (as blurrily_storage_sync_device would; call that first to keep it out);
 *   - the first call after a blurrily_storage_delete uploads the deleted ranks and
 *     sets their tombstone bits (a synchronous copy and a stream synchronise);
 *   - with "ws_autotune" 1 (the default), the FIRST batch of a class -- limit up
 *     to / above 32 x 129.. / 16 384.. / 65 536.. / 262 144.. needles -- on an image runs
 *     every sweep that can serve it and waits for them once, to note the fastest
 *     (blurrily_storage_tune does that ahead of time; "ws_autotune" 0 never does);
 *   - blurrily_storage_set_timing(1) and blurrily_storage_set_stats(1).
 * With "devices" > 1 the batch is sharded over the replicas; `stream` then waits
 * (on the device, not the host) for every replica's rows.
 * d_nb_entries (optional, may be NULL) receives per query the reference's
 * nb_entries (storage.c:498-502), the unit of the matched-entries/s metric. */
int blurrily_storage_find_batch_device(trigram_map haystack, const char* d_packed,
                                       size_t packed_bytes, /* == offsets[n] */
                                       const uint64_t* d_offsets, size_t n, uint16_t limit,
                                       trigram_match d_results, uint32_t* d_counts,
                                       uint32_t* d_nb_entries, void* stream);

/* Needle normalisation on the device -- Blurrily::Map#normalize_string
 * (lib/blurrily/map.rb:40-47) for ASCII needles: A-Z -> a-z, every other byte
 * that is not a-z -> ' ', runs of spaces squeezed, ends stripped.  The result is
 * written to `d_out` at the needle's own offset (never longer than the input;
 * NUL-terminated when shorter), so `d_out` may be `d_packed` and the buffer goes
 * straight into blurrily_storage_find_batch_device.  d_non_ascii[i] (optional)
 * is set to 1 for a needle holding a byte >= 0x80: its NFKD decomposition is host
 * work (the reference uses ActiveSupport's tables) and the caller must normalise
 * that needle itself.  Asynchronous on `stream`.  0, or -1 with errno. */
int blurrily_normalize_batch_device(const char* d_packed, const uint64_t* d_offsets, size_t n,
                                    char* d_out, uint32_t* d_non_ascii, void* stream);

/* blurrily_storage_find_batch over un-normalised ASCII needles: normalised on the
 * device, then found (a handful -- up to "few_max" / "mid_max" -- by the library on the host, byte
 * for byte the same, so that they share the single find's launch or its pinned page).  non_ascii (optional,
 * n slots) as above; rows of a flagged needle are those of its bytes >= 0x80 read as
 * non-letters. */
int blurrily_storage_find_batch_raw(trigram_map haystack, const char* packed, const uint64_t* offsets,
                                    size_t n, uint16_t limit, trigram_match results, uint32_t* counts,
                                    uint32_t* non_ascii);

/* Build / refresh the device-resident index now (it is otherwise built lazily
 * by the first find after a mutation).  0, or -1 with errno. */
int blurrily_storage_sync_device(trigram_map haystack);

/* Measure NOW which sweep serves batches of `n` needles at `limit` on this map's
 * image (what the first such batch would otherwise do inside its find call): runs
 * `n` needles sampled from the host-side needles given -- packed / offsets as for
 * blurrily_storage_find_batch, at least one needle, repeated as needed -- through
 * every sweep the class can take and notes the fastest.  Synchronous.  After it,
 * blurrily_storage_find_batch_device on that class never waits for a measurement.
 * 0, or -1 with errno. */
int blurrily_storage_tune(trigram_map haystack, const char* packed, const uint64_t* offsets,
                          size_t n_given, size_t n, uint16_t limit);

/* By reference.  A map stores trigrams, not strings; these read a stored reference's trigrams back out of the
 * device image (a reference is a rank, its trigrams the (window, code) slices holding it) and find with them.
 * All four see the map as it is now: pending puts are served from the delta image, deleted references are not
 * found, a reference deleted and put again has its new string's trigrams.  Every string has at least one trigram,
 * so a reference the map holds always has some.  Without a usable GPU they return -1 with errno ENODEV (no CPU
 * fallback, as for find).  With "devices" > 1 the primary device alone serves them; the rows are the same. */

/* storage.h:72-87 of the reference, where it stayed commented out (there it would read the whole map).  Returns
 * < 0 on error, 0 if the map does not hold `reference`, else the number of its distinct trigrams.  If the
 * reference is found and `weight` is not NULL, *weight = the weight it was put with (strlen for weight 0).  Up
 * to `nb_trigrams` of its codes are copied into `trigrams` (when not NULL), ascending: exactly what
 * blurrily_tokeniser_parse_string returns for the string it was put with. */
int blurrily_storage_get(trigram_map haystack, uint32_t reference, uint32_t* weight,
                         int nb_trigrams, uint16_t* trigrams);

/* n calls of blurrily_storage_get in one.  Writes a CSR: reference i's codes are
 * codes[code_offsets[i] .. code_offsets[i+1]) (n + 1 offsets), an empty range meaning "not in the map";
 * weights (optional, n slots) as get's, 0 for a reference not found.  0, or -1 with errno; ERANGE when
 * codes_cap is too small, code_offsets then filled and code_offsets[n] the capacity needed. */
int blurrily_storage_get_batch(trigram_map haystack, const uint32_t* references, size_t n,
                               uint32_t* weights, uint64_t* code_offsets,
                               uint16_t* codes, size_t codes_cap);

/* Find what is like stored references, in one batch.  Element i is exactly
 * blurrily_storage_find(haystack, S_i, limit, ...) for any string S_i whose tokenisation is reference i's trigram
 * set (the normalised string it was put with): the reference itself is one of its rows, normally the first --
 * not filtered out.  A reference the map does not hold gets 0 rows.  results / counts as for
 * blurrily_storage_find_batch; nb_trigrams (optional, n slots) receives each reference's number of distinct
 * trigrams (0: not in the map).  The trigrams are read out of the image once and both the base and the delta
 * image are searched with them.  0, or -1 with errno. */
int blurrily_storage_find_references(trigram_map haystack, const uint32_t* references, size_t n,
                                     uint16_t limit, trigram_match results, uint32_t* counts,
                                     uint32_t* nb_trigrams);

/* Device-resident variant, under the rules of blurrily_storage_find_batch_device: device pointers on the map's
 * GPU, enqueued on `stream` (NULL = default stream), the same exceptions that block; in addition the first
 * by-reference call on a device image uploads its reference table (synchronous copies).  d_nb_trigrams may be
 * NULL. */
int blurrily_storage_find_references_device(trigram_map haystack, const uint32_t* d_references, size_t n,
                                            uint16_t limit, trigram_match d_results, uint32_t* d_counts,
                                            uint32_t* d_nb_trigrams, void* stream);

/* Scoped find.  A scope is a set of references, fixed when it is made; a scoped find of needle s at `limit`
 * returns exactly what blurrily_storage_find(s) at an unbounded limit would, with every row whose reference is
 * not in the scope removed, truncated to `limit` (the same order and rows).  Membership is read against the map
 * as it is at each find: a deleted member is not found, a member put after the scope was made is, a member
 * deleted and put again is found with its new string's trigrams; references the map never held are ignored,
 * duplicates count once.  A scope belongs to the map it was made from (EINVAL with any other).  Making a scope
 * and counting its members need no GPU; a scoped find without a usable GPU returns -1 with errno ENODEV.  With
 * "devices" > 1 the primary device alone serves a scoped find.  0, or -1 with errno. */
typedef struct blurrily_scope_t* blurrily_scope;

/* A scope of the n references (host memory; sorted and de-duplicated, nothing reaches the device yet). */
int blurrily_scope_new(trigram_map haystack, const uint32_t* references, size_t n, blurrily_scope* scope);

/* Frees the scope and NULLs *scope (a NULL *scope is a no-op).  Close scopes before their map. */
int blurrily_scope_close(blurrily_scope* scope);

/* *held = the scope's members the map holds now (host side, no GPU). */
int blurrily_scope_members(blurrily_scope scope, uint32_t* held);

/* blurrily_storage_find within the scope: the number of rows, or -1 with errno. */
int blurrily_storage_find_in(trigram_map haystack, blurrily_scope scope, const char* needle, uint16_t limit,
                             trigram_match results);

/* blurrily_storage_find_batch within the scope. */
int blurrily_storage_find_batch_in(trigram_map haystack, blurrily_scope scope, const char* packed,
                                   const uint64_t* offsets, size_t n, uint16_t limit, trigram_match results,
                                   uint32_t* counts);

/* blurrily_storage_find_batch_device within the scope, under the same rules (device pointers on the map's GPU,
 * enqueued on `stream`); the first scoped find after the map changed prepares the scope's device state
 * (synchronous copies). */
int blurrily_storage_find_batch_in_device(trigram_map haystack, blurrily_scope scope, const char* d_packed,
                                          size_t packed_bytes, const uint64_t* d_offsets, size_t n,
                                          uint16_t limit, trigram_match d_results, uint32_t* d_counts,
                                          void* stream);

/* A scope per needle.  Needle i of a batch is a scoped find in scopes[which[i]] (the array may repeat a handle), or
 * a plain blurrily_storage_find when which[i] == BLURRILY_NO_SCOPE: element i is exactly what
 * blurrily_storage_find_in(haystack, scopes[which[i]], needle_i, limit) -- or blurrily_storage_find -- would return,
 * under the same membership rules.  EINVAL, before anything needs a GPU: which[i] >= n_scopes (other than the
 * sentinel), a NULL handle or a scope of another map, n_scopes > 0 with scopes NULL.  Valid arguments without a
 * usable GPU: ENODEV.  With "devices" > 1 the primary device alone serves the call.  Every scope a call names that
 * the map has changed under is prepared again, all of them together.  0, or -1 with errno. */
#define BLURRILY_NO_SCOPE 0xFFFFFFFFu

/* blurrily_storage_find_batch with a scope per needle: rows of needle i at results + i * limit, counts[i]. */
int blurrily_storage_find_batch_each_in(trigram_map haystack, const blurrily_scope* scopes, size_t n_scopes,
                                        const uint32_t* which, const char* packed, const uint64_t* offsets, size_t n,
                                        uint16_t limit, trigram_match results, uint32_t* counts);

/* The same with device pointers on the map's GPU, enqueued on `stream`.  d_which lives in device memory: the call
 * copies it back and waits for that copy to group the needles (so a bad index is EINVAL only then), and when a scope
 * the mask strategy serves, or BLURRILY_NO_SCOPE, is named it copies d_offsets back the same way.  Preparing a scope
 * takes synchronous copies, as for blurrily_storage_find_batch_in_device. */
int blurrily_storage_find_batch_each_in_device(trigram_map haystack, const blurrily_scope* scopes, size_t n_scopes,
                                               const uint32_t* d_which, const char* d_packed, size_t packed_bytes,
                                               const uint64_t* d_offsets, size_t n, uint16_t limit,
                                               trigram_match d_results, uint32_t* d_counts, void* stream);

/* blurrily_storage_find_references with a scope per reference: element i is blurrily_storage_find_references for
 * references[i] restricted as above (an absent reference: 0 rows); nb_trigrams (may be NULL) as there. */
int blurrily_storage_find_references_each_in(trigram_map haystack, const blurrily_scope* scopes, size_t n_scopes,
                                             const uint32_t* which, const uint32_t* references, size_t n,
                                             uint16_t limit, trigram_match results, uint32_t* counts,
                                             uint32_t* nb_trigrams);

/* Threshold find: every row with at least the needle's bar of matches, not the best `limit`.  With T the needle's
 * distinct trigrams (what blurrily_tokeniser_parse_string returns for it), the bar is
 * t = max(1, min_matches, ceil(min_permille * T / 1000)).  A needle's rows are every row blurrily_storage_find would
 * return at an unbounded limit whose matches are >= t, in that order (matches descending, weight ascending,
 * reference ascending); a needle with T == 0 or t > T has none.  The map is read as find reads it.  With "devices" > 1
 * the primary device alone serves the call.
 * Rows of needle i are results[row_off[i] .. row_off[i+1]) (n + 1 offsets, always filled on success or ERANGE).
 * results == NULL: count only -- row_off filled, 0 returned.  capacity < row_off[n]: -1, errno ERANGE, results
 * untouched.  0, or -1 with errno (EINVAL before anything needs a GPU: min_permille > 1000, row_off NULL, packed or
 * offsets NULL with n > 0; ENODEV without a usable GPU). */
int blurrily_storage_find_batch_above(trigram_map haystack, const char* packed, const uint64_t* offsets, size_t n,
                                      uint32_t min_matches, uint32_t min_permille,
                                      trigram_match results, uint64_t capacity, uint64_t* row_off);
/* One needle: the same with n == 1; *total (optional) = its row count, also on ERANGE. */
int blurrily_storage_find_above(trigram_map haystack, const char* needle, uint32_t min_matches,
                                uint32_t min_permille, trigram_match results, uint64_t capacity, uint64_t* total);
/* By reference: element i is blurrily_storage_find_batch_above of any string whose tokenisation is reference i's
 * trigram set; the reference itself is among its rows (matches == T).  An absent reference: no rows,
 * nb_trigrams[i] == 0 (nb_trigrams may be NULL).  EINVAL also for references NULL with n > 0. */
int blurrily_storage_find_references_above(trigram_map haystack, const uint32_t* references, size_t n,
                                           uint32_t min_matches, uint32_t min_permille,
                                           trigram_match results, uint64_t capacity, uint64_t* row_off,
                                           uint32_t* nb_trigrams);

/* Similarity find: the best `limit` rows by trigram Jaccard similarity J = m / (T + R - m), with T the needle's
 * distinct trigrams (as for find), R the reference's (what blurrily_storage_get returns for it now) and m the matches
 * find reports for the pair.  A reference is a row iff m >= 1 and 1000 * m >= min_permille * (T + R - m) (exact, 64-bit
 * integers).  Order: J descending (m_a * u_b > m_b * u_a, u = T + R - m: no floating point), then find's order
 * (matches descending, weight ascending, reference ascending); cut at `limit`.  Dice similarity, 2m / (T + R), is a
 * monotone function of J: it gives the same rows in the same order.  T == 0 or limit == 0: no rows.  The map is read
 * as find reads it; with "devices" > 1 the primary device alone serves the call.
 * 0, or -1 with errno (EINVAL before anything needs a GPU: min_permille > 1000, counts NULL, results NULL with
 * limit > 0 and n > 0, packed or offsets NULL with n > 0; ENODEV without a usable GPU). */
/* Top-`limit` rows by trigram Jaccard similarity at or above min_permille / 1000.
 * results: n * limit rows (needle i owns [i*limit, i*limit + counts[i])); row_ntri (optional, n * limit slots):
 * each row's R, so the caller can compute the similarity exactly.  0, or -1 with errno. */
int blurrily_storage_find_batch_similar(trigram_map haystack, const char* packed, const uint64_t* offsets, size_t n,
                                        uint16_t limit, uint32_t min_permille,
                                        trigram_match results, uint32_t* counts, uint32_t* row_ntri);
/* One needle: the row count, or -1 with errno. */
int blurrily_storage_find_similar(trigram_map haystack, const char* needle, uint16_t limit, uint32_t min_permille,
                                  trigram_match results, uint32_t* row_ntri);
/* By stored reference (section 11's front end): element i is find_batch_similar of any string whose tokenisation is
 * reference i's trigram set; the reference itself is a row with similarity 1 (first unless another reference has the
 * same set).  Absent reference: 0 rows, nb_trigrams[i] == 0 (nb_trigrams may be NULL).  EINVAL also for references
 * NULL with n > 0. */
int blurrily_storage_find_references_similar(trigram_map haystack, const uint32_t* references, size_t n,
                                             uint16_t limit, uint32_t min_permille, trigram_match results,
                                             uint32_t* counts, uint32_t* row_ntri, uint32_t* nb_trigrams);

/* Scoped similarity find: the similarity find among a scope's members only.  A needle's rows
 * are the rows of ALL references passing the similarity find's row test, in its order, with every row whose reference
 * is not a held member of the scope removed, cut at `limit` -- not the unscoped call's rows at some limit, filtered.
 * T, R, m, the row test and the order are the similarity find's; membership is the scoped find's, read against the map
 * as it is at each call (a deleted member is not found; one put after the scope was made is, pending or folded; one
 * deleted and put again is found with its new trigrams and its new R; an empty scope, or one with no held member,
 * gives no rows).  T == 0: no rows; limit == 0: counts 0.  results, counts and row_ntri (optional) are laid out as for
 * blurrily_storage_find_batch_similar, host memory.  With "devices" > 1 the primary device alone serves the call.
 * 0, or -1 with errno.  EINVAL, before anything needs a GPU and with nothing written: a NULL map, a NULL scope or a
 * scope of another map, which[i] >= n_scopes (other than BLURRILY_NO_SCOPE), n_scopes > 0 with scopes NULL, counts
 * NULL, results NULL with n and limit non-zero, needles (or which) NULL with n > 0, n above the batch's cap,
 * min_permille > 1000.  Valid arguments without a usable GPU: ENODEV. */
int blurrily_storage_find_batch_similar_in(trigram_map haystack, blurrily_scope scope, const char* packed,
                                           const uint64_t* offsets, size_t n, uint16_t limit, uint32_t min_permille,
                                           trigram_match results, uint32_t* counts, uint32_t* row_ntri);
/* One needle: the row count, or -1 with errno. */
int blurrily_storage_find_similar_in(trigram_map haystack, blurrily_scope scope, const char* needle, uint16_t limit,
                                     uint32_t min_permille, trigram_match results, uint32_t* row_ntri);
/* A scope per needle: element i is the single-scope call on scopes[which[i]], or blurrily_storage_find_similar when
 * which[i] == BLURRILY_NO_SCOPE. */
int blurrily_storage_find_batch_similar_each_in(trigram_map haystack, const blurrily_scope* scopes, size_t n_scopes,
                                                const uint32_t* which, const char* packed, const uint64_t* offsets,
                                                size_t n, uint16_t limit, uint32_t min_permille,
                                                trigram_match results, uint32_t* counts, uint32_t* row_ntri);
/* blurrily_storage_find_references_similar with a scope per reference: an absent reference gets no rows and
 * nb_trigrams[i] == 0 (nb_trigrams may be NULL); a held one that is a member of its own scope is its own row at
 * similarity 1 (first unless another member has the same trigram set). */
int blurrily_storage_find_references_similar_each_in(trigram_map haystack, const blurrily_scope* scopes,
                                                     size_t n_scopes, const uint32_t* which,
                                                     const uint32_t* references, size_t n, uint16_t limit,
                                                     uint32_t min_permille, trigram_match results, uint32_t* counts,
                                                     uint32_t* row_ntri, uint32_t* nb_trigrams);

/* Scoped threshold find: the threshold find among a scope's members only.  A needle's rows are
 * exactly the rows blurrily_storage_find_batch_above gives for it with the same min_matches and min_permille, in the
 * same order, with every row removed whose reference is not a held member of the scope (a threshold find has no cut, so
 * this is the unscoped call filtered -- without sweeping the map or moving its rows).  T, the bar t and the order are
 * the threshold find's; membership is the scoped find's, read against the map as it is at each call (a deleted member is
 * not found; one put after the scope was made is, pending or folded; one deleted and put again is found with its new
 * trigrams; an empty scope, or one with no held member, gives no rows).  T == 0 or t > T: no rows.  results, capacity
 * and row_off follow blurrily_storage_find_batch_above's protocol: row_off[n + 1] is filled on success and on ERANGE;
 * results == NULL counts only; capacity < row_off[n] is -1 / ERANGE with results untouched.  With "devices" > 1 the
 * primary device alone serves the call.
 * 0, or -1 with errno.  EINVAL, before anything needs a GPU and with nothing written: a NULL map, a NULL scope or a
 * scope of another map, which[i] >= n_scopes (other than BLURRILY_NO_SCOPE), n_scopes > 0 with scopes NULL, row_off
 * NULL, needles (or which, or references) NULL with n > 0, n above the batch's cap, min_permille > 1000.  Valid
 * arguments without a usable GPU: ENODEV. */
int blurrily_storage_find_batch_above_in(trigram_map haystack, blurrily_scope scope, const char* packed,
                                         const uint64_t* offsets, size_t n, uint32_t min_matches,
                                         uint32_t min_permille, trigram_match results, uint64_t capacity,
                                         uint64_t* row_off);
/* One needle: the same with n == 1; *total (optional) = its row count, also on ERANGE. */
int blurrily_storage_find_above_in(trigram_map haystack, blurrily_scope scope, const char* needle,
                                   uint32_t min_matches, uint32_t min_permille, trigram_match results,
                                   uint64_t capacity, uint64_t* total);
/* A scope per needle: element i is the single-scope call on scopes[which[i]], or blurrily_storage_find_batch_above
 * when which[i] == BLURRILY_NO_SCOPE. */
int blurrily_storage_find_batch_above_each_in(trigram_map haystack, const blurrily_scope* scopes, size_t n_scopes,
                                              const uint32_t* which, const char* packed, const uint64_t* offsets,
                                              size_t n, uint32_t min_matches, uint32_t min_permille,
                                              trigram_match results, uint64_t capacity, uint64_t* row_off);
/* blurrily_storage_find_references_above with a scope per reference: an absent reference gets no rows and
 * nb_trigrams[i] == 0 (nb_trigrams may be NULL); a held one that is a member of its own scope is among its own rows
 * with matches == T. */
int blurrily_storage_find_references_above_each_in(trigram_map haystack, const blurrily_scope* scopes,
                                                   size_t n_scopes, const uint32_t* which,
                                                   const uint32_t* references, size_t n, uint32_t min_matches,
                                                   uint32_t min_permille, trigram_match results, uint64_t capacity,
                                                   uint64_t* row_off, uint32_t* nb_trigrams);

/* Clusters: connected components of the similarity self-join, computed on the device.  T, R, m
 * and J = m / (T + R - m) as for the similarity find; the map is read as find reads it.
 *   Nodes: the distinct references of the list that the map holds (a reference listed twice is one node).
 *   Edges: unordered pairs {a, b} of distinct nodes with m >= 1 and 1000 * m >= min_permille * (T_a + T_b - m), in 64-bit
 *          integers (min_permille 0: every pair sharing a trigram).  A reference the map holds but the list does not
 *          name is no node and joins nothing.
 *   Label: the smallest reference among the nodes of a node's connected component (itself, for a node without an
 *          edge).  The labels depend on the map's contents, the list as a set and min_permille only: not on the
 *          list's order, nor on the order in which the device joins nodes; two runs give identical bytes.
 * labels[i] belongs to references[i]; a listed reference the map does not hold gets BLURRILY_NO_CLUSTER.  (A held
 * reference of exactly that value cannot be told from an absent one by its label; blurrily_storage_get can.)
 * n_clusters (may be NULL): the components; n_edges (may be NULL): the edges as defined above, each pair once -- labels
 * alone cannot show that an edge was missed where another path joins the same nodes; this count can.  The pairs
 * themselves never exist, on the device or the host.  n == 0: success, nothing written but the two counts (0).  With
 * "devices" > 1 the primary device alone serves the call.
 * 0, or -1 with errno: EINVAL before anything needs a GPU (haystack NULL, min_permille > 1000, references or labels NULL
 * with n > 0, n above 0xFFFFFFF0 -- the call is not cut into chunks by references: every node must meet every other);
 * ENODEV without a usable GPU; EIO if a bounded loop of the device's union-find ran out (not seen; the bound is
 * a multiple of the longest chain there can be). */
#define BLURRILY_NO_CLUSTER 0xFFFFFFFFu
int blurrily_storage_cluster(trigram_map haystack, const uint32_t* references, size_t n, uint32_t min_permille,
                             uint32_t* labels, uint32_t* n_clusters, uint64_t* n_edges);

/* Cluster levels: the clusters above at several floors from one sweep -- the single-linkage
 * dendrogram cut at up to BLURRILY_CLUSTER_MAX_LEVELS heights, for a caller who picks the floor afterwards.  floors[0 ..
 * n_floors) are per mille, strictly ascending, each <= 1000; the device sweeps once, at floors[0], and keeps a forest
 * per floor.  Nodes, edges, labels, BLURRILY_NO_CLUSTER, repeats, absent references, unlisted bridges, deletes and
 * pending puts: exactly as for blurrily_storage_cluster.  Level k's outputs -- labels[k * n .. k * n + n), n_clusters[k]
 * and n_edges[k] (either array may be NULL) -- are byte for byte what blurrily_storage_cluster returns for the same
 * map, the same list and floors[k].  Levels nest: two references with one label at floors[k] have one label at every
 * lower floor.  n == 0: success, nothing written but the counts given (0 each).  With "devices" > 1 the primary device
 * alone serves the call.
 * 0, or -1 with errno: EINVAL before anything needs a GPU and with nothing written (haystack or floors NULL, n_floors 0
 * or above the cap, a floor above 1000, floors not strictly ascending, references or labels NULL with n > 0, n above
 * 0xFFFFFFF0); ENODEV without a usable GPU; EIO if a bounded loop of the device's union-find ran out. */
#define BLURRILY_CLUSTER_MAX_LEVELS 8
int blurrily_storage_cluster_levels(trigram_map haystack, const uint32_t* references, size_t n,
                                    const uint32_t* floors, uint32_t n_floors, uint32_t* labels, uint32_t* n_clusters,
                                    uint64_t* n_edges);

/* Cluster centres: the clusters above with what a deduplication job needs to pick a survivor and to judge a cluster
 * (DESIGN.md section 19).  Nodes, edges, labels, BLURRILY_NO_CLUSTER, repeats, absent references, unlisted bridges,
 * deletes, pending puts and min_permille: exactly as for blurrily_storage_cluster, and labels, n_clusters and n_edges
 * are byte for byte what that call returns for the same map, list and floor.
 *   degrees[i]:  the edges at references[i]'s node (0 for a reference that is no node); over the nodes they sum to
 *                2 * n_edges.
 *   centres[i]:  the reference of the node with the highest degree in references[i]'s component, the smallest
 *                reference among equal degrees (a node without an edge: itself); BLURRILY_NO_CLUSTER for no node.
 *   attached[i]: 1 if references[i]'s node is its component's centre or shares an edge with it, else 0 (no node: 0).  A
 *                component whose members are all attached is a star around its centre; an unattached member hangs
 *                on a chain.
 * All three depend on the map's contents, the list as a set and min_permille only; repeated elements get equal values.
 * degrees, centres, attached, n_clusters and n_edges may each be NULL.  attached costs a second sweep of the device,
 * which is not run when it is NULL.  n == 0: success, nothing written but the two counts (0).  With "devices" > 1 the
 * primary device alone serves the call.
 * 0, or -1 with errno: EINVAL before anything needs a GPU and with nothing written (haystack NULL, min_permille > 1000,
 * references or labels NULL with n > 0, n above 0xFFFFFFF0); ENODEV without a usable GPU; EIO if a bounded loop of the
 * device ran out. */
int blurrily_storage_cluster_centres(trigram_map haystack, const uint32_t* references, size_t n, uint32_t min_permille,
                                     uint32_t* labels, uint32_t* degrees, uint32_t* centres, uint8_t* attached,
                                     uint32_t* n_clusters, uint64_t* n_edges);

/* Cluster cores: density-based clusters (DBSCAN) over the edges above, which a chain of sparsely connected nodes cannot
 * bridge.  Nodes, edges, degrees, BLURRILY_NO_CLUSTER, repeats, absent references, unlisted
 * bridges, deletes, pending puts and min_permille: exactly as for blurrily_storage_cluster_centres.
 *   Core:    a node with degree >= min_degree.
 *   Cluster: a connected component of the graph that keeps only the edges whose both ends are cores; its label is the
 *            smallest reference among its cores.
 *   Border:  a node that is no core and has a core neighbour.  It takes the label of its anchor's cluster, the anchor
 *            being its core neighbour of the highest degree, the smallest reference among equals.  A border joins one
 *            cluster and never merges two.
 *   Noise:   a node that is neither.  Its label is its own reference, so the labels partition the nodes as
 *            blurrily_storage_cluster's do; its kind tells it from a cluster.
 *   kinds[i]:     BLURRILY_KIND_NONE for a reference that is no node (label BLURRILY_NO_CLUSTER, degree 0), else
 *                 BLURRILY_KIND_NOISE, BLURRILY_KIND_BORDER or BLURRILY_KIND_CORE.
 *   n_clusters:   the components of cores.  n_edges: every edge, byte for byte blurrily_storage_cluster's.
 *   n_core_edges: the edges with both ends core, each once -- labels cannot show that the second sweep missed an edge
 *                 where another path joins the same cores; this count can.
 * All outputs depend on the map's contents, the list as a set, min_permille and min_degree only.  min_degree 0: every
 * node is a core, and labels, n_clusters and n_edges are blurrily_storage_cluster's, n_core_edges == n_edges.
 * min_degree 1: the nodes with an edge keep blurrily_storage_cluster's labels, its singletons are noise.
 * degrees, kinds, n_clusters, n_edges and n_core_edges may each be NULL.  The device sweeps twice.  n == 0: success,
 * nothing written but the three counts (0).  With "devices" > 1 the primary device alone serves the call.
 * 0, or -1 with errno: EINVAL before anything needs a GPU and with nothing written (haystack NULL, min_permille > 1000,
 * references or labels NULL with n > 0, n above 0xFFFFFFF0); ENODEV without a usable GPU; EIO if a bounded loop of the
 * device ran out.  Not built: a _device variant, a protocol verb.  (Within blocks:
 * blurrily_storage_cluster_cores_within.) */
#define BLURRILY_KIND_NONE   0
#define BLURRILY_KIND_NOISE  1
#define BLURRILY_KIND_BORDER 2
#define BLURRILY_KIND_CORE   3
int blurrily_storage_cluster_cores(trigram_map haystack, const uint32_t* references, size_t n, uint32_t min_permille,
                                   uint32_t min_degree, uint32_t* labels, uint32_t* degrees, uint8_t* kinds,
                                   uint32_t* n_clusters, uint64_t* n_edges, uint64_t* n_core_edges);

/* Cluster extend: the clusters of old and new references together, from labels the caller already holds for the old
 * ones -- what a job that has clustered its map does after a put, without sweeping the old references again (DESIGN.md
 * section 22).  T, R, m, J, the edge test, BLURRILY_NO_CLUSTER, deletes, pending puts and a reference put again: exactly
 * as for blurrily_storage_cluster.
 *   Nodes:  the distinct references of old_refs and new_refs together that the map holds.  A node named by new_refs is
 *           NEW, whatever old_refs says of it; every other node is OLD.
 *   Seeds:  a pair (old_refs[i], old_labels[i]) whose two ends are both old nodes joins them.  A pair with an end that
 *           is not held, not listed or new does not exist.  A label need not be a component's smallest reference: any
 *           listed old reference serves (must-link stars or chains).
 *   Edges:  blurrily_storage_cluster's edges that have at least one new end.  Pairs of two old nodes are not looked
 *           at: the seeds speak for them.
 *   Label:  the smallest reference among the nodes of a node's component in the graph of seeds plus edges.
 * labels_old[i] belongs to old_refs[i], labels_new[j] to new_refs[j]; a listed reference the map does not hold gets
 * BLURRILY_NO_CLUSTER.  n_clusters (may be NULL): the components; n_edges (may be NULL): the edges above, each once --
 * seeds are not counted.  All outputs depend on the map's contents, the two lists as sets of pairs and min_permille
 * only: not on the lists' order, the images the references live in, or the order of the device's unions.
 * The contract: when old_labels is what blurrily_storage_cluster(old_refs, min_permille) returns on the map as it is
 * now and the two lists are disjoint, the two label arrays together and n_clusters are byte for byte what
 * blurrily_storage_cluster gives for the two lists in one, and n_edges is that call's minus the old call's.
 * A seed group is taken on trust.  A delete, or a put-again, of a member may have split a group, and the seeds cannot
 * show that: run blurrily_storage_cluster over that one group's remaining members, put its labels into old_labels, then
 * extend.  n_new == 0: the components of the seeds alone, n_edges 0; n_old == 0: blurrily_storage_cluster(new_refs).
 * Both 0: success, nothing written but the two counts (0).  With "devices" > 1 the primary device alone serves the call.
 * 0, or -1 with errno: EINVAL before anything needs a GPU and with nothing written (haystack NULL, min_permille > 1000,
 * old_refs, old_labels or labels_old NULL with n_old > 0, new_refs or labels_new NULL with n_new > 0, n_old + n_new
 * above 0xFFFFFFF0); ENODEV without a usable GPU; EIO if a bounded loop of the device's union-find ran out.  The labels
 * are written only on success. */
int blurrily_storage_cluster_extend(trigram_map haystack, const uint32_t* old_refs, const uint32_t* old_labels,
                                    size_t n_old, const uint32_t* new_refs, size_t n_new, uint32_t min_permille,
                                    uint32_t* labels_old, uint32_t* labels_new, uint32_t* n_clusters,
                                    uint64_t* n_edges);

/* Clusters within blocks: blurrily_storage_cluster's components where an edge also needs both ends in one block --
 * what entity resolution does after blocking by country, tenant or postcode, in one call for all blocks (DESIGN.md
 * section 29).  blocks[i] is an opaque 32-bit key for references[i].  Nodes, T, R, m, the edge test,
 * BLURRILY_NO_CLUSTER, deletes, pending puts and a reference put again: exactly as for blurrily_storage_cluster.
 *   Edges:  that call's edges whose two ends carry the same key.  A component never spans two blocks.
 *   Label:  the smallest reference among the nodes of a node's component.
 * labels[i] belongs to references[i]; n_clusters (may be NULL): the components over all blocks; n_edges (may be NULL):
 * the edges above, each once.  All outputs depend on the map's contents, the set of (reference, key) pairs and
 * min_permille only: not on the list's order, the images the references live in, or the order of the device's unions.
 * With all keys equal the outputs are byte for byte blurrily_storage_cluster's; with all keys distinct every held
 * reference is its own label and n_edges is 0; in general the labels are those of one blurrily_storage_cluster call
 * per block, and the two counts are the sums over those calls.  A reference may be listed more than once, under one
 * key.  n == 0: success, nothing written but the two counts (0).  A small block is scored member against member from
 * the device's copy of its members' trigrams, a large one sweeps the map as blurrily_storage_cluster does; option
 * "scope_strategy" 1 forces the sweep for every block, 2 the direct form, 0 (the default) chooses per block.  With
 * "devices" > 1 the primary device alone serves the call.
 * 0, or -1 with errno: EINVAL before anything needs a GPU and with nothing written (haystack NULL, min_permille > 1000,
 * references, blocks or labels NULL with n > 0, n above 0xFFFFFFF0, a reference listed more than once with different
 * keys); ENODEV without a usable GPU; EIO if a bounded loop of the device's union-find ran out.  The labels are written
 * only on success.  Not built: levels and centres within blocks, a _device variant, a protocol verb.  (Cores within
 * blocks: blurrily_storage_cluster_cores_within; extend within blocks: blurrily_storage_cluster_extend_within.) */
int blurrily_storage_cluster_within(trigram_map haystack, const uint32_t* references, const uint32_t* blocks, size_t n,
                                    uint32_t min_permille, uint32_t* labels, uint32_t* n_clusters, uint64_t* n_edges);

/* Cluster tree: the single-linkage dendrogram of the clusters above, at per-mille resolution, for a caller who wants
 * the floor at which two references first meet or wants to slide the cut afterwards.  Nodes, T,
 * R, m, the edge test, BLURRILY_NO_CLUSTER, repeats, absent references, unlisted bridges, deletes, pending puts and a
 * reference put again: exactly as for blurrily_storage_cluster.
 *   Height: an edge's height is h = floor(1000 * m / (T_a + T_b - m)) in 64-bit integers, so h >= f exactly when the
 *           edge passes that call's test at floor f.  Edges below min_permille do not exist.
 *   Order:  edges are totally ordered by (height descending, lower reference ascending, higher reference ascending).
 *   Merges: the maximum spanning forest of the edges under that order, which is unique: the edges Kruskal's algorithm
 *           keeps when it takes them in that order.  merges[0 .. *n_merges) are its edges {a, b, permille} with a < b
 *           as references and permille the height, sorted by that same order; merges needs room for n records.
 *           n_merges == nodes - n_clusters, always.
 * Uniting the ends of the merges with permille >= f, for any f >= min_permille, gives exactly the components of
 * blurrily_storage_cluster at floor f.  labels, n_clusters and n_edges are byte for byte what that call returns at
 * min_permille.  All outputs depend on the map's contents, the list as a set and min_permille only; two runs give
 * identical bytes.  The device sweeps the map once per Boruvka round, a handful of times.  n_merges, n_clusters and
 * n_edges may each be NULL.  n == 0: success, nothing written but the counts given (0).  With "devices" > 1 the primary
 * device alone serves the call.
 * 0, or -1 with errno: EINVAL before anything needs a GPU and with nothing written (haystack NULL, min_permille > 1000,
 * references, labels or merges NULL with n > 0, n above BLURRILY_CLUSTER_TREE_MAX: the device orders edges by one
 * 64-bit word that holds the height and both ends in 27 bits each); ENODEV without a usable GPU; EIO if a bounded loop
 * of the device's union-find or the bound on the rounds ran out.  The labels and merges are written only on success.
 * Not built: a tree within scopes, a _device variant, other linkages, a protocol verb.  (Within blocks:
 * blurrily_storage_cluster_tree_within below.) */
#define BLURRILY_CLUSTER_TREE_MAX 0x8000000u
typedef struct { uint32_t a, b, permille; } blurrily_cluster_merge_t;
int blurrily_storage_cluster_tree(trigram_map haystack, const uint32_t* references, size_t n, uint32_t min_permille,
                                  uint32_t* labels, blurrily_cluster_merge_t* merges, uint32_t* n_merges,
                                  uint32_t* n_clusters, uint64_t* n_edges);

/* Cluster tree extend: the cluster tree of old and new references together, from the records the caller already holds
 * for the old ones -- what a job that keeps a tree does after a put, without sweeping the old references again
 * (DESIGN.md section 37).  Nodes, T, R, m, the height h, the total order, the records' form and order,
 * BLURRILY_NO_CLUSTER, repeats, absent references, unlisted bridges, deletes, pending puts, a reference put again and
 * the cap BLURRILY_CLUSTER_TREE_MAX (on n_old + n_new): exactly as for blurrily_storage_cluster_tree.  Old and new:
 * exactly as for blurrily_storage_cluster_extend -- a node named by new_refs is NEW, whatever old_refs says of it.
 *   Candidates: (a) every old record {a, b, permille} with permille >= min_permille whose two ends are both OLD nodes;
 *           its height is taken on trust, nothing is computed again.  A record with an end that is not held, not
 *           listed or new does not exist.  (b) Every edge of blurrily_storage_cluster_tree at min_permille with at
 *           least one new end, at its height h.  Pairs of two old nodes are not looked at: the records speak for them.
 *   Merges: the maximum spanning forest of the candidates under the total order, as that call gives its own;
 *           merges needs room for n_old + n_new records.  Labels: the smallest reference of a node's component in it.
 * labels_old[i] belongs to old_refs[i], labels_new[j] to new_refs[j].  n_edges: the edges of (b), each once; the
 * records are not counted.
 * The contract: when the lists are disjoint, every listed reference is held, and old_merges is what
 * blurrily_storage_cluster_tree(old_refs, f_old) returned for some f_old <= min_permille with the map's old rows
 * unchanged since, then the records, the two label arrays together and n_clusters are byte for byte what
 * blurrily_storage_cluster_tree gives for the two lists in one at min_permille, and n_edges is that call's minus the
 * tree call's over old_refs at min_permille.  (Under a strict total order the forest is unique, and an old edge the old
 * forest left out is the worst of a cycle that is still there: it stays out.)  So a floor above the old tree's is
 * allowed: the records below it are passed over.
 * The records are taken on trust.  A floor BELOW the old tree's cannot be told -- the old-old edges between the two
 * floors are missing, and nothing looks for them -- nor can a tree made before a delete or a put-again of a member,
 * whose component may have split: run blurrily_storage_cluster_tree over that one component's remaining members, put
 * its records in the place of the component's, then extend.  Records that are no tree's (cycles, duplicates, made-up
 * heights) are accepted all the same: the result is the forest of the candidate set as it stands, and the call returns.
 * n_new == 0: the forest of the records at or above the floor, n_edges 0; n_old == 0:
 * blurrily_storage_cluster_tree(new_refs).  Both 0: success, nothing written but the counts given (0).  n_merges,
 * n_clusters and n_edges may each be NULL.  With "devices" > 1 the primary device alone serves the call.
 * 0, or -1 with errno: EINVAL before anything needs a GPU and with nothing written (haystack NULL, min_permille > 1000,
 * old_refs or labels_old NULL with n_old > 0, new_refs or labels_new NULL with n_new > 0, old_merges NULL with
 * n_old_merges > 0, merges NULL with n_old + n_new > 0, n_old + n_new above BLURRILY_CLUSTER_TREE_MAX, n_old_merges
 * above n_old, an old record with a >= b or permille > 1000); ENODEV without a usable GPU; EIO if a bounded loop of the
 * device's union-find or the bound on the rounds ran out.  The labels and merges are written only on success.
 * Not built: taking references out of a tree, extending the core tree, blocks or scopes, a _device variant, a protocol
 * verb. */
int blurrily_storage_cluster_tree_extend(trigram_map haystack, const uint32_t* old_refs, size_t n_old,
                                         const blurrily_cluster_merge_t* old_merges, size_t n_old_merges,
                                         const uint32_t* new_refs, size_t n_new, uint32_t min_permille,
                                         uint32_t* labels_old, uint32_t* labels_new,
                                         blurrily_cluster_merge_t* merges, uint32_t* n_merges,
                                         uint32_t* n_clusters, uint64_t* n_edges);

/* Cluster core tree: the dendrogram of blurrily_storage_cluster_cores' cores, for a caller who does not know the floor
 * in advance.  Uniting the ends of the merges with permille >= f, for any f >= min_permille,
 * gives every reference with core_permille >= f (BLURRILY_NO_CORE aside) the label blurrily_storage_cluster_cores
 * gives it at (f, min_degree).  The cores of that call are exactly those references.
 * Nodes, T, R, m, the edge test, the height h, BLURRILY_NO_CLUSTER, repeats, absent references, unlisted bridges,
 * deletes, pending puts, a reference put again, "devices" > 1 and the cap BLURRILY_CLUSTER_TREE_MAX: exactly as for
 * blurrily_storage_cluster_tree.  Edges below min_permille do not exist.
 *   Core height: c(x) is the min_degree-th largest h among x's edges, ties counted as often as they occur, so x is a
 *           core at floor f exactly when c(x) >= f.  core_permille[i] is that of references[i]; BLURRILY_NO_CORE for
 *           a reference that is no node and for a node with fewer than min_degree edges.  With min_degree == 0 every
 *           node's is 1000.
 *   Tree edges: the edges whose two ends both have a core height, each at the capped height
 *           H = min(h, c(a), c(b)): H >= f exactly when the edge joins two cores at floor f.
 *   Merges: the maximum spanning forest of the tree edges under blurrily_storage_cluster_tree's total order with H as
 *           the height, unique: {a, b, permille = H} with a < b, sorted by that order; merges needs room for n records.
 *   Labels: for a node with a core height the smallest reference of its component in that forest, for any other node
 *           its own reference, BLURRILY_NO_CLUSTER for no node.
 *   Counts: n_clusters, the components among the nodes with a core height -- blurrily_storage_cluster_cores'
 *           n_clusters at (min_permille, min_degree) -- and n_merges == those nodes - n_clusters; n_edges, every edge,
 *           byte for byte blurrily_storage_cluster's; n_core_edges, the tree edges, each once: that call's
 *           n_core_edges.  Each of the four, and n_merges, may be NULL.
 * All outputs depend on the map's contents, the list as a set, min_permille and min_degree only; two runs give
 * identical bytes.  The device sweeps the map at most twice for the core heights (not at all with min_degree == 0) and
 * once per Boruvka round.  n == 0: success, nothing written but the counts given (0).
 * 0, or -1 with errno: EINVAL before anything needs a GPU and with nothing written (haystack NULL, min_permille > 1000,
 * references, labels, core_permille or merges NULL with n > 0, n above BLURRILY_CLUSTER_TREE_MAX; any min_degree is
 * valid); ENODEV without a usable GPU; EIO if a bounded loop of the device or the bound on the rounds ran out.  labels,
 * core_permille and merges are written only on success.
 * Not built: the borders' anchors at a cut (they need the degree at that floor), a _device variant, a protocol verb.
 * (Within blocks: blurrily_storage_cluster_core_tree_within below.) */
#define BLURRILY_NO_CORE 0xFFFFFFFFu
int blurrily_storage_cluster_core_tree(trigram_map haystack, const uint32_t* references, size_t n,
                                       uint32_t min_permille, uint32_t min_degree,
                                       uint32_t* labels, uint32_t* core_permille,
                                       blurrily_cluster_merge_t* merges, uint32_t* n_merges,
                                       uint32_t* n_clusters, uint64_t* n_edges, uint64_t* n_core_edges);

/* Cluster tree within blocks: the single-linkage dendrogram inside caller-given blocks, one call for all blocks -- for
 * the caller who blocks by country, tenant or postcode and does not know the floor in advance.
 * blocks[i] is an opaque 32-bit key for references[i].  Nodes, T, R, m, the edge test, the height
 * h = floor(1000 * m / (T + R - m)), the total order, the records' form and order, BLURRILY_NO_CLUSTER, repeats (under one
 * key), a shuffled list, absent references, unlisted bridges, deletes, pending puts, a reference put again,
 * "devices" > 1 and the cap BLURRILY_CLUSTER_TREE_MAX: exactly as for blurrily_storage_cluster_within and
 * blurrily_storage_cluster_tree.
 *   Edges:  blurrily_storage_cluster's edges at min_permille whose two ends carry the same key.
 *   Merges: the maximum spanning forest of those edges under blurrily_storage_cluster_tree's total order (height
 *           descending, lower reference ascending, higher reference ascending), which is unique.
 *           merges[0 .. *n_merges) are its edges {a, b, permille} with a < b, sorted by that order; merges needs room
 *           for n records.  No record joins two keys.  n_merges == nodes - n_clusters, always.
 *   Labels: labels, n_clusters and n_edges are byte for byte blurrily_storage_cluster_within's at min_permille.
 * Uniting the ends of the merges with permille >= f, for any f >= min_permille, gives exactly the labels of
 * blurrily_storage_cluster_within at floor f.  The result equals one blurrily_storage_cluster_tree call per block: the
 * records of those calls merged into one list under the total order, the labels put back in place, the counts
 * summed.  With all keys equal it is blurrily_storage_cluster_tree, byte for byte; with all keys distinct there is no
 * record and every held reference is its own label.  All outputs depend on the map's contents, the set of (reference,
 * key) pairs and min_permille only; two runs give identical bytes.  A small block is scored member against member from
 * the device's copy of its members' trigrams once per Boruvka round, a large one sweeps the map once per round; option
 * "scope_strategy" chooses as for blurrily_storage_cluster_within.  n_merges, n_clusters and n_edges may each be NULL.
 * n == 0: success, nothing written but the counts given (0).
 * 0, or -1 with errno: EINVAL before anything needs a GPU and with nothing written (haystack NULL, min_permille > 1000,
 * references, blocks, labels or merges NULL with n > 0, n above BLURRILY_CLUSTER_TREE_MAX, a reference listed more than
 * once with different keys); ENODEV without a usable GPU; EIO if a bounded loop of the device's union-find or the bound
 * on the rounds ran out.  The labels and merges are written only on success.
 * Not built: tree extend within blocks, a _device variant, a protocol verb.  (The core tree within blocks:
 * blurrily_storage_cluster_core_tree_within below.) */
int blurrily_storage_cluster_tree_within(trigram_map haystack, const uint32_t* references, const uint32_t* blocks,
                                         size_t n, uint32_t min_permille, uint32_t* labels,
                                         blurrily_cluster_merge_t* merges, uint32_t* n_merges,
                                         uint32_t* n_clusters, uint64_t* n_edges);

/* Cluster edges: the edges of blurrily_storage_cluster's graph themselves, each pair once, with its similarity -- what
 * feeds a second-stage matcher, a review queue or a clustering of the caller's own, and what every other cluster result
 * can be checked against.  Nodes, T, R, m, the edge test
 * 1000 * m >= min_permille * (T_a + T_b - m), repeats in the list, a shuffled list, absent references, unlisted
 * references (never an end, never a bridge), deletes, pending puts, a reference put again and "devices" > 1: exactly as
 * for blurrily_storage_cluster.  blurrily_storage_cluster_edges_within is the same over
 * blurrily_storage_cluster_within's graph: blocks[i] is an opaque 32-bit key for references[i], and an edge needs both
 * ends under one key ("scope_strategy" chooses the kernel per block as it does there).
 *   Records: one {a, b, permille} per edge, a < b as references, permille = floor(1000 * m / (T_a + T_b - m)) in 64-bit
 *            integers: blurrily_storage_cluster_tree's height, so permille >= min_permille always.
 *   Order:   blurrily_storage_cluster_tree's total order -- permille descending, a ascending, b ascending.  Each edge
 *            appears once, so the records are distinct under it.  blurrily_storage_cluster_tree's merges at the same
 *            floor are a subsequence of them.
 *   Count:   *n_edges (required) is the graph's edge count, byte for byte the n_edges of blurrily_storage_cluster
 *            (blurrily_storage_cluster_within) at that floor, on success, on ERANGE and on EOVERFLOW.
 * The capacity protocol is blurrily_storage_find_batch_above's: edges == NULL counts only (capacity is ignored, nothing
 * is sorted or emitted); otherwise edges has room for `capacity` records, and capacity < *n_edges is ERANGE with edges
 * untouched -- call again with the room *n_edges names.  Option "cluster_edges_max" (default 2^28 records, 1 .. 2^31)
 * bounds the device scratch of one call, 28 bytes a record (7 GiB at the default): the call keeps room for
 * min(capacity, cluster_edges_max) records on the device, and a count that fits capacity but not that room is EOVERFLOW
 * with edges untouched.  Then raise the floor, cut the list into blocks (blurrily_storage_cluster_edges_within), split
 * the list, or raise the option if the device has the memory.  The output depends on the map's contents, the list as a
 * set (with its keys) and min_permille only; two runs give identical bytes.  n == 0: success, *n_edges = 0.
 * 0, or -1 with errno: EINVAL before anything needs a GPU and with nothing written (haystack NULL, min_permille > 1000,
 * references NULL with n > 0, n_edges NULL, n above BLURRILY_CLUSTER_TREE_MAX -- the device orders edges by one 64-bit
 * word that holds both ends in 27 bits each -- and for the blocked form blocks NULL with n > 0 or a reference listed
 * more than once with different keys); ENODEV without a usable GPU; EIO for a device error word.  The records are
 * written only on success.
 * Not built: scopes, _device variants, protocol verbs. */
int blurrily_storage_cluster_edges(trigram_map haystack, const uint32_t* references, size_t n,
                                   uint32_t min_permille, blurrily_cluster_merge_t* edges,
                                   uint64_t capacity, uint64_t* n_edges);
int blurrily_storage_cluster_edges_within(trigram_map haystack, const uint32_t* references,
                                          const uint32_t* blocks, size_t n, uint32_t min_permille,
                                          blurrily_cluster_merge_t* edges, uint64_t capacity,
                                          uint64_t* n_edges);

/* Cluster edges extend and between: blurrily_storage_cluster_edges over two lists, cut down to the edges a caller who
 * already holds some of them is missing.  Only one side sweeps the map, so the cost follows that
 * side, not the lists together.  Nodes, T, R, m, the edge test, repeats, shuffled lists, absent references, unlisted
 * references (never an end), deletes, pending puts, a reference put again and "devices" > 1: exactly as for
 * blurrily_storage_cluster.  Old and new are blurrily_storage_cluster_extend's: a reference the second list names is NEW
 * (on the RIGHT), whatever the first list says of it.  Records, their permille, their total order, the capacity
 * protocol (edges == NULL counts only; ERANGE leaves edges untouched and fills *n_edges; EOVERFLOW against
 * min(capacity, "cluster_edges_max")) and the required n_edges are blurrily_storage_cluster_edges'.
 *   _extend:  the edges of blurrily_storage_cluster over both lists that have at least one new end, each once.
 *             *n_edges is byte for byte blurrily_storage_cluster_extend's n_edges for the same lists and floor.  The
 *             records of blurrily_storage_cluster_edges over the old references that are not new, and of this call,
 *             merged under the total order, are byte for byte blurrily_storage_cluster_edges over both lists: how a
 *             caller keeps an edge list current after a put.  n_old == 0 gives blurrily_storage_cluster_edges(new_refs);
 *             n_new == 0 gives success with no edge.
 *   _between: the edges with exactly one end on each side -- record linkage: which rows of one list match which of
 *             another.  _extend(L, R) is _between(L, R) merged with blurrily_storage_cluster_edges(R).  For disjoint
 *             lists _between(L, R) and _between(R, L) are identical bytes.  Either n being 0 gives no edge.  The side
 *             with fewer distinct listed references sweeps (a tie: the right), whichever way round the lists are named.
 * The output depends on the map's contents, the two lists as sets and min_permille only; two runs give identical bytes.
 * 0, or -1 with errno: EINVAL before anything needs a GPU and with nothing written (haystack NULL, min_permille > 1000,
 * a list NULL with its n > 0, n_edges NULL, the two n together above BLURRILY_CLUSTER_TREE_MAX); ENODEV without a
 * usable GPU; ERANGE and EOVERFLOW as above; EIO for a device error word.  The records are written only on success.
 * Not built: blocks or scopes on either entry, _device variants, protocol verbs, Ruby methods. */
int blurrily_storage_cluster_edges_extend(trigram_map haystack, const uint32_t* old_refs, size_t n_old,
                                          const uint32_t* new_refs, size_t n_new, uint32_t min_permille,
                                          blurrily_cluster_merge_t* edges, uint64_t capacity, uint64_t* n_edges);
int blurrily_storage_cluster_edges_between(trigram_map haystack, const uint32_t* left_refs, size_t n_left,
                                           const uint32_t* right_refs, size_t n_right, uint32_t min_permille,
                                           blurrily_cluster_merge_t* edges, uint64_t capacity, uint64_t* n_edges);

/* Cluster cores within blocks: blurrily_storage_cluster_cores' density clusters inside caller-given blocks, one call
 * for all blocks -- the second look of a job that has blocked its records and found that single linkage chains
 * look-alikes together.  blocks[i] is an opaque 32-bit key for references[i].  Nodes, T, R, m,
 * the edge test, BLURRILY_NO_CLUSTER, repeats (under one key), a shuffled list, absent references, unlisted bridges,
 * deletes, pending puts, a reference put again, "devices" > 1 and "scope_strategy" (0 chooses per block, 1 sweeps
 * every block, 2 scores every block directly): exactly as for blurrily_storage_cluster_within.  Core, cluster, border,
 * anchor (the core neighbour of the highest degree, the smallest reference among equals), noise, the BLURRILY_KIND_*
 * values and the meaning of the three counts: exactly as for blurrily_storage_cluster_cores.
 *   Edges:   blurrily_storage_cluster_within's: an edge needs both ends under one key.
 *   Degrees: a degree counts those edges only.  So a core, a border's anchor and a cluster never reach across a key.
 * With all keys equal every output is byte for byte blurrily_storage_cluster_cores'.  With min_degree 0 every node is a
 * core, labels, n_clusters and n_edges are byte for byte blurrily_storage_cluster_within's, and n_core_edges == n_edges.
 * With all keys distinct every held reference is its own label with degree 0 -- noise for min_degree >= 1, a core for
 * 0 -- and the three counts are 0, except that n_clusters is the number of nodes when min_degree is 0.  In general the
 * result equals one blurrily_storage_cluster_cores call per block: labels, degrees and kinds put back in place, the
 * three counts summed.  degrees equals the degrees read off blurrily_storage_cluster_edges_within's records at the same
 * floor.  All outputs depend on the map's contents, the set of (reference, key) pairs, min_permille and min_degree
 * only; two runs give identical bytes under each strategy, and the three strategies give identical bytes.  Each block
 * is served twice, first for the degrees and then for the unions and anchors: a small one is scored member against
 * member from the device's copy of its members' trigrams, a large one sweeps the map.
 * degrees, kinds, n_clusters, n_edges and n_core_edges may each be NULL.  n == 0: success, nothing written but the
 * counts given (0).
 * 0, or -1 with errno: EINVAL before anything needs a GPU and with nothing written (haystack NULL, min_permille > 1000,
 * references, blocks or labels NULL with n > 0, n above 0xFFFFFFF0, a reference listed more than once with different
 * keys; any min_degree is valid); ENODEV without a usable GPU; EIO if a bounded loop of the device ran out.  The outputs
 * are written only on success.
 * Not built: levels, centres and extend within blocks, a _device variant, a protocol verb, a Ruby method.  (The core
 * tree within blocks: blurrily_storage_cluster_core_tree_within below.) */
int blurrily_storage_cluster_cores_within(trigram_map haystack, const uint32_t* references, const uint32_t* blocks,
                                          size_t n, uint32_t min_permille, uint32_t min_degree,
                                          uint32_t* labels, uint32_t* degrees, uint8_t* kinds,
                                          uint32_t* n_clusters, uint64_t* n_edges, uint64_t* n_core_edges);

/* Cluster core tree within blocks: the dendrogram of blurrily_storage_cluster_cores_within's cores inside caller-given
 * blocks, one call for all blocks -- for the job that blocks its records, has found that single linkage chains
 * look-alikes together, and does not know the floor in advance.  blocks[i] is an opaque 32-bit
 * key for references[i].  Nodes, T, R, m, the edge test, the height h, core heights, tree edges, the capped height
 * H = min(h, c(a), c(b)), the total order, the records' form and order, BLURRILY_NO_CLUSTER and BLURRILY_NO_CORE:
 * exactly as for blurrily_storage_cluster_core_tree.  Repeats (under one key), a shuffled list, absent references,
 * unlisted bridges, deletes, pending puts, a reference put again, "devices" > 1, "scope_strategy" and the cap
 * BLURRILY_CLUSTER_TREE_MAX: exactly as for blurrily_storage_cluster_tree_within.
 *   Edges:  blurrily_storage_cluster_within's: an edge needs both ends under one key.
 *   Core height: the min_degree-th largest h among those edges only, so no core height, tree edge or record reaches
 *           across a key.
 *   Counts: n_edges is blurrily_storage_cluster_within's; n_clusters and n_core_edges are
 *           blurrily_storage_cluster_cores_within's at (min_permille, min_degree); n_merges == the nodes with a core
 *           height - n_clusters.  Each of the four may be NULL.
 * Uniting the ends of the merges with permille >= f, for any f >= min_permille, gives every reference with
 * core_permille >= f the label blurrily_storage_cluster_cores_within gives it at (f, min_degree), and the cores of that
 * call are exactly those references.  The result equals one blurrily_storage_cluster_core_tree call per block: the
 * records merged into one list under the total order, labels and core heights put back in place, the counts summed.
 * With all keys equal it is blurrily_storage_cluster_core_tree, byte for byte.  With min_degree 0 or 1 merges and labels
 * are blurrily_storage_cluster_tree_within's; with 0 the counts are too, and every node's core_permille is 1000.  With
 * all keys distinct and min_degree >= 1 there is no record, every core_permille is BLURRILY_NO_CORE and every held
 * reference is its own label.  All outputs depend on the map's contents, the set of (reference, key) pairs,
 * min_permille and min_degree only; two runs give identical bytes, and so do the three strategies.  Each block is
 * served at most twice for the core heights (not at all with min_degree == 0) and once per Boruvka round: a small one
 * is scored member against member from the device's copy of its members' trigrams, a large one sweeps the map.
 * n == 0: success, nothing written but the counts given (0).
 * 0, or -1 with errno: EINVAL before anything needs a GPU and with nothing written (haystack NULL, min_permille > 1000,
 * references, blocks, labels, core_permille or merges NULL with n > 0, n above BLURRILY_CLUSTER_TREE_MAX, a reference
 * listed more than once with different keys; any min_degree is valid); ENODEV without a usable GPU; EIO if a bounded
 * loop of the device or the bound on the rounds ran out.  labels, core_permille and merges are written only on success.
 * Not built: extend forms of the core tree, scopes on any tree, the borders' anchors at a cut, levels or centres
 * within blocks, a _device variant, a protocol verb, a Ruby method. */
int blurrily_storage_cluster_core_tree_within(trigram_map haystack, const uint32_t* references, const uint32_t* blocks,
                                              size_t n, uint32_t min_permille, uint32_t min_degree,
                                              uint32_t* labels, uint32_t* core_permille,
                                              blurrily_cluster_merge_t* merges, uint32_t* n_merges,
                                              uint32_t* n_clusters, uint64_t* n_edges, uint64_t* n_core_edges);

/* Cluster extend within blocks: blurrily_storage_cluster_extend inside caller-given blocks -- what a job that blocks its
 * records and has clustered them with blurrily_storage_cluster_within does after a put, without scoring any block
 * against itself again and without losing the labels it holds.  old_blocks[i] is an opaque
 * 32-bit key for old_refs[i], new_blocks[j] for new_refs[j].  T, R, m, J, the edge test, BLURRILY_NO_CLUSTER, deletes,
 * pending puts and a reference put again: exactly as for blurrily_storage_cluster.
 *   Nodes:  the distinct references of old_refs and new_refs together that the map holds.  A node named by new_refs is
 *           NEW, whatever old_refs says of it; every other node is OLD.
 *   Keys:   a reference may be listed more than once, in one list or across the two, under one key.
 *   Seeds:  a pair (old_refs[i], old_labels[i]) whose two ends are both old nodes under the same key joins them.  A
 *           pair with an end that is not held, not listed or new does not exist, and neither does a pair whose ends
 *           carry different keys (this is no error).  A label need not be a component's smallest reference: any listed
 *           old reference serves (must-link stars or chains).
 *   Edges:  blurrily_storage_cluster_within's edges (both ends under one key) that have at least one new end.  Pairs of
 *           two old nodes are not looked at: the seeds speak for them.
 *   Label:  the smallest reference among the nodes of a node's component in the graph of seeds plus edges.  A
 *           component never spans two keys.
 * labels_old[i] belongs to old_refs[i], labels_new[j] to new_refs[j]; a listed reference the map does not hold gets
 * BLURRILY_NO_CLUSTER.  n_clusters (may be NULL): the components; n_edges (may be NULL): the edges above, each once --
 * seeds are not counted.  All outputs depend on the map's contents, the two lists as sets of (reference, key[, label])
 * and min_permille only: not on the lists' order, the images the references live in, or the order of the device's
 * unions; the three values of "scope_strategy" give identical bytes.
 * The contract: when old_labels is what blurrily_storage_cluster_within(old_refs, old_blocks, min_permille) returns on
 * the map as it is now and the two lists are disjoint, the two label arrays together and n_clusters are byte for byte
 * what blurrily_storage_cluster_within gives for the two lists in one with the keys concatenated, and n_edges is that
 * call's minus the old call's.  With all keys equal every output is byte for byte blurrily_storage_cluster_extend's.
 * n_old == 0: blurrily_storage_cluster_within(new_refs, new_blocks).  n_new == 0: the components of the seeds alone,
 * n_edges 0.  Both 0: success, nothing written but the two counts (0).
 * A seed group is taken on trust.  A delete, or a put-again, of a member may have split a group, and the seeds cannot
 * show that: run blurrily_storage_cluster_within over that one group's remaining members, put its labels into
 * old_labels, then extend.
 * Only a block that has a new member is looked at: its new members are scored against every member of the block from
 * the device's copy of their trigrams (new x block pair scores, not block x block), or, for a large block, sweep the
 * map as blurrily_storage_cluster_extend's do.  Option "scope_strategy" 1 forces the sweep for every such block, 2 the
 * direct form, 0 (the default) chooses per block.  With "devices" > 1 the primary device alone serves the call.
 * 0, or -1 with errno: EINVAL before anything needs a GPU and with nothing written (haystack NULL, min_permille > 1000,
 * old_refs, old_blocks, old_labels or labels_old NULL with n_old > 0, new_refs, new_blocks or labels_new NULL with
 * n_new > 0, n_old + n_new above 0xFFFFFFF0, a reference listed more than once with different keys); ENODEV without a
 * usable GPU; EIO if a bounded loop of the device's union-find ran out.  The labels are written only on success.
 * Not built: the tree and the edge list extended within blocks, extend forms of cores, centres and levels, a _device
 * variant, a protocol verb, a Ruby method. */
int blurrily_storage_cluster_extend_within(trigram_map haystack,
        const uint32_t* old_refs, const uint32_t* old_blocks, const uint32_t* old_labels, size_t n_old,
        const uint32_t* new_refs, const uint32_t* new_blocks, size_t n_new,
        uint32_t min_permille,
        uint32_t* labels_old, uint32_t* labels_new, uint32_t* n_clusters, uint64_t* n_edges);

/* Tokeniser (ext/blurrily/tokeniser.h:34, tokeniser.c:59-119): `output` needs
 * strlen(input)+1 slots; returns the number of distinct codes, ascending. */
int blurrily_tokeniser_parse_string(const char* input, uint16_t* output);

/* Introspection for tests / bench (no reference counterpart). */
typedef struct blurrily_device_info_t {
  int32_t  device_ordinal;      /* -1 if no usable GPU                           */
  uint32_t n_refs;              /* distinct references in the device index       */
  uint32_t n_windows;           /* reference-rank windows                        */
  uint32_t window_bits;         /* log2(ranks per window)                        */
  uint64_t n_entries;           /* (trigram, ref) entries resident               */
  uint64_t device_bytes;        /* HBM bytes held by the index                   */
  double   last_find_kernel_ms; /* HIP-event time of the last find kernel launch */
  double   last_tokenise_kernel_ms;
  uint32_t n_pending;           /* puts since the base image was built (served by a delta image) */
  uint32_t n_tombstones;        /* base references deleted since the build                       */
  uint64_t base_builds;         /* full device-image builds so far                               */
  double   mean_hit_slice;      /* postings a needle trigram finds per window, on average: what the
                                   choice between the two sweeps is gated on ("ws_min_slice")     */
  uint32_t n_bitmaps;           /* dense slices that also exist as bitmaps (0: the window-major
                                   sweep cannot run on this image)                               */
  uint32_t reserved_;
  double   dense_share;         /* share of those postings in slices dense enough to have a bitmap  */
  double   ws_gain;             /* the four biggest buckets' part of mean_hit_slice x postings per
                                   reference: postings a needle can expect to leave out per window */
  /* option "devices" (round 5): what the replicas of the image actually sit on */
  uint32_t n_replicas;          /* copies of the image beside the primary's (0: "devices" 1, or none made yet)   */
  uint32_t distinct_devices;    /* PHYSICAL devices holding a copy, the primary's included (by PCI bus id): more
                                   replicas than devices share devices, and a batch is then no faster for them   */
  uint32_t peer_access_mask;    /* bit k: replica k's device and the primary's reach each other's memory directly
                                   (hipDeviceCanAccessPeer both ways, enabled): rows travel point to point over
                                   xGMI; bit clear: the peer copies of that replica are staged by the runtime     */
  uint32_t same_device_mask;    /* bit k: replica k sits on the primary's own device (no link involved)          */
  char     pci_bus_id[16];      /* the primary's device, "0000:c1:00.0"                                          */
} blurrily_device_info_t;
int blurrily_storage_device_info(trigram_map haystack, blurrily_device_info_t* info);
/* The same for a caller compiled against another version of this header: at most
 * `info_size` bytes are written (pass sizeof(blurrily_device_info_t) as the caller
 * knows it); returns the size of the structure as the LIBRARY knows it, so that a
 * caller can tell which trailing fields it got.  The structure only ever grows at
 * its end. */
size_t blurrily_storage_device_info_sized(trigram_map haystack, void* info, size_t info_size);

/* When non-zero, find_batch_device brackets its kernels with hipEvents on the
 * launch stream and synchronises to fill last_*_kernel_ms (bench/profiling). */
void blurrily_storage_set_timing(trigram_map haystack, int enabled);

/* Request counters of the find kernels (bench/profiling; no reference counterpart).  While
 * enabled, every find launch sequence counts -- exactly, from wave-uniform values -- what it
 * asks of the memory system and of the LDS; blurrily_storage_find_stats synchronises the
 * device and copies the counters of the LAST find call into out8[8]:
 *   [0] 16-bit postings loaded (x 2 = bytes; each is also one LDS-atomic lane)
 *   [1] sweep steps   [2] slice-table words loaded (x 4 = bytes)   [3] needles (or ranges) swept
 *   [4] candidate-pool compactions   [5] windows swept again after a pool overflow
 *   [6] wave-loads of postings issued by the window-major sweep   [7] bitmap words read for its candidates
 * Collecting costs a few scalar instructions per wave-load; leave it off when timing. */
void blurrily_storage_set_stats(trigram_map haystack, int enabled);
int  blurrily_storage_find_stats(trigram_map haystack, uint64_t* out8);
/* While the counters are on, every needle of a find call also gets a word saying which paths of the
 * kernels its find went through (4-bit / byte / 16-bit counters, cold-start bisection, pool overflow
 * and re-sweep, windows stepped over, latency-mode ranges, the window-major sweep's left-out slices,
 * robust scan, overflows ...: the kPath* bits of csrc/find_kernels.h, mirrored in blurrily_amd/map.py).
 * Copies the words of the first n needles of the LAST such call.  The parity tests use it to compare
 * needles of every class row for row.  0, or -1 with errno EINVAL (no such call, n too large). */
int  blurrily_storage_find_path_flags(trigram_map haystack, uint32_t* out, size_t n);
/* The find kernels the LAST batched find on this map launched for its needles, in launch order, distinct names joined by
 * '+' (e.g. "find_kernel<uint8_t,1024,false,true,true>", "find_small_kernel+find_kernel<uint8_t,1024,false,true,false>",
 * "find_kernel<uint8_t,1024,false,true,false>+wsweep_kernel"): what a measured sweep choice actually ran, for a bench
 * line or a profile to name.  NUL-terminated into out[cap] (truncated to cap - 1); returns the untruncated length. */
size_t blurrily_storage_last_kernels(trigram_map haystack, char* out, size_t cap);

/* Tunables (no reference counterpart; nothing on the find path reads the environment).
 * Per map -- read by the map's next find; calls on one map are serial, as in the reference:
 *   "wsweep"          1 (default) / 0: whether the window-major sweep may be taken at all
 *   "ws_min_windows"  (8)     fewest windows of an image it is taken on
 *   "ws_min_slice"    (1550)  least mean postings a needle trigram finds per window for the sweep to be possible on
 *                             an image at all (such an image carries bitmaps of its dense slices)
 *   "ws_autotune"     (1)     which sweep serves a class of batches (limit up to / above 32; 129.. / 16 384.. / 65 536.. /
 *                             262 144.. needles) is MEASURED: the first such batch on an image runs every sweep it can
 *                             take -- needle-major, window-major, needle-major with dense slices left out of the count
 *                             -- TWICE, the better run counting (same rows; that one call waits for them, see
 *                             blurrily_storage_tune) and the fastest serves the class until the image is rebuilt or an
 *                             option changes; leaving slices out has to win by 3 %, the window-major sweep by 5 %.  The
 *                             choice is watched: two batches of the class in a row that run over 10 % slower per needle
 *                             than the measurement saw have the class measured again, at most once in sixteen batches
 *                             ("retunes", get: how often that happened).  0: the static rules below
 *   "ws_static_slice" (2200)  the static rule: window-major iff mean postings per window >= this, x1.7 for batches
 *                             under 65 536 needles, x1.7 for limits above 32, x4 for both (measured table)
 *   "ws_choice"       get: what has been measured (class c in bits 2c+1:2c: 0 not yet, 1 needle-major,
 *                             2 window-major, 3 needle-major with slices left out; classes 0..2: limits up to 32 by
 *                             batch size 16 384.. / 65 536.. / 262 144.., 3..5: the same for limits above 32, 6 / 7:
 *                             batches of 129 .. 16 383 needles, limits up to / above 32); set 0: forget it
 *   "tuned_class", "tuned_nm_us", "tuned_ws_us", "tuned_leave_us"   get: the class measured most recently (-1: none)
 *                             and what its three sweeps took, in microseconds (0: that sweep could not run)
 *   "last_sweep"      get: which sweep the last large batch took (1 / 2 / 3 as above, 4: the small-haystack sweep; 0: latency mode)
 *   "nm_cmin"         (3)     the needle-major sweep may leave the largest dense slices of a (needle, window) out of
 *                             the count -- at most need - nm_cmin of them, eight at most -- and settle the candidates
 *                             that leaves pending through the slices' bitmaps; 0: never.  Limits up to 149 (the candidate pool's tail
 *                             has to hold the settled candidates beside what a glance at the pool lets pass)
 *   "nm_dense"        (3072)  ... slices of at least this many postings only (not below "dense_min")
 *   "nm_min_windows"  (256)   ... and, where the choice is not measured, on images of at least this many windows
 *   "small_sweep"     (1)     an image of at most eight windows serves batches of at least "small_min_needles" (4096)
 *                             needles at limits up to 64 with four waves and one window's counters per needle -- four
 *                             needles per CU at a time instead of two ("last_sweep" 4); 0: never
 *   "devices"         (1)     replicate the device image on the first n visible devices (replica k on device (primary
 *                             + k) mod visible) and shard every batch of at least 1 024 x n needles contiguously over
 *                             them: blurrily_storage_find_batch and _find_batch_device alike -- the rows land in the
 *                             caller's buffers, the answer does not depend on n.  Replicas follow puts and deletes
 *   "ws_min_needles"  (16384) smallest batch it is taken for
 *   "ws_cmin"         (3)     counted matches a left-out slice must leave
 *   "dense_min"       (1024)  postings from which a (window, trigram) slice also exists as a bitmap; changing
 *                             it rebuilds the device image at the next find.  Bitmaps are part of the postings
 *                             array (2^32 slots at most): a value that would overflow it is doubled for that build
 *                             until the image fits (a line on stderr says so)
 *   "one_launch"      (1)     blurrily_storage_find as ONE launch without copies where it can be (see there); 0: always the
 *                             batch's way.  "one_taken" (get): finds served that way so far.  "one_windows_per_wg" (0): at
 *                             least this many windows per workgroup of that launch (0: as few as 256 workgroups allow)
 *   "few_max"         (24)    blurrily_storage_find_batch / _raw: batches of up to this many needles (128 at most) share
 *                             the single find's launch, a row of the grid per needle; "mid_workgroups" (1024): the
 *                             workgroups such a launch aims at from nine needles on (a workgroup then takes several
 *                             window pairs)
 *   "mid_max"         (128)   ... and batches of more than "few_max" and up to this many needles (128 at most; 0: none)
 *                             are searched in latency mode without copies: tokenised on the host, the needle arrays
 *                             read from a pinned page, the merged rows written back into it and polled there (two
 *                             launches; larger batches, limits above 120 and needles of more than 64 distinct
 *                             trigrams take the staged copies, the device's tokeniser and a stream synchronise)
 *   "latency_tasks"   (0)     latency mode (batches too small to give every resident workgroup a needle): the tasks a
 *                             needle's windows are cut into, aimed at per resident workgroup; 0: one up to 60 needles,
 *                             two beyond (measured at Geonames scale)
 *   "host_chunk"      (131072) blurrily_storage_find_batch / _raw: a batch of at least twice as many needles goes
 *                             in chunks of this many through a three-stream pipeline (needles in, search, rows
 *                             out overlap); 0 = always one piece
 * Process-wide -- `haystack` NULL:
 *   "host_threads"    (0 = hardware threads, at most 64) threads of put_many and of the device-image build
 *   "build_trace"     (0) wall time of the build stages on stderr
 * set: 0, or -1 with errno EINVAL (unknown key, value out of range).  get: the value in effect. */
int blurrily_storage_set_option(trigram_map haystack, const char* key, long long value);
int blurrily_storage_get_option(trigram_map haystack, const char* key, long long* value);

#ifdef __cplusplus
}
#endif
#endif /* BLURRILY_AMD_STORAGE_H */
