// host_batch.hip -- host-buffer batches: the chunked three-stream pipeline, the one-piece batch through pinned
// staging, and a handful of needles (or ONE, the caller waiting) in one launch without copies (find_few).
#include "find_few_layout.h"
#include "map_internal.h"

using namespace blurrily;
using namespace blurrily::detail;

constexpr size_t kStageBytes = 1 << 20;   // pinned staging per direction for small host-buffer batches

// A large host-buffer batch in chunks through three streams: while chunk k is searched (s_run), chunk k+1's
// needles travel to the device (s_in) and chunk k-1's rows travel back (s_out) -- both through pinned staging,
// which the host fills / drains meanwhile.  Two slots by turns; a slot is reused only after its rows have been
// copied out to the caller.  Each element is still exactly one blurrily_storage_find.
static int find_batch_chunked_run(trigram_map m, const char* packed, const uint64_t* offsets, size_t n, uint16_t limit,
                              trigram_match results, uint32_t* counts, bool raw, uint32_t* non_ascii, size_t chunk) {
  auto& P = m->pipe;
  for (Stream* s : {&P.s_in, &P.s_run, &P.s_out}) if (s->make() < 0) return -1;
  for (Events<2>* e : {&P.ev_in, &P.ev_run, &P.ev_out}) if (e->make(hipEventDisableTiming) < 0) return -1;
  // staging sizes: the largest chunk's bytes in (rebased offsets | needles) and out (counts | flags | rows)
  size_t max_packed = 0;
  for (size_t a = 0; a < n; a += chunk) {
    const size_t b = std::min(n, a + chunk);
    max_packed = std::max<size_t>(max_packed, size_t(offsets[b] - offsets[a]));
  }
  const BatchBlocks C(chunk, max_packed, limit, raw);           // (a short last chunk keeps the full chunk's layout)
  const size_t in_cap = C.in_bytes, out_cap = C.out_bytes;
  if (P.h_in_bytes < in_cap || P.h_out_bytes < out_cap) {
    BLURRILY_HIP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < 2; ++i) { P.h_in[i].reset(); P.h_out[i].reset(); }
    P.h_in_bytes = P.h_out_bytes = 0;
    for (int i = 0; i < 2; ++i)
      if (P.h_in[i].alloc(in_cap) < 0 || P.h_out[i].alloc(out_cap) < 0) return -1;
    P.h_in_bytes = in_cap; P.h_out_bytes = out_cap;
  }
  for (int i = 0; i < 2; ++i)
    if (P.d_in[i].reserve(in_cap, P.s_run) < 0 || P.d_out[i].reserve(out_cap, P.s_run) < 0) return -1;

  struct Span { size_t a, b; };
  Span in_slot[2] = {{0, 0}, {0, 0}};
  // rows of the chunk slot `i` holds, from pinned staging to the caller's buffers (behind its D2H)
  auto drain = [&](int i) -> int {
    const Span sp = in_slot[i];
    if (sp.b == sp.a) return 0;
    BLURRILY_HIP_TRY(hipEventSynchronize(P.ev_out[i]));
    const size_t c = sp.b - sp.a;
    const BatchBlocks::Out h = C.out(P.h_out[i]);
    std::memcpy(counts + sp.a, h.counts, c * sizeof(uint32_t));
    if (raw && non_ascii) std::memcpy(non_ascii + sp.a, h.flags, c * sizeof(uint32_t));
    if (limit) std::memcpy(results + sp.a * size_t(limit), h.rows, c * size_t(limit) * sizeof(trigram_match_t));
    in_slot[i] = {0, 0};
    return 0;
  };
  size_t k = 0;
  for (size_t a = 0; a < n; a += chunk, ++k) {
    const size_t b = std::min(n, a + chunk), c = b - a;
    const int i = int(k & 1);
    if (drain(i) < 0) return -1;                                  // chunk k-2: its staging and device blocks are free again
    // ---- stage chunk k: offsets rebased to the chunk, its needles; how long they can be --------------
    uint64_t* h_off = reinterpret_cast<uint64_t*>(P.h_in[i].h);
    const uint64_t base = offsets[a];
    for (size_t j = 0; j <= c; ++j) h_off[j] = offsets[a + j] - base;
    const size_t bytes = size_t(offsets[b] - base);
    if (bytes) std::memcpy(P.h_in[i] + C.o_packed, packed + base, bytes);
    const size_t max_len = longest_needle(packed + base, h_off, c);
    unsigned char* d_in = static_cast<unsigned char*>(P.d_in[i].p);
    unsigned char* d_out = static_cast<unsigned char*>(P.d_out[i].p);
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_in, P.h_in[i], C.o_packed + std::max<size_t>(bytes, 16), hipMemcpyHostToDevice, P.s_in));
    BLURRILY_HIP_TRY(hipEventRecord(P.ev_in[i], P.s_in));
    // ---- search it ---------------------------------------------------------------------------------
    BLURRILY_HIP_TRY(hipStreamWaitEvent(P.s_run, P.ev_in[i], 0));
    const BatchBlocks::In in = C.in(d_in);
    const BatchBlocks::Out out = C.out(d_out);
    if (raw && launch_normalise(in.packed, in.offsets, uint32_t(c), in.packed, out.flags, P.s_run) < 0) return -1;
    if (run_find(m, in.packed, bytes, in.offsets, c, limit, out.rows, out.counts, nullptr, max_len > 126, max_len > 63,
                 P.s_run) < 0)
      return -1;
    BLURRILY_HIP_TRY(hipEventRecord(P.ev_run[i], P.s_run));
    // ---- and send its rows home ----------------------------------------------------------------------
    BLURRILY_HIP_TRY(hipStreamWaitEvent(P.s_out, P.ev_run[i], 0));
    BLURRILY_HIP_TRY(hipMemcpyAsync(P.h_out[i], d_out, C.o_rows + c * size_t(limit) * sizeof(trigram_match_t),
                                    hipMemcpyDeviceToHost, P.s_out));
    BLURRILY_HIP_TRY(hipEventRecord(P.ev_out[i], P.s_out));
    in_slot[i] = {a, b};
  }
  if (drain(int(k & 1)) < 0 || drain(int((k + 1) & 1)) < 0) return -1;
  return 0;
}

static int find_batch_chunked(trigram_map m, const char* packed, const uint64_t* offsets, size_t n, uint16_t limit,
                              trigram_match results, uint32_t* counts, bool raw, uint32_t* non_ascii, size_t chunk) {
  m->class_hint = n;
  const int rc = find_batch_chunked_run(m, packed, offsets, n, limit, results, counts, raw, non_ascii, chunk);
  m->class_hint = 0;
  if (rc < 0) {                                       // chunks may still be in flight on the three streams: let them
    const int e = errno;                              // finish before anybody reuses the slots
    (void)hipDeviceSynchronize();
    errno = e;
  }
  return rc;
}

// Blurrily::Map#normalize_string (lib/blurrily/map.rb:40-47) for ONE ASCII needle on the host -- normalise_kernel's two
// passes, byte for byte (kernels/tokenise.inc: downcase; unless some line is [a-z ]+ every byte that is not a-z becomes a
// space; whitespace runs squeezed, both ends stripped, trailing NULs too): a handful of raw needles is normalised here
// and shares find_one_kernel's launch instead of paying a copy in, a normalising launch and the batch's way.  `out` holds
// at least `cap` bytes; returns the normalised length (up to the first NUL: where the tokeniser stops); *high: whether
// the needle held a byte >= 0x80 (flagged, not guessed: NFKD is the caller's).
size_t normalise_one(const char* in, size_t cap, char* out, uint32_t* high_out) {
  bool plain = false, line_ok = true;
  size_t line_len = 0;
  uint32_t high = 0;
  for (size_t k = 0; k < cap; ++k) {
    unsigned char c = static_cast<unsigned char>(in[k]);
    high |= c >> 7;
    if (c == '\n') { plain |= line_ok && line_len > 0; line_ok = true; line_len = 0; continue; }
    if (c >= 'A' && c <= 'Z') c += 'a' - 'A';
    line_ok &= (c >= 'a' && c <= 'z') || c == ' ';
    ++line_len;
  }
  plain |= line_ok && line_len > 0;
  size_t w = 0, keep = 0;
  bool gap = false;
  for (size_t k = 0; k < cap; ++k) {
    unsigned char c = static_cast<unsigned char>(in[k]);
    if (c >= 'A' && c <= 'Z') c += 'a' - 'A';
    const bool letter = c >= 'a' && c <= 'z';
    if (!plain && !letter) c = ' ';
    if (c == ' ' || (c >= '\t' && c <= '\r')) { gap = true; continue; }
    if (gap && w > 0) out[w++] = ' ';
    gap = false;
    out[w++] = static_cast<char>(c);
    if (c != 0) keep = w;
  }
  if (high_out) *high_out = high;
  return needle_len(out, keep);
}

namespace blurrily {
namespace detail {

size_t needle_len(const char* s, size_t cap) {
  const void* nul = std::memchr(s, 0, cap);
  return nul ? size_t(static_cast<const char*>(nul) - s) : cap;
}

size_t longest_needle(const char* packed, const uint64_t* offsets, size_t n) {
  size_t max_len = 0;
  for (size_t i = 0; i < n && max_len <= 126; ++i) {
    const size_t cap = size_t(offsets[i + 1] - offsets[i]);
    if (cap > max_len) max_len = std::max(max_len, needle_len(packed + offsets[i], cap));
  }
  return max_len;
}

BatchBlocks::BatchBlocks(size_t n, size_t packed_bytes_, uint16_t limit, bool flags)
    : off_bytes((n + 1) * sizeof(uint64_t)), packed_bytes(packed_bytes_), cnt_bytes(n * sizeof(uint32_t)),
      row_bytes(n * size_t(limit) * sizeof(trigram_match_t)),
      o_packed(align_up(off_bytes, 256)), in_bytes(o_packed + std::max<size_t>(packed_bytes, 16)),
      o_flags(align_up(cnt_bytes, 256)), o_rows(o_flags + (flags ? o_flags : 0)),
      out_bytes(o_rows + std::max<size_t>(row_bytes, 16)) {}

BatchBlocks::In BatchBlocks::in(unsigned char* base) const {
  return In{reinterpret_cast<const uint64_t*>(base), reinterpret_cast<char*>(base + o_packed)};
}
BatchBlocks::Out BatchBlocks::out(unsigned char* base) const {
  return Out{reinterpret_cast<uint32_t*>(base), reinterpret_cast<uint32_t*>(base + o_flags),
             reinterpret_cast<trigram_match>(base + o_rows)};
}
void BatchBlocks::fill_in(unsigned char* h_in, const char* packed, const uint64_t* offsets) const {
  std::memcpy(h_in, offsets, off_bytes);
  if (packed_bytes) std::memcpy(h_in + o_packed, packed, packed_bytes);
}
int BatchBlocks::copy_in(unsigned char* d_in, const char* packed, const uint64_t* offsets, hipStream_t stream) const {
  BLURRILY_HIP_TRY(hipMemcpyAsync(d_in, offsets, off_bytes, hipMemcpyHostToDevice, stream));
  if (packed_bytes)
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_in + o_packed, packed, packed_bytes, hipMemcpyHostToDevice, stream));
  return 0;
}
void BatchBlocks::take_out(const Out& h, uint32_t* counts, uint32_t* flags, trigram_match results) const {
  std::memcpy(counts, h.counts, cnt_bytes);
  if (flags) std::memcpy(flags, h.flags, cnt_bytes);
  if (row_bytes) std::memcpy(results, h.rows, row_bytes);
}
int BatchBlocks::copy_out(const uint32_t* d_counts, const uint32_t* d_flags, const trigram_match_t* d_rows,
                          uint32_t* counts, uint32_t* flags, trigram_match results, hipStream_t stream) const {
  BLURRILY_HIP_TRY(hipMemcpyAsync(counts, d_counts, cnt_bytes, hipMemcpyDeviceToHost, stream));
  if (flags) BLURRILY_HIP_TRY(hipMemcpyAsync(flags, d_flags, cnt_bytes, hipMemcpyDeviceToHost, stream));
  if (row_bytes) BLURRILY_HIP_TRY(hipMemcpyAsync(results, d_rows, row_bytes, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

// Host-buffer batch: needles in, rows out.  raw = the needles are un-normalised ASCII (see
// blurrily_storage_find_batch_raw); non_ascii (raw only, may be null) receives the per-needle flags.
int find_batch_host(trigram_map m, const char* packed, const uint64_t* offsets, size_t n, uint16_t limit,
                    trigram_match results, uint32_t* counts, bool raw, uint32_t* non_ascii) {
  if (n == 0) return 0;
  if (n <= std::max(m->one.few_max, m->one.mid_max)) { // a handful of needles: no copies (find_few; options "few_max", "mid_max")
    const char* s[kMidMaxNeedles];
    size_t len[kMidMaxNeedles];
    std::vector<char> norm;                             // raw needles: normalised here, as normalise_kernel would
    bool fits = true;
    if (raw) {
      if (offsets[n] - offsets[0] > (1u << 16)) fits = false;      // (a handful of very long needles: the batch's way)
      else norm.resize(size_t(offsets[n] - offsets[0]) + 1);
    }
    for (size_t i = 0; fits && i < n; ++i) {
      const size_t cap = size_t(offsets[i + 1] - offsets[i]);
      if (raw) {
        char* out = norm.data() + (offsets[i] - offsets[0]);
        uint32_t high = 0;
        len[i] = normalise_one(packed + offsets[i], cap, out, &high);
        s[i] = out;
        if (non_ascii) non_ascii[i] = high;
      } else {
        s[i] = packed + offsets[i];
        len[i] = needle_len(s[i], cap);
      }
    }
    if (fits) {
      const int few = find_few(m, s, len, n, limit, results, counts);
      if (few != kOneNotTaken) return few;
    }
  }
  DeviceScope scope(m->dev.device);
  // what the reference's find does first: tokenise, sort the needle's dirty buckets
  size_t max_len = 0;
  const bool any_dirty = m->host->dirty_buckets() != 0;
  std::vector<uint16_t> codes;
  for (size_t i = 0; i < n; ++i) {
    const char* s = packed + offsets[i];
    const size_t len = needle_len(s, size_t(offsets[i + 1] - offsets[i]));
    max_len = std::max(max_len, len);
    if (any_dirty && !raw) {
      codes.resize(len + 1);
      const int nt = tokenise(s, len, codes.data());
      for (int k = 0; k < nt; ++k) m->host->sort_bucket_if_dirty(codes[k]);
    }
  }
  // (raw needles are only normalised on the device: sort every dirty bucket, as the device entry does)
  if (any_dirty && raw) m->host->sort_dirty_buckets();
  if (ensure_device(m) < 0) return -1;
  // (timing and request counters describe ONE launch sequence: those runs stay in one piece)
  const bool multi = wants_multi(m, n);   // (the batch then goes in one piece through the primary: its rows come home over ONE PCIe link)
  if (!multi && m->host_chunk && n >= 2 * size_t(m->host_chunk) && !m->timing && !m->collect_stats) {
    size_t chunk = m->host_chunk;
    const size_t row_cap = size_t(32) << 20;                      // at most 32 MiB of rows per chunk in pinned staging
    while (chunk > 1024 && chunk * size_t(limit) * sizeof(trigram_match_t) > row_cap) chunk >>= 1;
    return find_batch_chunked(m, packed, offsets, n, limit, results, counts, raw, non_ascii, chunk);
  }

  hipStream_t stream = nullptr;
  const BatchBlocks B(n, size_t(offsets[n]), limit, raw);
  if (m->ws_io_in.reserve(B.in_bytes, stream) < 0 || m->ws_io_out.reserve(B.out_bytes, stream) < 0) return -1;
  unsigned char* d_in = static_cast<unsigned char*>(m->ws_io_in.p);
  unsigned char* d_out = static_cast<unsigned char*>(m->ws_io_out.p);
  const BatchBlocks::In in = B.in(d_in);
  const BatchBlocks::Out out = B.out(d_out);

  // Small batches (the single blurrily_storage_find above all) go through pinned staging: one
  // copy in, one copy out, instead of four pageable ones.
  const bool staged = B.in_bytes <= kStageBytes && B.out_bytes <= kStageBytes;
  if (staged && !m->h_stage && m->h_stage.alloc(2 * kStageBytes) < 0) return -1;
  if (staged) {
    B.fill_in(m->h_stage, packed, offsets);
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_in, m->h_stage, B.in_bytes, hipMemcpyHostToDevice, stream));
  } else if (B.copy_in(d_in, packed, offsets, stream) < 0) {
    return -1;
  }
  if (raw && launch_normalise(in.packed, in.offsets, uint32_t(n), in.packed, out.flags, stream) < 0) return -1;
  if ((multi ? run_find_multi(m, in.packed, B.packed_bytes, in.offsets, n, limit, out.rows, out.counts, nullptr, stream)
             : run_find(m, in.packed, B.packed_bytes, in.offsets, n, limit, out.rows, out.counts, nullptr, max_len > 126,
                        max_len > 63, stream)) < 0)
    return -1;
  if (!staged) return B.copy_out(out.counts, out.flags, out.rows, counts, raw ? non_ascii : nullptr, results, stream);
  unsigned char* h_out = m->h_stage + kStageBytes;
  BLURRILY_HIP_TRY(hipMemcpyAsync(h_out, d_out, B.out_bytes, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  B.take_out(B.out(h_out), counts, raw ? non_ascii : nullptr, results);
  return 0;
}

// ---- ONE needle, the caller waiting -- or a handful: one launch, no copies (find_kernels.hip: find_one_kernel) --------
// find_few, at the end, is the sequence; its steps stand here in its order.  The pinned page and the device lists it
// shares with the kernels are laid out in find_few_layout.h; what it decides is find_choice.h's arithmetic.
namespace {

constexpr FewPage  kPage(kOneMaxKeep, kMidMaxNeedles);
constexpr FewLists kLists(kOneMaxKeep, kOneMaxGrid, kOneMaxNeedles, kMidMaxNeedles);

// A call's needles -- tokenised, then compacted to the rows of the grid: the needles that have a posting -- and what the
// launches share.  (Declared without an initialiser: nothing clears the 16 KiB of codes.)
struct FewCall {
  trigram_map m;
  uint32_t    limit;
  uint16_t    codes[kMidMaxNeedles * 64];                          // [row][64]
  uint32_t    T[kMidMaxNeedles];
  uint32_t    row_of[kMidMaxNeedles], row_nb[kMidMaxNeedles], n_rows;   // a row's needle, its postings (saturated)
  uint32_t    ranges;                                              // latency mode's, on the base image (1: the shared launch)
  uint32_t    seq;
  bool mid() const { return ranges > 1; }
  // more rows than travel as kernel arguments: the shared launch reads the codes from the pinned page (both images' launches the first image's copy)
  bool far() const { return n_rows > kOneMaxNeedles; }
};

// false: a needle the launch does not take (more than 255 bytes, more than 64 distinct trigrams)
bool tokenise_needles(FewCall& c, const char* const* s, const size_t* len, size_t n) {
  uint16_t buf[256];
  for (size_t i = 0; i < n; ++i) {
    if (len[i] > 255) return false;
    const int t = tokenise(s[i], len[i], buf);              // tokeniser.c:59-119
    if (t > 64) return false;
    c.T[i] = uint32_t(t);
    std::memcpy(c.codes + i * 64, buf, size_t(t) * sizeof(uint16_t));
  }
  return true;
}

// what the reference's find does first: sort the needle's dirty buckets (storage.c:516), sum their sizes (:498-503: compact_rows)
void sort_dirty_buckets_of(const FewCall& c, size_t n) {
  if (!c.m->host->dirty_buckets()) return;
  for (size_t i = 0; i < n; ++i)
    for (uint32_t k = 0; k < c.T[i]; ++k) c.m->host->sort_bucket_if_dirty(c.codes[i * 64 + k]);
}

// needles without a posting return no rows (storage.c:503) and take no row of the grid; returns the rows
uint32_t compact_rows(FewCall& c, size_t n, uint32_t* counts) {
  uint32_t n_rows = 0;
  for (size_t i = 0; i < n; ++i) {
    uint64_t nb = 0;
    for (uint32_t k = 0; k < c.T[i]; ++k) nb += c.m->host->bucket(c.codes[i * 64 + k]).used;
    counts[i] = 0;
    if (nb == 0) continue;
    if (n_rows != i) { std::memmove(c.codes + n_rows * 64, c.codes + i * 64, 64 * sizeof(uint16_t)); c.T[n_rows] = c.T[i]; }
    c.row_nb[n_rows] = nb > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(nb);
    c.row_of[n_rows++] = uint32_t(i);
  }
  return c.n_rows = n_rows;
}

// On first use: stream, pinned page and its device address, built in locals and kept only when ALL of them exist (a
// half-made set -- a stream without its page -- would have the next find skip this step and poll a null page)
int make_page(trigram_map_t::One& O) {
  if (O.h_out) return 0;
  Stream st;
  HostPage h;
  unsigned char* d = nullptr;
  if (st.make() < 0 || h.alloc(2 * kPage.bytes, hipHostMallocMapped | hipHostMallocCoherent) < 0) return -1;
  BLURRILY_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&d), h, 0));
  std::memset(h, 0, 2 * kPage.bytes);
  O.stream = std::move(st); O.h_out = std::move(h); O.d_out = d;
  return 0;
}

// ... and both images' lists, zeroed once: every launch leaves tickets and queue at zero and the flags at a spent seq
int make_lists(trigram_map_t::One& O) {
  if (O.d_parts.p) return 0;
  if (O.d_parts.reserve(2 * kLists.bytes, O.stream) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemsetAsync(O.d_parts.p, 0, 2 * kLists.bytes, O.stream));
  return 0;
}

// Into the base image's page, each behind a release fence: latency mode's needle arrays -- what its tokeniser would have
// left on the device: postings, the window of the needle's own length class, where its codes start --, and the codes
// and trigram counts where they do not travel as kernel arguments.
void stage_needles(const FewCall& c, const size_t* len) {
  unsigned char* page = c.m->one.h_out;
  if (c.mid()) {
    uint32_t *h_nb = kPage.nb(page), *h_start = kPage.start(page);
    uint64_t* h_off = kPage.offsets(page);
    for (uint32_t r = 0; r < c.n_rows; ++r) {
      h_nb[r] = c.row_nb[r];
      h_start[r] = c.m->dev.h_start_win[std::min<size_t>(len[c.row_of[r]], 255)];   // (tokenise_kernel: start_win[len])
      h_off[r] = uint64_t(r) * 63;                          // a needle's codes start at qcodes + offsets[q] + q: [needle][64]
    }
    h_off[c.n_rows] = uint64_t(c.n_rows) * 63;
    __atomic_thread_fence(__ATOMIC_RELEASE);
  }
  if (c.far() || c.mid()) {
    std::memcpy(kPage.codes(page), c.codes, size_t(c.n_rows) * 64 * sizeof(uint16_t));
    std::memcpy(kPage.T(page), c.T, size_t(c.n_rows) * sizeof(uint32_t));
    __atomic_thread_fence(__ATOMIC_RELEASE);
  }
}

// what either launch on image `which` reads: the image, the limit, the deleted ranks
int few_args(const FewCall& c, const DeviceIndex& ix, const uint32_t* d_tomb, [[maybe_unused]] int which, FindArgs* a) {
  image_args(ix, a);
  a->limit = c.limit; a->keep = c.limit; a->pool_cap = 512;
  a->tomb = d_tomb;
#ifdef BLURRILY_TRACE
  if (c.m->d_phase.alloc(kPhaseWords) < 0) return -1;
  if (which == 0) a->phase_clocks = c.m->d_phase;        // (trace build: find_one_kernel's wall-clock marks, 16 per workgroup)
#endif
  return 0;
}

// More than few_max rows: the BASE image is searched in latency mode -- find_kernel<..., RANGED>, a needle's windows cut
// into ranges, a task per workgroup: beyond about thirty needles its pipelined steps beat find_one_kernel's exact
// selects -- but without the batch path's copies: the tasks read the needle arrays from the pinned
// page, over the link, and the merge writes rows, counts and sequence words back into it (merge_parts_pinned_kernel),
// where the host polls them as it does find_one_kernel's.  Two launches, no copy, no stream synchronise (the batch
// path: a copy in, the tokeniser, the find, the merge, a copy out, a synchronise).
int launch_latency(const FewCall& c, const uint32_t* d_tomb) {
  trigram_map m = c.m;
  auto& O = m->one;
  FindArgs a{};
  if (few_args(c, m->dev, d_tomb, 0, &a) < 0) return -1;
  unsigned char* lists = static_cast<unsigned char*>(O.d_parts.p);
  const size_t wgs = size_t(m->n_cus) * find_wgs_per_cu();
  const uint32_t tasks = c.n_rows * c.ranges;             // (<= kLists.max_lists: few_ranges)
  a.offsets = kPage.offsets(O.d_out); a.qcodes = kPage.codes(O.d_out); a.q_ntri = kPage.T(O.d_out);
  a.q_nb = kPage.nb(O.d_out); a.q_start = kPage.start(O.d_out);
  a.nm_dense = std::max((m->sweep.nm_dense + 7u) & ~7u, m->dev.dense_min8);
  a.nm_cmin = 0;                                          // (ranges leave nothing out of a step's count: measured, slower)
  a.n_work = tasks; a.ranges = c.ranges; a.short_only = 1;
  a.part_keys = kLists.keys(lists);
  a.part_count = kLists.mid_counts(lists);
  a.queue = kLists.queue(lists);
  a.pool_cap = find_pool_cap(c.limit);
  if (launch_find(a, false, uint32_t(std::min<size_t>(tasks, wgs)), O.stream) < 0) return -1;
  a.pool_cap = merge_pool_cap(c.ranges, c.limit);
  return launch_merge_parts_pinned(a, c.n_rows, kPage.rows(O.d_out), kPage.words(O.d_out), c.seq, O.stream);
}

// The shared launch on image `which` ([0] the base image, [1] the delta image of the pending puts: its own lists, flags,
// tickets and rows): find_one_kernel, a row of the grid per needle.
int launch_shared(const FewCall& c, const DeviceIndex& ix, const uint32_t* d_tomb, int which) {
  trigram_map m = c.m;
  auto& O = m->one;
  FindArgs a{};
  if (few_args(c, ix, d_tomb, which, &a) < 0) return -1;
  unsigned char* lists = kLists.image(static_cast<unsigned char*>(O.d_parts.p), which);
  unsigned char* page = kPage.image(O.d_out, which);
  const OneGrid g = one_grid(ix.n_windows, c.n_rows, O.mid_workgroups, O.min_per, kOneMaxGrid, kLists.max_lists);
  const bool far = c.far();
  return launch_find_one(a, c.codes, c.T, c.n_rows, g.per, g.grid, kLists.keys(lists), kLists.flags(lists), kPage.rows(page),
                         kPage.words(page), c.seq, O.stream, uint32_t(m->n_cus), far ? kPage.codes(O.d_out) : nullptr,
                         far ? kPage.T(O.d_out) : nullptr, far ? kLists.tickets(lists) : nullptr);
}

// A row's last store is its sequence word; the host polls the words in the pinned page instead of waiting for the
// runtime to notice the kernel's completion signal (an interrupt or a slower poll: 10 us and more).
int wait_for_rows(const trigram_map_t::One& O, uint32_t n_rows, int n_images, uint32_t seq) {
  uint64_t spins = 0;
  for (int which = 0; which < n_images; ++which) {
    volatile uint32_t* words = kPage.words(kPage.image(O.h_out, which));
    for (uint32_t r = 0; r < n_rows; ++r) {
      while (words[2 * r + 1] != seq) {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
        if ((++spins & 0xFFFFFu) == 0) {                  // every few milliseconds: is the stream still alive?
          const hipError_t q = hipStreamQuery(O.stream);
          if (q == hipSuccess && words[2 * r + 1] != seq) { std::fprintf(stderr, "blurrily_hip: find_one finished without its rows\n"); errno = EIO; return -1; }
          if (q != hipSuccess && q != hipErrorNotReady) { std::fprintf(stderr, "blurrily_hip: find_one: %s\n", hipGetErrorString(q)); errno = EIO; return -1; }
        }
      }
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return 0;
}

// The rows of the page to the caller: the base image's as they are, or a needle's two lists merged
void rows_out(const FewCall& c, bool with_delta, trigram_match results, uint32_t* counts) {
  unsigned char *page0 = kPage.image(c.m->one.h_out, 0), *page1 = kPage.image(c.m->one.h_out, 1);
  const volatile uint32_t *w0 = kPage.words(page0), *w1 = kPage.words(page1);
  const uint32_t limit = c.limit;
  for (uint32_t r = 0; r < c.n_rows; ++r) {
    const uint32_t i = c.row_of[r];
    trigram_match_t* out = results + size_t(i) * limit;
    if (with_delta) { counts[i] = merge_rows(kPage.rows(page0, r), w0[2 * r], kPage.rows(page1, r), w1[2 * r], limit, out); continue; }
    const uint32_t got = w0[2 * r], na = got < limit ? got : limit;
    counts[i] = na;
    std::memcpy(out, kPage.rows(page0, r), size_t(na) * sizeof(trigram_match_t));
  }
}

}  // namespace

// The reference's only call shape (ext/blurrily/map_ext.c:131-162 -> storage.c:477-580), and small host-buffer batches
// (a server's coalesced FINDs under light load).  needle i = s[i][0 .. len[i]) (up to its first NUL).  Returns 0 with
// counts[] and rows filled (results + i * limit), -1 with errno, or kOneNotTaken when the finds have to go the batch's
// way: a limit of 0 or above kOneMaxKeep, more than kMidMaxNeedles needles, a needle of more than 64 distinct trigrams,
// timing or request counters switched on, option "one_launch" 0.  Mutations the base image does not hold yet are
// served (DESIGN.md "Mutation and device sync"): deletes are tombstone bits the select looks at, pending puts live in a
// small delta image searched by a SECOND launch -- a window or two: always the shared launch --, and the two lists of a
// needle are merged here (they hold disjoint references).  A log that has overflowed is folded by ensure_device.
int find_few(trigram_map m, const char* const* s, const size_t* len, size_t n, uint16_t limit, trigram_match results,
             uint32_t* counts) {
  if (!m->one.enabled || limit == 0 || limit > kOneMaxKeep || n == 0 || n > kMidMaxNeedles || m->timing || m->collect_stats)
    return kOneNotTaken;
  FewCall c;
  c.m = m; c.limit = limit;
  if (!tokenise_needles(c, s, len, n)) return kOneNotTaken;
  DeviceScope scope(m->dev.device);
  sort_dirty_buckets_of(c, n);
  if (ensure_device(m) < 0) return -1;
  const bool with_tomb = log_of(m)->n_tomb != 0, with_delta = !log_of(m)->pending.empty() && m->delta.device >= 0;
  if (compact_rows(c, n, counts) == 0) return 0;
  auto& O = m->one;
  NameScope name_scope(&m->last_kernels);                 // (the launches below note their kernels' names in the map)
  m->last_kernels.clear();
  m->last_sweep = 0;                                      // (no sweep of a class of batches: a single launch, or latency mode)
  if (make_page(O) < 0) return -1;
  if (with_tomb && apply_tombstones(m, O.stream) < 0) return -1;       // (deletes since the last find: their bits are set first)
  if (make_lists(O) < 0) return -1;
  c.ranges = few_ranges(c.n_rows, O.few_max, O.mid_max, limit, m->dev.n_windows, size_t(m->n_cus) * find_wgs_per_cu(),
                        m->latency_tasks, kLists.max_lists);
  stage_needles(c, len);
  c.seq = ++O.seq ? O.seq : ++O.seq;                      // (never 0: what the words hold before the first find)
  const uint32_t* d_tomb = with_tomb ? m->dev.d_tomb : nullptr;
  if ((c.mid() ? launch_latency(c, d_tomb) : launch_shared(c, m->dev, d_tomb, 0)) < 0) return -1;
  if (with_delta && launch_shared(c, m->delta, nullptr, 1) < 0) return -1;
  if (wait_for_rows(O, c.n_rows, with_delta ? 2 : 1, c.seq) < 0) return -1;
  rows_out(c, with_delta, results, counts);
  O.taken += c.n_rows;
  return 0;
}

}  // namespace detail
}  // namespace blurrily
