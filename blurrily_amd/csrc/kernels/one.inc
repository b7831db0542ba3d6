// kernels/one.inc -- one needle, now: find_one_kernel (blurrily_storage_find in one launch).
// Part of find_kernels.hip (included inside namespace blurrily, BLURRILY_KERNELS_BEGIN, the anonymous namespace).
// ============================================================ one needle, now ==================
// blurrily_storage_find -- the reference's only call shape (ext/blurrily/map_ext.c:131-162, bin/bench:93-95): ONE
// needle, the caller waiting.  Through round 4 it went the batch's way: a staged copy in, tokenise_wave_kernel,
// find_kernel in latency mode, merge_parts_small_kernel, a copy out, a stream synchronise -- six operations, each a
// packet the command processor orders behind the one before (68 us at Geonames scale, 39 of them the find kernel's:
// queue pop, needle scalars, codes, a learning sweep of the needle's own length class, then its own range).  Here it
// is ONE launch and no copy:
//   * the host tokenises (csrc/tokeniser.h: what put() runs) and passes the needle's codes AS KERNEL ARGUMENTS;
//   * workgroup g owns windows [g * per, (g + 1) * per) -- one window each at Geonames scale, so every workgroup runs
//     exactly ONE step: slice table (every wave its own copy, lane t = trigram t), the wave's units with four loads
//     in flight (a workgroup is alone on its CU: 128 VGPRs), count, barrier, select -- no queue, no learning sweep,
//     no ring;
//   * SELECT takes a window's best `keep` counters EXACTLY, whatever ties it holds (one_select): every thread reads
//     its four vectors of counters once; a bisection over the counter value IN REGISTERS finds the largest c that at
//     least `keep` counters reach; counters above c enter the pool, and of the counters AT c only the lowest ranks
//     that are still missing -- found by a prefix count in rank order (wave w owns a contiguous 4 KiB of counters).
//     A window of thousands of identical strings -- thousands of counters tied at the bound, the common case of a
//     needle made of popular words -- therefore costs what any window costs; admitting every tie, overflowing the
//     pool and sweeping the window again (scan_window's way, made for a sweep that arrives with a threshold) took
//     30 us in such windows, measured;
//   * a workgroup leaves its best `keep` keys in global memory and sets its flag; the grid's LAST workgroup waits for
//     the flags, loads all the lists at once, keeps the keys not above the keep-th smallest list head, sorts those few, looks the
//     references and weights up and writes rows, count and a sequence word straight into host-coherent pinned
//     memory, where the host thread is polling.
// Same answer by construction: every posting of every window counted, a window's best `keep` candidates that beat the
// workgroup's threshold taken exactly, the best `keep` of the union of per-workgroup best `keep` lists (nothing can be
// lost).  Served: needles of at most 64 distinct trigrams, limits up to kOneMaxKeep, images without tombstones or
// pending puts (host_batch.hip: find_few); everything else goes the batch's way as before.
constexpr uint32_t kOnePool = 512;
constexpr int      kOneThreads = 1024;                   // (512 -- eight waves, 256 VGPRs each -- measured: 35.4 against 33.5 us)
constexpr uint32_t kOneAhead = 4;                        // units a wave loads before it counts the first of them

// find_one_kernel's third counter layout: ONE window in 4-bit counters, 32 KiB -- wsweep_kernel's (ws_bump_pair_nib: word
// (r >> 2) & 0x1FFF, nibble (r & 3) | (r >> 15) << 2: the low nibbles of a word hold ranks 4 w .. 4 w + 3 of the window's
// lower half, the high ones ranks 32768 + 4 w ..).  A workgroup that owns a single window (every workgroup up to 256
// windows) then reads and selects over 2 048 vectors instead of the pair layout's 4 096, half of whose nibbles it would
// never touch: the select is VALU work per word (bisection 4.5 us, ties 4 us of a find's 31 at Geonames scale).
struct Nib1 {};
template <> struct Packing<Nib1> : Packing<Nib> {};
template <> struct ScanTraits<Nib1> : ScanTraits<Nib> {
  static constexpr uint32_t kVecs = kWsCntWords / 4;                // 2 048
  static constexpr uint32_t kHalf = 32768;
  // vector i holds ranks 16 i .. 16 i + 15 of the lower half and kHalf + 16 i .. of the upper half
  static __device__ __forceinline__ uint32_t nvec(uint32_t wlen) { return (min(wlen, kHalf) + 15) / 16; }
  // counter index = 8 * word + nibble
  static __device__ __forceinline__ uint32_t rank_of(uint32_t wbase, uint32_t idx) {
    return wbase + ((idx >> 3) << 2) + (idx & 3u) + ((idx >> 2) & 1u) * kHalf;
  }
  // slot 0xFFFF -- the padding -- is the top nibble of the last word: cleared here where the scan does not reach it,
  // masked by the select where it does (a full window)
  static __device__ __forceinline__ void clear_unreached_pad(uint4* cnt128, uint32_t nv, uint32_t tid) {
    if (nv < kVecs && tid == 0) reinterpret_cast<uint32_t*>(cnt128)[kVecs * 4 - 1] = 0;
  }
};

// this wave's units of one step: lane t holds trigram t's slice of the step's (even) window (a0, b0) and, with 4-bit
// counters, of the odd one (a1, b1); unit k of the step belongs to wave k mod 16
template <typename CT, int NT>
__device__ __forceinline__ void one_count(const uint16_t* __restrict__ ent, uint32_t* cnt32, const uint32_t a0,
                                          const uint32_t b0, const uint32_t a1, const uint32_t b1, const uint32_t wid,
                                          const uint32_t lane) {
  constexpr bool kNib = std::is_same<CT, Nib>::value;
  constexpr uint32_t kNW = NT / 64;
  const uint32_t units0 = slice_units(a0, b0), units1 = kNib ? slice_units(a1, b1) : 0u;
  const uint32_t incl = wave_inclusive_sum(units0 + units1);
  const uint32_t total = __builtin_amdgcn_readlane(incl, 63);
  const uint32_t excl = incl - units0 - units1;
  for (uint32_t k0 = wid; k0 < total; k0 += kOneAhead * kNW) {
    uint4 v[kOneAhead];
    uint32_t half[kOneAhead];
#pragma unroll
    for (uint32_t i = 0; i < kOneAhead; ++i) {
      const uint32_t k = k0 + i * kNW;
      v[i] = make_uint4(kPadPair, kPadPair, kPadPair, kPadPair);
      half[i] = 0;
      if (k < total) {                                   // (uniform)
        const uint32_t t = uint32_t(__builtin_ctzll(__ballot(incl > k)));
        const uint32_t ji = k - __builtin_amdgcn_readlane(excl, t), u0 = __builtin_amdgcn_readlane(units0, t);
        const bool odd = ji >= u0;
        const uint32_t start = odd ? __builtin_amdgcn_readlane(a1, t) + (ji - u0) * 512u
                                   : __builtin_amdgcn_readlane(a0, t) + ji * 512u;
        const uint32_t end = odd ? __builtin_amdgcn_readlane(b1, t) : __builtin_amdgcn_readlane(b0, t);
        half[i] = odd ? 1u : 0u;
        v[i] = load_group(ent, start + lane * 8, end);
      }
    }
#pragma unroll
    for (uint32_t i = 0; i < kOneAhead; ++i) {
      if constexpr (std::is_same<CT, Nib1>::value) ws_bump8<false>(cnt32, v[i], 0u);
      else bump_unit<CT>(cnt32, v[i], half[i]);
    }
  }
}

// The window's counters are complete: take its best `keep` candidates that beat the threshold -- EXACTLY that many at
// most, whatever ties there are -- into the pool, and clear the counters.  Wave w owns vectors [256 w, 256 w + 256) of
// the 4 096 (lane l its j-th round's vector 256 w + 64 j + l: conflict-free reads, and (w, j, l) ascending is rank
// ascending inside a window -- with 4-bit counters inside each of the pair's two windows, the even one's ranks first).
struct OneShared {
  uint32_t tally[12];           // the bisection's tallies, one per pass and bound
  uint32_t above[16], tie0[16];  // per wave: counters above the bound, counters at it (even | odd window << 16, clamped)
};
template <typename CT, int NT>
__device__ __forceinline__ void one_select(const FindArgs& A, uint4* cnt128, const uint32_t T, const uint32_t keep, Control* ctl,
                                           unsigned long long* pool, OneShared* sh, const uint32_t wbase,
                                           const uint32_t wlen) {
  using S = ScanTraits<CT>;
  using P = Packing<CT>;
  constexpr bool kNib1 = std::is_same<CT, Nib1>::value;             // one window, 4-bit: lower half in a word's low nibbles
  constexpr bool kNib = std::is_same<CT, Nib>::value || kNib1;       // two rank ranges per word (a pair's windows / a window's halves)
  constexpr uint32_t kNW = NT / 64, kR = S::kVecs / NT;      // rounds: a wave owns kR * 64 consecutive vectors
  static_assert(kNW * kR * 64 == S::kVecs && kR >= 1 && kNW <= 16, "the waves share the vectors evenly");
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint32_t nvec = S::nvec(wlen);
  uint4 v[kR];
#pragma unroll
  for (uint32_t j = 0; j < kR; ++j) {
    const uint32_t i = (wid * kR + j) * 64 + lane;
    v[j] = make_uint4(0, 0, 0, 0);
    if (i < nvec) v[j] = cnt128[i];
  }
#pragma unroll
  for (uint32_t j = 0; j < kR; ++j) {                    // cleared at once: the rest works on the registers
    const uint32_t i = (wid * kR + j) * 64 + lane;
    if (i < nvec) cnt128[i] = make_uint4(0, 0, 0, 0);
  }
  S::clear_unreached_pad(cnt128, nvec, tid);
  if (kNib1) {                                           // (the padding's nibble, where the scan reaches it)
#pragma unroll
    for (uint32_t j = 0; j < kR; ++j)
      if ((wid * kR + j) * 64 + lane == S::kVecs - 1) v[j].w &= 0x0FFFFFFFu;
  }
  if (A.tomb) {
    // References deleted since the image was built (storage.c:584-612) must not take a place: their counters go to zero
    // in the registers, before anything is counted.  Vector i holds the byte cells of in-window ranks 16 i .. 16 i + 15
    // -- of BOTH windows of a pair with 4-bit counters (even window: low nibbles) --, byte 3 - (r & 3) of word (r >> 2) & 3:
    // sixteen tombstone bits per window, aligned (a window starts at a multiple of sixteen ranks).
    static_assert(kWindowRanks % 16 == 0, "a vector's tombstone bits sit in one half of one word");
#pragma unroll
    for (uint32_t j = 0; j < kR; ++j) {
      const uint32_t i = (wid * kR + j) * 64 + lane;
      if (i >= nvec) continue;
      const uint32_t r0 = wbase + 16 * i, r1 = r0 + (kNib1 ? 32768u : kWindowRanks);
      const uint32_t dead0 = r0 < A.n_refs ? (A.tomb[r0 >> 5] >> (r0 & 31u)) & 0xFFFFu : 0u;
      const uint32_t dead1 = kNib && r1 < A.n_refs ? (A.tomb[r1 >> 5] >> (r1 & 31u)) & 0xFFFFu : 0u;
      if ((dead0 | dead1) == 0) continue;
      uint32_t d[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        // rank 4 k + b of the vector is dead: byte 3 - b of word k goes (one window: nibble b, and 4 + b for the upper
        // half).  The four bits of a word are spread by arithmetic -- no table of masks, which the compiler would keep
        // in registers for the kernel's life (that was the kernel's one spilled VGPR).
        const uint32_t n0 = (dead0 >> (4 * k)) & 0xFu, n1 = (dead1 >> (4 * k)) & 0xFu;
        uint32_t gone;
        if (kNib1) {
          auto nibbles = [](uint32_t n) {                // bit b -> bit 4 b
            n = (n | (n << 6)) & 0x0303u;
            return (n | (n << 3)) & 0x1111u;
          };
          gone = (nibbles(n0) | (nibbles(n1) << 16)) * 0xFu;
        } else {
          auto bytes = [](uint32_t n) {                  // bit b -> bit 8 (3 - b): reversed, then bit j -> bit 8 j (no two partial products meet)
            return ((__brev(n) >> 28) * 0x00204081u) & 0x01010101u;
          };
          gone = kNib ? bytes(n0) * 0x0Fu | bytes(n1) * 0xF0u : bytes(n0) * 0xFFu;
        }
        d[k] &= ~gone;
      }
      v[j] = make_uint4(d[0], d[1], d[2], d[3]);
    }
  }
  // counters of this thread that reach `bound`
  auto reach = [&](const uint32_t bound) {
    const typename S::Need nq = S::prepare(bound);
    uint32_t n = 0;
#pragma unroll
    for (uint32_t j = 0; j < kR; ++j)
      n += __popc(S::hits(v[j].x, nq)) + __popc(S::hits(v[j].y, nq)) + __popc(S::hits(v[j].z, nq)) + __popc(S::hits(v[j].w, nq));
    return n;
  };
  uint32_t pass = 0;
  auto tally = [&](const uint32_t bound) {               // the workgroup's counters that reach `bound` (one barrier)
    const uint32_t incl = wave_inclusive_sum(reach(bound));
    if (lane == 63 && incl) atomicAdd(&sh->tally[pass], incl);
    __syncthreads();
    return sh->tally[pass++];
  };
  // the bound a counter has to reach to beat the threshold (1: no threshold yet); c: the largest value >= that bound
  // which at least `keep` counters reach -- or the bound itself, with fewer reaching it: then all of them are taken
  const unsigned long long thr = ctl->thr;
  const uint32_t cap = min(T, S::kMaxCount);
  uint32_t lo = matches_needed(thr, T, wbase), hi = cap;
  bool all = false;
  if (lo > cap) {
    all = true; lo = cap + 1;                            // nothing of this window can enter
  } else if (tally(lo) < keep) {
    all = true;
  } else {
    // (The bound read off a histogram the COUNT keeps -- find_small_kernel's cold start, ws_bump8_hist, a row per wave --
    // measured here: median workgroup's count 3.2 -> 3.8 us, the SLOWEST's count barrier 5.0 -> 8.2 us -- windows where
    // thousands of postings meet a counter at work queue on a handful of histogram words -- and the find's p50 28.4 ->
    // 31.5 us, p90 33 -> 89.  The bisection's five passes cost every workgroup the same 3 us; left as it is.)
    while (lo < hi) {                                    // (at most seven passes with byte counters, four with 4-bit ones)
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (tally(mid) >= keep) lo = mid; else hi = mid - 1;
    }
  }
  const uint32_t c = lo;
  ONE_MARK(A, 6);
  // per lane and round: counters above c, counters AT c in the even / odd window
  const typename S::Need at_c = S::prepare(min(c, cap)), above_c = S::prepare(min(c + 1, S::kMaxCount));
  const bool has_above = c + 1 <= cap, none = c > cap;
  // a field's top bit, by window of the pair (by half of the one window)
  constexpr uint32_t kEven = kNib1 ? 0x00008888u : kNib ? 0x08080808u : 0x80808080u, kOdd = kNib1 ? 0x88880000u : kNib ? 0x80808080u : 0u;
  auto masks = [&](const uint32_t wv, uint32_t& up, uint32_t& tie) {
    const uint32_t r = none ? 0u : S::hits(wv, at_c);
    up = has_above ? S::hits(wv, above_c) : 0u;
    tie = all ? 0u : r & ~up;
    if (all) up = r;                                     // (fewer than keep reach the bound: every one of them is taken)
  };
  // per lane and round j: ties of the even window in bits 15:0, of the odd one in bits 31:16 (at most 16 each: one
  // inclusive sum serves both); whether the round holds anything above the bound: bit j of up_rounds
  uint32_t n_up = 0, up_rounds = 0, nt[kR];
#pragma unroll
  for (uint32_t j = 0; j < kR; ++j) {
    const uint32_t d[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
    uint32_t ups = 0;
    nt[j] = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      uint32_t up, tie;
      masks(d[k], up, tie);
      ups += __popc(up);
      nt[j] += __popc(tie & kEven) + (kNib ? __popc(tie & kOdd) << 16 : 0u);
    }
    n_up += ups;
    up_rounds |= ups ? 1u << j : 0u;
  }
  uint32_t in[kR];                                      // inclusive sums over the lanes, per round (both windows, packed)
#pragma unroll
  for (uint32_t j = 0; j < kR; ++j) in[j] = wave_inclusive_sum(nt[j]);
  const uint32_t up_incl = wave_inclusive_sum(n_up);
  if (lane == 63) {
    // (a wave's ties: at most 4 096 per window; published clamped to 2 047 -- sixteen waves' sum then stays inside 16
    // bits, and a clamped figure is still at least any quota, which is all a prefix has to tell)
    uint32_t tot = 0;
#pragma unroll
    for (uint32_t j = 0; j < kR; ++j) tot += in[j];
    sh->above[wid] = up_incl;
    sh->tie0[wid] = min(tot & 0xFFFFu, 2047u) | (min(tot >> 16, 2047u) << 16);   // (a lane-63 figure: the wave's)
  }
  __syncthreads();
  // what lies in front of this wave: lanes 0..15 hold the sixteen waves' figures
  const uint32_t wa = lane < kNW ? sh->above[lane] : 0u, wt = lane < kNW ? sh->tie0[lane] : 0u;
  const uint32_t ia = wave_inclusive_sum(wa), it = wave_inclusive_sum(wt);
  const uint32_t n_above = __builtin_amdgcn_readlane(ia, kNW - 1), n_tie0 = __builtin_amdgcn_readlane(it, kNW - 1) & 0xFFFFu;
  const uint32_t quota = all ? 0u : keep - min(keep, n_above);            // ties still wanted, lowest ranks first
  const uint32_t front = __builtin_amdgcn_readlane(it, wid) - __builtin_amdgcn_readlane(wt, wid);   // ties in front of this wave, packed
  uint32_t run0 = front & 0xFFFFu;                       // even-window ties in front of this wave
  uint32_t run1 = n_tie0 + (front >> 16);                // odd-window ties: behind ALL even ones
  auto admit = [&](const uint32_t cnt, const uint32_t rank) {
    const unsigned long long key = (static_cast<unsigned long long>(T - cnt) << 32) | rank;
    if (key <= thr) {                                    // (the bound came from the threshold's match count; its rank decides ties with it)
      const uint32_t at = atomicAdd(&ctl->pool_n, 1u);
      if (at < kOnePool) pool[at] = key;                 // (at most keep + keep keys: never full)
    }
  };
#pragma unroll
  for (uint32_t j = 0; j < kR; ++j) {
    const uint32_t i = (wid * kR + j) * 64 + lane;
    const uint32_t d[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
    const uint32_t mine_ex = in[j] - nt[j];              // this lane's ties of the round come behind these (packed)
    uint32_t at0 = run0 + (mine_ex & 0xFFFFu), at1 = run1 + (mine_ex >> 16);
    const uint32_t round_tot = __builtin_amdgcn_readlane(in[j], 63);
    run0 += round_tot & 0xFFFFu;
    run1 += round_tot >> 16;
    // (a lane with nothing above the bound and all of its ties behind the quota -- nearly every lane of a window of
    // thousands of ties -- has nothing to admit)
    if (!((up_rounds >> j) & 1u) && !((nt[j] & 0xFFFFu) && at0 < quota) && !(kNib && (nt[j] >> 16) && at1 < quota)) continue;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      uint32_t up, tie;
      masks(d[k], up, tie);
      // ties in rank order: inside a word the byte positions DESCEND with the rank (one window: the nibbles ascend)
      uint32_t m = at0 < quota ? tie & kEven : 0u;       // (behind the quota: nothing of this lane's any more)
      while (m) {
        const uint32_t bit = kNib1 ? __ffs(m) - 1u : 31u - __clz(m);
        m &= ~(1u << bit);
        if (at0++ < quota) {
          const uint32_t pos = bit / P::kBits;
          admit((d[k] >> (pos * P::kBits)) & P::kMask, S::rank_of(wbase, (i * 4 + k) * P::kPerWord + pos));
        }
      }
      if (kNib) {
        m = at1 < quota ? tie & kOdd : 0u;
        while (m) {
          const uint32_t bit = kNib1 ? __ffs(m) - 1u : 31u - __clz(m);
          m &= ~(1u << bit);
          if (at1++ < quota) {
            const uint32_t pos = bit / P::kBits;
            admit((d[k] >> (pos * P::kBits)) & P::kMask, S::rank_of(wbase, (i * 4 + k) * P::kPerWord + pos));
          }
        }
      }
      while (up) {
        const uint32_t bit = __ffs(up) - 1;
        up &= up - 1;
        const uint32_t pos = bit / P::kBits;
        admit((d[k] >> (pos * P::kBits)) & P::kMask, S::rank_of(wbase, (i * 4 + k) * P::kPerWord + pos));
      }
    }
  }
  __syncthreads();
  if (tid < 12) sh->tally[tid] = 0;
}

// one step of a workgroup's windows: windows [w, w_end) of ONE pair (4-bit counters: both windows of the pair count
// in one byte's nibbles, wbase is the even window's) or the one window w (byte counters)
template <typename CT, int NT>
__device__ __forceinline__ void one_step(const FindArgs& A, const uint32_t T, const uint32_t code, uint32_t* cnt32,
                                         unsigned long long* pool, Control* ctl, OneShared* sh, const uint32_t w,
                                         const uint32_t w_end) {
  constexpr bool kNib = std::is_same<CT, Nib>::value;      // (Nib1: one window, like the byte counters)
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint32_t w_even = kNib ? (w & ~1u) : w;
  uint32_t a0 = 0, b0 = 0, a1 = 0, b1 = 0;
  if (lane < T) {
    if (!kNib || w == w_even) { const uint2 se = A.slice_se[size_t(w_even) * kNumCodes + code]; a0 = se.x; b0 = se.y; }
    if (kNib && w_even + 1 >= w && w_even + 1 < w_end) {
      const uint2 se = A.slice_se[size_t(w_even + 1) * kNumCodes + code]; a1 = se.x; b1 = se.y;
    }
  }
  if ((__ballot(b0 > a0) | __ballot(b1 > a1)) == 0) return;     // nothing of the needle in these windows (uniform)
  ONE_MARK(A, 2);
  const uint32_t wbase = w_even * kWindowRanks;
  const uint32_t wlen = min((kNib ? 2u : 1u) * kWindowRanks, A.n_refs - wbase);
  one_count<CT, NT>(A.ent, cnt32, a0, b0, a1, b1, wid, lane);
  ONE_MARK(A, 3);
  __syncthreads();
  ONE_MARK(A, 4);
  one_select<CT, NT>(A, reinterpret_cast<uint4*>(cnt32), T, A.keep, ctl, pool, sh, wbase, wlen);
  ONE_MARK(A, 5);
  // keep the best `keep` of what the pool holds now (at most twice that); the threshold follows
  compact_pool<NT>(pool, ctl, kOnePool, A.keep);
}

struct OneArgs {
  uint16_t codes[kOneMaxNeedles][64];   // a needle's distinct trigram codes, ascending (tokeniser.c:59-119, by the host)
  uint32_t T[kOneMaxNeedles];           // how many
  // more than kOneMaxNeedles needles (a server's coalesced FINDs: up to kMidMaxNeedles): codes [needle][64] and counts in
  // host-coherent pinned memory, read over the link by every workgroup of the needle's row (132 bytes) -- still no copy
  // and one launch; nullptr: the arrays above
  const uint16_t* codes_far;
  const uint32_t* T_far;
  // ... and a row's lists are then merged by the workgroup that leaves its list LAST (a ticket per row, zero between
  // launches) instead of by the row's last workgroup spinning on the others' flags: a grid of a thousand workgroups is
  // more than the chip holds at once, and a spinner must not depend on the order they are dispatched in.  (A single
  // needle keeps the flags: 129 tickets on one word are performed one after the other at the memory side, 13 us.)
  uint32_t* tickets;
  uint32_t per;                  // windows per workgroup
  unsigned long long* part_keys; // [needle][grid.x * keep]: a workgroup's best keys ascending, padded with kKeyInf
  uint32_t* flags;               // [needle][grid.x] workgroup g's list is complete: the launch's sequence word
  trigram_match_t* out_rows;     // host-coherent pinned memory: [needle][kOneMaxKeep]
  uint32_t* out_count;           //   ... [needle][2]: rows, the sequence word (written last)
  uint32_t seq;
};

// find_one_kernel's last workgroup: the best `keep` of the G lists of `keep` slots (its own, the last, still in its pool)
// into `pool` (the head of s_counters), unsorted.
// A list is sorted, a key is level << 32 | rank with level = T - matches, and list g's windows lie in front of list
// g + 1's: LOWER ranks.  The union's order is therefore: by level, inside a level by list, inside a list by place -- and
// its best `keep` are every key of a level below L, the first level at which the levels' sizes add up to `keep`, plus
// the first keep - (keys below L) keys of level L in list order: of every list a PREFIX.  Nothing is sorted to find them:
//   * every slot's LEVEL goes to LDS as a byte (the lists' padding, kKeyInf, counts as one more level): all of a
//     thread's loads of a round in flight at once, one global round trip per 8 192 slots;
//   * for every (list, level l = 1 .. T) the place where the list's levels reach l -- a binary search over the list's
//     bytes, a wave per level, a lane per list; their sum over the lists is the number of keys BELOW level l, which
//     gives L, and the places themselves say where a list's keys of level L start and end: work per (list, level),
//     not per slot (a walk over the slots, however lean, costs the VALU 12 900 x 25 instructions at Geonames scale and
//     limit 100: 2 us a pass);
//   * one wave's prefix sums over the lists turn the places into the length of every list's passing prefix and its
//     offset in the output; output slot i finds its (list, place) by a binary search over the offsets and loads that key.
// Exactly min(keep, keys there are) keys arrive, and are put in order by counting, for every key, the keys below it --
// eight threads per key, each over an eighth of the keys, all of its reads in flight at once (compact_pool's rank count,
// made for pools that change under a sweep, walks them in a dependent loop of two keys a read: 4 us for 100 keys on
// the two waves that hold them).
// (Through round 5's first version: the keys not above the keep-th smallest list head, and of those the ones at place p
// of a list with r smaller heads in front where r + p < keep -- up to keep (keep + 1) / 2 keys, sorted by compact_pool's
// bitonic network: 32 us at Geonames scale and limit 100, 64 us on a haystack of massive ties, of a find's 70 and 104.
// Before that, one wave advancing one list per round: a dependent load from memory per row.  And a version of THIS
// merge with a thread's slots in registers, an unrolled loop over the 30 of the largest grid times the largest limit
// with a uniform skip per unused slot: every jump was an instruction-cache miss, 3 us at limit 10 -- this code runs
// once per launch, cold: its loops are rolled.)
template <int NT>
__device__ __forceinline__ void one_merge(const FindArgs& A, const unsigned long long* part_keys, uint32_t* s_counters,
                                          const unsigned long long* s_pool, Control* ctl, const uint32_t nres,
                                          const uint32_t T, const uint32_t keep, const uint32_t g, const uint32_t G,
                                          const bool own_in_memory = false) {
  (void)A;                                                             // (the trace build's marks)
  constexpr uint32_t kPadLevel = 64;                                   // (a needle's levels: 0 .. T - 1 <= 63)
  constexpr uint32_t kRound = 8, kNW = NT / 64;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t* const w32 = s_counters;                                    // (the counters are done with)
  unsigned long long* const pool = reinterpret_cast<unsigned long long*>(w32);   // [kOnePool]
  uint32_t* const below = w32 + 2 * kOnePool;                          // [128] keys of a level below l, l = 1 .. T
  constexpr uint32_t kPerLane = (kOneMaxGrid + 63) / 64, kOffN = 64 * kPerLane;   // lists per lane of the one wave that sums them
  uint32_t* const off = below + 128;                                   // [kOffN] where a list's passing prefix starts in the output
  uint32_t* const place = off + kOffN;                                 // [128] an arriving key's place in the output order
  unsigned char* const reach = reinterpret_cast<unsigned char*>(place + 128);   // [65][kOneMaxGrid] the place where a list's levels reach l
  unsigned char* const lvl = reach + 65 * kOneMaxGrid;                 // [G * keep] a slot's level
  static_assert((2 * kOnePool + 128 + kOffN + 128) * 4 + 65 * kOneMaxGrid + kOneMaxGrid * kOneMaxKeep <= kWindowSize &&
                kOnePool >= kOneMaxKeep && kOneMaxKeep <= 128 && NT % 128 == 0, "merge scratch");
  // (this workgroup's own list -- the last -- comes from its pool; merging by ticket, every list lies in memory)
  const uint32_t total = G * keep, own0 = own_in_memory ? total : g * keep;
  if (tid == 0) { ctl->pool_n = 0; ctl->overflow = 0; ctl->thr = kKeyInf; ctl->adm_n = 0; }
  if (tid < 128) place[tid] = 0;
  auto slot = [&](const uint32_t idx) -> unsigned long long {
    if (idx < own0) return __hip_atomic_load(&part_keys[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return idx - own0 < nres ? s_pool[idx - own0] : kKeyInf;
  };
#pragma unroll 1
  for (uint32_t base = tid; base < total; base += kRound * NT) {       // (base - tid: uniform)
    unsigned long long k[kRound];
#pragma unroll
    for (uint32_t j = 0; j < kRound; ++j) {
      const uint32_t idx = base + j * NT;
      k[j] = kKeyInf;
      if (idx < total) k[j] = slot(idx);
    }
#pragma unroll
    for (uint32_t j = 0; j < kRound; ++j) {
      const uint32_t idx = base + j * NT;
      if (idx < total) lvl[idx] = static_cast<unsigned char>(min(uint32_t(k[j] >> 32), kPadLevel));
    }
  }
  __syncthreads();                                       // the levels are there
  ONE_MARK(A, 10);
#pragma unroll 1
  for (uint32_t l = 1 + wv; l <= T; l += kNW) {          // a wave per level (uniform), a lane per list
    uint32_t sum = 0;
#pragma unroll 1
    for (uint32_t g0 = 0; g0 < G; g0 += 64) {
      const uint32_t li = g0 + lane;
      uint32_t lo = 0;
      if (li < G) {
        const unsigned char* const row = lvl + li * keep;
        uint32_t n = keep;
        while (n) {                                      // the first place whose level is not below l
          const uint32_t half = n >> 1;
          if (row[lo + half] < l) { lo += half + 1; n -= half + 1; } else { n = half; }
        }
        reach[l * kOneMaxGrid + li] = static_cast<unsigned char>(lo);
      }
      sum += lo;
    }
    sum = wave_inclusive_sum(sum);
    if (lane == 63) below[l] = sum;                      // (this wave's alone)
  }
  __syncthreads();
  // every wave for itself: lane j holds the keys of levels up to j
  const uint32_t upto = lane < T ? below[lane + 1] : 0u;
  const unsigned long long reached = __ballot(lane < T && upto >= keep);
  const uint32_t L = reached ? uint32_t(__builtin_ctzll(reached)) : kPadLevel;      // (kPadLevel: fewer than keep keys in all, every one passes)
  const uint32_t quota = L < kPadLevel ? keep - (L ? __builtin_amdgcn_readlane(upto, L - 1) : 0u) : 0u;
  ONE_MARK(A, 11);
  if (tid < 64) {                                        // lane t: lists kPerLane t .. kPerLane t + kPerLane - 1
    uint32_t at[kPerLane], cnt[kPerLane], sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPerLane; ++i) {
      const uint32_t li = kPerLane * tid + i;
      at[i] = 0; cnt[i] = 0;
      if (li < G) {
        at[i] = L == kPadLevel ? reach[T * kOneMaxGrid + li] : (L ? reach[L * kOneMaxGrid + li] : 0u);
        if (L != kPadLevel) cnt[i] = reach[(L + 1) * kOneMaxGrid + li] - at[i];
      }
      sum += cnt[i];
    }
    uint32_t in_front = wave_inclusive_sum(sum) - sum;   // keys of level L in the lists in front
    sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPerLane; ++i) {            // a list's passing prefix: its keys below L, and of level L what the quota still wants
      at[i] += min(cnt[i], quota > in_front ? quota - in_front : 0u);
      in_front += cnt[i];
      sum += at[i];
    }
    uint32_t o = wave_inclusive_sum(sum) - sum;
#pragma unroll
    for (uint32_t i = 0; i < kPerLane; ++i) { off[kPerLane * tid + i] = o; o += at[i]; }
    if (tid == 63) ctl->pool_n = o;
  }
  __syncthreads();
  const uint32_t n_out = ctl->pool_n;
  if (tid < n_out) {                                     // the list whose prefix holds output slot tid: the last with off <= tid
    uint32_t lo = 0;
#pragma unroll
    for (uint32_t step = 256; step; step >>= 1)
      if (lo + step < kOffN && off[lo + step] <= tid) lo += step;
    pool[tid] = slot(lo * keep + (tid - off[lo]));
  }
  __syncthreads();
  ONE_MARK(A, 15);
  {
    constexpr uint32_t kParts = NT / 128, kShare = 128 / kParts;
    const uint32_t i = tid & 127u, first = (tid >> 7) * kShare;
    const unsigned long long mine = i < n_out ? pool[i] : kKeyInf;
    uint32_t lower = 0;
#pragma unroll
    for (uint32_t j = 0; j < kShare; ++j)
      if (first + j < n_out) lower += pool[first + j] < mine ? 1u : 0u;   // (one address per wave and read: broadcasts)
    if (i < n_out && lower) atomicAdd(&place[i], lower);
    __syncthreads();
    const unsigned long long key = tid < n_out ? pool[tid] : kKeyInf;
    const uint32_t to = tid < n_out ? place[tid] : 0u;
    __syncthreads();
    if (tid < n_out) pool[to] = key;                     // (keys are distinct: the places are a permutation)
    __syncthreads();
  }
}

template <int NT>
__global__ __launch_bounds__(NT) void find_one_kernel(const FindArgs A, const OneArgs O) {
  __shared__ __attribute__((aligned(16))) uint32_t s_counters[kWindowSize / 4];
  __shared__ __attribute__((aligned(16))) unsigned long long s_pool[kOnePool];
  __shared__ Control s_ctl;
  __shared__ OneShared s_sh;
  uint4* const cnt128 = reinterpret_cast<uint4*>(s_counters);
  Control* const ctl = &s_ctl;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t g = blockIdx.x, G = gridDim.x;
  ONE_MARK(A, 0);
  // a row of the grid per needle (a handful of needles share the launch: blockIdx.y); its lists, flags and rows
  const uint32_t nd_i = blockIdx.y;
  const uint32_t T = O.codes_far ? O.T_far[nd_i] : O.T[nd_i];
  unsigned long long* const part_keys = O.part_keys + size_t(nd_i) * G * A.keep;
  uint32_t* const flags = O.flags + size_t(nd_i) * G;
  trigram_match_t* const out_rows = O.out_rows + size_t(nd_i) * kOneMaxKeep;
  uint32_t* const out_count = O.out_count + 2 * nd_i;
  // the needle's codes: lane t = trigram t (a load from the kernel-argument segment)
  const uint32_t code = lane < T ? (O.codes_far ? uint32_t(O.codes_far[nd_i * 64u + lane]) : uint32_t(O.codes[nd_i][lane])) : 0u;
  for (uint32_t i = tid; i < kWindowSize / 16; i += NT) cnt128[i] = make_uint4(0, 0, 0, 0);
  if (tid == 0) { ctl->pool_n = 0; ctl->overflow = 0; ctl->thr = kKeyInf; ctl->adm_n = 0; ctl->pend_n[0] = 0; ctl->pend_n[1] = 0; }
  if (tid < 12) s_sh.tally[tid] = 0;
  __syncthreads();
  ONE_MARK(A, 1);
  const uint32_t w0 = g * O.per, w1 = min(A.n_windows, w0 + O.per);
  for (uint32_t w = w0; w < w1;) {
    // 4-bit counters, both windows of a pair per step: any window for a needle of at most 15 trigrams, and for ANY
    // needle the leading windows whose references have at most 15 (nib_windows: an even count) -- find_kernel's rule
    if (T <= 15 || w < A.nib_windows) {
      const uint32_t w_end = min(w1, (w | 1u) + 1u);
      if (w_end - w == 1) one_step<Nib1, NT>(A, T, code, s_counters, s_pool, ctl, &s_sh, w, w_end);   // (a single window: 32 KiB)
      else one_step<Nib, NT>(A, T, code, s_counters, s_pool, ctl, &s_sh, w, w_end);
      w = w_end;
    } else {
      one_step<uint8_t, NT>(A, T, code, s_counters, s_pool, ctl, &s_sh, w, w + 1);
      ++w;
    }
  }
  ONE_MARK(A, 7);
  const uint32_t nres = ctl->pool_n;                     // (sorted: every step ends with a compaction)
  // ---- this workgroup's best keys (the list padded to `keep` slots, so that nobody needs its length), then its
  // flag; the grid's LAST workgroup waits for everybody's flag and merges ------------------------------------------
  // Keys and flags are written THROUGH to memory (agent-scope atomic stores: an XCD's L2 is not coherent with the
  // others') and the flag goes out when the keys' stores have been acknowledged; the merging workgroup reads both the
  // same way.  (First version: plain stores, __threadfence() -- a write-back of the XCD's whole L2, the sixteen
  // workgroups of an XCD one after the other: 14 us -- and a ticket, atomicAdd on one word by 129 workgroups, performed
  // at the memory side one after the other: another 13 us.  A workgroup that only spins on flags needs every other
  // workgroup to RUN, not to be co-resident: the grid never exceeds the CUs, and nobody waits for the spinner.)
  const uint32_t keep = A.keep;
  if (O.tickets) {
    __shared__ uint32_t s_ticket;
    for (uint32_t i = tid; i < keep; i += NT)
      __hip_atomic_store(&part_keys[size_t(g) * keep + i], i < nres ? s_pool[i] : kKeyInf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the list is in memory before the ticket is taken
    __syncthreads();
    ONE_MARK(A, 8);
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(&O.tickets[nd_i], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_ticket != G - 1) return;                       // (not the last to arrive)
    if (tid == 0) __hip_atomic_store(&O.tickets[nd_i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch
    ONE_MARK(A, 9);
    one_merge<NT>(A, part_keys, s_counters, s_pool, ctl, nres, T, keep, g, G, true);
  } else if (g != G - 1) {
    for (uint32_t i = tid; i < keep; i += NT)
      __hip_atomic_store(&part_keys[size_t(g) * keep + i], i < nres ? s_pool[i] : kKeyInf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    ONE_MARK(A, 8);
    if (tid == 0) __hip_atomic_store(&flags[g], O.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (!O.tickets) {
    ONE_MARK(A, 8);
    {
      // (The spinner needs the row's other workgroups to RUN, not to be co-resident with it: it is the row's last, and
      // workgroups are dispatched in the order of their flattened index, so that every workgroup it waits for was started
      // before it -- an assumption about the dispatcher HIP does not write down; it holds on every AMD part, a single
      // needle's 129 workgroups fit the chip whatever the order, and larger batches take tickets instead.)
      uint32_t pending;
      do {                                               // lanes 0..G-2 of the first waves watch one flag each
        const uint32_t f = tid < G - 1 ? __hip_atomic_load(&flags[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : O.seq;
        pending = __syncthreads_or(f != O.seq);
      } while (pending);
    }
    ONE_MARK(A, 9);
    one_merge<NT>(A, part_keys, s_counters, s_pool, ctl, nres, T, keep, g, G);   // (leaves the keys in order, ctl->pool_n of them)
  }
  unsigned long long* const pool = reinterpret_cast<unsigned long long*>(s_counters);
  ONE_MARK(A, 12);
  const uint32_t n_out = ctl->pool_n;
  if (tid < n_out) {
    const unsigned long long key = pool[tid];
    const uint32_t rk = uint32_t(key);
    trigram_match_t row;
    row.reference = A.ref_of_rank[rk];
    row.matches = T - uint32_t(key >> 32);
    row.weight = A.weight_of_rank[rk];
    out_rows[tid] = row;
  }
  if (tid == 0) out_count[0] = n_out;
  ONE_MARK(A, 13);
  if (tid < ((n_out + 63u) & ~63u) || tid < 64) __threadfence_system();   // rows and count are in host memory before the sequence word
  __syncthreads();
  ONE_MARK(A, 14);
  if (tid == 0) __hip_atomic_store(&out_count[1], O.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
