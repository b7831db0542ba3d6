// kernels/needle_major.inc -- the cooperative needle-major sweep (sweep_role: a manager wave and fifteen workers, dense
// slices left out of a step's count where a threshold allows) and find_kernel.
// Part of find_kernels.hip (included inside namespace blurrily, BLURRILY_KERNELS_BEGIN, the anonymous namespace).
// ---- cooperative flavour (needles with <= 64 distinct trigrams: nearly all of them) --------
// In sweep_pipelined every wave walks the needle's slice table itself to find its units: sixteen times the same work.
// Here ONE wave -- the manager -- chooses the next visited step (windows that cannot hold a candidate are stepped over
// without a barrier), fetches its slice table a step ahead and publishes it through LDS; the other fifteen read the table
// of the step and stream their units of it, one unit's LDS atomics running under the next unit's load (sweep_role below).
// (Rounds 2-5 kept a second flavour beside it, every wave doing everything with the publishing turn rotating --
// sweep_coop_plain, the sweep of launches that leave nothing out of a step's count: limits above ~150, phase 1 of the
// window-major sweep, "nm_cmin" 0, latency mode.  sweep_role with nothing left out measures the same -- 151.0 against
// 153.0 ms per 300 k needles at configs[2], 126.0 against 127.1 at configs[4] -- and serves them since round 6.)
// The dynamic LDS behind the counters is one budget (two workgroups per CU), shared by the candidate pool, the step's
// published tables and the pending lists: its size follows the pool's (ring_units_for: kept from the descriptor ring of
// rounds 2-4, whose room the tables -- 3 KiB -- now take a part of).
constexpr uint32_t kRingUnitsMax = 512;
__host__ __device__ constexpr uint32_t ring_units_for(uint32_t pool_cap) {
  return pool_cap <= 512 ? kRingUnitsMax : 256u;
}
// Inclusive prefix sum over the 64 lanes of a wave with DPP moves (row shifts inside the rows of 16, then the two
// row broadcasts of gfx9): ten VALU instructions, against six dependent ds_bpermute round trips for __shfl_up.
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t x) {
#define BLURRILY_DPP_ADD(ctrl_, rows_) x += uint32_t(__builtin_amdgcn_update_dpp(0, int(x), ctrl_, rows_, 0xF, false))
  BLURRILY_DPP_ADD(0x111, 0xF);                                 // row_shr:1
  BLURRILY_DPP_ADD(0x112, 0xF);                                 // row_shr:2
  BLURRILY_DPP_ADD(0x114, 0xF);                                 // row_shr:4
  BLURRILY_DPP_ADD(0x118, 0xF);                                 // row_shr:8
  BLURRILY_DPP_ADD(0x142, 0xA);                                 // row_bcast:15 -> rows 1 and 3
  BLURRILY_DPP_ADD(0x143, 0xC);                                 // row_bcast:31 -> rows 2 and 3
#undef BLURRILY_DPP_ADD
  return x;
}
// Fill-forward over the 64 lanes of a wave with the same moves: a lane whose d.y is 0 takes the pair of the nearest
// lane below it whose d.y is not (none: it stays 0) -- "mine if I have one, else theirs" is associative, so the
// scan's steps apply as they do to the sum.
__device__ __forceinline__ void wave_fill_forward(uint2& d) {
#define BLURRILY_DPP_FILL(ctrl_, rows_)                                                                        \
  do {                                                                                                         \
    const uint32_t px_ = uint32_t(__builtin_amdgcn_update_dpp(0, int(d.x), ctrl_, rows_, 0xF, false));         \
    const uint32_t py_ = uint32_t(__builtin_amdgcn_update_dpp(0, int(d.y), ctrl_, rows_, 0xF, false));         \
    const bool none_ = d.y == 0;                                                                               \
    d.x = none_ ? px_ : d.x; d.y = none_ ? py_ : d.y;                                                          \
  } while (0)
  BLURRILY_DPP_FILL(0x111, 0xF);                                // row_shr:1
  BLURRILY_DPP_FILL(0x112, 0xF);                                // row_shr:2
  BLURRILY_DPP_FILL(0x114, 0xF);                                // row_shr:4
  BLURRILY_DPP_FILL(0x118, 0xF);                                // row_shr:8
  BLURRILY_DPP_FILL(0x142, 0xA);                                // row_bcast:15 -> rows 1 and 3
  BLURRILY_DPP_FILL(0x143, 0xC);                                // row_bcast:31 -> rows 2 and 3
#undef BLURRILY_DPP_FILL
}

struct UnitRing {
  // a step's header, ONE 16-byte read: .x the step the slot's table belongs to (past the end: none left); .y its units (bits
  // 15:0), the scan's admission bound (bits 23:16; 0: the slow scan, which works it out itself -- cold start) and the
  // slices left out of the even / odd window's count (bits 27:24 / 31:28); .z, .w the bound's SWAR constants for the scan (ScanTraits::Need: bias, pre) -- worked out by the
  // manager, once, instead of by fifteen workers behind the count barrier (twenty scalar instructions each)
  uint4    hdr4[2];
  // per step (e & 3: a step's candidates are settled while the step after the next is being published) and window
  // parity: where the postings of the slices LEFT OUT of the count start in `ent` (their bitmaps sit in front of them)
  uint32_t hot[4][2][8];
  // behind it, in an area of 2 x ring_units_for(pool_cap) x 8 bytes: the two slots' tables (BLURRILY_TAB: 2 x 64 x 16
  // bytes, BLURRILY_BND: 2 x 64 x 8 bytes -- what a step of more than kDescUnits units, and a step swept again, are
  // walked by) and the two slots' unit descriptors (BLURRILY_DESC: 2 x kDescUnits x 8 bytes: entry k = unit k of the
  // step, .x its first entry in `ent`, .y where its slice ends | its window's parity -- all a worker reads of a step
  // of up to kDescUnits units); behind the area: pend[2][kPendMax]
};
constexpr uint32_t kNmMaxLeftOut = 8;                           // slices left out of one window's count at most (UnitRing::hot)
constexpr uint32_t kDescUnits = 64;                             // units of a step the manager publishes descriptors of (a lane each)
static_assert(kDescUnits == 64, "a lane of the manager per descriptor");
constexpr uint32_t kRingTableBytes = 2 * 64 * 16 + 2 * 64 * 8 + 2 * kDescUnits * 8;
static_assert(kRingTableBytes <= 2 * ring_units_for(512) * 8 && kRingTableBytes <= 2 * ring_units_for(1024) * 8,
              "tables and descriptors lie in the ring area, in front of the pending lists (8 KiB and 4 KiB areas)");
// the pending lists: behind the descriptors in the dynamic LDS
__device__ __forceinline__ uint32_t* pend_list(UnitRing* ring, uint32_t slot, uint32_t ring_units) {
  return reinterpret_cast<uint32_t*>(reinterpret_cast<uint2*>(ring + 1) + 2 * ring_units) + slot * kPendMax;
}

// sweep_coop leaves slices out of a step's count only where the candidates that leaves pending are sure of their
// place in the pool (sweep_role); the pool's last kAdmMax slots are then theirs
__device__ __forceinline__ bool coop_can_leave(const FindArgs& A) {
  return A.nm_cmin != 0 && A.pool_cap <= 1024 && !A.own_only && select_at(A) + 32 <= adm_max(A.pool_cap);
}

// A workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every global load in flight
// (s_waitcnt vmcnt(0)): behind a step's count that is the manager's table of the step after the next, just requested,
// behind its scan a worker's first unit of the next step -- loads that are meant to travel across the barriers.  The
// waves of a sweep exchange data through LDS only.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// Between LDS stores of a wave's lanes and reads of them by OTHER lanes of the same wave: no instruction -- the LDS
// serves a wave's accesses in order -- but the compiler, to which lanes are threads, may otherwise hand a lane its own
// earlier store for the read (it did: the descriptors' read-back moved under the storing lanes' branch).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// why sweep_coop's hot loop was left
enum : uint32_t { kLeftDone = 0, kLeftSlowScan = 2, kLeftSelect = 3 };

// One needle's sweep as ONE of two roles (round 4).  Through round 3 every wave of the workgroup did everything: its
// share of a step's units, its share of the scan -- and, by turns, the choosing of the next step, the fetching of
// its slice table and the publishing of its units, so that every wave held the table's registers and the turns' code,
// and the wave with a turn, which took it BEHIND its own units, was the one the count barrier waited for.  Now the
// workgroup's last wave is the MANAGER: it chooses, fetches and publishes (and, since this round, decides which dense
// slices a step leaves out of its count and settles the candidates that leaves pending) while the fifteen WORKERS
// count -- and counts and scans nothing itself; the workers count, scan and glance at the pool, and hold none of the
// manager's state.  Both roles run the same sequence of barriers and leave their hot loops on the same, uniform
// conditions (the step's header, the pool's state behind a scan); the rare paths behind the loops are common code.
// The two are separate instantiations called from disjoint branches, so that what one role keeps in registers is not
// live in the other's loop (every attempt of this round to add the left-out slices' bookkeeping to the shared loop cost
// 6-17 % with NOTHING left out: 64 VGPRs, two workgroups a CU).
template <typename CT, int NT, bool MANAGER, bool LEARNS>
__device__ __forceinline__ void sweep_role(const FindArgs& A, const Needle& nd, const uint16_t* codes, uint32_t* cnt32,
                                           unsigned long long* pool, Control* ctl, UnitRing* ring, const uint8_t* wmt,
                                           const uint32_t w0, const uint32_t w1, const uint32_t ws) {
  // A step covers kWPS windows: one with byte counters, two with 4-bit counters (CT = Nib).  Lane
  // t of the table holds trigram t's slice of the step's window -- of both windows with 4-bit
  // counters (second slot) -- and a unit's descriptor carries its window's parity in bit 0.
  constexpr bool kNib = std::is_same<CT, Nib>::value;
  constexpr uint32_t kWPS = kNib ? 2 : 1;
  constexpr uint32_t kNW = NT / 64, kWorkers = kNW - 1;
  const uint32_t tid = threadIdx.x;
  // (the lane number taken HERE, opaquely: derived from threadIdx.x it is a kernel-lifetime value, and with it every
  // address and mask computed from it -- hoisted to the kernel's entry for both roles and all four sweeps, spilled there
  // and reloaded from scratch inside the hot loops, each reload a wait for every global load in flight)
  uint32_t lane;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
  const uint32_t wid = MANAGER ? kWorkers : __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t tc = nd.T;                                     // <= 64
  const uint32_t v0 = w0 / kWPS, v1 = (w1 + kWPS - 1) / kWPS, vs = ws / kWPS;   // steps [v0, v1), first one vs
  const uint32_t n_visit = v1 - v0;
  uint4* const cnt128 = reinterpret_cast<uint4*>(cnt32);
  const uint32_t ring_units = ring_units_for(A.pool_cap);      // (where the pending lists start behind the ring: pend_list)
  // Slices are left out of a step's count only where the candidates that leaves pending are sure of their place in the
  // pool: limits up to 64 (the 512-entry pool), its last kAdmMax slots theirs alone, a step's pending list no longer than
  // what those slots hold beside the keys a glance lets pass (select_at()); not in phase 1 of the window-major sweep.
  const uint32_t sel_at = select_at(A);
  const bool can_leave = coop_can_leave(A);
  const uint32_t scan_pool_cap = can_leave ? A.pool_cap - adm_max(A.pool_cap) : A.pool_cap;
  const uint32_t pend_cap = can_leave ? min(kPendMax, adm_max(A.pool_cap) - sel_at) : 0u;
  // (the i-th step visited: upward from the needle's own length class, round the end.  Outward from it instead --
  // one step above, one below, by turns -- measured in round 3: 270.0 vs 253.2 ms per 500 k needles, 6.7 % slower;
  // downward from it, round the start: 292.7 ms, 16 % slower -- every window visited later lies BEHIND the threshold's
  // rank when the sweep goes upward, and needs one match more)
#define BLURRILY_STEP_AT(i_) ((i_) < n_visit ? (vs + (i_) < v1 ? vs + (i_) : vs + (i_) - n_visit) : v1)
  // Which step comes next: the first visit index >= from_ whose windows can hold a candidate (n_visit: none) -- a window
  // is stepped over when no reference of it has as many trigrams as a candidate needs (win_max_tri).  The manager keeps
  // the bounds of 64 visits in a register (lane l: visit wm_base + l; reloaded every 64 visits) and the threshold in
  // scalar registers (thr_c: it moves only in compact_pool, i.e. outside the hot loop), so that choosing is one compare
  // and a ballot -- no LDS round trip, which behind the workers' atomics takes 500 to 1 000 clocks each (through the first
  // version of this round two dependent ones per step looked at: the bound's byte, the threshold).
#define BLURRILY_LOAD_WMT(base_)                                                 \
  do {                                                                           \
    const uint32_t i_ = (base_) + lane;                                          \
    uint32_t m_ = 0;                                                             \
    if (i_ < n_visit) {                                                          \
      const uint32_t p_ = BLURRILY_STEP_AT(i_) * kWPS;                           \
      if (wmt) {                     /* the workgroup's LDS copy (clamped to 255 >= tc) */ \
        m_ = wmt[p_];                                                            \
        if (kNib && p_ + 1 < w1) m_ = max(m_, uint32_t(wmt[p_ + 1]));            \
      } else {                                                                   \
        m_ = A.win_max_tri[p_];                                                  \
        if (kNib && p_ + 1 < w1) m_ = max(m_, A.win_max_tri[p_ + 1]);            \
      }                                                                          \
    }                                                                            \
    wm_l = m_; wm_base = (base_);                                                \
  } while (0)
#define BLURRILY_NEXT_VISIT(from_, out_)                                         \
  do {                                                                           \
    uint32_t f_ = (from_);                                                       \
    out_ = n_visit;                                                              \
    while (f_ < n_visit) {                                                       \
      const uint32_t b_ = f_ & ~63u;                                             \
      if (b_ != wm_base) BLURRILY_LOAD_WMT(b_);                                  \
      const uint32_t i_ = b_ + lane;                                             \
      const uint32_t need_l_ = matches_needed(thr_c, tc, BLURRILY_STEP_AT(i_) * kWPS * kWindowRanks); \
      const unsigned long long ok_ = __ballot(i_ < n_visit && min(tc, wm_l) >= need_l_) >> (f_ - b_); \
      if (ok_) { out_ = f_ + uint32_t(__builtin_ctzll(ok_)); break; }           \
      f_ = b_ + 64u;                                                             \
    }                                                                            \
  } while (0)
  // slice table of step p_ (lane t: the needle's trigram code_): (A0, B0) the (even) window, (A1, B1) the odd one
  // with 4-bit counters; a dense slice's postings start behind its bitmap (postings_start)
#define BLURRILY_FETCH_TABLE(p_, code_, A0, B0, A1, B1)                          \
  do {                                                                           \
    A0 = B0 = A1 = B1 = 0;                                                       \
    const uint32_t w_ = (p_) * kWPS;                                             \
    if (STATS(A) && w_ < w1) st_tab += 2u * tc * (kNib && w_ + 1 < w1 ? 2u : 1u); \
    if (w_ < w1 && lane < tc) {                                                  \
      const uint32_t idx_ = w_ * kNumCodes + (code_);                            \
      const uint2 se_ = A.slice_se[idx_]; A0 = se_.x; B0 = se_.y;                \
    }                                                                            \
    if (kNib && w_ + 1 < w1 && lane < tc) {                                      \
      const uint32_t idx_ = (w_ + 1) * kNumCodes + (code_);                      \
      const uint2 se_ = A.slice_se[idx_]; A1 = se_.x; B1 = se_.y;                \
    }                                                                            \
  } while (0)
  // The header of step step_ in ring slot s_, by lane 0 of the manager: the step, its unit count, the bound its scan
  // admits counters from -- worked out HERE, once, from the threshold as it is now, instead of by every wave behind
  // the count barrier -- and how many slices each of its windows leaves out of the count.  The threshold can only
  // tighten until that scan runs (in the select of the step in between), so the published bound is at most too low:
  // the scan then looks at a few counters more, and every counter it looks at is tested against the threshold of the
  // moment before it enters the pool.  A bound of 0 = no threshold yet and a cold start due: the slow scan.
#define BLURRILY_PUBLISH_HDR(s_, step_, nu_, need_, ls_)                         \
  do {                                                                           \
    const typename ScanTraits<CT>::Need nq_ = ScanTraits<CT>::prepare(need_);    \
    if (lane == 0) ring->hdr4[s_] = make_uint4((step_), (nu_) | ((need_) << 16) | ((ls_) << 24), nq_.bias, nq_.pre); \
  } while (0)
  // (A window in which fewer of the needle's trigrams occur AT ALL than a candidate needs, left out by the publishing
  // wave -- two ballots over the table it holds -- measured in round 3: 255.5 vs 252.9 ms, 1 % slower: at Geonames
  // scale the bound hardly ever bites.)
  // What the manager publishes of a step is its SLICE TABLE, two stores for the wave (16 + 8 bytes a lane): lane t = the
  // needle's trigram t.  A step's units are numbered with the EVEN window's first -- E of them, slice after slice --, then
  // the odd window's.  TAB: .x / .y where the slice's postings start in `ent` (even / odd window) MINUS 512 entries per
  // unit in front of the slice's first, so that unit k of the slice starts at .x + 512 k; .z / .w where the slices end (a
  // slice that is empty, or left out of the count: start = end).  BND: the inclusive unit sums, .x over the even slices,
  // .y = E + the sums over the odd ones.  Unit k of the step belongs to worker k mod 15; a worker reads table and sums
  // once per step and finds unit k's slice with one compare and ballot over the sums of k's window (k < E: even), its
  // bounds with two v_readlane, one shift and one add -- ten scalar instructions where round 4's table (both windows'
  // units interleaved per slice, lengths and sums packed in 16-bit halves: 16 bytes) took twenty-two and four v_readlane
  // per unit, SALU being the pipe the step is most sensitive to (tools/experiments/r6_salu64.py: 64 more a worker and
  // step cost 15 % where 64 more VALU cost 9 %).  (Through
  // round-4's first version the manager listed every UNIT -- a store per unit from lanes looping over their slices,
  // queued behind the workers' atomics: 4 300 clocks per step, the wave the count barrier waited for in nine steps of ten.)
  // Since the unit descriptors (BLURRILY_DESC) a worker goes through table and sums only for the units kDescUnits and
  // up of a step that has them, and for a step swept again; the search above is then the manager's, once, for the
  // step's first kDescUnits units: lane k = unit k.  No loop over units and no store per unit: a slice's lane stores
  // its biased start and its end | parity where its FIRST unit's descriptor lies, the wave reads the 64 entries back --
  // the one LDS round trip of a publish -- and every lane takes the entry of the last slice that starts at or in front
  // of it (a fill-forward over the lanes in DPP moves); the unit's first entry is that start + 512 k.
#define BLURRILY_TAB(s_) (reinterpret_cast<uint4*>(ring + 1) + (s_) * 64u)
#define BLURRILY_BND(s_) (reinterpret_cast<uint2*>(reinterpret_cast<uint4*>(ring + 1) + 128u) + (s_) * 64u)
#define BLURRILY_DESC(s_) (reinterpret_cast<uint2*>(reinterpret_cast<uint4*>(ring + 1) + 128u) + 128u + (s_) * kDescUnits)
  // the descriptors of a worker's units of ring slot s_: lane j its j-th (unit wid + kWorkers j) of the first kDescUnits
#define BLURRILY_DESC_MINE(s_) (BLURRILY_DESC(s_)[min(wid + kWorkers * lane, kDescUnits - 1u)])
  // scalar bounds of a worker's j_-th unit from its descriptors ds_
#define BLURRILY_UNIT_AT(ds_, j_, start_, end_, half_)                           \
  do {                                                                           \
    start_ = __builtin_amdgcn_readlane((ds_).x, (j_));                           \
    end_ = __builtin_amdgcn_readlane((ds_).y, (j_));                             \
    half_ = kNib ? (end_) & 1u : 0u;                                             \
  } while (0)
  // scalar bounds of the step's unit k_ from the table in tb_ / its sums bd_ (E_: the even window's units)
#define BLURRILY_UNIT_OF(tb_, bd_, E_, k_, start_, end_, half_)                  \
  do {                                                                           \
    if (!kNib || (k_) < (E_)) {                                                  \
      const uint32_t t_ = uint32_t(__builtin_ctzll(__ballot((bd_).x > (k_)) | (1ull << 63))); \
      start_ = __builtin_amdgcn_readlane((tb_).x, t_) + ((k_) << 9);             \
      end_ = __builtin_amdgcn_readlane((tb_).z, t_);                             \
      half_ = 0u;                                                                \
    } else {                                                                     \
      const uint32_t t_ = uint32_t(__builtin_ctzll(__ballot((bd_).y > (k_)) | (1ull << 63))); \
      start_ = __builtin_amdgcn_readlane((tb_).y, t_) + ((k_) << 9);             \
      end_ = __builtin_amdgcn_readlane((tb_).w, t_);                             \
      half_ = 1u;                                                                \
    }                                                                            \
  } while (0)
  // LEFT OUT of the count (round 4; the MaxScore argument of wsweep_kernel, inside the needle-major step): once the
  // needle has a threshold -- `need_` matches to enter its top `keep` in this step's windows -- the l_max_ = need_ -
  // nm_cmin LARGEST slices of at least nm_dense postings of a window need not be counted.  A reference with need_
  // matches has at least need_ - L of them among the counted slices, so the scan finds it with the bound lowered by
  // L; what it finds goes to the step's pending list, and the manager settles its exact count from the left-out
  // slices' bitmaps during the next step (PEND_SETTLE).  Lane t ranks its slice among the window's dense ones by size
  // (one readlane per dense slice); the chosen ones note where their postings start (UnitRing::hot) and list no units.
#define BLURRILY_LEAVE_OUT(hs_, h_, A_, rk_, units_)                             \
  do {                                                                           \
    const bool skip_ = (rk_) < l_max_;                                           \
    const unsigned long long sm_ = __ballot(skip_);                              \
    if (skip_) {                                                                 \
      ring->hot[hs_][h_][__builtin_amdgcn_mbcnt_hi(uint32_t(sm_ >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(sm_), 0u))] = (A_); \
      units_ = 0;                                                                \
    }                                                                            \
    ls_ |= uint32_t(__popcll(sm_)) << (4u * (h_));                               \
  } while (0)
  // A slice's rank by size among the dense slices of its window (lane t: trigram t's; 0xFF: not dense) -- what
  // BLURRILY_LEAVE_OUT holds against l_max_.  It does not depend on the threshold, so the manager works it out for the
  // table it will publish NEXT while the workers scan (it has the time there: the count barrier is the one that waits
  // for it), one v_readlane per dense slice of the window.
#define BLURRILY_RANK_ONE(A_, B_, rk_)                                           \
  do {                                                                           \
    const uint32_t size_ = (B_) - (A_);                                          \
    const bool dense_ = size_ >= A.nm_dense;                                     \
    uint32_t bigger_ = 0;                                                        \
    for (unsigned long long m_ = __ballot(dense_); m_; m_ &= m_ - 1) {           \
      const uint32_t u_ = __builtin_ctzll(m_);                                   \
      const uint32_t su_ = __builtin_amdgcn_readlane(size_, u_);                 \
      bigger_ += (su_ > size_ || (su_ == size_ && u_ < lane)) ? 1u : 0u;         \
    }                                                                            \
    rk_ = dense_ ? bigger_ : 0xFFu;                                              \
  } while (0)
#define BLURRILY_RANK()                                                          \
  do {                                                                           \
    BLURRILY_RANK_ONE(ta, tb, rk0);                                              \
    if (kNib) BLURRILY_RANK_ONE(ta1, tb1, rk1);                                  \
    ranked = true;                                                               \
  } while (0)
  // the manager publishes the step's slice table into ring slot s_ (a lane's even-window units come first, then its
  // odd-window units)
#define BLURRILY_PRODUCE(s_, hs_, step_, A0, B0, A1, B1)                         \
  do {                                                                           \
    const unsigned long long thr_ = thr_c;                                       \
    uint32_t need_ = min(matches_needed(thr_, tc, (step_) * kWPS * kWindowRanks), 0xFFu); \
    uint32_t units0_ = slice_units(A0, B0), units1_ = kNib ? slice_units(A1, B1) : 0u; \
    uint32_t ls_ = 0;                                                            \
    /* (the bound kept at a power of two where that costs a slice, so that the scan's first test is exact -- round 6:   \
       128.8 against 127.8 ms per 300 k needles, the slice's postings cost more than the second tests saved) */         \
    const uint32_t l_max_ = (can_leave && thr_ != kKeyInf && need_ > A.nm_cmin) ? min(need_ - A.nm_cmin, kNmMaxLeftOut) : 0u; \
    if (l_max_) {                                                                \
      if (!ranked) BLURRILY_RANK();            /* (the first step of a sweep, the one behind a rare path) */ \
      BLURRILY_LEAVE_OUT(hs_, 0u, A0, rk0, units0_);                             \
      if (kNib) BLURRILY_LEAVE_OUT(hs_, 1u, A1, rk1, units1_);                   \
    }                                                                            \
    ranked = false;                            /* (the table is about to be replaced) */ \
    if (thr_ == kKeyInf && !nd.has_floor && !A.tomb && tc > 1) need_ = 0;        \
    const uint32_t incl0_ = wave_inclusive_sum(units0_);                         \
    const uint32_t even_ = __builtin_amdgcn_readlane(incl0_, 63);                \
    const uint32_t incl1_ = kNib ? even_ + wave_inclusive_sum(units1_) : even_;  \
    const uint32_t total_ = kNib ? __builtin_amdgcn_readlane(incl1_, 63) : even_; \
    const uint32_t ex0_ = incl0_ - units0_, ex1_ = incl1_ - units1_;             /* the slices' first units */ \
    const uint32_t bs0_ = (A0) - (ex0_ << 9), bs1_ = (A1) - (ex1_ << 9);         /* their biased starts */ \
    /* the descriptors' round trip first: the table's stores travel behind it.  (Slices end on multiples of eight \
       entries -- device_index.hip --: bit 0 of an end is free for the parity, and an end with units is not 0.) */ \
    uint2* const dsc_ = BLURRILY_DESC(s_);                                       \
    dsc_[lane] = make_uint2(0u, 0u);                                             \
    wave_lds_sync();                                                             \
    if (units0_ && ex0_ < kDescUnits) dsc_[ex0_] = make_uint2(bs0_, (B0));       \
    if (kNib && units1_ && ex1_ < kDescUnits) dsc_[ex1_] = make_uint2(bs1_, (B1) | 1u); \
    wave_lds_sync();                            /* (lanes read what OTHER lanes stored) */ \
    const unsigned long long dq_ = __hip_atomic_load(reinterpret_cast<unsigned long long*>(dsc_ + lane), __ATOMIC_RELAXED, \
                                                     __HIP_MEMORY_SCOPE_WAVEFRONT); \
    uint2 d_ = make_uint2(uint32_t(dq_), uint32_t(dq_ >> 32));                   \
    /* (a slice left out of the count lists no units: it is published as empty) */ \
    BLURRILY_TAB(s_)[lane] = make_uint4(bs0_, bs1_, units0_ ? (B0) : bs0_, units1_ ? (B1) : bs1_); \
    BLURRILY_BND(s_)[lane] = make_uint2(incl0_, incl1_);                         \
    wave_fill_forward(d_);                                                       \
    dsc_[lane] = make_uint2(d_.x + (lane << 9), d_.y);   /* (lanes past the step's units: never read) */ \
    /* the scan's bound, lowered by the most slices either window leaves out (a harvested counter is settled    \
       exactly, so a bound that is too low for the other window costs a look, nothing else) */ \
    const uint32_t lmost_ = max(ls_ & 15u, ls_ >> 4);                            \
    BLURRILY_PUBLISH_HDR(s_, step_, total_, need_ - min(need_, lmost_), ls_);    \
  } while (0)
  // The units of ring slot s_ that belong to this worker (k = wid, wid + 15, ...): one unit's LDS
  // atomics run while the next unit's load is in flight.  Which lanes loaded a group travels as a lane
  // predicate -- an SGPR pair -- beside the unit in flight: no sentinels to fill idle lanes with, no liveness
  // test before the atomics.  A unit's address is a scalar base (its first entry) plus the lane's 16 bytes:
  // nothing per unit and lane but the load itself and one compare.  (Up to four of a wave's units loaded before
  // the first is counted -- four loads in flight -- measured in round 3: 3.2 % SLOWER, 317.2 vs 307.4 ms.)
#define BLURRILY_UNIT_STEP(x_, y_, h_)                                           \
  do {                                                                           \
    const bool live_ = lane8p < (y_) - (x_);    /* (y_ may carry the parity in bit 0: lane8p = 8 lane + 1) */ \
    uint4 v_ = pend_;                                                            \
    if (live_) v_ = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(A.ent + (x_)) + lane16); \
    if (STATS(A)) st_ent += min(512u, ((y_) & ~1u) - (x_));                      \
    if (pend_live_) bump_unit_loaded<CT>(cnt32, pend_, pend_h_);                 \
    pend_ = v_; pend_h_ = (h_); pend_live_ = live_;                              \
  } while (0)
  // (a worker's j-th unit of the step's first kDescUnits: two v_readlane of its descriptors, read a step ago behind the
  // count barrier; the units behind them, of the few steps that have any: table and sums, read here)
#define BLURRILY_COUNT_UNITS(s_, n_, have_mine_)                                 \
  do {                                                                           \
    uint4 pend_ = make_uint4(0, 0, 0, 0);                                        \
    uint32_t pend_h_ = 0;                                                        \
    bool pend_live_ = false;                                                     \
    uint2 dl_ = ds_mine;                                                         \
    if (!(have_mine_)) dl_ = BLURRILY_DESC_MINE(s_);                             \
    uint32_t k_ = wid, j_ = 0;                                                   \
    if ((have_mine_) && pre_valid) {            /* the first unit is on its way since the scan before */ \
      pend_ = pre_v; pend_h_ = pre_h; pend_live_ = pre_live;                     \
      if (STATS(A) && wid < (n_)) {                                              \
        const uint32_t x_ = __builtin_amdgcn_readlane(dl_.x, 0), y_ = __builtin_amdgcn_readlane(dl_.y, 0); \
        st_ent += min(512u, (y_ & ~1u) - x_);                                    \
      }                                                                          \
      k_ = wid + kWorkers; j_ = 1;                                               \
    }                                                                            \
    pre_valid = false;                                                           \
    const uint32_t nd_ = min((n_), kDescUnits);                                  \
    for (; k_ < nd_; k_ += kWorkers, ++j_) {                                     \
      uint32_t x_, y_, h_;                                                       \
      BLURRILY_UNIT_AT(dl_, j_, x_, y_, h_);                                     \
      BLURRILY_UNIT_STEP(x_, y_, h_);                                            \
    }                                                                            \
    if ((n_) > kDescUnits) {                    /* (uniform: the header's count) */ \
      const uint4 tl_ = BLURRILY_TAB(s_)[lane];                                  \
      const uint2 bl_ = BLURRILY_BND(s_)[lane];                                  \
      const uint32_t even_ = kNib ? __builtin_amdgcn_readlane(bl_.x, 63) : 0u;   \
      for (; k_ < (n_); k_ += kWorkers) {                                        \
        uint32_t x_, y_, h_;                                                     \
        BLURRILY_UNIT_OF(tl_, bl_, even_, k_, x_, y_, h_);                       \
        BLURRILY_UNIT_STEP(x_, y_, h_);                                          \
      }                                                                          \
    }                                                                            \
    if (pend_live_) bump_unit_loaded<CT>(cnt32, pend_, pend_h_);                 \
  } while (0)
  // Behind a scan, in front of its barrier: the header of the next step and this wave's units of it have arrived
  // (requested before the scan), the scan's registers are free -- the load of the wave's first unit of the next step
  // goes out here and travels under the barrier and the glance at the pool: 288.0 -> 281.3 ms per 500 k needles.
  // (The first TWO units loaded here and two loads kept in flight through the count: 313.0 ms, 11 % slower -- as
  // with every other attempt at more loads in flight per wave, rounds 2 and 3.  Two units loaded here and ONE load
  // in flight through the count: 330 ms while the compiler kept the second unit in scratch -- a value carried through
  // the rare paths is spilled where it is loaded --, 289.4 vs 281.9 ms, 2.7 % slower, once it was declared dead there.
  // A read-only kernel with this shape of access reaches 7.5 TB/s on the chip with one load in flight per wave
  // (tools/micro/read_bw.hip): what the loads wait for is not more of them.  The units' loads marked
  // non-temporal, global_load_dwordx4 ... nt: 330.6 ms, 17 % slower -- the postings of the Geonames-scale image
  // are 253 MB, and the 256 MiB Infinity Cache holds most of them as long as they are allowed in.)
#define BLURRILY_PRELOAD()                                                       \
  do {                                                                           \
    const uint32_t np_ = __builtin_amdgcn_readfirstlane(h_next.x);               \
    const uint32_t nn_ = __builtin_amdgcn_readfirstlane(h_next.y) & 0xFFFFu;     \
    pre_valid = np_ < v1;                                                        \
    pre_live = false;                                                            \
    if (pre_valid && wid < nn_) {                                                \
      uint32_t x_, y_;                                                           \
      BLURRILY_UNIT_AT(ds_mine, 0u, x_, y_, pre_h);                              \
      pre_live = lane8p < y_ - x_;                                               \
      if (pre_live) pre_v = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(A.ent + x_) + lane16); \
    }                                                                            \
  } while (0)
  // a step swept AGAIN with every slice counted (pool overflow where slices were left out): every wave -- the manager
  // too -- fetches the table of step p_ itself and walks it
#define BLURRILY_COUNT_WALK(p_)                                                  \
  do {                                                                           \
    uint32_t fa0_, fb0_, fa1_, fb1_, k_ = 0;                                     \
    const uint32_t wcode_ = lane < tc ? codes[lane] : 0u;                        \
    BLURRILY_FETCH_TABLE(p_, wcode_, fa0_, fb0_, fa1_, fb1_);                    \
    BLURRILY_FOR_SLOT_UNITS(kNW, fa0_, fb0_, wid, lane, k_,                      \
                            { bump_unit<CT>(cnt32, load_group(A.ent, c, sb), 0u);   \
                              if (STATS(A)) st_ent += min(512u, sb - (c - lane * 8)); }); \
    if (kNib)                                                                    \
      BLURRILY_FOR_SLOT_UNITS(kNW, fa1_, fb1_, wid, lane, k_,                    \
                              { bump_unit<CT>(cnt32, load_group(A.ent, c, sb), 1u); \
                                if (STATS(A)) st_ent += min(512u, sb - (c - lane * 8)); }); \
  } while (0)
  // The manager's turn of a step: it publishes the next visited step (whose table arrived a step ago), then chooses the
  // step after the next (the threshold only changes behind select's barriers) and fetches its table, which travels
  // during the barrier and the scan.
#define BLURRILY_MANAGER_TURN(e_, s_)                                            \
  do {                                                                           \
    if (my_i < n_visit) {                                                        \
      BLURRILY_PRODUCE((s_) ^ 1u, ((e_) + 1u) & 3u, BLURRILY_STEP_AT(my_i), ta, tb, ta1, tb1); \
    } else if (lane == 0) {                                                      \
      ring->hdr4[(s_) ^ 1u] = make_uint4(v1, 0u, 0u, 0u);                        \
    }                                                                            \
    PHASE_MARK(7);                                  /* next step's units published */ \
    TRACE_MARK(A, nd.q, (e_), 1u, 7u);                                           \
    const uint32_t chosen_ = my_i;                                               \
    BLURRILY_NEXT_VISIT(chosen_ + 1, my_i);                                      \
    if (my_i != chosen_ + 1) PATH_FLAG(A, nd.q, kPathSkipped);                   \
    BLURRILY_FETCH_TABLE(BLURRILY_STEP_AT(my_i), mcode, ta, tb, ta1, tb1);       \
    PHASE_MARK(2);                                  /* step after the next chosen, its table requested */ \
  } while (0)
  // The manager settles the PENDING candidates of ring slot slot_ (step pstep_, whose windows left ls_ slices out,
  // noted in hot[hs_]): lane c takes candidate c -- in-window rank | parity << 16 | counted matches << 20 --, loads the
  // word of every left-out slice's bitmap that holds the candidate's bit (up to eight loads in flight), adds the bits
  // to the counted matches and admits the candidate to the pool, or not, like any harvested counter: into the pool's
  // tail, which is the manager's alone (compact_pool moves it up), so that nothing a flooding scan does to the pool
  // meanwhile can cost a settled candidate its place.  Done while the workers scan the next step.
#define BLURRILY_PEND_SETTLE(slot_, hs_, pstep_, ls_)                            \
  do {                                                                           \
    const uint32_t np_ = min(uint32_t(__builtin_amdgcn_readfirstlane(ctl->pend_n[slot_])), pend_cap); \
    if (np_) {                                                                   \
      const uint32_t* const pl_ = pend_list(ring, slot_, ring_units);            \
      for (uint32_t c_ = lane; c_ < np_; c_ += 64) {                             \
        const uint32_t e_ = pl_[c_];                                             \
        const uint32_t h_ = (e_ >> 16) & 1u, r16_ = e_ & 0xFFFFu;                \
        const uint32_t L_ = ((ls_) >> (4u * h_)) & 15u;                          \
        /* where the left-out slices' postings start: two 16-byte reads, then the loads together */ \
        const uint4 ha_ = *reinterpret_cast<const uint4*>(&ring->hot[hs_][h_][0]); \
        const uint4 hb_ = *reinterpret_cast<const uint4*>(&ring->hot[hs_][h_][4]); \
        const uint32_t hs8_[kNmMaxLeftOut] = {ha_.x, ha_.y, ha_.z, ha_.w, hb_.x, hb_.y, hb_.z, hb_.w}; \
        uint32_t w_[kNmMaxLeftOut];                                              \
        _Pragma("unroll") for (uint32_t k_ = 0; k_ < kNmMaxLeftOut; ++k_) {      \
          w_[k_] = 0;                                                            \
          if (k_ < L_)                                                           \
            w_[k_] = reinterpret_cast<const uint32_t*>(A.ent + (hs8_[k_] - kBitmapSlots))[r16_ >> 5]; \
        }                                                                        \
        uint32_t cnt_ = e_ >> 20;                                                \
        _Pragma("unroll") for (uint32_t k_ = 0; k_ < kNmMaxLeftOut; ++k_) cnt_ += (w_[k_] >> (r16_ & 31u)) & 1u; \
        if (STATS(A)) atomicAdd(&STATS(A)[kStatProbes], static_cast<unsigned long long>(L_)); \
        const uint32_t rank_ = (pstep_) * kWPS * kWindowRanks + h_ * kWindowRanks + r16_; \
        const unsigned long long key_ = (static_cast<unsigned long long>(tc - min(tc, cnt_)) << 32) | rank_; \
        bool pass_ = key_ <= thr_c;                                              \
        if (nd.has_floor) pass_ = pass_ && key_ > ctl->floor;                    \
        if (pass_) {                                     /* (tombstones were looked at where it was harvested) */ \
          const uint32_t at_ = atomicAdd(&ctl->adm_n, 1u);                       \
          if (at_ < adm_max(A.pool_cap)) pool[A.pool_cap - adm_max(A.pool_cap) + at_] = key_; \
        }                                                                        \
      }                                                                          \
      if (lane == 0) ctl->pend_n[slot_] = 0;                                     \
    }                                                                            \
  } while (0)

  const uint32_t lane8p = lane * 8 + 1, lane16 = lane * 16;     // (lane8p: BLURRILY_UNIT_STEP)
  PHASE_DECL;
  uint32_t st_ent = 0, st_tab = 0, st_steps = 0, st_redo = 0, st_past = 0;   // request counters (FindArgs::stats), wave-uniform
  // ---- the manager's state: the needle's codes, the table it will publish next and its visit index, the step before
  uint32_t mcode = 0, ta = 0, tb = 0, ta1 = 0, tb1 = 0, my_i = 0, p_prev = 0, ls_prev = 0;
  uint32_t rk0 = 0xFFu, rk1 = 0xFFu;                            // ranks of the held table's slices (BLURRILY_RANK)
  bool ranked = false;
  uint32_t wm_l = 0, wm_base = 0xFFFFFFFFu;                     // win_max_tri of 64 visits (BLURRILY_LOAD_WMT)
  // the threshold as scalars: set by compact_pool only, i.e. outside the hot loop -- read again behind every exit
  unsigned long long thr_c = ctl->thr;
  thr_c = (static_cast<unsigned long long>(__builtin_amdgcn_readfirstlane(uint32_t(thr_c >> 32))) << 32) |
          __builtin_amdgcn_readfirstlane(uint32_t(thr_c));
  // ---- a worker's: its units of the step about to start (lane j: its j-th), the first of them loaded ahead
  uint2 ds_mine = make_uint2(0, 0);
  uint4 pre_v = make_uint4(0, 0, 0, 0);
  uint32_t pre_h = 0;
  bool pre_live = false, pre_valid = false;
  (void)rk0; (void)rk1; (void)ranked; (void)wm_l; (void)wm_base; (void)thr_c; (void)mcode; (void)ta; (void)tb; (void)ta1; (void)tb1; (void)my_i; (void)p_prev; (void)ls_prev;
  (void)ds_mine; (void)pre_v; (void)pre_h; (void)pre_live; (void)pre_valid; (void)lane8p; (void)lane16; (void)pend_cap;
  if (MANAGER) PATH_FLAG(A, nd.q, kNib ? kPathNibble : kPathByte);
  if constexpr (MANAGER) {
    __builtin_amdgcn_s_setprio(3);                              // the wave everybody's next step waits for
    mcode = lane < tc ? codes[lane] : 0u;
    BLURRILY_FETCH_TABLE(BLURRILY_STEP_AT(0u), mcode, ta, tb, ta1, tb1);
    BLURRILY_PRODUCE(0u, 0u, BLURRILY_STEP_AT(0u), ta, tb, ta1, tb1);
    BLURRILY_NEXT_VISIT(1u, my_i);
    BLURRILY_FETCH_TABLE(BLURRILY_STEP_AT(my_i), mcode, ta, tb, ta1, tb1);
  }
  // a threshold exists (it is set by compact_pool only, i.e. outside the hot loop below: re-read behind every exit)
  bool have_thr = thr_c != kKeyInf;
  const uint32_t scan_cap = min(tc, ScanTraits<CT>::kMaxCount);  // a counter of this sweep cannot exceed it
  __syncthreads();
  uint4 h_next = ring->hdr4[0];                                  // header of the step about to start
  if constexpr (!MANAGER) ds_mine = BLURRILY_DESC_MINE(0u);

  // The sweep is a HOT LOOP of steps that need nothing special -- header, units (the manager: its turn), barrier,
  // scan with the published bound (the manager: the step before's pending candidates), barrier, a glance at the pool --
  // and is left for everything else (more units than the ring holds; no threshold yet: the cold start's bisection;
  // the pool to be compacted, perhaps the step swept again), which is dealt with behind it before the loop is entered
  // again.  Kept apart so that what only the rare paths need is not held in registers, nor worked out, step after step.
  uint32_t e = 0;
  for (;;) {
    uint32_t left, s, p, n_units, hy_;
    for (;; ++e) {
      s = e & 1;
      p = __builtin_amdgcn_readfirstlane(h_next.x);
      hy_ = __builtin_amdgcn_readfirstlane(h_next.y);
      n_units = hy_ & 0xFFFFu;
      if (p >= v1) { left = kLeftDone; break; }                 // no step left
      ++st_steps;
      if (STATS(A) && n_units > kDescUnits) ++st_past;
      if constexpr (MANAGER) __builtin_amdgcn_s_setprio(3);     // (the rare paths leave it at 0)
      PHASE_MARK(0);                                            // loop overhead
      const bool tr_ = MANAGER || wid == 0;
      if (tr_) TRACE_MARK(A, nd.q, e, MANAGER ? 1u : 0u, 0u);
      if constexpr (MANAGER) {
        BLURRILY_MANAGER_TURN(e, s);
      } else {
        BLURRILY_COUNT_UNITS(s, n_units, true);
        PHASE_MARK(2);                                          // units counted
      }
      if (tr_) TRACE_MARK(A, nd.q, e, MANAGER ? 1u : 0u, 1u);
      lds_barrier();                                            // counts and next descriptors visible
      if (tr_) TRACE_MARK(A, nd.q, e, MANAGER ? 1u : 0u, 2u);
      PHASE_MARK(3);                                            // barrier after count
      // The next step's header and a worker's units of it were published before that barrier: requested now,
      // they arrive under the scan instead of standing, one LDS round trip each (several hundred clocks behind the
      // other workgroup's atomics), between the scan barrier and the first load of the next step.
      // (this step's scan constants are taken out of the header before the next one is requested over it)
      const uint32_t nq_bias_ = __builtin_amdgcn_readfirstlane(h_next.z), nq_pre_ = __builtin_amdgcn_readfirstlane(h_next.w);
      h_next = ring->hdr4[s ^ 1u];
      if constexpr (!MANAGER) ds_mine = BLURRILY_DESC_MINE(s ^ 1u);
      if constexpr (MANAGER) {
        if (can_leave) {                                        // while the workers scan
          BLURRILY_PEND_SETTLE(s ^ 1u, (e - 1u) & 3u, p_prev, ls_prev);
          if (have_thr && n_units != 0 && ((hy_ >> 16) & 0xFFu) != 0) BLURRILY_RANK();   // (the table of the step after the next: fetched before the barrier)
        }
        p_prev = p; ls_prev = n_units ? hy_ >> 24 : 0u;
      }
      if (n_units == 0) continue;                               // nothing of the needle in this step's windows
      const uint32_t need = (hy_ >> 16) & 0xFFu;
      if (need == 0) { left = kLeftSlowScan; break; }
      if constexpr (!MANAGER) {
        const uint32_t wbase = p * kWPS * kWindowRanks;
        const uint32_t wlen = min(kWPS * kWindowRanks, A.n_refs - wbase);
        typename ScanTraits<CT>::Need nq_ = ScanTraits<CT>::from_published(need, nq_bias_, nq_pre_);
        scan_core<CT, NT>(cnt128, nd, need, scan_cap, &ctl->thr, &ctl->floor, A.tomb, pool, scan_pool_cap, &ctl->pool_n,
                          &ctl->overflow, wbase, wlen, STATS(A) && A.path_flags ? &A.path_flags[nd.q] : nullptr,
                          hy_ >> 24, pend_list(ring, s, ring_units), &ctl->pend_n[s], pend_cap, uint32_t(NT - 64), &nq_);
        if (tr_) TRACE_MARK(A, nd.q, e, 0u, 3u);
        BLURRILY_PRELOAD();
      }
      if (tr_) TRACE_MARK(A, nd.q, e, MANAGER ? 1u : 0u, 4u);
      PHASE_MARK(5);                                            // scan
      lds_barrier();                                            // counters are zero again
      if (tr_) TRACE_MARK(A, nd.q, e, MANAGER ? 1u : 0u, 5u);
      PHASE_MARK(6);                                            // barrier after scan
      // (Looking at the pool a count phase later -- the read requested here, used behind the next count barrier, a
      // compaction then running with the next step counted and not yet scanned -- was built and measured in round 3:
      // 2 % slower, 293.0 vs 287.2 ms per 500 k needles; the thresholds the headers carry are a step staler.)
      // (every lane holds the same three words: the test is three VALU instructions and one compare into a mask -- moved
      // to scalar registers first it was three v_readfirstlane and a dozen scalar instructions: 122.4 -> 121.3 ms per 300 k)
      const uint4 c_ = *reinterpret_cast<const uint4*>(&ctl->pool_n);          // pool_n, overflow, adm_n, (q)
      const uint32_t pn_ = c_.x + c_.z;
      const bool sel_ = (c_.y | uint32_t(pn_ > sel_at) | uint32_t(!have_thr && pn_ >= A.keep)) != 0;
      if (tr_) TRACE_MARK(A, nd.q, e, MANAGER ? 1u : 0u, 6u);
      if (__ballot(sel_) != 0) { left = kLeftSelect; break; }
    }
    // ---- behind the hot loop: pending candidates first -- the manager's business, all waves wait ----------------
    // Left in front of a count barrier: the step before's have not been looked at yet.  Left behind a scan with the
    // pool or the step's own pending list overflowed: the step is swept again with every slice counted, its pending
    // candidates would come twice and are dropped; not overflowed: they are settled behind the compaction below, which
    // makes room in the pool's tail first.
    const bool own_pending = can_leave && left == kLeftSelect && ctl->overflow == 0;   // (uniform: written behind barriers only)
    if (can_leave) {
      if constexpr (MANAGER) {
        if (left == kLeftDone) BLURRILY_PEND_SETTLE((e & 1u) ^ 1u, (e - 1u) & 3u, p_prev, ls_prev);
        if (left == kLeftSelect && !own_pending && lane == 0) ctl->pend_n[s] = 0;
        // (the step's own pending candidates, where it was not swept again, stay on their list: the next step's scan phase
        // settles them like any step's -- the compaction below empties the pool's tail first, so they have their room.
        // Settling them here, synchronously, was a global round trip with sixteen waves waiting, at every other compaction.)
        p_prev = p; ls_prev = own_pending ? hy_ >> 24 : 0u;
        if (!ranked && have_thr && left != kLeftDone) BLURRILY_RANK();   // (the others are at the barrier: off the next step's count phase)
      }
      __syncthreads();
    }
    if (left == kLeftDone) break;
    // ---- the rare paths of step p ----------------------------------------------------------------
    pre_valid = false;                                          // (a unit loaded ahead is dropped)
    const uint32_t wbase = p * kWPS * kWindowRanks;
    const uint32_t wlen = min(kWPS * kWindowRanks, A.n_refs - wbase);
    // kLeftSelect: the step is scanned, select_after_scan finds the pool as the hot loop saw it; else: scan first
    bool scanned = left == kLeftSelect;
    for (;;) {
      if (!scanned) {
        scan_window<CT, NT, LEARNS>(A, nd, cnt128, pool, ctl, wbase, wlen, scan_pool_cap);
        __syncthreads();
      }
      scanned = false;
      if (!select_after_scan<NT>(A, pool, ctl, wbase, wlen, nd.q, scan_pool_cap)) break;
      ++st_redo;                                                // pool overflow: sweep step p again -- every slice of it
      if ((hy_ >> 24) != 0) BLURRILY_COUNT_WALK(p);             // (the published table lists no units of left-out slices)
      else if constexpr (!MANAGER) BLURRILY_COUNT_UNITS(s, n_units, false);
      __syncthreads();
    }
    thr_c = ctl->thr;
    thr_c = (static_cast<unsigned long long>(__builtin_amdgcn_readfirstlane(uint32_t(thr_c >> 32))) << 32) |
            __builtin_amdgcn_readfirstlane(uint32_t(thr_c));
    have_thr = thr_c != kKeyInf;
    ++e;
    h_next = ring->hdr4[e & 1];                                 // (published behind step p's count barrier)
    if constexpr (!MANAGER) ds_mine = BLURRILY_DESC_MINE(e & 1);
  }
  if constexpr (MANAGER) PHASE_FLUSH_MANAGER(A); else PHASE_FLUSH(A);
  // (counted build: the needle's steps, summed over its sweeps, in bits 31:23 of its path word -- tools/steps_hist.py)
  if (STATS(A) && A.path_flags && MANAGER && lane == 0) atomicAdd(&A.path_flags[nd.q], min(st_steps, 511u) << 23);
  if (STATS(A) && lane == 0) {
    atomicAdd(&STATS(A)[kStatPostingEntries], static_cast<unsigned long long>(st_ent));
    atomicAdd(&STATS(A)[kStatTableWords], static_cast<unsigned long long>(st_tab));
    if (wid == 0) {
      atomicAdd(&STATS(A)[kStatSteps], static_cast<unsigned long long>(st_steps));
      atomicAdd(&STATS(A)[kStatResweeps], static_cast<unsigned long long>(st_redo));
      atomicAdd(&STATS(A)[kStatStepsPastDesc], static_cast<unsigned long long>(st_past));
    }
  }
  if constexpr (MANAGER) __builtin_amdgcn_s_setprio(0);
  __syncthreads();                                              // ring and ctl quiet before the needle ends
#undef BLURRILY_PEND_SETTLE
#undef BLURRILY_MANAGER_TURN
#undef BLURRILY_COUNT_WALK
#undef BLURRILY_COUNT_UNITS
#undef BLURRILY_UNIT_STEP
#undef BLURRILY_PRELOAD
#undef BLURRILY_PRODUCE
#undef BLURRILY_RANK
#undef BLURRILY_RANK_ONE
#undef BLURRILY_LEAVE_OUT
#undef BLURRILY_UNIT_OF
#undef BLURRILY_UNIT_AT
#undef BLURRILY_DESC_MINE
#undef BLURRILY_DESC
#undef BLURRILY_TAB
#undef BLURRILY_PUBLISH_HDR
#undef BLURRILY_FETCH_TABLE
#undef BLURRILY_NEXT_VISIT
#undef BLURRILY_LOAD_WMT
#undef BLURRILY_STEP_AT
}

// ---- cooperative flavour (needles with <= 64 distinct trigrams: nearly all of them): the workgroup's last wave
// manages the sweep, the others work through it (sweep_role)
template <typename CT, int NT, bool LEARNS>
__device__ __forceinline__ void sweep_coop(const FindArgs& A, const Needle& nd, const uint16_t* codes, uint32_t* cnt32,
                                           unsigned long long* pool, Control* ctl, UnitRing* ring, const uint8_t* wmt,
                                           const uint32_t w0, const uint32_t w1, const uint32_t ws) {
  if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == NT / 64 - 1)
    sweep_role<CT, NT, true, LEARNS>(A, nd, codes, cnt32, pool, ctl, ring, wmt, w0, w1, ws);
  else
    sweep_role<CT, NT, false, LEARNS>(A, nd, codes, cnt32, pool, ctl, ring, wmt, w0, w1, ws);
}

// RANGED = latency mode (a needle's windows cut into ranges); a separate instantiation so the
// throughput kernel does not carry the extra live registers.  SHORT = the launch owns only
// needles with <= 64 distinct trigrams (one table slot per lane, which frees the registers for a
// fourth unit in flight); 65..127 follow in a launch over the tokeniser's mid list.
// Residency is set by LDS: two workgroups per CU with byte counters, one with 16-bit counters;
// the second launch bound (waves per SIMD) asks the register allocator for exactly that.
// Whether a sweep leaves dense slices out of a step's count is a RUN-TIME property of the launch (coop_can_leave: "nm_cmin",
// the pool's room, not phase 1 of the window-major sweep): one instantiation serves both (rounds 4-5: a template flag, LEAVE,
// and sweep_coop_plain without it).
template <typename CT, int NT, bool RANGED, bool SHORT>
__global__ __launch_bounds__(NT, (sizeof(CT) == 1 ? NT / 128 : NT / 256)) void find_kernel(const FindArgs A) {
  // The counters are a static array: their LDS address is a compile-time constant, so the
  // per-posting ds_add needs no base add.  Dynamic LDS behind them: candidate pool | slice table
  // (long needles) | control.
  constexpr uint32_t kCntBytes = kWindowSize * sizeof(CT);
  __shared__ __attribute__((aligned(16))) uint32_t s_counters[kCntBytes / 4];
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* cnt32 = s_counters;
  uint4*    cnt128 = reinterpret_cast<uint4*>(s_counters);
  unsigned long long* pool = reinterpret_cast<unsigned long long*>(smem);
  uint32_t* s_tab = reinterpret_cast<uint32_t*>(pool + A.pool_cap);   // [2][kCodeChunk], long needles only
  Control*  ctl = reinterpret_cast<Control*>(s_tab + 2 * kCodeChunk);
  UnitRing* ring = reinterpret_cast<UnitRing*>(reinterpret_cast<unsigned char*>(ctl) + 64);
  (void)ring;

  const uint32_t tid = threadIdx.x;

  for (uint32_t i = tid; i < kCntBytes / 16; i += NT) cnt128[i] = make_uint4(0, 0, 0, 0);
  // The per-window bound the sweep steps over windows with (win_max_tri) as bytes in LDS, once per workgroup:
  // the wave that chooses the next step reads it in a dependent loop just before the count barrier, and a global
  // round trip there is a wait for all sixteen waves (barrier after count: 1 392 of a step's 6 619 clocks).  It
  // lives in the slice table of the long-needle sweep, which the SHORT instantiations never use; clamped to 255,
  // exact for the <= 64 trigrams of a needle that gets here.
  const uint8_t* wmt = nullptr;
  if constexpr (SHORT) {
    if (A.n_windows <= 2 * kCodeChunk * 4) {
      uint8_t* w8 = reinterpret_cast<uint8_t*>(s_tab);
      for (uint32_t i = tid; i < A.n_windows; i += NT) w8[i] = uint8_t(min(A.win_max_tri[i], 255u));
      wmt = w8;
    }
  }
  (void)wmt;
  __syncthreads();

  // (as a scalar: loaded through a VGPR it stayed in one for the kernel's lifetime -- in scratch, that is)
  const uint32_t n_work = __builtin_amdgcn_readfirstlane(A.n_work_dev ? *A.n_work_dev : A.n_work);

  PHASE_NEEDLE_DECL;
  for (;;) {
    __builtin_amdgcn_s_setprio(kSerialPrio);        // between two needles: one chain of round trips
    if (tid == 0) ctl->q = atomicAdd(A.queue, 1u);
    __syncthreads();
    const uint32_t slot = ctl->q;
    __syncthreads();                                   // everyone has read q before it is rewritten
    if (slot >= n_work) break;
    // latency mode: a needle's windows are cut into `ranges` tasks swept by different workgroups
    const uint32_t R = RANGED ? A.ranges : 1u;
    // (tasks are numbered range by range, every needle's LAST range first: the windows of the longest references are a long
    // needle's dearest -- one to a step beyond nib_windows -- and a batch of more tasks than workgroups ends with the tasks
    // started last: the cheap ones, then)
    const uint32_t n_items = RANGED ? n_work / R : 0u;
    const uint32_t item = RANGED ? slot % n_items : slot, range = RANGED ? R - 1u - slot / n_items : 0u;
    const uint32_t part = RANGED ? item * R + range : 0u;      // where the task leaves its keys (merge_parts_*: needle by needle)
    (void)part;
    const uint32_t q = A.work_list ? A.work_list[item] : item;
    // (ranges start on even windows: the 4-bit sweep takes windows in pairs)
    const uint32_t n_pairs = (A.n_windows + 1) / 2;
    // (own_only: the window pair of the needle's own length class -- phase 1 of the window-major sweep)
    const bool own_only = !RANGED && A.own_only;
    const uint32_t own0 = own_only ? (A.q_start[q] & ~1u) : 0u;
    const uint32_t w0 = RANGED ? 2 * uint32_t(uint64_t(n_pairs) * range / R) : own0;
    const uint32_t w1 = RANGED ? min(A.n_windows, 2 * uint32_t(uint64_t(n_pairs) * (range + 1) / R))
                               : own_only ? min(A.n_windows, own0 + 2) : A.n_windows;
    Needle nd;
    nd.q = q;
    nd.T = A.q_ntri[q];
    nd.learn = false;
    if (!A.work_list && nd.T > (SHORT ? 64u : 127u)) { // longer needles: the mid / wide-counter launches
      if (RANGED && tid == 0) A.part_count[part] = 0;
      // (latency mode: a task that ends here goes through a barrier of its own before the next pop.  Without it a needle of
      // more than 64 distinct trigrams in a batch small enough for ranges -- up to 224 needles -- never came back: the
      // ranged launch spun on its queue's barriers (every round of this kernel until round 6's last day; the suite's long
      // needles had only met it in large batches and on images too small for ranges).  tests/test_gpu_find_one.py)
      if (RANGED) __syncthreads();
      continue;
    }
    const uint32_t have = A.pass_base ? A.counts[q] : 0u;
    if (A.q_nb[q] == 0 || A.keep == 0 || have < A.pass_base) {
      if (tid == 0 && A.pass_base == 0) {
        if (RANGED) A.part_count[part] = 0; else A.counts[q] = 0;
      }
      if (RANGED) __syncthreads();                     // (as above)
      continue;
    }
    const uint16_t* codes = A.qcodes + A.offsets[q] + q;
    // the sweep starts at the window of the needle's own length class (inside this task's range)
    // -- worth it only when there are enough windows for the early threshold to pay back the
    // ties it forfeits (a window behind the threshold's rank needs one match more)
    const uint32_t qs = A.q_start[q];
    const uint32_t ws = ((w1 - w0 >= 8 || own_only) && qs >= w0 && qs < w1) ? qs : w0;
    // results after this key only (later passes of a limit larger than the pool)
    nd.has_floor = A.pass_base != 0;

    if (tid == 0) {
      ctl->pool_n = 0; ctl->overflow = 0; ctl->thr = kKeyInf;
      ctl->adm_n = 0; ctl->pend_n[0] = 0; ctl->pend_n[1] = 0;
      if (nd.has_floor) ctl->floor = A.floor[q];
    }
    __syncthreads();

    PHASE_NEEDLE(10);
    PATH_FLAG(A, q, (sizeof(CT) == 2 ? kPathWide : 0u) | (RANGED ? kPathRanged : 0u) | (nd.has_floor ? kPathMultiPass : 0u) |
                    (own_only ? kPathOwnOnly : 0u));
    __builtin_amdgcn_s_setprio(0);
    if (STATS(A) && tid == 0) atomicAdd(&STATS(A)[kStatTasks], 1ull);
    // (a macro, not a closure: closures capturing the kernel arguments end up in scratch memory)
#define BLURRILY_SWEEP(a_, b_, start_)                                                                  \
  do {                                                                                                  \
    const uint32_t sa = (a_), sb = (b_), st = (start_);                                                 \
    if constexpr (SHORT) {                                                                              \
      /* 4-bit counters, two windows per step: every window for a needle with <= 15 trigrams, and for   \
         ANY needle the leading windows whose references have <= 15 trigrams (ranks follow weight, i.e. \
         length: about half the windows at Geonames scale) -- a counter there cannot exceed 15 whatever \
         the needle.  The byte-counter part goes first: it holds the needle's own length class. */      \
      const uint32_t nib_end = nd.T <= 15 ? sb : min(sb, max(sa, A.nib_windows));                       \
      if (nib_end < sb)                                                                                 \
        sweep_coop<CT, NT, RANGED>(A, nd, codes, cnt32, pool, ctl, ring, wmt, nib_end, sb, max(st, nib_end)); \
      if (sa < nib_end)                                                                                 \
        sweep_coop<Nib, NT, RANGED>(A, nd, codes, cnt32, pool, ctl, ring, wmt, sa, nib_end, min(st, nib_end - 1)); \
    } else if constexpr (sizeof(CT) == 1) {      /* byte counters: T <= 127 by construction */          \
      sweep_pipelined<CT, NT>(A, nd, codes, cnt32, pool, ctl, sa, sb, st);                              \
    } else {                                                                                            \
      if (nd.T <= kCodeChunk) sweep_pipelined<CT, NT>(A, nd, codes, cnt32, pool, ctl, sa, sb, st);    \
      else                    sweep_chunked<CT, NT>(A, nd, codes, cnt32, pool, s_tab, ctl, sa, sb);     \
    }                                                                                                   \
  } while (0)
    uint32_t sw_a = 0, sw_b = 0, sw_st = 0;
    (void)sw_a; (void)sw_b; (void)sw_st;
#define BLURRILY_SWEEP_ARGS(a_, b_, st_) do { sw_a = (a_); sw_b = (b_); sw_st = (st_); } while (0)
    if constexpr (RANGED) {
      // A range that does not contain the needle's own length class first sweeps that window
      // only to learn a threshold (the keep-th best of real candidates bounds the answer), then
      // forgets those candidates -- the range that owns the window reports them -- and sweeps
      // its own windows with few admissions instead of a cold start.  (It pays even for a range
      // of one step: without it a single needle takes 88 us instead of 81.)
      // (ONE expansion of the sweep serves both: two of them -- four inlined sweeps -- cost the latency-mode
      // kernel 380 spilled registers)
      const bool learn = qs < A.n_windows && !(qs >= w0 && qs < w1);
      for (uint32_t pass = learn ? 0u : 1u; pass < 2u; ++pass) {
        if (pass == 0) {
          BLURRILY_SWEEP_ARGS(qs, qs + 1, qs);
        } else {
          BLURRILY_SWEEP_ARGS(w0, w1, ws);
        }
        nd.learn = pass == 0;
        BLURRILY_SWEEP(sw_a, sw_b, sw_st);
        if (pass == 0) {
          compact_pool<NT>(pool, ctl, A.pool_cap, A.keep, SHORT && coop_can_leave(A) ? A.pool_cap - adm_max(A.pool_cap) : A.pool_cap);
          if (tid == 0) ctl->pool_n = 0;
          __syncthreads();
        }
      }
    } else {
      BLURRILY_SWEEP(w0, w1, ws);
    }
#undef BLURRILY_SWEEP_ARGS
#undef BLURRILY_SWEEP
    PHASE_NEEDLE(11);

    // ---- emit: best `keep` in final order; weights are looked up only here ---------------
    compact_pool<NT>(pool, ctl, A.pool_cap, A.keep, SHORT && coop_can_leave(A) ? A.pool_cap - adm_max(A.pool_cap) : A.pool_cap);
    __builtin_amdgcn_s_setprio(kSerialPrio);
    const uint32_t nres = ctl->pool_n;
    if (RANGED) {
      // latency mode: leave this range's best keys for merge_parts_kernel
      for (uint32_t i = tid; i < nres; i += NT) A.part_keys[size_t(part) * A.keep + i] = pool[i];
      if (tid == 0) A.part_count[part] = nres;
      __syncthreads();
      continue;
    }
    if (own_only) {
      // the needle's state for wsweep_kernel: its best keys so far, two words each, where its rows will be
      uint32_t* st = reinterpret_cast<uint32_t*>(A.results + size_t(q) * A.limit);
      for (uint32_t i = tid; i < nres; i += NT) {
        const unsigned long long key = pool[i];
        st[2 * i] = uint32_t(key); st[2 * i + 1] = uint32_t(key >> 32);
      }
      if (tid == 0) A.counts[q] = nres;
      __syncthreads();
      continue;
    }
    trigram_match_t* out = A.results + size_t(q) * A.limit + A.pass_base;
    for (uint32_t i = tid; i < nres; i += NT) {
      const unsigned long long key = pool[i];
      const uint32_t rk = uint32_t(key);
      trigram_match_t r;
      r.reference = A.ref_of_rank[rk];
      r.matches = nd.T - uint32_t(key >> 32);
      r.weight = A.weight_of_rank[rk];
      out[i] = r;
    }
    if (tid == 0) {
      A.counts[q] = A.pass_base + nres;
      if (A.floor && nres > 0) A.floor[q] = pool[nres - 1];
    }
    __syncthreads();                                   // pool reads done before the next needle resets it
    PHASE_NEEDLE(12);
  }
}
