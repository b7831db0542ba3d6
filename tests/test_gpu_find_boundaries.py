"""Every sweep of the core find at its needle-class and counter boundaries, on the two maps of
tests/boundary_case.py: needles of EXACTLY 1, 2, 15, 16, 17, 64, 65, 127, 128, 129, 255, 256, 257 and 1 200 distinct
trigrams, needles whose byte length and trigram count fall on different sides of 64 and 127, references that put a counter
exactly on its ceiling, a 16-trigram reference exactly on the last rank of a window pair.

Every route is forced through the map's options and ASSERTED TAKEN ("last_sweep", last_kernels(), "one_taken", the path
flags).  In every route every needle's rows equal the oracle's, the counted build's rows equal the timed build's, and the
per-needle path flags equal a table written here from the kernels' dispatch rules, keyed by T.  Flags that depend on
the data met on the way (cold start, compaction, a step swept again or stepped over) are left out of that comparison;
the ones an assertion below names are checked there."""
import ctypes as C

import numpy as np
import pytest

from blurrily_amd import _native
from boundary_built import (COPIES, LEAVE, PLAIN, SMALL, WINDOW_MAJOR, Built, F, counters_of,  # noqa: F401
                            passes_of, STRUCT, names)

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module", params=["a", "b"])
def built(request):
    b = Built(request.param)
    yield b
    b.m.close()


# ---- 1. the plain needle-major sweep; 2. its later passes ------------------------------------------------------------
@pytest.mark.parametrize("limit", [1, 10, 64, 65, 1024])
def test_plain_needle_major_sweep(built, limit):
    b = built
    b.options(PLAIN)
    flags, sweep, kernels = b.check(b.many, limit, COPIES)
    assert sweep == 1 and kernels[0] == "find_kernel<uint8_t,1024,false,true>", (sweep, kernels)
    assert "find_kernel<uint16_t,1024,false,false>" in kernels and "find_kernel<uint8_t,1024,false,false>" in kernels
    b.assert_flags(flags, lambda i, t: counters_of(t, b.which) | passes_of(b, i, t, limit), ("plain", limit))


@pytest.mark.parametrize("limit", [1025, 65535])
def test_later_passes_start_behind_a_tie(built, limit):
    """Limits beyond a pass: the row at position 1 024 / 1 025 (256 / 257 for the 16-bit needles) lies across a tie on
    (matches, weight) -- tests/test_boundary_case.py -- so the floor key's rank alone separates the passes."""
    b = built
    b.options(PLAIN)
    flags, sweep, kernels = b.check(b.once, limit, 1)
    assert sweep == 1
    b.assert_flags(flags, lambda i, t: counters_of(t, b.which) | passes_of(b, i, t, limit), ("passes", limit))
    multi = [t for i, t in enumerate(b.T.tolist()) if flags[i] & F["multi_pass"]]
    assert {15, 16, 64, 65, 127, 128, 1200} <= set(multi), multi


# ---- 3. the needle-major sweep that leaves dense slices out ------------------------------------------------------------
@pytest.mark.parametrize("cmin", [1, 3])
@pytest.mark.parametrize("limit", [10, 149, 150])
def test_slices_left_out(built, limit, cmin):
    """find_can_leave: limits up to 149 have room in the pool for the settled candidates, 150 has not and is served by
    the plain sweep.  A step leaves min(need - "nm_cmin", 8) dense slices out once the needle has a threshold
    (needle_major.inc: BLURRILY_PRODUCE), so never in the step a sweep starts with.  Every class needle of 15 .. 64
    trigrams starts with the hot word, whose four slices are dense in all three windows, and more than 149 references
    of every window hold those four: whichever window the sweep of a 16 .. 64 needle starts in, a later step needs
    four matches or more and holds a reference that has them partly in the left-out slices -- hot fillers in windows 0
    and 1, the twin and the superstring in window 2 -- which is then settled through the bitmaps ("nm_left_out")."""
    b = built
    b.options(dict(LEAVE, nm_cmin=cmin))
    flags, sweep, kernels = b.check(b.many, limit, COPIES)
    b.assert_flags(flags, lambda i, t: counters_of(t, b.which), ("leave", limit, cmin))
    left = {t for i, t in enumerate(b.T.tolist()) if flags[i] & F["nm_left_out"]}
    print("leave", b.which, limit, cmin, sweep, sorted(left))
    if limit == 150:
        assert sweep == 1 and not left, (sweep, left)
    else:
        assert sweep == 3
        assert left <= {t for t in b.T.tolist() if 15 < t <= 64}, left     # (T <= 15: two steps, see the next test)
        assert {16, 17, 64} <= left, left


@pytest.fixture(scope="module")
def built_long():
    b = Built("c")
    yield b
    b.m.close()


@pytest.mark.parametrize("cmin", [1, 3])
@pytest.mark.parametrize("limit", [10, 149])
def test_slices_left_out_of_a_4_bit_sweep(built_long, limit, cmin):
    """A needle of at most 15 trigrams sweeps windows in pairs, and a step's table is published -- with what it leaves
    out -- while the step before is counted: on three windows the second and last step is out before the first has
    given a threshold, so nothing is ever left out for such a needle there.  Map C has five windows; window 4 has dense
    slices and a second twin of every short class needle, which the third step settles through the bitmaps.  At
    "nm_cmin" 1 that holds for T = 2 as well (two matches needed behind the threshold's rank, one slice left out); T = 1
    can never need more than one."""
    b = built_long
    b.options(dict(LEAVE, nm_cmin=cmin))
    flags, sweep, kernels = b.check(b.many, limit, COPIES)
    assert sweep == 3
    b.assert_flags(flags, lambda i, t: counters_of(t, "a"), ("leave, five windows", limit, cmin))
    left = {t for i, t in enumerate(b.T.tolist()) if flags[i] & F["nm_left_out"]}
    print("leave c", limit, cmin, sorted(left))
    assert left <= {t for t in b.T.tolist() if cmin < t <= 64}, left
    assert ({2, 15, 16, 17, 64} if cmin == 1 else {15, 16, 17, 64}) <= left, left


# ---- 4. the window-major sweep -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [10, 128, 129])
def test_window_major_sweep(built, limit):
    """kWsMaxKeep: limits up to 128.  Phase 1 sweeps the window pair of the needle's own length class ("own_only"): the
    weights are 1 and 2, so a needle of two bytes and more starts at window 2 -- alone in its pair, byte counters for
    T > 15 whatever "nib_windows" is -- and the empty and the one-letter needle at the pair (0, 1).  The other windows
    are the window-major tasks'; needles of more than 64 trigrams go to the mid and 16-bit launches behind."""
    b = built
    b.options(WINDOW_MAJOR)
    flags, sweep, kernels = b.check(b.many, limit, COPIES)
    c = b.case
    if limit == 129:
        assert sweep == 1 and "wsweep_kernel" not in "+".join(kernels), (sweep, kernels)
        b.assert_flags(flags, lambda i, t: counters_of(t, b.which), ("not window-major", limit))
        return
    assert sweep == 2 and any(k.startswith("wsweep_kernel") for k in kernels), (sweep, kernels)

    def expect(i, t):
        if t > 64:
            return counters_of(t, b.which)
        return F["own_only"] | F["ws_task"] | counters_of(t, b.which, own_window_only=len(c.needles[i]) >= 2)
    b.assert_flags(flags, expect, ("window-major", limit))
    short = [i for i, t in enumerate(b.T.tolist()) if t <= 64]
    assert any(flags[i] & F["ws_left_out"] for i in short)
    # "ws_wide": byte counters where min(T - L, win_max_tri) > 15 -- never for T <= 15, never on map A (its window 2 is
    # every longer needle's own, windows 0 and 1 hold 15 trigrams at most); on map B window 1 holds X's 16
    wide = {t for i, t in enumerate(b.T.tolist()) if flags[i] & F["ws_wide"]}
    print("ws_wide", b.which, limit, sorted(wide))
    assert wide <= ({t for t in b.T.tolist() if 16 <= t <= 64} if b.which == "b" else set()), wide
    if b.which == "b":
        # the T = 64 class needle: its task in window 1 needs at most one match more than its last row has, m + 1 <= 16 =
        # win_max_tri, so the task runs; it leaves out at most need - "ws_cmin" <= m - 2 slices, and 64 - (m - 2) > 15
        i = c.classes[64]
        m_last = int(b.want(limit)["rows"][i, limit - 1, 1])
        assert b.want(limit)["counts"][i] == limit and m_last + 1 <= 16, m_last
        assert 64 in wide, wide


# ---- 5. the small-haystack sweep ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [64, 65])
def test_small_haystack_sweep(built, limit):
    """kSmallMaxKeep: limits up to 64.  T <= 15 is the sweep's own; 16 .. 64 it lists for the byte launch behind it
    (over_list), 65 .. 127 the tokeniser listed for the mid launch."""
    b = built
    b.options(SMALL)
    flags, sweep, kernels = b.check(b.many, limit, COPIES)
    if limit == 65:
        assert sweep == 1 and not any(flags & F["small"]), sweep
        b.assert_flags(flags, lambda i, t: counters_of(t, b.which), ("not small", limit))
        return
    assert sweep == 4 and kernels[0].startswith("find_small_kernel"), (sweep, kernels)
    b.assert_flags(flags, lambda i, t: counters_of(t, b.which) | (F["small"] if t <= 15 else 0), ("small", limit))


# ---- 6. latency mode on the device entry -------------------------------------------------------------------------------
def _device_find(m, packed, off, limit):
    import torch
    dev = torch.device("cuda", 0)
    n = len(off) - 1
    d_packed = torch.from_numpy(np.concatenate([packed, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_rows = torch.zeros((n, limit, 3), dtype=torch.int32, device=dev)
    d_counts = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_nb = torch.full((n,), -1, dtype=torch.int32, device=dev)
    res = _native.lib().blurrily_storage_find_batch_device(m.handle, d_packed.data_ptr(), int(off[-1]), d_off.data_ptr(), n,
                                                           limit, d_rows.data_ptr(), d_counts.data_ptr(), d_nb.data_ptr(),
                                                           torch.cuda.current_stream().cuda_stream)
    assert res == 0, C.get_errno()
    torch.cuda.synchronize()
    return d_rows.cpu().numpy().view(np.uint32), d_counts.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("limit", [10, 64, 65])
def test_latency_mode_on_the_device_entry(built, limit):
    """The needle list once, device-resident: twenty needles cannot fill the chip, so every short needle's windows are
    cut into ranges of whole window pairs (find_run.hip: latency_ranges).  Three windows are the smallest image that
    is cut at all -- two ranges, (0, 1) and (2) -- so no window had to be appended.  A range that does not hold the
    needle's own window first learns a threshold there: a 16 .. 64 needle meets both counter widths on map A."""
    b = built
    b.options(PLAIN)
    m, n = b.m, len(b.T)
    m.set_stats(True)
    rows, counts = _device_find(m, *b.once, limit)
    flags, kernels = m.find_path_flags(n), m.last_kernels()
    m.set_stats(False)
    want = b.want(limit)
    live = np.arange(limit)[None, :] < want["counts"][:, None].astype(np.int64)
    assert np.array_equal(counts, want["counts"])
    assert np.array_equal(np.where(live[:, :, None], rows, 0), np.where(live[:, :, None], want["rows"], 0))
    rows_t, counts_t = _device_find(m, *b.once, limit)
    assert np.array_equal(counts_t, counts) and np.array_equal(np.where(live[:, :, None], rows_t, 0), np.where(live[:, :, None], rows, 0))
    assert kernels[0] == "find_kernel<uint8_t,1024,true,true>", kernels
    b.assert_flags(flags, lambda i, t: counters_of(t, b.which) | (F["ranged"] if t <= 64 else 0), ("latency", limit))


# ---- 7. host batches over the pinned page; 8. the single find ----------------------------------------------------------
def _host_batch(b, needles, limit, taken):
    m = b.m
    before = m.get_option("one_taken")
    rows, counts = m.find_batch_packed(*b.case.pack(needles), limit)
    assert (m.get_option("one_taken") > before) == taken, (len(needles), limit, taken)
    for i, nd in enumerate(needles):
        assert rows[i, :counts[i]].tolist() == b.o.find(nd, limit), (b.which, len(needles), limit, i, len(nd))
    return m.last_kernels()


@pytest.mark.parametrize("n", [1, 16, 17, 24, 25, 128])
def test_host_batches_over_the_pinned_page(built, n):
    """host_batch.hip: find_few takes up to kMidMaxNeedles = 128 needles of at most 64 trigrams at limits up to
    kOneMaxKeep = 120 -- up to sixteen as kernel arguments, up to "few_max" = 24 through find_one_kernel, more in
    latency mode over the pinned page -- their codes in a [needle][64] block that a 64-trigram needle fills to its last
    slot.  One needle of 65 trigrams, or limit 121, sends the batch the copying way; the rows are the same."""
    b = built
    b.options(PLAIN)
    c = b.case
    short = [nd for nd, t in zip(c.needles, c.T) if t <= 64 and len(nd) <= 255]   # (find_few takes needles of up to 255 bytes)
    full = [nd for nd, t in zip(c.needles, c.T) if t == 64]      # the class needle, 63 bytes, 64 bytes with a repeat
    assert len(full) == 3
    batch = (full + short * 16)[:n] if n > 1 else full[2:]       # (alone: the 64-byte one -- the host's length rule says "maybe mid")
    batch = batch[1:] + batch[:1]                                 # a 64-trigram needle in the LAST row of the block
    kernels = _host_batch(b, batch, 120, True)
    assert kernels[0].startswith("find_one_kernel" if n <= 24 else "find_kernel<uint8_t,1024,true,true>"), kernels
    _host_batch(b, batch, 121, False)
    mid = c.needles[c.classes[65]]
    _host_batch(b, batch[:-1] + [mid], 120, False)


def test_single_find_per_class(built):
    """blurrily_storage_find: its own launch for T <= 64, the batch's way from 65 on."""
    b = built
    b.options(PLAIN)
    m, c = b.m, b.case
    for nd, t in zip(c.needles, c.T):
        before = m.get_option("one_taken")
        assert m.find(nd, 10) == b.o.find(nd, 10), (b.which, t, len(nd))
        assert (m.get_option("one_taken") > before) == (t <= 64 and len(nd) <= 255), (t, len(nd))


# ---- 9. the delta image and tombstones (last: it changes the maps) -----------------------------------------------------
def test_second_twins_in_the_delta_image_and_the_first_ones_deleted(built):
    """After the base build every needle's twin is put again under a new reference (the delta image) and the base twin is
    deleted (a tombstone bit): the row the twin held is the new reference's.  The sweeps run again; "tombstone" shows
    where the deleted twin passed the threshold and was dropped for its bit.  One base build."""
    b = built
    m, o, c = b.m, b.o, b.case
    w = c.weights(b.which)
    try:
        for i in range(len(c.needles)):
            twin = c.ref_at(i, 0)
            wt = int(w[c._at[twin]])
            assert m.put(c.needles[i], 900000 + i, wt) == o.put(c.needles[i], 900000 + i, wt)
            assert m.delete(twin) == o.delete(twin) > 0
        b._want.clear()
        b.options(PLAIN)
        flags, sweep, kernels = b.check(b.many, 10, COPIES)
        assert sweep == 1
        b.assert_flags(flags, lambda i, t: counters_of(t, b.which), ("plain over tombstones", 10))
        tomb = {t for i, t in enumerate(b.T.tolist()) if flags[i] & F["tombstone"]}
        print("tombstone", b.which, sorted(tomb))
        assert tomb == set(b.T.tolist()), tomb                    # (a twin has every match there is: it passes any threshold)
        for i in range(len(c.needles)):                           # the new twin holds a row of T matches, the old one none
            full = [r[0] for r in b.want(10)["rows"][i, :b.want(10)["counts"][i]].tolist() if r[1] == c.T[i]]
            assert 900000 + i in full and c.ref_at(i, 0) not in full, (c.T[i], full)
        b.options(WINDOW_MAJOR)
        _, sweep, _ = b.check(b.many, 10, COPIES)
        assert sweep == 2
        b.options(SMALL)
        _, sweep, _ = b.check(b.many, 10, COPIES)
        assert sweep == 4
        b.options(PLAIN)
        short = [nd for nd, t in zip(c.needles, c.T) if t <= 64 and len(nd) <= 255]
        for n in (1, 16, 25, 128):
            _host_batch(b, (short * 16)[:n], 120, True)
        info = m.device_info()
        assert info["base_builds"] == 1 and info["n_pending"] == len(c.needles) == info["n_tombstones"], info
    finally:
        c._oracles.pop(b.which, None)                             # the oracle was changed with the map: the next user builds its own
