"""The plain find on tests/dense_delta_case.py's map, and the log budget's edge.

run_find_on makes the same choice of sweep for the delta image as for the base, the needle-major sweep that leaves dense
slices out and the window-major sweep's dense handling included; the suite's tests of both sweeps with pending puts
(tests/test_gpu_leave.py, tests/test_gpu_wsweep.py) put 300 strings under "dense_min" 256, a delta image without a bitmap.
Here the delta image has 1 175 dense slices, and the base image's tombstones sit behind bitmaps.  The same base and
mutations under tests/test_gpu_leave.py's forced options, under tests/test_gpu_wsweep.py's, and with everything at its
default except "dense_min"; every row of find_batch_packed at limits 1, 10 and 100 against an oracle that replays every
put and delete.  The path flags' left-out counts are printed, not asserted: nothing in the API tells which image set a
flag.  (On an MI355X both counts were 0 under all three sets of options and the tombstone flag was set for 2 071 of the
2 072 needles -- presumably because a needle leaves slices out only once it has a threshold, and here an image is one
window, or one and a small second.  So these rows prove the choice of sweep, the merge of the two images and the
tombstones on a dense delta image, not a candidate settled through left-out bitmaps; that wants images of more windows,
as tests/test_gpu_leave.py's.)

The log budget (map_log.hip): `pending + tombstones > max(4096, n_refs / 64)` rebuilds the base image, and a put that
finds `pending >= budget` stops logging.  The other tests go thousands past it; here a map of 3 000 words stands exactly
at 4 096, then one past.

Not covered: a delta image of more than one window or with ranks of 32 768 and more (a base of millions of references);
DeviceInfo.n_bitmaps counts the base image's bitmaps only."""
import numpy as np
import pytest

import dense_delta_case as C
import workloads as W
from blurrily_amd import RawMap
from blurrily_amd.map import _pack
from helpers import Oracle

pytestmark = pytest.mark.gpu
NM_LEFT_OUT, WS_LEFT_OUT, TOMBSTONE = 1 << 21, 1 << 15, 1 << 12   # find_kernels.h: kPathNmLeftOut, kPathWsLeftOut, kPathTombstone
SWEEP_WINDOWS, SWEEP_LEAVE = 2, 3                                  # find_choice.h: kSweepWindows, kSweepLeave
LIMITS = (1, 10, 100)
LEAVE = dict(ws_autotune=0, wsweep=0, nm_min_windows=0, small_sweep=0, nm_dense=64, nm_cmin=2)        # test_gpu_leave.py's _pair
WINDOWS = dict(ws_autotune=0, small_sweep=0, ws_min_slice=0, ws_static_slice=0, ws_min_windows=1, ws_min_needles=1000)
BUDGET = C.LOG_BUDGET


def _packed(strings):
    """_pack with the bytes as an array (what workloads.queries and the oracle's batch take)."""
    packed, offsets = _pack(strings)
    return np.frombuffer(packed, dtype=np.uint8), offsets


@pytest.fixture(scope="module")
def replay():
    """The oracle with every put and delete replayed, and the needles: tests/dense_delta_case.py's find needles and 2 000
    edited pending phrases."""
    h = C.host()
    o = Oracle()
    for r, s, w in zip(h.base.refs.tolist(), h.base.strings, h.base.weights.tolist()):
        assert o.put(s, r, w) > 0
    C.apply(o, h.steps)
    assert o.stats()["references"] == len(h.held)
    q, qo = W.queries(*_packed([h.held[int(r)] for r in h.phrases]), 2000, 84)
    packed, offsets = _packed(C.find_needles(h) + W.unpack(q, qo))
    return h, o, packed, offsets


def _check(m, o, packed, offsets, sweep, what):
    n = len(offsets) - 1
    for limit in LIMITS:
        m.set_stats(True)
        rows, counts = m.find_batch_packed(packed, offsets, limit)
        flags = m.find_path_flags(n)
        m.set_stats(False)
        if sweep is not None:
            assert m.get_option("last_sweep") == sweep, (what, limit, m.get_option("last_sweep"))
        print(f"{what}, limit {limit}: sweep {m.get_option('last_sweep')}, needles flagged nm_left_out "
              f"{int((flags & NM_LEFT_OUT != 0).sum())}, ws_left_out {int((flags & WS_LEFT_OUT != 0).sum())}, tombstone "
              f"{int((flags & TOMBSTONE != 0).sum())} of {n}")
        want = o.batch_upto(packed, offsets, limit, LIMITS[-1])
        assert np.array_equal(counts, want["counts"]), (what, limit)
        live = np.arange(limit)[None, :] < counts[:, None].astype(np.int64)
        bad = np.nonzero((np.where(live[:, :, None], rows, 0) != np.where(live[:, :, None], want["rows"], 0)).any(axis=(1, 2)))[0]
        if len(bad):
            i = int(bad[0])
            needle = bytes(packed[int(offsets[i]):int(offsets[i + 1])])
            raise AssertionError((what, limit, len(bad), i, needle[:60], rows[i, :counts[i]].tolist()[:12],
                                  want["rows"][i, :counts[i]].tolist()[:12]))
        # ... and the uncounted build of the same kernels writes the same rows
        rows_u, counts_u = m.find_batch_packed(packed, offsets, limit)
        assert np.array_equal(counts_u, counts) and np.array_equal(np.where(live[:, :, None], rows_u, 0),
                                                                   np.where(live[:, :, None], rows, 0)), (what, limit)


@pytest.mark.parametrize("what,options,sweep", [("slices left out", LEAVE, SWEEP_LEAVE), ("window-major", WINDOWS, SWEEP_WINDOWS),
                                                ("defaults", {}, None)])
def test_find_batch_equals_the_oracle_row_for_row_on_both_images(replay, what, options, sweep):
    h, o, packed, offsets = replay
    m, _ = C.build(options)
    try:
        _check(m, o, packed, offsets, sweep, what)
        C.assert_log(m, h)                                          # (two images and tombstones all along)
        # a deleted twin and a moved row's old text are not found; the moved row is, under its new weight
        for x, twin in zip(h.twin_heads, h.twins):
            got = [r[0] for r in m.find(h.held[x], 10)]
            assert x in got and twin not in got
        for r in h.moved:
            assert m.find(h.held[r], 1) == [[r, h.T(r), h.weight_of[r]]]
    finally:
        m.close()


# ---- the log budget's edge -------------------------------------------------------------------------------------------------

N_WORDS, N_PUTS, N_DELETES = 3000, 4000, 96


def _small_pair():
    hay, off = W.words(N_WORDS, seed=85)
    m, o = RawMap(), Oracle()
    refs = np.arange(1, N_WORDS + 1, dtype=np.uint32)
    m.put_many_packed(hay, off, refs)
    o.put_many(hay, off)
    m.sync_device()
    more, mo = W.words(BUDGET + 1, seed=86)
    extra = [s + b" x" for s in W.unpack(more, mo)]              # (no string of the base)
    q, qo = W.queries(hay, off, 300, 87)
    needles = _packed(W.unpack(q, qo) + extra[:40] + extra[-40:])
    return m, o, extra, needles


def _put(m, o, strings, ref0):
    refs = np.arange(ref0, ref0 + len(strings), dtype=np.uint32)
    assert m.put_many_packed(*_pack(strings), refs, np.zeros(len(strings), dtype=np.uint32)) > 0
    for r, s in zip(refs.tolist(), strings):
        o.put(s, r, 0)


def _rows_equal(m, o, needles, limit=10):
    rows, counts = m.find_batch_packed(*needles, limit)
    want = o.batch(*needles, limit=limit)
    live = np.arange(limit)[None, :] < counts[:, None].astype(np.int64)
    assert np.array_equal(counts, want["counts"])
    assert np.array_equal(np.where(live[:, :, None], rows, 0), np.where(live[:, :, None], want["rows"], 0))
    return rows, counts


def _log(m):
    info = m.device_info()
    return info["base_builds"], info["n_pending"], info["n_tombstones"]


def test_a_log_of_exactly_its_budget_is_served_by_two_images_and_one_more_delete_rebuilds_the_base():
    m, o, extra, needles = _small_pair()
    try:
        assert max(BUDGET, N_WORDS // 64) == BUDGET == N_PUTS + N_DELETES
        _put(m, o, extra[:N_PUTS], 10 ** 6)
        for r in range(1, 1 + 7 * N_DELETES, 7):
            assert m.delete(r) == o.delete(r) > 0
        assert _log(m) == (1, N_PUTS, N_DELETES)
        at_budget = _rows_equal(m, o, needles)
        assert _log(m) == (1, N_PUTS, N_DELETES)                   # pending + tombstones == budget: no rebuild
        assert m.delete(2) == o.delete(2) > 0                      # one past it
        assert _log(m) == (1, N_PUTS, N_DELETES + 1)
        past = _rows_equal(m, o, needles)
        assert _log(m) == (2, 0, 0)
        # the same rows from one image as from two: the oracle's both times, the deleted reference in none
        live = np.arange(10)[None, :] < past[1][:, None].astype(np.int64)
        assert not ((past[0][:, :, 0] == 2) & live).any() and (at_budget[1] > 0).sum() == (past[1] > 0).sum()
    finally:
        m.close()


def test_the_put_that_finds_the_log_full_stops_logging_and_the_next_find_rebuilds():
    m, o, extra, needles = _small_pair()
    try:
        _put(m, o, extra[:BUDGET], 10 ** 6)
        assert _log(m) == (1, BUDGET, 0)
        _rows_equal(m, o, needles)
        assert _log(m) == (1, BUDGET, 0)                           # 4 096 pending: the delta image serves them
        _put(m, o, extra[BUDGET:], 2 * 10 ** 6)                    # the 4 097th put finds pending >= budget: logging stops
        assert _log(m)[:2] == (1, 0)
        rows, counts = _rows_equal(m, o, needles)
        assert _log(m) == (2, 0, 0)
        assert (rows[:, 0, 0] == 2 * 10 ** 6).any()                # the last put is found, from the rebuilt base
    finally:
        m.close()
