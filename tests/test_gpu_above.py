"""Threshold find on the GPU (above.hip, above_kernels.hip: above_sweep_kernel, above_rows_kernel): every row with at
least the needle's bar of matches, bar = max(1, min_matches, ceil(min_permille * T / 1000)), equals the oracle's
complete find (limit >= the haystack) filtered to matches >= bar, row for row and in order -- over the oracle cases, a
multi-window haystack, needles at the counter-width boundaries, batch shapes, mutations, by reference, the capacity
protocol, and beside the top-k find, which it leaves as it was."""
import ctypes as C
import errno

import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, RawMap, _native
from blurrily_amd.map import _pack
from above_truth import Truth, bar
from helpers import ORACLE_CASES, HIP_CASES, Oracle, hip_case_inputs, oracle_case_inputs

pytestmark = pytest.mark.gpu
MATCHES = (0, 1, 2, 3)
PERMILLE = (0, 1, 500, 999, 1000)


def want_rows(full, T, mm, mp):
    t = bar(T, mm, mp)
    if T == 0 or t > T:
        return []
    return [r for r in full if r[1] >= t]


def split(rows, row_off):
    return [rows[int(row_off[i]):int(row_off[i + 1])].tolist() for i in range(len(row_off) - 1)]


def _load(strings, refs=None, weights=None):
    m, o = RawMap(), Oracle()
    refs = np.arange(1, len(strings) + 1, dtype=np.uint32) if refs is None else np.asarray(refs, dtype=np.uint32)
    weights = np.zeros(len(strings), dtype=np.uint32) if weights is None else np.asarray(weights, dtype=np.uint32)
    packed, offsets = _pack(strings)
    m.put_many_packed(packed, offsets, refs, weights)
    for s, r, w in zip(strings, refs.tolist(), weights.tolist()):
        o.put(s, r, w)
    return m, o


_CASES = {}


def oracle_case(kind, n):
    if (kind, n) not in _CASES:
        hay, off, needles = oracle_case_inputs(kind, n)
        strings = W.unpack(hay, off)
        m, o = _load(strings)
        _CASES[(kind, n)] = (m, o, strings, needles)
    return _CASES[(kind, n)]


@pytest.mark.parametrize("kind,n,_limit", ORACLE_CASES)
def test_rows_equal_the_oracle_filtered_at_every_bar(kind, n, _limit):
    m, o, strings, needles = oracle_case(kind, n)
    full = [o.find(s, min(65535, n)) for s in needles]
    T = [len(Oracle.tokenise(s)) for s in needles]
    packed, offsets = _pack(needles)
    for mm in MATCHES:
        for mp in PERMILLE:
            rows, row_off = m.find_batch_above_packed(packed, offsets, mm, mp)
            got = split(rows, row_off)
            for i, s in enumerate(needles):
                assert got[i] == want_rows(full[i], T[i], mm, mp), (kind, s, mm, mp)
    # a bar of T and of T + 1 matches, needle by needle
    for i, s in enumerate(needles[:40]):
        for mm in (T[i], T[i] + 1):
            for mp in (0, 500, 1000):
                assert m.find_above(s, mm, mp) == want_rows(full[i], T[i], mm, mp), (kind, s, mm, mp)


def _needle_of(rng, t):
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz ", dtype=np.uint8)
    while True:
        s = bytes(rng.choice(letters, size=t + 40).tolist())
        codes = Oracle.tokenise(s)
        if len(codes) >= t:
            # cut to exactly t distinct trigrams where a prefix has them
            for k in range(t - 1, len(s) + 1):
                if len(Oracle.tokenise(s[:k])) == t:
                    return s[:k]


def test_needle_shapes_at_the_class_and_counter_boundaries():
    m, o, strings, _ = oracle_case("geonames", 30000)
    rng = np.random.default_rng(41)
    needles = [_needle_of(rng, t) for t in (16, 64, 65, 127, 128)]
    long_ = bytes(rng.choice(np.frombuffer(b"abcdefghijklmnopqrstuvwxyz ", dtype=np.uint8), size=600).tolist())
    assert len(Oracle.tokenise(long_)) > 255
    # a long needle that shares many trigrams with stored strings: matches above 255 where the counters are 16 bits
    glued = b" ".join(strings[:120])
    needles += [long_, glued, b"", b" ,,  ", b"q", b"a"]
    for s in needles:
        T = len(Oracle.tokenise(s))
        full = o.find(s, 30000)
        for mm, mp in ((1, 0), (0, 500), (3, 700), (0, 1000)):
            assert m.find_above(s, mm, mp) == want_rows(full, T, mm, mp), (s[:40], mm, mp)
    assert len(Oracle.tokenise(glued)) > 255 and max(r[1] for r in o.find(glued, 10)) > 0


def test_batch_shapes_with_a_huge_segment_beside_empty_ones():
    m, o, strings, needles = oracle_case("geonames", 30000)
    rng = np.random.default_rng(5)
    pool = needles[:150] + [b"", b"a", b"e"]
    full = {s: o.find(s, 30000) for s in pool}
    for size in (1, 2, 17, 129):
        batch = [pool[int(i)] for i in rng.integers(0, len(pool), size=size)]
        if size > 2:
            batch[size // 2] = b"a"
            batch[size // 2 - 1] = b""
            batch[size // 2 + 1] = b""
        rows, row_off = m.find_batch_above_packed(*_pack(batch), 1, 0)
        got = split(rows, row_off)
        for s, g in zip(batch, got):
            assert g == want_rows(full[s], len(Oracle.tokenise(s)), 1, 0), s
    # 4 096 needles in one call: each equals the oracle (the same needles over and over)
    batch = [pool[int(i)] for i in rng.integers(0, len(pool), size=4096)]
    batch[2048] = b"a"
    for mp in (0, 700):
        rows, row_off = m.find_batch_above_packed(*_pack(batch), 1, mp)
        got = split(rows, row_off)
        for s, g in zip(batch, got):
            assert g == want_rows(full[s], len(Oracle.tokenise(s)), 1, mp), s
        if mp == 0:
            assert int(row_off[2049] - row_off[2048]) > 1000      # the one-letter needle's segment


def test_a_multi_window_haystack_equals_the_numpy_restatement():
    kind, n, _ = HIP_CASES[0]
    hay, off, needles = hip_case_inputs(kind, n)
    strings = W.unpack(hay, off)
    m = RawMap()
    m.put_many_packed(hay, off, np.arange(1, n + 1, dtype=np.uint32), np.zeros(n, dtype=np.uint32))
    truth = Truth(strings, np.arange(1, n + 1), np.zeros(n, dtype=np.int64))
    o = Oracle()
    o.put_many(hay, off)
    for s in needles[:8]:                                     # the restatement anchored on the oracle
        want = truth.rows(s, 1, 0)
        assert want[:60000] == o.find(s, 60000)[:len(want)], s
    sample = needles[:120] + [b"a"]
    for mm, mp in ((0, 700), (3, 0), (1, 0), (0, 1000)):
        rows, row_off = m.find_batch_above_packed(*_pack(sample), mm, mp)
        got = split(rows, row_off)
        for s, g in zip(sample, got):
            assert g == truth.rows(s, mm, mp), (s, mm, mp)
    assert m.device_info()["n_windows"] >= 4


def test_mutations_pending_deleted_and_put_again_then_folded():
    hay, off, needles = oracle_case_inputs("words", 5000)
    strings = W.unpack(hay, off)
    m, o = _load(strings)
    m.sync_device()
    rng = np.random.default_rng(9)
    probe = needles[:60]
    packed, offsets = _pack(probe)

    def check():
        rows, row_off = m.find_batch_above_packed(packed, offsets, 0, 600)
        got = split(rows, row_off)
        for s, g in zip(probe, got):
            assert g == want_rows(o.find(s, 65535), len(Oracle.tokenise(s)), 0, 600), s

    # deletes of references that qualify, puts that qualify (pending), a delete and put again with a new string
    first = [m.find_above(s, 0, 600) for s in probe[:10]]
    gone = sorted({r[0] for rows in first for r in rows[:2]})
    for r in gone:
        m.delete(r)
        o.delete(r)
    for k, s in enumerate(probe[:10]):
        m.put(s + b"x", 100000 + k, 0)
        o.put(s + b"x", 100000 + k, 0)
    again = int(rng.integers(1, 5000))
    while again in gone:
        again += 1
    m.delete(again)
    o.delete(again)
    m.put(probe[11], again, 3)
    o.put(probe[11], again, 3)
    check()
    m.sync_device()
    check()


def test_by_reference_equals_the_strings_and_absent_references_get_nothing():
    m, o, strings, _ = oracle_case("geonames", 30000)
    refs = np.array([5, 77, 29999, 123456789, 1, 30000], dtype=np.uint32)
    for mm, mp in ((0, 800), (2, 0), (1, 500)):
        rows, row_off, ntri = m.find_batch_by_reference_above(refs, mm, mp)
        got = split(rows, row_off)
        held = [strings[int(r) - 1] if r <= 30000 else None for r in refs]
        srows, soff = m.find_batch_above_packed(*_pack([h or b"" for h in held]), mm, mp)
        sgot = split(srows, soff)
        for i, h in enumerate(held):
            if h is None:
                assert got[i] == [] and ntri[i] == 0
                continue
            assert ntri[i] == len(Oracle.tokenise(h))
            assert got[i] == sgot[i]
            assert [int(refs[i]), int(ntri[i])] in [g[:2] for g in got[i]]
    # the self-join's arrays over the held references
    jr, joff, jrows = Map.join_above(m, refs, 0, 800)
    assert jr.tolist() == [5, 77, 29999, 1, 30000]
    rows, row_off, _ = m.find_batch_by_reference_above(jr, 0, 800)
    assert joff.tolist() == row_off.tolist() and jrows.tolist() == rows.tolist()


def test_count_only_and_erange_leave_the_rows_untouched():
    m, o, strings, needles = oracle_case("words", 5000)
    lib = _native.lib()
    packed, offsets = _pack(needles[:40])
    n = 40
    row_off = np.zeros(n + 1, dtype=np.uint64)
    assert lib.blurrily_storage_find_batch_above(m.handle, packed, offsets.ctypes.data, n, 1, 0, None, 0,
                                                 row_off.ctypes.data) == 0
    rows, filled = m.find_batch_above_packed(packed, offsets, 1, 0)
    assert row_off.tolist() == filled.tolist()
    total = int(row_off[n])
    assert total > 2
    buf = np.full((total, 3), 0xDEADBEEF, dtype=np.uint32)
    off2 = np.zeros(n + 1, dtype=np.uint64)
    C.set_errno(0)
    assert lib.blurrily_storage_find_batch_above(m.handle, packed, offsets.ctypes.data, n, 1, 0, buf.ctypes.data,
                                                 total - 1, off2.ctypes.data) == -1
    assert C.get_errno() == errno.ERANGE
    assert off2.tolist() == row_off.tolist()
    assert (buf == 0xDEADBEEF).all()
    assert lib.blurrily_storage_find_batch_above(m.handle, packed, offsets.ctypes.data, n, 1, 0, buf.ctypes.data,
                                                 total, off2.ctypes.data) == 0
    assert buf.tolist() == rows.tolist()
    # one needle: *total on ERANGE too
    tot = C.c_uint64(0)
    one = np.full((1, 3), 7, dtype=np.uint32)
    want = m.find_above(needles[0], 1, 0)
    assert len(want) > 1
    C.set_errno(0)
    assert lib.blurrily_storage_find_above(m.handle, needles[0], 1, 0, one.ctypes.data, 1, C.byref(tot)) == -1
    assert C.get_errno() == errno.ERANGE and tot.value == len(want) and (one == 7).all()


def test_top_k_rows_at_or_above_the_bar_are_a_prefix_of_the_threshold_rows():
    m, o, strings, needles = oracle_case("skewed", 20000)
    packed, offsets = _pack(needles)
    for limit in (10, 1024):
        trows, counts = m.find_batch_packed(packed, offsets, limit)
        for mm, mp in ((0, 500), (2, 0), (0, 900)):
            rows, row_off = m.find_batch_above_packed(packed, offsets, mm, mp)
            got = split(rows, row_off)
            for i, s in enumerate(needles):
                t = bar(len(Oracle.tokenise(s)), mm, mp)
                top = [r for r in trows[i, :counts[i]].tolist() if r[1] >= t]
                assert got[i][:len(top)] == top, (s, limit, mm, mp)


def test_the_top_k_find_is_unchanged_by_threshold_calls():
    m, o, strings, needles = oracle_case("geonames", 30000)
    packed, offsets = _pack(needles)
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    before_kernels = m.last_kernels()
    m.find_batch_above_packed(packed, offsets, 0, 700)
    assert "above_sweep_kernel" in m.last_kernels() and "above_rows_kernel" in m.last_kernels()
    m.find_batch_by_reference_above([1, 2, 3], 0, 700)
    assert "above_sweep_kernel" in m.last_kernels()
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == before_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)


def test_the_map_surface_normalises():
    mp = Map()
    mp.put("San José", 1)
    mp.put("san jose de la montana", 2)
    mp.put("london", 3)
    a = mp.find_above("SAN JOSE", 0, 500)
    assert a[0][:2] == [1, len(Oracle.tokenise(b"san jose"))] and 3 not in [r[0] for r in a]
    assert mp.find_batch_above(["SAN JOSE", "", "London"], 0, 500) == [a, [], mp.find_above("london", 0, 500)]
    mp.close()
