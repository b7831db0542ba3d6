"""Similarity find on the GPU (similar.hip, similar_kernels.hip): a needle's best `limit` rows by trigram Jaccard
similarity J = m / (T + R - m) at or above min_permille / 1000, J descending, then matches descending, weight ascending,
reference ascending -- equal to the oracle's complete find re-ranked exactly on the host, over the oracle cases, a
multi-window haystack (default weights and weights unrelated to length), needles at the counter-width boundaries,
built ties, mutations, by reference, batch shapes, the threshold-find workaround, and beside the top-k find, which it
leaves as it was."""
from fractions import Fraction

import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, RawMap
from blurrily_amd.map import _pack
from helpers import ORACLE_CASES, HIP_CASES, Oracle, hip_case_inputs, oracle_case_inputs
from similar_truth import Truth, cut, ranked

pytestmark = pytest.mark.gpu
LIMITS = (1, 10, 65, 121, 1000)
FLOORS = (0, 1, 300, 500, 999, 1000)


def rerank(cands, T, limit, p):
    return cut(ranked(cands, T), T, limit, p)


def got_rows(rows, counts, ntri):
    return [[r + [t] for r, t in zip(rows[i, :counts[i]].tolist(), ntri[i, :counts[i]].tolist())]
            for i in range(len(counts))]


def _load(strings, refs=None, weights=None):
    m, o = RawMap(), Oracle()
    refs = np.arange(1, len(strings) + 1, dtype=np.uint32) if refs is None else np.asarray(refs, dtype=np.uint32)
    weights = np.zeros(len(strings), dtype=np.uint32) if weights is None else np.asarray(weights, dtype=np.uint32)
    packed, offsets = _pack(strings)
    m.put_many_packed(packed, offsets, refs, weights)
    for s, r, w in zip(strings, refs.tolist(), weights.tolist()):
        o.put(s, r, w)
    return m, o


class Case:
    """A map, the oracle beside it, and every reference's R (the tokenisation of the string it was put with)."""

    def __init__(self, strings, refs=None, weights=None):
        self.m, self.o = _load(strings, refs, weights)
        refs = range(1, len(strings) + 1) if refs is None else refs
        self.R = {int(r): len(Oracle.tokenise(s)) for s, r in zip(strings, refs)}
        self.n = len(strings)
        self._ranked = {}

    def put(self, s, ref, w=0):
        self._ranked.clear()
        self.m.put(s, ref, w)
        self.o.put(s, ref, w)
        self.R[ref] = len(Oracle.tokenise(s))

    def delete(self, ref):
        self._ranked.clear()
        self.m.delete(ref)
        self.o.delete(ref)
        self.R.pop(ref, None)

    def want(self, s, limit, p):
        T = len(Oracle.tokenise(s))
        if s not in self._ranked:
            self._ranked[s] = ranked([(r, mm, w, self.R[r]) for r, mm, w in self.o.find(s, 65535)], T)
        return cut(self._ranked[s], T, limit, p)


_CASES = {}


def oracle_case(kind, n):
    if (kind, n) not in _CASES:
        hay, off, needles = oracle_case_inputs(kind, n)
        _CASES[(kind, n)] = (Case(W.unpack(hay, off)), needles)
    return _CASES[(kind, n)]


@pytest.mark.parametrize("kind,n,_limit", ORACLE_CASES)
def test_rows_equal_the_oracle_reranked_at_every_limit_and_floor(kind, n, _limit):
    c, needles = oracle_case(kind, n)
    packed, offsets = _pack(needles)
    for limit in LIMITS:
        for p in FLOORS:
            rows, counts, ntri = c.m.find_batch_similar_packed(packed, offsets, limit, p)
            got = got_rows(rows, counts, ntri)
            for i, s in enumerate(needles):
                assert got[i] == c.want(s, limit, p), (kind, s, limit, p)
    for s in needles[:20]:
        assert c.m.find_similar(s, 10, 300) == c.want(s, 10, 300), s


_BIG = {}


def big_case():
    if "m" not in _BIG:
        kind, n, _ = HIP_CASES[0]
        hay, off, needles = hip_case_inputs(kind, n)
        strings = W.unpack(hay, off)
        m = RawMap()
        m.put_many_packed(hay, off, np.arange(1, n + 1, dtype=np.uint32), np.zeros(n, dtype=np.uint32))
        _BIG.update(m=m, strings=strings, needles=needles, truth=Truth(strings, np.arange(1, n + 1), np.zeros(n)))
    return _BIG


def test_a_multi_window_haystack_equals_the_numpy_restatement():
    b = big_case()
    m, truth, needles = b["m"], b["truth"], b["needles"]
    o = Oracle()
    hay, off = _pack(b["strings"][:60000])
    o.put_many(np.frombuffer(hay, dtype=np.uint8), off)     # the restatement anchored on the oracle (one window's worth)
    t_small = Truth(b["strings"][:60000], np.arange(1, 60001), np.zeros(60000))
    for s in needles[:4]:
        assert t_small.rows(s, 65535, 0) == rerank([(r, mm, w, int(t_small.R[r - 1])) for r, mm, w in o.find(s, 65535)],
                                                   len(Oracle.tokenise(s)), 65535, 0)
    sample = needles[:60] + [b"a"]
    for limit, p in ((10, 0), (10, 500), (65, 700), (1000, 300)):
        rows, counts, ntri = m.find_batch_similar_packed(*_pack(sample), limit, p)
        got = got_rows(rows, counts, ntri)
        for s, g in zip(sample, got):
            assert g == truth.rows(s, limit, p), (s, limit, p)
    assert m.device_info()["n_windows"] >= 3


def test_weights_unrelated_to_length_leave_the_rows_exact():
    hay, off, needles = hip_case_inputs("geonames", 150000)
    strings = W.unpack(hay, off)
    n = len(strings)
    rng = np.random.default_rng(23)
    weights = rng.integers(1, 1 << 20, size=n).astype(np.uint32)
    m = RawMap()
    m.put_many_packed(hay, off, np.arange(1, n + 1, dtype=np.uint32), weights)
    truth = Truth(strings, np.arange(1, n + 1), weights)
    sample = needles[:50]
    for limit, p in ((10, 0), (10, 600), (300, 400)):
        rows, counts, ntri = m.find_batch_similar_packed(*_pack(sample), limit, p)
        for s, g in zip(sample, got_rows(rows, counts, ntri)):
            assert g == truth.rows(s, limit, p), (s, limit, p)
    assert m.device_info()["n_windows"] >= 3
    m.close()


def _needle_of(rng, t):
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz ", dtype=np.uint8)
    while True:
        s = bytes(rng.choice(letters, size=t + 40).tolist())
        if len(Oracle.tokenise(s)) >= t:
            for k in range(0, len(s) + 1):
                if len(Oracle.tokenise(s[:k])) == t:
                    return s[:k]


def test_needles_at_the_counter_boundaries():
    c, _ = oracle_case("geonames", 30000)
    rng = np.random.default_rng(43)
    needles = [b""] + [_needle_of(rng, t) for t in (15, 16, 255, 256)]
    strings = [s for s in (W.unpack(*oracle_case_inputs("geonames", 30000)[:2]))[:150]]
    needles += [b" ".join(strings[:100])]                     # matches above 255 where the counters are 16 bits
    assert [len(Oracle.tokenise(s)) for s in needles[:5]] == [1, 15, 16, 255, 256]
    assert len(Oracle.tokenise(needles[5])) > 256
    for s in needles:
        for limit, p in ((10, 0), (121, 0), (10, 100), (1000, 1)):
            assert c.m.find_similar(s, limit, p) == c.want(s, limit, p), (s[:40], limit, p)


def test_built_ties_order_by_matches_then_weight_then_reference():
    # short strings over a two-letter alphabet: many references share a similarity with different matches, and
    # duplicated strings under other references (equal or different weights) tie on similarity and matches
    rng = np.random.default_rng(3)
    base = sorted({bytes(rng.choice([97, 98], size=int(k)).tolist()) for k in rng.integers(1, 9, size=400)})
    strings, weights = [], []
    for s in base:
        for w in (5, 5, 2):
            strings.append(s)
            weights.append(w)
    refs = rng.permutation(np.arange(1, len(strings) + 1)).astype(np.uint32)
    c = Case(strings, refs, weights)
    saw_frac_tie = saw_weight_tie = saw_ref_tie = False
    for s in base:
        want = c.want(s, 1000, 0)
        assert c.m.find_similar(s, 1000, 0) == want, s
        T = len(Oracle.tokenise(s))
        for a, b in zip(want, want[1:]):
            if Fraction(a[1], T + a[3] - a[1]) == Fraction(b[1], T + b[3] - b[1]):
                saw_frac_tie |= a[1] != b[1]
                saw_weight_tie |= a[1] == b[1] and a[2] != b[2]
                saw_ref_tie |= a[1] == b[1] and a[2] == b[2]
    assert saw_frac_tie and saw_weight_tie and saw_ref_tie
    rows, counts, ntri = c.m.find_batch_similar_packed(*_pack(base), 7, 250)
    assert got_rows(rows, counts, ntri) == [c.want(s, 7, 250) for s in base]


def test_mutations_deletes_pending_puts_and_a_reference_put_again():
    hay, off, needles = oracle_case_inputs("words", 5000)
    strings = W.unpack(hay, off)
    c = Case(strings)
    c.m.sync_device()
    probe = needles[:60]
    packed, offsets = _pack(probe)

    def check():
        for limit, p in ((10, 0), (10, 400), (2000, 0)):
            rows, counts, ntri = c.m.find_batch_similar_packed(packed, offsets, limit, p)
            for s, g in zip(probe, got_rows(rows, counts, ntri)):
                assert g == c.want(s, limit, p), (s, limit, p)

    first = [c.m.find_similar(s, 3, 0) for s in probe[:10]]
    gone = sorted({r[0] for rows in first for r in rows[:2]})
    for r in gone:
        c.delete(r)                                           # tombstones
    for k, s in enumerate(probe[:10]):
        c.put(s + b"x", 100000 + k)                           # pending puts: the delta image
    again = next(r for r in range(100, 5001) if r not in gone)
    old_R = c.R[again]
    target = probe[11]
    c.delete(again)
    c.put(target + b" and a good deal more", again)           # deleted and put again, with a different R
    assert c.R[again] != old_R
    check()
    row = [r for r in c.m.find_similar(target, 1000, 0) if r[0] == again]
    assert row and row[0][3] == c.R[again]
    c.m.sync_device()                                         # folded into a rebuilt base
    check()


def test_by_reference_equals_the_stored_strings():
    c, _ = oracle_case("geonames", 30000)
    strings = W.unpack(*oracle_case_inputs("geonames", 30000)[:2])
    refs = np.array([5, 77, 29999, 123456789, 1, 30000], dtype=np.uint32)
    for limit, p in ((10, 0), (10, 800), (1000, 300)):
        rows, counts, ntri, nb = c.m.find_batch_by_reference_similar(refs, limit, p)
        got = got_rows(rows, counts, ntri)
        held = [strings[int(r) - 1] if r <= 30000 else None for r in refs]
        srows, scounts, sntri = c.m.find_batch_similar_packed(*_pack([h or b"" for h in held]), limit, p)
        sgot = got_rows(srows, scounts, sntri)
        for i, h in enumerate(held):
            if h is None:
                assert got[i] == [] and nb[i] == 0
                continue
            T = len(Oracle.tokenise(h))
            assert nb[i] == T and got[i] == sgot[i]
            own = [g for g in got[i] if g[0] == int(refs[i])]
            assert own and own[0][1] == T and own[0][3] == T  # similarity 1
            assert got[i][0][1] == got[i][0][3] == T          # (first: itself, or a reference with the same set)


def test_batch_shapes_limit_zero_and_the_largest_limit():
    c, needles = oracle_case("words", 5000)
    pool = needles[:150] + [b"", b"q"]
    want10 = {s: c.want(s, 10, 200) for s in pool}
    rng = np.random.default_rng(11)
    for size in (0, 1, 24, 25, 129, 4097):
        idx = rng.integers(0, len(pool), size=size)
        batch = [pool[int(i)] for i in idx]
        rows, counts, ntri = c.m.find_batch_similar_packed(*_pack(batch), 10, 200)
        assert counts.shape == (size,)
        assert got_rows(rows, counts, ntri) == [want10[s] for s in batch], size
    # more needles than one chunk of the sweep (2^20): checked in arrays, needle by needle
    n_big = (1 << 20) + 3
    idx = rng.integers(0, len(pool), size=n_big)
    rows, counts, ntri = c.m.find_batch_similar_packed(*_pack([pool[int(i)] for i in idx]), 10, 200)
    w_rows = np.zeros((len(pool), 10, 4), dtype=np.uint32)
    w_counts = np.array([len(want10[s]) for s in pool], dtype=np.uint32)
    for k, s in enumerate(pool):
        if want10[s]:
            w_rows[k, :len(want10[s])] = np.array(want10[s], dtype=np.uint32)
    assert np.array_equal(counts, w_counts[idx])
    live = np.arange(10)[None, :] < counts[:, None].astype(np.int64)
    assert np.array_equal(np.where(live[:, :, None], rows, 0), np.where(live[:, :, None], w_rows[idx, :, :3], 0))
    assert np.array_equal(np.where(live, ntri, 0), np.where(live, w_rows[idx, :, 3], 0))
    # limit 0: no rows anywhere
    rows, counts, ntri = c.m.find_batch_similar_packed(*_pack(pool[:5]), 0, 0)
    assert rows.shape == (5, 0, 3) and not counts.any()
    # limit 65 535: every row at or above the floor, on a haystack smaller than the limit
    g, gneedles = oracle_case("geonames", 30000)
    sample = gneedles[:20] + [b"e", b"a", b"ing"]
    for p in (0, 400):
        rows, counts, ntri = g.m.find_batch_similar_packed(*_pack(sample), 65535, p)
        for s, r in zip(sample, got_rows(rows, counts, ntri)):
            assert r == g.want(s, 65535, p), (s, p)
    assert max(len(g.want(s, 65535, 0)) for s in sample) > 1024      # (more than the largest list in LDS)


def test_the_threshold_find_workaround_gives_the_same_rows():
    b = big_case()
    m, needles = b["m"], b["needles"][:200]
    packed, offsets = _pack(needles)
    for limit, p in ((10, 500), (10, 700), (50, 300)):
        rows, counts, ntri = m.find_batch_similar_packed(packed, offsets, limit, p)
        got = got_rows(rows, counts, ntri)
        arows, row_off = m.find_batch_above_packed(packed, offsets, 0, p)
        refs = np.unique(arows[:, 0])
        _, code_off, _ = m.get_batch(refs)
        R = dict(zip(refs.tolist(), np.diff(code_off.astype(np.int64)).tolist()))
        for i, s in enumerate(needles):
            part = arows[int(row_off[i]):int(row_off[i + 1])].tolist()
            want = rerank([(r, mm, w, R[r]) for r, mm, w in part], len(Oracle.tokenise(s)), limit, p)
            assert got[i] == want, (s, limit, p)


def test_repeat_calls_and_the_top_k_find_are_unchanged():
    c, needles = oracle_case("geonames", 30000)
    m = c.m
    packed, offsets = _pack(needles)
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    before_kernels = m.last_kernels()
    one = m.find_batch_similar_packed(packed, offsets, 10, 300)
    assert "similar_sweep_kernel" in m.last_kernels() and "similar_rows_kernel" in m.last_kernels()
    two = m.find_batch_similar_packed(packed, offsets, 10, 300)
    assert all(np.array_equal(x, y) for x, y in zip(one, two))
    m.find_batch_by_reference_similar([1, 2, 3], 10, 300)
    assert "similar_sweep_kernel" in m.last_kernels()
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == before_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)


def test_the_map_surface_normalises():
    mp = Map()
    mp.put("San José", 1)
    mp.put("san jose de la montana", 2)
    mp.put("london", 3)
    a = mp.find_similar("SAN JOSE")
    T = len(Oracle.tokenise(b"san jose"))
    assert a[0] == [1, T, len("san jose"), T] and 3 not in [r[0] for r in a]
    assert mp.find_similar("SAN JOSE", 0) == a
    assert mp.find_batch_similar(["SAN JOSE", "", "London"], -1) == [a, mp.find_similar(""), mp.find_similar("london")]
    assert [r[0] for r in mp.find_similar("san jose", 10, 600)] == [1]
    mp.close()
