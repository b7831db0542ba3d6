"""Scoped threshold find on the GPU (scope_above.hip, scope_above_kernels.hip: scope_above_kernel / scope_above_each_kernel;
the mask strategy through above.hip's count and emit steps): rows, row_off and nb_trigrams equal the restatement of
tests/scope_above_truth.py exactly -- and, the definition, the library's own unscoped find_batch_above rows filtered
to the scope's live set on the host -- with each strategy forced and under auto, at the slab and 64-lane edges, at
every bar, for needles and members at the counter widths, for a needle whose members take every match count, under a
run of ties that crosses wave steps and slabs, on a multi-window haystack, under mutations, with a scope per needle and
by reference, through the capacity protocol and across the emit chunk bound; the unscoped paths are left as they were
and repeated calls are byte for byte equal."""
import ctypes as C
import errno
import itertools

import numpy as np
import pytest

import workloads as W
from blurrily_amd import RawMap, _native
from blurrily_amd.map import _pack
from helpers import Oracle
from scope_above_truth import ScopedTruth

pytestmark = pytest.mark.gpu
SWEEP, DIRECT, EACH = "above_sweep_kernel", "scope_above_kernel", "scope_above_each_kernel"
SENTINEL = 0xDEADBEEF


def split(rows, row_off):
    assert int(row_off[0]) == 0 and int(row_off[-1]) == len(rows)
    return [rows[int(row_off[i]):int(row_off[i + 1])].tolist() for i in range(len(row_off) - 1)]


def _put(m, t, strings, refs, weights):
    packed, offsets = _pack(strings)
    m.put_many_packed(packed, offsets, np.asarray(refs, dtype=np.uint32), np.asarray(weights, dtype=np.uint32))
    for s, r, w in zip(strings, refs, weights):
        t.put(s, int(r), int(w))


def _buf(needles):
    packed, offsets = _pack(needles)
    return np.frombuffer(packed, dtype=np.uint8), offsets


def _in(m, sc, needles, mm, mp):
    return split(*m.find_batch_above_in_packed(sc, *_buf(needles), mm, mp))


def _filtered(m, t, scope_refs, needles, mm, mp):
    """the definition: the library's own unscoped threshold rows, filtered to the scope's live set on the host"""
    live = t.live(scope_refs)
    return [[r for r in rows if r[0] in live] for rows in split(*m.find_batch_above_packed(*_buf(needles), mm, mp))]


def _needle_of(rng, t):
    """a string of exactly t distinct trigrams"""
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz ", dtype=np.uint8)
    while True:
        s = bytes(rng.choice(letters, size=t + 40).tolist())
        if len(Oracle.tokenise(s)) >= t:
            for k in range(0, len(s) + 1):
                if len(Oracle.tokenise(s[:k])) == t:
                    return s[:k]


def _stair(rng, length):
    """letters whose trigrams are all distinct: T = length + 1, and the prefix of k letters shares k of them"""
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    while True:
        s = bytes(rng.choice(letters, size=length).tolist())
        if len(Oracle.tokenise(s)) == length + 1:
            return s


def _served_by(names, strategy):
    if strategy == 2:
        assert names == [DIRECT], names
    elif strategy == 1:
        assert SWEEP in names and DIRECT not in names and EACH not in names, names


def check(m, t, sc, scope_refs, needles, mm, mp, strategy, what=None):
    """the scoped call under `strategy` against the truth and the definition; returns (rows, the kernels it launched)"""
    m.set_option("scope_strategy", strategy)
    try:
        got = _in(m, sc, needles, mm, mp)
        names = m.last_kernels()
    finally:
        m.set_option("scope_strategy", 0)
    want = [t.rows(s, scope_refs, mm, mp) for s in needles]
    assert got == want, (what, mm, mp, strategy)
    assert got == _filtered(m, t, scope_refs, needles, mm, mp), (what, mm, mp, strategy)
    return want, names


class Case:
    """~4 000 multi-word strings in one window, weights unrelated to length, references sparse and shuffled; members of
    R = 1, 255 and 256 trigrams; a stair needle's prefixes; the restatement anchored on the oracle for a whole-map
    scope."""

    def __init__(self):
        hay, off = W.geonames(4000, 400, 31)
        rng = np.random.default_rng(32)
        self.plain = W.unpack(hay, off)
        self.r255, self.r256 = _needle_of(rng, 255), _needle_of(rng, 256)
        self.stair = _stair(rng, 69)
        steps = [self.stair[:k] for k in range(1, len(self.stair) + 1)] + [self.stair + b"x"]
        strings = self.plain + [b"", b"1234 !!", self.r255, self.r256] + steps
        n = len(strings) - len(steps)
        self.refs = np.concatenate([rng.permutation(np.arange(1, 3 * n, 3, dtype=np.uint32))[:n],
                                    np.arange(50000, 50000 + len(steps), dtype=np.uint32)])
        weights = np.concatenate([rng.integers(1, 400, size=n), np.full(len(steps), 7)]).astype(np.uint32)
        self.m, self.t = RawMap(), ScopedTruth()
        _put(self.m, self.t, strings, self.refs, weights)
        self.m.sync_device()
        self.n_plain = len(self.plain)
        self.ref_empty, self.ref_digits, self.ref_255, self.ref_256 = (int(r) for r in self.refs[n - 4:n])
        self.step_refs = self.refs[n:]
        o = Oracle()
        for s, r, w in zip(strings, self.refs.tolist(), weights.tolist()):
            o.put(s, r, w)
        for s in (self.plain[5], self.plain[17][:6], b"", self.r255, self.stair):
            want = o.find(s, 65535)
            assert self.t.rows(s, self.refs, 1, 0) == want == self.t.rows(s, None, 1, 0)

    def scope_of(self, k, seed):
        """k plain members at random"""
        return np.random.default_rng(seed).choice(self.refs[:self.n_plain], k, replace=False)

    def needles_for(self, scope_refs, k=10):
        """members' strings, prefixes of them and strings of non-members"""
        where = {int(r): i for i, r in enumerate(self.refs[:self.n_plain].tolist())}
        mine = [self.plain[where[int(r)]] for r in scope_refs[:k // 2]]
        out = mine + [s[: max(3, len(s) - 3)] for s in mine[:2]] + self.plain[100:100 + k]
        return out[:k]

    def check(self, sc, scope_refs, needles, mm, mp, strategy, what=None):
        return check(self.m, self.t, sc, scope_refs, needles, mm, mp, strategy, what)


@pytest.fixture(scope="module")
def case():
    c = Case()
    yield c
    c.m.close()


@pytest.mark.parametrize("size", [1, 3, 255, 256, 257, 600])
def test_both_strategies_and_auto_equal_the_truth_across_sizes_and_bars(case, size):
    scope_refs = case.scope_of(size, 40 + size)
    needles = case.needles_for(scope_refs)
    rows_seen = 0
    with case.m.scope(scope_refs) as sc:
        for mp, mm in itertools.product((0, 300, 700, 1000), (0, 3, 300)):
            for strategy in (1, 2, 0):
                want, names = case.check(sc, scope_refs, needles, mm, mp, strategy, size)
                _served_by(names, strategy)
            rows_seen += sum(len(w) for w in want)
        for s in needles:                                  # a bar of T and of T + 1 matches, needle by needle
            T = len(Oracle.tokenise(s))
            for mm, strategy in itertools.product((T, T + 1), (1, 2)):
                case.m.set_option("scope_strategy", strategy)
                assert case.m.find_above_in(sc, s, mm, 0) == case.t.rows(s, scope_refs, mm, 0), (s, mm, strategy)
        case.m.set_option("scope_strategy", 0)
    assert rows_seen > 0


def test_needles_at_the_counter_widths_and_members_of_one_and_255_trigrams(case):
    rng = np.random.default_rng(43)
    needles = [b""] + [_needle_of(rng, k) for k in (15, 16)] + [case.r255, case.r256, b" ".join(case.plain[:140])]
    T = [len(Oracle.tokenise(s)) for s in needles]
    assert T[:5] == [1, 15, 16, 255, 256] and 650 <= T[5] <= 750
    scope_refs = np.concatenate([case.scope_of(600, 3), case.refs[:100],
                                 np.array([case.ref_empty, case.ref_digits, case.ref_255], dtype=np.uint32)])
    with case.m.scope(scope_refs) as sc:
        for strategy in (1, 2):
            for mm, mp in ((0, 0), (3, 0), (0, 300), (0, 1000), (255, 0), (256, 0), (300, 0)):
                want, names = case.check(sc, scope_refs, needles, mm, mp, strategy, "widths")
                _served_by(names, strategy)
                if (mm, mp) == (0, 0):
                    # the members of one trigram are the empty needle's rows; the member of 255 leads its own needle's
                    assert [r[0] for r in want[0]] == sorted([case.ref_empty, case.ref_digits],
                                                             key=lambda r: (case.t.entries[r][1], r))
                    assert want[3][0] == [case.ref_255, 255, case.t.entries[case.ref_255][1]]
                    assert len(want[5]) > 100 and max(r[1] for r in want[5]) > 15
                if mm == 255:
                    assert want[3] == [[case.ref_255, 255, case.t.entries[case.ref_255][1]]]
                if mm >= 256:
                    assert not any(want)                   # a member has at most 255 trigrams


def test_a_needle_whose_members_take_every_match_count_and_are_its_prefixes(case):
    T = len(Oracle.tokenise(case.stair))
    scope_refs = np.concatenate([case.step_refs, case.scope_of(30, 12)])
    with case.m.scope(scope_refs) as sc:
        for strategy in (1, 2):
            want, names = case.check(sc, scope_refs, [case.stair, case.stair[:40], case.stair[5:]], 0, 0, strategy, "stair")
            _served_by(names, strategy)
            steps = [r for r in want[0] if r[0] >= 50000]
            assert sorted({r[1] for r in steps}) == list(range(1, T + 1))      # every count from 1 to T
            assert [r[1] for r in steps] == sorted((r[1] for r in steps), reverse=True)
            for mm, mp in ((T, 0), (T - 1, 0), (T // 2, 0), (0, 500), (0, 1000), (T + 1, 0)):
                case.check(sc, scope_refs, [case.stair, case.stair[:40]], mm, mp, strategy, "stair bars")
        assert case.m.find_above_in(sc, case.stair, T, 0) == [[int(case.step_refs[len(case.stair) - 1]), T, 7]]


def test_a_run_of_ties_across_wave_steps_and_slabs():
    rng = np.random.default_rng(5)
    m, t = RawMap(), ScopedTruth()
    hay, off = W.geonames(1500, 200, 9)
    plain = W.unpack(hay, off)
    strings = plain + [b"santa maria"] * 300
    refs = rng.permutation(np.arange(1, len(strings) + 1, dtype=np.uint32))
    weights = np.concatenate([rng.integers(1, 400, size=len(plain)), rng.integers(1, 6, size=300)]).astype(np.uint32)
    _put(m, t, strings, refs, weights)
    m.sync_device()
    same = refs[len(plain):]
    scope_refs = np.concatenate([same, refs[:200]])
    T = len(Oracle.tokenise(b"santa maria"))
    with m.scope(scope_refs) as sc:
        for strategy in (1, 2):
            for mm, mp in ((0, 0), (3, 0), (0, 1000), (T, 0)):
                want, names = check(m, t, sc, scope_refs, [b"santa maria", b"santa mari", b"maria"], mm, mp, strategy, "ties")
                _served_by(names, strategy)
            ties = [r for r in want[0] if r[1] == T]      # the 300, in (weight, reference) order
            assert len(ties) == 300 and {r[0] for r in ties} == set(same.tolist())
            assert [(r[2], r[0]) for r in ties] == sorted((r[2], r[0]) for r in ties)
    m.close()


def test_a_member_of_256_trigrams_has_no_direct_form_and_the_mask_serves_it(case):
    inner = case.scope_of(300, 8)
    wide = np.concatenate([inner, np.array([case.ref_256], dtype=np.uint32)])
    needles = [case.r256, case.r255] + case.needles_for(inner, 4)
    with case.m.scope(wide) as sc, case.m.scope(inner) as sc_inner:
        for strategy in (0, 2):                            # (forced direct: there is no direct form to serve it)
            want, names = case.check(sc, wide, needles, 0, 0, strategy, "wide")
            assert SWEEP in names and DIRECT not in names
        assert want[0][0] == [case.ref_256, 256, case.t.entries[case.ref_256][1]]
        case.m.set_option("scope_strategy", 2)
        assert case.m.find_above_in(sc, case.r256, 256, 0) == [want[0][0]]
        _, names = case.check(sc_inner, inner, needles, 0, 0, 0, "inner")
        assert names == [DIRECT]


def test_the_mask_and_direct_on_a_multi_window_haystack_with_every_third_reference():
    n = 70000
    hay, off = W.words(n, seed=17)
    strings = W.unpack(hay, off)
    refs = np.arange(1, n + 1, dtype=np.uint32)
    weights = np.random.default_rng(23).integers(1, 1 << 20, size=n).astype(np.uint32)   # ranks unrelated to length
    m, t = RawMap(), ScopedTruth()
    _put(m, t, strings, refs, weights)
    m.sync_device()
    assert m.device_info()["n_windows"] >= 2
    scope_refs = refs[::3]
    needles = [strings[0], strings[3], strings[30001][:5], strings[69999], strings[40000] + b"x", b"zzzzqq"]
    with m.scope(scope_refs) as sc:
        for strategy in (1, 2):                            # (23 334 members scored directly: slabs of 92 steps)
            for mm, mp in ((0, 0), (0, 700), (3, 0), (0, 1000)):
                want, names = check(m, t, sc, scope_refs, needles, mm, mp, strategy, "words")
                _served_by(names, strategy)
                if (mm, mp) == (0, 0):
                    assert max(len(w) for w in want) > 1000
    m.close()


def test_mutations_between_calls_on_one_scope():
    rng = np.random.default_rng(61)
    hay, off = W.geonames(3000, 300, 17)
    strings = W.unpack(hay, off)
    n = len(strings)
    refs = np.arange(1, n + 1, dtype=np.uint32)
    m, t = RawMap(), ScopedTruth()
    _put(m, t, strings, refs, rng.integers(1, 50, size=n).astype(np.uint32))
    m.sync_device()
    scope_refs = np.concatenate([rng.choice(refs, 300, replace=False), np.array([n + 10, n + 11], dtype=np.uint32)])
    needles = [strings[int(r) - 1] for r in scope_refs[:6]] + [strings[0][::-1] + b" new", strings[7] + b" again"]
    sc = m.scope(scope_refs)

    def check_all(what):
        for strategy in (1, 2):
            want, _ = check(m, t, sc, scope_refs, needles, 0, 300, strategy, what)
            m.set_option("scope_strategy", strategy)
            assert m.find_above_in(sc, needles[0], 0, 300) == want[0], (what, strategy)
        m.set_option("scope_strategy", 0)
        return want

    want = check_all("fresh")
    best = want[1][0][0]                                   # a best row, deleted
    m.delete(best)
    t.delete(best)
    assert all(r[0] != best for r in check_all("deleted")[1])
    m.put(needles[6], n + 10, 3)                           # a member put after the scope was made: pending
    t.put(needles[6], n + 10, 3)
    assert check_all("pending")[6][0] == [n + 10, len(Oracle.tokenise(needles[6])), 3]
    victim = int(scope_refs[2])                            # deleted and put again with another text: new trigrams
    m.delete(victim)
    t.delete(victim)
    m.put(needles[7], victim, 1)
    t.put(needles[7], victim, 1)
    assert check_all("put again")[7][0][0] == victim
    before = m.device_info()["base_builds"]                # the log outgrows its budget: the pending member is folded
    bulk = [s + b" bulk" + bytes([97 + k]) for k in range(2) for s in strings[:2300]]   # (the log holds 4 096 puts)
    _put(m, t, bulk, list(range(n + 100, n + 100 + len(bulk))), [2] * len(bulk))
    assert check_all("folded")[6][0][0] == n + 10
    assert m.device_info()["base_builds"] > before
    sc.close()
    absent = np.arange(10 ** 6, 10 ** 6 + 50, dtype=np.uint32)
    for strategy in (0, 1, 2):
        m.set_option("scope_strategy", strategy)
        for members in (np.zeros(0, dtype=np.uint32), absent):      # an empty scope; one whose members are all absent
            with m.scope(members) as none:
                rows, row_off = m.find_batch_above_in_packed(none, *_buf(needles), 0, 0)
                assert len(rows) == 0 and not row_off.any() and len(row_off) == len(needles) + 1
                assert m.last_kernels() == []
                assert m.find_above_in(none, needles[0], 0, 0) == []
    m.set_option("scope_strategy", 0)
    m.close()


def _each(m, scopes, which, needles, mm, mp):
    return split(*m.find_batch_above_each_in(scopes, which, *_buf(needles), mm, mp))


def test_a_scope_per_needle_equals_the_single_scope_calls_and_the_truth(case):
    m, t = case.m, case.t
    direct = case.scope_of(600, 21)
    wide = np.concatenate([case.scope_of(300, 22), np.array([case.ref_256], dtype=np.uint32)])   # the mask alone serves it
    small = case.scope_of(40, 23)
    family = [direct, wide, np.zeros(0, dtype=np.uint32), small]
    scopes = [m.scope(f) for f in family]
    handles = scopes + [scopes[0]]                         # 4: the same handle as 0
    family = family + [direct]
    try:
        needles = case.needles_for(direct, 8) + [case.r256, b"", case.plain[9]] + case.needles_for(small, 4)
        which = [0, 1, None, 2, 4, 3, 0, 1, 1, None, 2, 3, 3, 4, 0]
        assert len(which) == len(needles)
        for mm, mp in ((0, 0), (3, 300), (0, 1000)):
            got = _each(m, handles, which, needles, mm, mp)
            names = m.last_kernels()
            assert EACH in names and SWEEP in names and DIRECT not in names
            want = [t.rows(s, None if w is None else family[w], mm, mp) for s, w in zip(needles, which)]
            assert got == want, (mm, mp)
            for i, (s, w) in enumerate(zip(needles, which)):           # element for element the single calls
                one = m.find_above(s, mm, mp) if w is None else m.find_above_in(handles[w], s, mm, mp)
                assert one == got[i], (i, mm, mp)
        # an all-direct batch: the one kernel, nothing else
        only = [0, 3, 4, 3, 0]
        got = _each(m, handles, only, needles[:5], 0, 200)
        assert m.last_kernels() == [EACH]
        assert got == [t.rows(s, family[w], 0, 200) for s, w in zip(needles[:5], only)]
        # only empty scopes: no rows, no launch
        rows, row_off = m.find_batch_above_each_in(handles, [2, 2], *_buf(needles[:2]), 0, 0)
        assert len(rows) == 0 and row_off.tolist() == [0, 0, 0] and m.last_kernels() == []
        # by reference: the stored strings' rows; an absent reference has none
        by = [int(direct[0]), int(direct[1]), int(small[0]), case.ref_256, 2, int(wide[0]), int(direct[2])]
        bw = [0, 4, 3, 1, 0, None, 2]
        for strategy in (0, 1, 2):
            m.set_option("scope_strategy", strategy)
            rows, row_off, nb = m.find_batch_by_reference_above_each_in(handles, bw, by, 0, 300)
            got = split(rows, row_off)
            assert got == [t.by_reference(r, None if w is None else family[w], 0, 300) for r, w in zip(by, bw)]
            assert got[4] == [] and nb[4] == 0 and nb[3] == 256 and got[6] == []
            assert nb.tolist() == [len(Oracle.tokenise(t.entries[r][0])) if r in t.entries else 0 for r in by]
            for k in (0, 1, 2, 3):                         # a member of its own scope: among its own rows, matches == T
                assert [by[k], int(nb[k])] in [x[:2] for x in got[k]]
        m.set_option("scope_strategy", 0)
        m.find_batch_by_reference_above_each_in(handles, [0, 3], [int(direct[0]), int(small[0])], 0, 0)
        assert m.last_kernels() == [EACH]
    finally:
        m.set_option("scope_strategy", 0)
        for sc in scopes:
            sc.close()


def test_a_small_plan_with_pending_puts_by_strings_and_by_reference_in_every_shape():
    """ the each-in's plan upload, swept-group description and needle carrier with the delta
    masks live: 300 references and five pending puts, a scope of three members, one holding a member of 256 trigrams
    (it declines direct), one of unheld references, an unscoped needle -- as a plan of both kinds with the empty scope
    and NO_SCOPE in the call, of swept groups only (the mask forced) and of direct needles only."""
    rng = np.random.default_rng(71)
    strings = W.unpack(*W.geonames(300, 60, 19)) + [_needle_of(rng, 256)]
    n = len(strings)
    m, t = RawMap(), ScopedTruth()
    _put(m, t, strings, np.arange(1, n + 1, dtype=np.uint32), rng.integers(1, 50, size=n).astype(np.uint32))
    m.sync_device()
    family = [np.array([3, 4, n + 1], np.uint32), np.array([n, 10, 11, 12, n + 2], np.uint32),
              np.arange(10 ** 6, 10 ** 6 + 4, dtype=np.uint32)]    # three members; the 256-trigram member; unheld
    scopes = [m.scope(f) for f in family]
    for k in range(5):                                     # pending: n + 1 in `three`, n + 2 in `wide`, three in neither
        m.put(strings[k] + b" late", n + 1 + k, 2)
        t.put(strings[k] + b" late", n + 1 + k, 2)
    needles = [strings[0], strings[1], strings[2], strings[2], strings[3], strings[9], strings[n - 1], strings[2]]
    by = [3, n + 1, n, 10, n + 3, n + 3, 10 ** 6, 4]
    both, direct_only = [0, 1, 0, 1, None, 1, 2, None], [0] * 8
    # (a pending put outside both scopes matches needles asked within them: only the delta mask keeps it out)
    assert n + 3 in [r[0] for r in t.rows(strings[2], None, 0, 0)] and n + 3 not in family[0] and n + 3 not in family[1]
    try:
        for strategy, which, each, sweep in ((0, both, True, True), (1, both, False, True), (0, direct_only, True, False)):
            m.set_option("scope_strategy", strategy)
            for mm, mp in ((0, 0), (2, 300)):
                got = _each(m, scopes, which, needles, mm, mp)
                names = m.last_kernels()
                assert (EACH in names) == each and (SWEEP in names) == sweep, (strategy, names)
                assert got == [t.rows(s, None if w is None else family[w], mm, mp) for s, w in zip(needles, which)]
                rows, row_off, nb = m.find_batch_by_reference_above_each_in(scopes, which, by, mm, mp)
                names = m.last_kernels()
                assert (EACH in names) == each and (SWEEP in names) == sweep, (strategy, names)
                assert split(rows, row_off) == [t.by_reference(r, None if w is None else family[w], mm, mp)
                                                for r, w in zip(by, which)], (strategy, mm, mp)
                assert nb.tolist() == [len(Oracle.tokenise(t.entries[r][0])) if r in t.entries else 0 for r in by]
    finally:
        m.set_option("scope_strategy", 0)
        for sc in scopes:
            sc.close()
        m.close()


def test_join_above_within_over_three_blocks(case):
    blocks = [case.scope_of(120, 51), case.scope_of(257, 52), np.concatenate([case.scope_of(30, 53), np.array([2, 5], np.uint32)])]
    refs, which, row_off, rows = RawMap.join_above_within(case.m, blocks, 0, 700)
    held = [(int(r), k) for k, b in enumerate(blocks) for r in np.unique(b).tolist() if r in case.t.entries]
    assert list(zip(refs.tolist(), which.tolist())) == held
    got = split(rows, row_off)
    assert got == [case.t.by_reference(r, blocks[k], 0, 700) for r, k in held]
    for row, (r, _) in zip(got, held):                     # each among its own rows with matches == T
        assert [r, len(Oracle.tokenise(case.t.entries[r][0]))] in [x[:2] for x in row]
    assert case.m.last_kernels() == [EACH]


def test_count_only_erange_one_short_and_exact_capacity(case):
    m, lib = case.m, _native.lib()
    scope_refs = case.scope_of(600, 21)
    needles = case.needles_for(scope_refs, 10)
    packed, offsets = _pack(needles)
    n = len(needles)
    which = np.array([0, 1] * (n // 2), dtype=np.uint32)
    with m.scope(scope_refs) as sc, m.scope(case.scope_of(257, 5)) as sc2:
        handles = m._handles([sc, sc2])
        calls = {
            "in": lambda res, cap, off: lib.blurrily_storage_find_batch_above_in(
                m.handle, sc._h, packed, offsets.ctypes.data, n, 1, 0, res, cap, off),
            "each": lambda res, cap, off: lib.blurrily_storage_find_batch_above_each_in(
                m.handle, handles, 2, which.ctypes.data, packed, offsets.ctypes.data, n, 1, 0, res, cap, off),
        }
        for strategy, (name, call) in itertools.product((1, 2), calls.items()):
            m.set_option("scope_strategy", strategy)
            row_off = np.zeros(n + 1, dtype=np.uint64)
            assert call(None, 0, row_off.ctypes.data) == 0                       # count only
            rows, filled = (m.find_batch_above_in_packed(sc, packed, offsets, 1, 0) if name == "in" else
                            m.find_batch_above_each_in([sc, sc2], which, packed, offsets, 1, 0))
            assert row_off.tolist() == filled.tolist()
            total = int(row_off[n])
            assert total > 2
            buf = np.full((total, 3), SENTINEL, dtype=np.uint32)
            off2 = np.zeros(n + 1, dtype=np.uint64)
            C.set_errno(0)
            assert call(buf.ctypes.data, total - 1, off2.ctypes.data) == -1      # one short
            assert C.get_errno() == errno.ERANGE
            assert off2.tolist() == row_off.tolist() and (buf == SENTINEL).all()
            assert call(buf.ctypes.data, total, off2.ctypes.data) == 0           # exact
            assert buf.tolist() == rows.tolist() and off2.tolist() == row_off.tolist()
            # one needle: *total on ERANGE too
            tot = C.c_uint64(0)
            one = np.full((1, 3), 7, dtype=np.uint32)
            want = case.t.rows(needles[0], scope_refs, 1, 0)
            assert len(want) > 1
            C.set_errno(0)
            assert lib.blurrily_storage_find_above_in(m.handle, sc._h, needles[0], 1, 0, one.ctypes.data, 1,
                                                      C.byref(tot)) == -1
            assert C.get_errno() == errno.ERANGE and tot.value == len(want) and (one == 7).all()
        m.set_option("scope_strategy", 0)


def test_scoped_threshold_calls_leave_the_unscoped_paths_as_they_were(case):
    m = case.m
    rng = np.random.default_rng(60)
    needles = [case.plain[i][: max(3, len(case.plain[i]) - int(rng.integers(0, 4)))] for i in rng.choice(case.n_plain, 3000)]
    buf, offsets = _buf(needles)
    scope_refs = case.scope_of(600, 90)

    def unscoped():
        out = []
        rows, counts = m.find_batch_packed(buf, offsets, 10)
        live = np.arange(rows.shape[1])[None, :] < counts[:, None].astype(np.int64)
        out.append((m.last_kernels(), counts.tobytes(), np.where(live[:, :, None], rows, 0).tobytes()))
        rows, row_off = m.find_batch_above_packed(buf, offsets, 0, 700)
        out.append((m.last_kernels(), row_off.tobytes(), rows.tobytes()))
        return out

    with m.scope(scope_refs) as sc:
        for _ in range(2):                                 # (the first batch of a class may measure every sweep)
            before = unscoped()
        choice0, tuned0 = m.get_option("ws_choice"), m.get_option("tuned_class")
        for strategy in (0, 1, 2):
            m.set_option("scope_strategy", strategy)
            m.find_batch_above_in_packed(sc, buf, offsets, 0, 700)
            m.find_batch_above_each_in([sc, sc], [0, None] * (len(needles) // 2), buf, offsets, 0, 700)
        m.set_option("scope_strategy", 0)
        assert m.get_option("ws_choice") == choice0 and m.get_option("tuned_class") == tuned0
        after = unscoped()
    assert before == after


def test_three_repeated_calls_are_byte_for_byte_equal(case):
    m = case.m
    direct, wide = case.scope_of(600, 21), np.concatenate([case.scope_of(300, 22), np.array([case.ref_256], np.uint32)])
    needles = case.needles_for(direct, 10)
    buf, offsets = _buf(needles)
    which = [0, 1, None, 0, 1, None, 0, 1, 0, 0]
    with m.scope(direct) as a, m.scope(wide) as b:
        for call in (lambda: m.find_batch_above_in_packed(a, buf, offsets, 0, 0),
                     lambda: m.find_batch_above_in_packed(b, buf, offsets, 0, 0),
                     lambda: m.find_batch_above_each_in([a, b], which, buf, offsets, 2, 200),
                     lambda: m.find_batch_by_reference_above_each_in([a, b], [0, 1, 0], direct[:3], 2, 200)):
            first = [x.tobytes() for x in call()]
            assert len(first[0]) > 0
            for _ in range(2):
                assert [x.tobytes() for x in call()] == first


def test_a_call_of_more_rows_than_one_emit_chunk_holds():
    """320 identical needles over 56 000 members that all share the needle's first trigram, at a bar of one match:
    17 920 000 rows, more than the 2^24 of one emit chunk."""
    n_members, n_needles = 56000, 320
    letters = b"abcdefghijklmnopqrstuvwxyz"
    strings = [b"a" + bytes([letters[(k // 676) % 26], letters[(k // 26) % 26], letters[k % 26]]) + b" " +
               bytes([letters[(k // 17576) % 26]]) for k in range(n_members)]
    refs = np.arange(1, n_members + 1, dtype=np.uint32)
    weights = (np.arange(n_members, dtype=np.uint32) * 7919) % 1000 + 1
    m, t = RawMap(), ScopedTruth()
    _put(m, t, strings, refs, weights)
    m.sync_device()
    m.set_option("scope_strategy", 2)
    with m.scope(refs) as sc:
        rows, row_off = m.find_batch_above_in_packed(sc, *_buf([b"a"] * n_needles), 1, 0)
        assert m.last_kernels() == [DIRECT]
    assert row_off.tolist() == [n_members * i for i in range(n_needles + 1)] and len(rows) > 1 << 24
    first = rows[:n_members]
    assert first.tolist() == t.rows(b"a", refs, 1, 0)
    per = rows.reshape(n_needles, n_members, 3)
    assert (per == first[None, :, :]).all()
    m.close()
