"""Scoped similarity find on the GPU (scope_similar.hip, scope_similar_kernels.hip: scope_similar_kernel /
scope_similar_each_kernel; the mask strategy through similar.hip's sweep): rows, counts and row_ntri equal the
restatement of tests/scope_similar_truth.py exactly -- every reference passing the row test, ranked, the rows outside
the scope's live set removed, cut at the limit -- with each strategy forced, at the workgroup's stride and the
select's boundaries, under ties, for needles and members at the counter widths, on a multi-window haystack, under
mutations, with a scope per needle and by reference; the unscoped path is left as it was and repeated calls are
byte for byte equal."""
import itertools

import numpy as np
import pytest

import workloads as W
from blurrily_amd import RawMap
from blurrily_amd.map import _pack
from helpers import Oracle
from scope_similar_truth import ScopedTruth
from similar_truth import cut, ranked

pytestmark = pytest.mark.gpu
SWEEP, DIRECT, EACH = "similar_sweep_kernel", "scope_similar_kernel", "scope_similar_each_kernel"


def _put(m, t, strings, refs, weights):
    packed, offsets = _pack(strings)
    m.put_many_packed(packed, offsets, np.asarray(refs, dtype=np.uint32), np.asarray(weights, dtype=np.uint32))
    for s, r, w in zip(strings, refs, weights):
        t.put(s, int(r), int(w))


def _got(rows, counts, ntri):
    return [[r + [t] for r, t in zip(rows[i, :c].tolist(), ntri[i, :c].tolist())] for i, c in enumerate(counts.tolist())]


def _in(m, sc, needles, limit, p):
    packed, offsets = _pack(needles)
    return _got(*m.find_batch_similar_in_packed(sc, np.frombuffer(packed, dtype=np.uint8), offsets, limit, p))


def _needle_of(rng, t):
    """a string of exactly t distinct trigrams"""
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz ", dtype=np.uint8)
    while True:
        s = bytes(rng.choice(letters, size=t + 40).tolist())
        if len(Oracle.tokenise(s)) >= t:
            for k in range(0, len(s) + 1):
                if len(Oracle.tokenise(s[:k])) == t:
                    return s[:k]


def _served_by(m, strategy):
    names = m.last_kernels()
    if strategy == 2:
        assert names == [DIRECT], names
    else:
        assert SWEEP in names and DIRECT not in names and EACH not in names, names


class Case:
    """~4 000 multi-word strings in one window, weights unrelated to length, references sparse and shuffled; members of
    R = 1, 255 and 256 trigrams; the restatement anchored on the oracle for a whole-map scope."""

    def __init__(self):
        hay, off = W.geonames(4000, 400, 31)
        rng = np.random.default_rng(32)
        self.plain = W.unpack(hay, off)
        self.r255, self.r256 = _needle_of(rng, 255), _needle_of(rng, 256)
        strings = self.plain + [b"", b"1234 !!", self.r255, self.r256]
        n = len(strings)
        self.refs = rng.permutation(np.arange(1, 3 * n, 3, dtype=np.uint32))[:n]
        weights = rng.integers(1, 400, size=n).astype(np.uint32)
        self.m, self.t = RawMap(), ScopedTruth()
        _put(self.m, self.t, strings, self.refs, weights)
        self.m.sync_device()
        self.n_plain = len(self.plain)
        self.ref_empty, self.ref_digits, self.ref_255, self.ref_256 = (int(r) for r in self.refs[-4:])
        self.rng = rng
        o = Oracle()
        for s, r, w in zip(strings, self.refs.tolist(), weights.tolist()):
            o.put(s, r, w)
        R = {int(r): len(Oracle.tokenise(s)) for s, r in zip(strings, self.refs)}
        for s in (self.plain[5], self.plain[17][:6], b"", self.r255):
            T = len(Oracle.tokenise(s))
            want = cut(ranked([(r, mm, w, R[r]) for r, mm, w in o.find(s, 65535)], T), T, 65535, 0)
            assert self.t.rows(s, self.refs, 65535, 0) == want == self.t.rows(s, None, 65535, 0)

    def scope_of(self, k, seed):
        """k plain members at random"""
        return np.random.default_rng(seed).choice(self.refs[:self.n_plain], k, replace=False)

    def needles_for(self, scope_refs, k=10):
        """members' strings (J = 1 within the scope), prefixes and strings of non-members"""
        where = {int(r): i for i, r in enumerate(self.refs[:self.n_plain].tolist())}
        mine = [self.plain[where[int(r)]] for r in scope_refs[:k // 2]]
        out = mine + [s[: max(3, len(s) - 3)] for s in mine[:2]] + self.plain[100:100 + k]
        return out[:k]

    def check(self, sc, scope_refs, needles, limit, p, strategy, what=None):
        self.m.set_option("scope_strategy", strategy)
        try:
            got = _in(self.m, sc, needles, limit, p)
        finally:
            self.m.set_option("scope_strategy", 0)
        want = [self.t.rows(s, scope_refs, limit, p) for s in needles]
        assert got == want, (what, limit, p, strategy)
        return want


@pytest.fixture(scope="module")
def case():
    c = Case()
    yield c
    c.m.close()


@pytest.mark.parametrize("size", [1, 255, 256, 257, 600])
def test_both_strategies_equal_the_truth_across_sizes_limits_and_floors(case, size):
    scope_refs = case.scope_of(size, 40 + size)
    needles = case.needles_for(scope_refs)
    rows_seen = 0
    with case.m.scope(scope_refs) as sc:
        for limit, p in itertools.product((1, 10, 256), (0, 300, 500, 1000)):
            for strategy in (1, 2):
                want = case.check(sc, scope_refs, needles, limit, p, strategy, size)
                _served_by(case.m, strategy)
            rows_seen += sum(len(w) for w in want)
        assert case.m.find_similar_in(sc, needles[0], 10, 500) == case.t.rows(needles[0], scope_refs, 10, 500)
    assert rows_seen > 0


def test_the_select_boundary_limit_at_one_below_and_one_above_the_passing_members(case):
    scope_refs = case.scope_of(600, 77)
    needles = case.needles_for(scope_refs, 6)
    with case.m.scope(scope_refs) as sc:
        for s in needles:
            for p in (0, 200):
                passing = len(case.t.rows(s, scope_refs, 10 ** 6, p))
                for limit in {max(passing - 1, 1), max(passing, 1), passing + 1}:
                    if limit <= 256:
                        for strategy in (1, 2):
                            case.check(sc, scope_refs, [s], limit, p, strategy, ("boundary", passing))


def _built_tie():
    """a needle of T = 4, a member with m = 2 and R = 2 and one with m = 3 and R = 5: J = 1/2 both"""
    words = [bytes(w) for k in range(1, 6) for w in itertools.product(b"ab ", repeat=k)]
    words = [w for w in words if w.strip() == w and b"  " not in w]
    codes = {w: set(Oracle.tokenise(w)) for w in words}
    for nd in words:
        if len(codes[nd]) != 4:
            continue
        a = [w for w in words if len(codes[w]) == 2 and len(codes[w] & codes[nd]) == 2]
        b = [w for w in words if len(codes[w]) == 5 and len(codes[w] & codes[nd]) == 3]
        if a and b:
            return nd, a[0], b[0]
    raise AssertionError("no such strings")


def test_ties_identical_strings_equal_similarity_with_different_matches_and_a_pair_at_its_floor():
    rng = np.random.default_rng(5)
    m, t = RawMap(), ScopedTruth()
    hay, off = W.geonames(1500, 200, 9)
    plain = W.unpack(hay, off)
    nd, two_of_two, three_of_five = _built_tie()
    strings = plain + [b"santa maria"] * 300 + [two_of_two, three_of_five]
    refs = rng.permutation(np.arange(1, len(strings) + 1, dtype=np.uint32))
    weights = np.concatenate([rng.integers(1, 400, size=len(plain)), rng.integers(1, 6, size=300), [7, 7]]).astype(np.uint32)
    _put(m, t, strings, refs, weights)
    m.sync_device()
    same = refs[len(plain):len(plain) + 300]
    ra, rb = int(refs[-2]), int(refs[-1])
    scope_refs = np.concatenate([same, refs[:200], refs[-2:]])
    with m.scope(scope_refs) as sc:
        for strategy in (1, 2):
            m.set_option("scope_strategy", strategy)
            # 300 members of one string: the cut goes through them, in (weight, reference) order
            for limit in (1, 100, 150, 256):
                for s in (b"santa maria", b"santa mari", b"maria"):
                    got = _in(m, sc, [s], limit, 0)[0]
                    assert got == t.rows(s, scope_refs, limit, 0), (strategy, limit, s)
            got = _in(m, sc, [b"santa maria"], 150, 1000)[0]
            assert len(got) == 150 and [(r[2], r[0]) for r in got] == sorted((r[2], r[0]) for r in got)
            assert {r[0] for r in got} <= set(same.tolist())
            # equal J, different m: the row of more matches first
            got = _in(m, sc, [nd], 256, 0)[0]
            assert got == t.rows(nd, scope_refs, 256, 0)
            at = {r[0]: k for k, r in enumerate(got)}
            assert got[at[rb]][1:] == [3, 7, 5] and got[at[ra]][1:] == [2, 7, 2] and at[rb] + 1 == at[ra]
            # J = 1/2 exactly: rows at 500 per mille, none at 501
            at_floor = {r[0] for r in _in(m, sc, [nd], 256, 500)[0]}
            above = {r[0] for r in _in(m, sc, [nd], 256, 501)[0]}
            assert {ra, rb} <= at_floor and not ({ra, rb} & above)
            assert _in(m, sc, [nd], 256, 500)[0] == t.rows(nd, scope_refs, 256, 500)
            assert _in(m, sc, [nd], 256, 501)[0] == t.rows(nd, scope_refs, 256, 501)
        m.set_option("scope_strategy", 0)
    m.close()


def test_needles_at_the_counter_widths_and_members_of_one_and_255_trigrams(case):
    rng = np.random.default_rng(43)
    needles = [b""] + [_needle_of(rng, k) for k in (15, 16)] + [case.r255, case.r256, b" ".join(case.plain[:140])]
    T = [len(Oracle.tokenise(s)) for s in needles]
    assert T[:5] == [1, 15, 16, 255, 256] and 650 <= T[5] <= 750
    scope_refs = np.concatenate([case.scope_of(600, 3), case.refs[:100],
                                 np.array([case.ref_empty, case.ref_digits, case.ref_255], dtype=np.uint32)])
    with case.m.scope(scope_refs) as sc:
        for strategy in (1, 2):
            for limit, p in ((10, 0), (256, 0), (10, 300), (10, 1000)):
                want = case.check(sc, scope_refs, needles, limit, p, strategy, "widths")
                _served_by(case.m, strategy)
        # the member of one trigram is the empty needle's row at J = 1; the member of 255 its own needle's
        assert [r[0] for r in want[0]] == sorted([case.ref_empty, case.ref_digits], key=lambda r: (case.t.entries[r][1], r))
        assert want[3][0] == [case.ref_255, 255, case.t.entries[case.ref_255][1], 255]


def test_a_member_of_256_trigrams_declines_direct_and_the_mask_serves_it(case):
    inner = case.scope_of(300, 8)
    wide = np.concatenate([inner, np.array([case.ref_256], dtype=np.uint32)])
    needles = [case.r256, case.r255] + case.needles_for(inner, 4)
    with case.m.scope(wide) as sc, case.m.scope(inner) as sc_inner:
        for strategy in (0, 2):                            # (forced direct: there is no direct form to serve it)
            want = case.check(sc, wide, needles, 10, 0, strategy, "wide")
            names = case.m.last_kernels()
            assert SWEEP in names and DIRECT not in names
        assert want[0][0] == [case.ref_256, 256, case.t.entries[case.ref_256][1], 256]
        case.check(sc_inner, inner, needles, 10, 0, 0, "inner")
        assert case.m.last_kernels() == [DIRECT]


def test_the_mask_on_a_multi_window_haystack_with_every_third_reference():
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
        m.set_option("scope_strategy", 1)
        for limit, p in ((10, 0), (10, 500), (2000, 0), (2000, 500)):
            assert _in(m, sc, needles, limit, p) == [t.rows(s, scope_refs, limit, p) for s in needles], (limit, p)
            assert SWEEP in m.last_kernels()
        m.set_option("scope_strategy", 2)                  # (23 334 members scored directly: a select of several steps)
        for limit, p in ((10, 0), (256, 0), (10, 500)):
            assert _in(m, sc, needles, limit, p) == [t.rows(s, scope_refs, limit, p) for s in needles], (limit, p)
            assert m.last_kernels() == [DIRECT]
        m.set_option("scope_strategy", 0)
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

    def check(what):
        want = [t.rows(s, scope_refs, 20, 300) for s in needles]
        for strategy in (1, 2):
            m.set_option("scope_strategy", strategy)
            assert _in(m, sc, needles, 20, 300) == want, (what, strategy)
            assert m.find_similar_in(sc, needles[0], 20, 300) == want[0], (what, strategy)
        m.set_option("scope_strategy", 0)
        return want

    want = check("fresh")
    best = want[1][0][0]                                   # a best row, deleted
    m.delete(best)
    t.delete(best)
    assert all(r[0] != best for r in check("deleted")[1])
    m.put(needles[6], n + 10, 3)                           # a member put after the scope was made: pending
    t.put(needles[6], n + 10, 3)
    assert check("pending")[6][0] == [n + 10, len(Oracle.tokenise(needles[6])), 3, len(Oracle.tokenise(needles[6]))]
    victim = int(scope_refs[2])                            # deleted and put again with another text: new trigrams, new R
    m.delete(victim)
    t.delete(victim)
    m.put(needles[7], victim, 1)
    t.put(needles[7], victim, 1)
    assert check("put again")[7][0][0] == victim
    before = m.device_info()["base_builds"]                # the log outgrows its budget: the pending member is folded
    bulk = [s + b" bulk" + bytes([97 + k]) for k in range(2) for s in strings[:2300]]   # (the log holds 4 096 puts)
    _put(m, t, bulk, list(range(n + 100, n + 100 + len(bulk))), [2] * len(bulk))
    assert check("folded")[6][0][0] == n + 10
    assert m.device_info()["base_builds"] > before
    sc.close()
    absent = np.arange(10 ** 6, 10 ** 6 + 50, dtype=np.uint32)
    for strategy in (0, 1, 2):
        m.set_option("scope_strategy", strategy)
        for members in (np.zeros(0, dtype=np.uint32), absent):      # an empty scope; one whose members are all absent
            with m.scope(members) as none:
                rows, counts, ntri = m.find_batch_similar_in_packed(none, *_pack(needles), 20, 0)
                assert not counts.any() and m.last_kernels() == []
                assert m.find_similar_in(none, needles[0], 20, 0) == []
    m.set_option("scope_strategy", 0)
    m.close()


def _each(m, scopes, which, needles, limit, p):
    packed, offsets = _pack(needles)
    return _got(*m.find_batch_similar_each_in(scopes, which, np.frombuffer(packed, dtype=np.uint8), offsets, limit, p))


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
        for limit, p in ((10, 0), (256, 300), (10, 1000)):
            got = _each(m, handles, which, needles, limit, p)
            names = m.last_kernels()
            assert EACH in names and SWEEP in names and DIRECT not in names
            want = [t.rows(s, None if w is None else family[w], limit, p) for s, w in zip(needles, which)]
            assert got == want, (limit, p)
            for i, (s, w) in enumerate(zip(needles, which)):           # element for element the single calls
                one = m.find_similar(s, limit, p) if w is None else m.find_similar_in(handles[w], s, limit, p)
                assert one == got[i], (i, limit, p)
        # an all-direct batch: one launch, nothing else
        only = [0, 3, 4, 3, 0]
        got = _each(m, handles, only, needles[:5], 10, 200)
        assert m.last_kernels() == [EACH]
        assert got == [t.rows(s, family[w], 10, 200) for s, w in zip(needles[:5], only)]
        # by reference: the stored strings' rows; an absent reference has none
        by = [int(direct[0]), int(direct[1]), int(small[0]), case.ref_256, 2, int(wide[0]), int(direct[2])]
        bw = [0, 4, 3, 1, 0, None, 2]
        for strategy in (0, 1):
            m.set_option("scope_strategy", strategy)
            rows, counts, rntri, nb = m.find_batch_by_reference_similar_each_in(handles, bw, by, 10, 300)
            got = _got(rows, counts, rntri)
            assert got == [t.by_reference(r, None if w is None else family[w], 10, 300) for r, w in zip(by, bw)]
            assert got[4] == [] and nb[4] == 0 and nb[3] == 256 and got[6] == []
            for k in (0, 1, 2, 3):                         # a member of its own scope: its own row at J = 1, behind only
                at = [x[0] for x in got[k]].index(by[k])   # members of the very same trigrams
                assert all(x[1] == x[3] == nb[k] for x in got[k][:at + 1])
        m.set_option("scope_strategy", 0)
        rows, counts, rntri, nb = m.find_batch_by_reference_similar_each_in(handles, [0, 3], [int(direct[0]), int(small[0])], 10, 0)
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
    assert n + 3 in [r[0] for r in t.rows(strings[2], None, 1000, 0)] and n + 3 not in family[0] and n + 3 not in family[1]
    try:
        for strategy, which, each, sweep in ((0, both, True, True), (1, both, False, True), (0, direct_only, True, False)):
            m.set_option("scope_strategy", strategy)
            for limit, p in ((10, 0), (3, 300)):
                got = _each(m, scopes, which, needles, limit, p)
                names = m.last_kernels()
                assert (EACH in names) == each and (SWEEP in names) == sweep, (strategy, names)
                assert got == [t.rows(s, None if w is None else family[w], limit, p) for s, w in zip(needles, which)]
                rows, counts, rntri, nb = m.find_batch_by_reference_similar_each_in(scopes, which, by, limit, p)
                names = m.last_kernels()
                assert (EACH in names) == each and (SWEEP in names) == sweep, (strategy, names)
                assert _got(rows, counts, rntri) == [t.by_reference(r, None if w is None else family[w], limit, p)
                                                     for r, w in zip(by, which)], (strategy, limit, p)
                assert nb.tolist() == [len(Oracle.tokenise(t.entries[r][0])) if r in t.entries else 0 for r in by]
    finally:
        m.set_option("scope_strategy", 0)
        for sc in scopes:
            sc.close()
        m.close()


def test_join_similar_within_over_three_blocks(case):
    blocks = [case.scope_of(120, 51), case.scope_of(257, 52), np.concatenate([case.scope_of(30, 53), np.array([2, 5], np.uint32)])]
    refs, which, rows = RawMap.join_similar_within(case.m, blocks, 10, 700)
    held = [(int(r), k) for k, b in enumerate(blocks) for r in np.unique(b).tolist() if r in case.t.entries]
    assert list(zip(refs.tolist(), which.tolist())) == held
    assert rows == [case.t.by_reference(r, blocks[k], 10, 700) for r, k in held]
    for row, (r, _) in zip(rows, held):                    # each its own row at J = 1, behind only members of the very
        T = len(Oracle.tokenise(case.t.entries[r][0]))     # same trigrams (which fill the limit for a popular name)
        k = [x[0] for x in row].index(r) if r in [x[0] for x in row] else len(row) - 1
        assert (r in [x[0] for x in row] or len(row) == 10) and all(x[1] == x[3] == T for x in row[:k + 1])
    assert case.m.last_kernels() == [EACH]


def test_scoped_similarity_calls_leave_the_unscoped_path_as_it_was(case):
    m = case.m
    rng = np.random.default_rng(60)
    needles = [case.plain[i][: max(3, len(case.plain[i]) - int(rng.integers(0, 4)))] for i in rng.choice(case.n_plain, 3000)]
    packed, offsets = _pack(needles)
    buf = np.frombuffer(packed, dtype=np.uint8)
    scope_refs = case.scope_of(600, 90)
    which = rng.integers(0, 2, size=len(needles)).astype(np.uint32)

    def unscoped(sc):
        out = []
        for call in (lambda: m.find_batch_packed(buf, offsets, 10), lambda: m.find_batch_similar_packed(buf, offsets, 10, 300),
                     lambda: m.find_batch_in(sc, buf, offsets, 10), lambda: m.find_batch_each_in([sc, sc], which, buf, offsets, 10)):
            res = call()
            counts = res[1]
            live = np.arange(res[0].shape[1])[None, :] < counts[:, None].astype(np.int64)
            out.append((m.last_kernels(), counts.copy(), np.where(live[:, :, None], res[0], 0)))
        return out

    with m.scope(scope_refs) as sc:
        for _ in range(2):                                 # (the first batch of a class may measure every sweep)
            before = unscoped(sc)
        choice0, tuned0 = m.get_option("ws_choice"), m.get_option("tuned_class")
        for strategy in (0, 1, 2):
            m.set_option("scope_strategy", strategy)
            m.find_batch_similar_in_packed(sc, buf, offsets, 10, 300)
            m.find_batch_similar_each_in([sc, sc], [0, None] * (len(needles) // 2), buf, offsets, 10, 300)
        m.set_option("scope_strategy", 0)
        assert m.get_option("ws_choice") == choice0 and m.get_option("tuned_class") == tuned0
        after = unscoped(sc)
    for (k0, c0, r0), (k1, c1, r1) in zip(before, after):
        assert k0 == k1 and np.array_equal(c0, c1) and np.array_equal(r0, r1)


def test_three_repeated_calls_are_byte_for_byte_equal(case):
    m = case.m
    direct, wide = case.scope_of(600, 21), np.concatenate([case.scope_of(300, 22), np.array([case.ref_256], np.uint32)])
    needles = case.needles_for(direct, 10)
    packed, offsets = _pack(needles)
    buf = np.frombuffer(packed, dtype=np.uint8)
    which = [0, 1, None, 0, 1, None, 0, 1, 0, 0]
    with m.scope(direct) as a, m.scope(wide) as b:
        for call in (lambda: m.find_batch_similar_in_packed(a, buf, offsets, 256, 0),
                     lambda: m.find_batch_similar_in_packed(b, buf, offsets, 256, 0),
                     lambda: m.find_batch_similar_each_in([a, b], which, buf, offsets, 100, 200),
                     lambda: m.find_batch_by_reference_similar_each_in([a, b], [0, 1, 0], direct[:3], 100, 200)):
            first = [x.tobytes() for x in call()]
            for _ in range(2):
                assert [x.tobytes() for x in call()] == first
