"""The mask strategy of the scoped threshold and similarity finds on tests/dense_case.py's map.  A scoped call hands the
scope's masks to above_sweep_kernel and to the similarity sweep in the tombstone bitmaps' place; the mask test sits
behind the bitmap probes, and in the similarity sweep in front of the list whose worst row raises t, rlo, rhi and with
t the number L of slices left out from one window to the next -- so a scope decides L.  The maps of
tests/test_gpu_scope_above.py and tests/test_gpu_scope_similar.py leave no slice out; here every family head has more
than 64 dense slices in window 0.  Rows equal the scoped truths of tests/dense_truths.py exactly (the whole-map rows
filtered to the scope's live set; for the similarity find filtered BEFORE the cut) and the library's own unscoped rows
filtered on the host, two calls give identical bytes -- the check that the count pass and the emit pass agree whichever
64 slices were listed -- and last_kernels() names the kernel that served the call.  The scopes: `short` (812 listed
references), `nofirst` (without each family's two identical strings: a head's best rows, J = 1000, are no members and
the list fills from what remains), `half` and `upper` (half the map each; `upper` leaves only rows of the second half
window and of window 1), `nolow` (without the lower member of the family pair) and `words97` (words alone, the one
scope with a direct form).  tests/test_dense_scoped_case.py proves their conditions on the host."""
import numpy as np
import pytest

import dense_case as D
import dense_truths as DT
import workloads as W
from blurrily_amd import RawMap
from blurrily_amd.map import _pack
from dense_truths import _same_bytes
from test_gpu_dense_floor_sweeps import ABOVE_BARS, _needles

pytestmark = pytest.mark.gpu
A_SWEEP, A_DIRECT, A_EACH = "above_sweep_kernel", "scope_above_kernel", "scope_above_each_kernel"
S_SWEEP, S_DIRECT, S_EACH = "similar_sweep_kernel", "scope_similar_kernel", "scope_similar_each_kernel"
SCOPES = ("short", "nofirst", "half", "upper", "nolow", "words97")
LIMITS = (1, 10, 1000)                                         # 1000 is above the direct pool and the list: count and emit passes
FLOORS = DT.FIXED_FLOORS
DIRECT_LIMIT = 256                                             # find_kernels.h: kScopeMaxKeep


class Case:
    def __init__(self):
        self.m, self.h = D.build()
        h = self.h
        c = DT.inputs(h)
        self.scopes, self.family, self.pair = c.scopes, c.family, c.pair
        self.needles = _needles(h, h.strings[:D.N_WORDS])
        assert len(self.needles) == 15 + 2 + 2 + 40
        self.packed, self.offsets = _pack(self.needles)
        self.above = DT.ScopedAbove(DT.ArrayAbove(h.strings, h.refs, h.weights))
        self.similar = DT.ScopedSimilar(DT.FlooredSimilar(h.strings, h.refs, h.weights, DT.LEAST))
        self.handles = {name: self.m.scope(refs) for name, refs in self.scopes.items()}
        self._unscoped = {}

    def unscoped_above(self, mm, mp):
        """The library's own whole-map threshold rows, needle by needle."""
        if (mm, mp) not in self._unscoped:
            rows, row_off = self.m.find_batch_above_packed(self.packed, self.offsets, mm, mp)
            self._unscoped[mm, mp] = [rows[int(row_off[i]):int(row_off[i + 1])] for i in range(len(self.needles))]
        return self._unscoped[mm, mp]

    def unscoped_similar(self, p):
        """... and its whole-map similarity rows at the largest limit: [ref, m, weight, R] lists and the counts."""
        if p not in self._unscoped:
            rows, counts, ntri = self.m.find_batch_similar_packed(self.packed, self.offsets, LIMITS[-1], p)
            self._unscoped[p] = (_similar_lists((rows, counts, ntri)), counts.tolist())
        return self._unscoped[p]

    def close(self):
        for sc in self.handles.values():
            sc.close()
        self.m.close()


@pytest.fixture(scope="module")
def case():
    c = Case()
    yield c
    c.close()


def _under(m, strategy, call):
    """call() under "scope_strategy" `strategy`: (its result, the kernels it launched)."""
    m.set_option("scope_strategy", strategy)
    try:
        out = call()
        return out, m.last_kernels()
    finally:
        m.set_option("scope_strategy", 0)


def _above_equal(rows, row_off, needles, scopes, truth, mm, mp):
    """rows / row_off against the scoped truth: needle i among scopes[i] (None: the whole map)."""
    assert rows.dtype == np.uint32 and len(row_off) == len(needles) + 1 and int(row_off[0]) == 0
    assert int(row_off[-1]) == len(rows)
    for i, (s, scope) in enumerate(zip(needles, scopes)):
        want = truth.rows(s, scope, mm, mp)
        assert int(row_off[i + 1]) - int(row_off[i]) == len(want), (s[:40], mm, mp, len(want))
        assert np.array_equal(rows[int(row_off[i]):int(row_off[i + 1])], want), (s[:40], mm, mp)


def _similar_lists(out):
    rows, counts, ntri = out[:3]
    return [[r + [t] for r, t in zip(rows[i, :c].tolist(), ntri[i, :c].tolist())] for i, c in enumerate(counts.tolist())]


def _similar_equal(out, needles, scopes, truth, limit, p):
    got = _similar_lists(out)
    for i, (s, scope) in enumerate(zip(needles, scopes)):
        assert got[i] == truth.rows(s, scope, limit, p), (s[:40], limit, p)
    return got


# ---- the scoped threshold find -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCOPES)
def test_scoped_threshold_find_through_the_mask_equals_the_truth_and_the_filtered_unscoped_rows(case, name):
    m, sc, scope = case.m, case.handles[name], case.scopes[name]
    live = DT.live_of(case.above.above, scope)
    n_rows = []
    for mm, mp in ABOVE_BARS:
        call = lambda: m.find_batch_above_in_packed(sc, case.packed, case.offsets, mm, mp)
        one, names = _under(m, 1, call)
        assert A_SWEEP in names and A_DIRECT not in names and A_EACH not in names, names
        _above_equal(*one, case.needles, [scope] * len(case.needles), case.above, mm, mp)
        # the definition: the library's own unscoped rows, filtered to the scope's live set on the host
        rows, row_off = one
        for i, whole in enumerate(case.unscoped_above(mm, mp)):
            kept = whole[np.isin(whole[:, 0].astype(np.int64), live)]
            assert np.array_equal(rows[int(row_off[i]):int(row_off[i + 1])], kept), (i, mm, mp)
        two, _ = _under(m, 1, call)
        _same_bytes(one, two)
        n_rows.append(len(rows))
        print(f"{name}, above {mm, mp}: {len(rows)} rows")
        # forced direct: a scope with a wide member has no direct form and the mask serves it; words97 has one
        forced, names = _under(m, 2, call)
        if name == "words97":
            assert names == [A_DIRECT], names
        else:
            assert A_SWEEP in names and A_DIRECT not in names, names
        _same_bytes(one, forced)
    assert n_rows[0] > n_rows[1] > 0 and (n_rows[3] > 0 or name == "words97")


def test_nolow_takes_exactly_the_lower_member_from_the_higher_members_rows(case):
    m, h = case.m, case.h
    low, high = case.pair
    s = h.held[high]
    m.set_option("scope_strategy", 1)
    try:
        short = m.find_above_in(case.handles["short"], s, 0, 600)
        nolow = m.find_above_in(case.handles["nolow"], s, 0, 600)
    finally:
        m.set_option("scope_strategy", 0)
    assert low in [r[0] for r in short] and nolow == [r for r in short if r[0] != low]
    assert short == case.above.rows(s, case.scopes["short"], 0, 600).tolist()


# ---- the scoped similarity find ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCOPES)
def test_scoped_similarity_find_through_the_mask_equals_the_truth_and_the_filtered_unscoped_rows(case, name):
    m, sc, scope = case.m, case.handles[name], case.scopes[name]
    live = set(DT.live_of(case.similar.similar, scope).tolist())
    seen = compared = 0
    for limit in LIMITS:
        for p in FLOORS:
            call = lambda: m.find_batch_similar_in_packed(sc, case.packed, case.offsets, limit, p)
            one, names = _under(m, 1, call)
            assert S_SWEEP in names and S_DIRECT not in names and S_EACH not in names, names
            got = _similar_equal(one, case.needles, [scope] * len(case.needles), case.similar, limit, p)
            # the definition: where the unscoped find at the largest limit is not cut, its rows filtered, then the limit
            whole, counts = case.unscoped_similar(p)
            for i, rows in enumerate(whole):
                if counts[i] < LIMITS[-1]:
                    assert got[i] == [r for r in rows if r[0] in live][:limit], (i, limit, p)
                    compared += 1
            two, _ = _under(m, 1, call)
            _same_bytes(one, two)
            seen += sum(len(g) for g in got)
            forced, names = _under(m, 2, call)
            if name == "words97" and limit <= DIRECT_LIMIT:
                assert names == [S_DIRECT], names
            else:                                                   # a wide member, or a limit above the direct pool
                assert S_SWEEP in names and S_DIRECT not in names, names
            assert _similar_lists(forced) == got and forced[1].tobytes() == one[1].tobytes()
    assert seen > 0 and compared >= len(LIMITS) * len(FLOORS) * 50
    if name == "nofirst":
        # a head's two best rows are no members: its first row is one the whole-map find ranks third or lower
        for i, x in enumerate(case.h.heads):
            rows = _similar_lists(m.find_batch_similar_in_packed(sc, *_pack([case.needles[i]]), 1, 200))[0]
            assert rows and rows[0][0] not in (x, x + 1) and rows[0][0] in case.h.family(x), x
    if name == "upper":
        rows = _similar_lists(m.find_batch_similar_in_packed(sc, case.packed, case.offsets, 1000, 200))
        at = [case.h.loc[r[0]] for rs in rows for r in rs]
        assert at and all(w == 1 or r >= D.HALF for w, r in at) and {w for w, _ in at} == {0, 1}


# ---- a scope per needle ------------------------------------------------------------------------------------------------

EACH = ("short", "nofirst", "words97", None)                  # `which` cycles over these; None: NO_SCOPE


def _cycle(n):
    which = [k % len(EACH) if EACH[k % len(EACH)] is not None else None for k in range(n)]
    return which, [EACH[k % len(EACH)] for k in range(n)]


def test_a_scope_per_needle_threshold_find_equals_the_single_scope_calls_and_the_truth(case):
    m = case.m
    handles = [case.handles[name] for name in EACH[:3]]
    which, names_of = _cycle(len(case.needles))
    scopes = [None if name is None else case.scopes[name] for name in names_of]
    for mm, mp in ABOVE_BARS:
        one = m.find_batch_above_each_in(handles, which, case.packed, case.offsets, mm, mp)
        names = m.last_kernels()
        assert A_EACH in names and A_SWEEP in names and A_DIRECT not in names, names   # words97 directly, the others swept
        _above_equal(*one, case.needles, scopes, case.above, mm, mp)
        _same_bytes(one, m.find_batch_above_each_in(handles, which, case.packed, case.offsets, mm, mp))
        forced, names = _under(m, 1, lambda: m.find_batch_above_each_in(handles, which, case.packed, case.offsets, mm, mp))
        assert A_SWEEP in names and A_EACH not in names, names     # three masked groups and the NO_SCOPE group
        _same_bytes(one, forced)
        # each needle's rows are those of the single-scope call of its scope
        rows, row_off = one
        for k, name in enumerate(EACH):
            mine = [i for i in range(len(case.needles)) if names_of[i] == name]
            packed, offsets = _pack([case.needles[i] for i in mine])
            s_rows, s_off = (m.find_batch_above_packed(packed, offsets, mm, mp) if name is None else
                             m.find_batch_above_in_packed(case.handles[name], packed, offsets, mm, mp))
            for j, i in enumerate(mine):
                assert np.array_equal(rows[int(row_off[i]):int(row_off[i + 1])], s_rows[int(s_off[j]):int(s_off[j + 1])]), (name, i)


def test_a_scope_per_reference_threshold_find_equals_the_truth(case):
    m, h = case.m, case.h
    handles = [case.handles[name] for name in EACH[:3]]
    refs = np.concatenate([case.family, np.array([123456789], dtype=np.uint32)])
    which, names_of = _cycle(len(refs))
    scopes = [None if name is None else case.scopes[name] for name in names_of]
    strings = [h.held[int(r)] for r in case.family]
    for strategy in (0, 1):
        for mm, mp in ((3, 0), (0, 200), (0, 600), (0, 1000)):
            (rows, row_off, ntri), names = _under(m, strategy, lambda: m.find_batch_by_reference_above_each_in(
                handles, which, refs, mm, mp))
            assert A_SWEEP in names and (A_EACH in names) == (strategy == 0), names
            assert ntri.tolist() == [h.T(int(r)) for r in case.family] + [0]
            assert row_off[-1] == row_off[-2]                      # (the absent reference: no rows)
            _above_equal(rows, row_off[:-1], strings, scopes[:-1], case.above, mm, mp)


def test_a_scope_per_needle_similarity_find_equals_the_single_scope_calls_and_the_truth(case):
    m = case.m
    handles = [case.handles[name] for name in EACH[:3]]
    which, names_of = _cycle(len(case.needles))
    scopes = [None if name is None else case.scopes[name] for name in names_of]
    for limit in LIMITS:
        for p in FLOORS:
            one = m.find_batch_similar_each_in(handles, which, case.packed, case.offsets, limit, p)
            names = m.last_kernels()
            assert S_SWEEP in names and (S_EACH in names) == (limit <= DIRECT_LIMIT) and S_DIRECT not in names, names
            got = _similar_equal(one, case.needles, scopes, case.similar, limit, p)
            _same_bytes(one, m.find_batch_similar_each_in(handles, which, case.packed, case.offsets, limit, p))
            forced, names = _under(m, 1, lambda: m.find_batch_similar_each_in(handles, which, case.packed, case.offsets,
                                                                              limit, p))
            assert S_SWEEP in names and S_EACH not in names, names
            assert _similar_lists(forced) == got
            for name in EACH:
                mine = [i for i in range(len(case.needles)) if names_of[i] == name]
                packed, offsets = _pack([case.needles[i] for i in mine])
                single = _similar_lists(m.find_batch_similar_packed(packed, offsets, limit, p) if name is None else
                                        m.find_batch_similar_in_packed(case.handles[name], packed, offsets, limit, p))
                assert single == [got[i] for i in mine], (name, limit, p)


def test_a_scope_per_reference_similarity_find_equals_the_truth(case):
    m, h = case.m, case.h
    handles = [case.handles[name] for name in EACH[:3]]
    refs = np.concatenate([case.family, np.array([123456789], dtype=np.uint32)])
    which, names_of = _cycle(len(refs))
    scopes = [None if name is None else case.scopes[name] for name in names_of]
    strings = [h.held[int(r)] for r in case.family]
    for strategy in (0, 1):
        for limit, p in ((1, 200), (10, 350), (1000, 200), (1000, 600)):
            (rows, counts, ntri, nb), names = _under(m, strategy, lambda: m.find_batch_by_reference_similar_each_in(
                handles, which, refs, limit, p))
            assert S_SWEEP in names, names
            assert nb.tolist() == [h.T(int(r)) for r in case.family] + [0] and counts[-1] == 0
            _similar_equal((rows[:-1], counts[:-1], ntri[:-1]), strings, scopes[:-1], case.similar, limit, p)


# ---- a scope made before puts ------------------------------------------------------------------------------------------

def test_a_scope_made_before_puts_has_the_pending_members_and_not_the_deleted_ones_before_and_after_the_fold():
    """The hand-made map (a bar of 6 at floor 500, five slices left out): a scope of the glued string and 35 copies that
    also names five references the map does not hold yet; ten more copies are put, five under those references and five
    outside the scope (the delta image, through the scope's delta mask), and two members are deleted.  Then a put of
    more strings than the log holds folds the pending puts into a rebuilt base image."""
    c = DT.handmade()
    held = dict(c.held)
    weight_of = dict(zip(c.refs.tolist(), c.weights.tolist()))
    m = RawMap()
    m.set_option("dense_min", D.DENSE_MIN)
    m.put_many_packed(*_pack([held[int(r)] for r in c.refs]), c.refs, c.weights)
    try:
        m.sync_device()
        builds = m.device_info()["base_builds"]
        inside, outside = list(range(300, 305)), list(range(310, 315))
        scope = np.array([1] + list(range(2, 37)) + inside, dtype=np.uint32)
        sc = m.scope(scope)
        needles = [c.glued, c.word, c.other]

        def check(what):
            refs = np.array(sorted(held), dtype=np.uint32)
            strings = [held[int(r)] for r in refs]
            weights = [weight_of[int(r)] for r in refs]
            above = DT.ScopedAbove(DT.ArrayAbove(strings, refs, weights))
            similar = DT.ScopedSimilar(DT.FlooredSimilar(strings, refs, weights, 0))
            packed, offsets = _pack(needles)
            for mm, mp in ((1, 0), (0, 500), (0, 501)):
                call = lambda: m.find_batch_above_in_packed(sc, packed, offsets, mm, mp)
                one, names = _under(m, 1, call)
                assert A_SWEEP in names and A_DIRECT not in names, (what, names)
                _above_equal(*one, needles, [scope] * 3, above, mm, mp)
                _same_bytes(one, _under(m, 1, call)[0])
            for limit in (1, 10, 1000):
                for p in (0, 500, 501):
                    call = lambda: m.find_batch_similar_in_packed(sc, packed, offsets, limit, p)
                    one, names = _under(m, 1, call)
                    assert S_SWEEP in names and S_DIRECT not in names, (what, names)
                    _similar_equal(one, needles, [scope] * 3, similar, limit, p)
            return above

        above = check("fresh")
        assert len(above.rows(c.glued, scope, 0, 500)) == 36 and len(above.rows(c.glued, scope, 0, 501)) == 1
        for r in inside + outside:                                 # ten more copies, pending
            m.put(c.word, r, 1)
            held[r], weight_of[r] = c.word, 1
        for r in (2, 36):                                          # two members deleted
            m.delete(r)
            del held[r]
        above = check("pending")
        info = m.device_info()
        assert info["n_pending"] == 10 and info["base_builds"] == builds
        got = set(above.rows(c.glued, scope, 0, 500)[:, 0].tolist())
        assert set(inside) <= got and not set(outside) & got and not {2, 36} & got and len(got) == 36 - 2 + 5
        # the fold: a log past its budget of 4 096 puts is folded into a rebuilt base image at the next find
        hay, off = W.words(4200, seed=34)
        bulk = np.arange(10 ** 6, 10 ** 6 + 4200, dtype=np.uint32)
        m.put_many_packed(hay, off, bulk, np.ones(4200, dtype=np.uint32))
        held.update(zip(bulk.tolist(), W.unpack(hay, off)))
        weight_of.update({r: 1 for r in bulk.tolist()})
        above = check("folded")
        info = m.device_info()
        assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
        assert set(above.rows(c.glued, scope, 0, 500)[:, 0].tolist()) == got
        sc.close()
    finally:
        m.close()
