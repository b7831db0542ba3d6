"""The threshold and the similarity find, their by-reference forms and their scoped forms under the mask strategy on
tests/dense_delta_case.py's map: a base image with tombstones behind its bitmaps and a delta image with dense slices of
its own.  above_sweep_kernel and the similarity sweep run once per image; on the delta image the list of at most 64 dense
slices, the L largest left out and the bitmap probes run for every delta head (more than 64 dense slices in the delta's
one window, both counter widths), and on the base image the tombstone bitmap -- or, in a scoped call, the scope's base
and delta masks in its place -- decides about ranks that pass their bar through left-out bitmaps alone: the deleted twins
of two family heads, the base ranks of the moved rows.  Rows equal the host's truths over what is held now
(tests/dense_truths.py: numpy over the strings' tokenisations, nothing of the library) exactly, three calls give
identical bytes, last_kernels() names the sweep, and after the log is folded into a rebuilt base image every answer is
the same bytes again: no output depends on positions, so two images and tombstones answer as one image does.
tests/test_dense_delta_case.py proves the map's conditions on the host.

Not covered: a delta image of more than one window or with ranks of 32 768 and more (a base of millions of references);
DeviceInfo.n_bitmaps counts the base image's bitmaps only."""
import numpy as np
import pytest

import dense_delta_case as C
import dense_truths as DT
from blurrily_amd.map import _pack
from dense_truths import _same_bytes

pytestmark = pytest.mark.gpu
A_SWEEP, A_DIRECT, A_EACH = "above_sweep_kernel", "scope_above_kernel", "scope_above_each_kernel"
S_SWEEP, S_DIRECT, S_EACH = "similar_sweep_kernel", "scope_similar_kernel", "scope_similar_each_kernel"
SIMILAR_LIMITS = (10, 1000)
ABSENT = 123456789


@pytest.fixture(scope="module")
def case():
    made = {}
    h = C.host()
    c0 = C.inputs(h)
    # the scopes: `before` is made on the base image in front of the first mutation and names references the map does not
    # hold yet, `after` once the log is full -- each with pending, deleted and moved members
    scopes = {"before": np.concatenate([c0.lists["short"], h.phrases[::4], h.handmade.listed]),
              "after": np.array(sorted(set(h.base.refs[DT.key_pairs(h.base.refs) == 0].tolist())
                                       | {r for r in h.pending if (r // 2) % 2 == 0}), dtype=np.uint32)}
    for name, refs in scopes.items():
        members = set(refs.tolist())
        assert members & set(h.pending) and members & set(h.tombstones) and members & set(h.moved), name
        assert members & set(h.twins) and members & set(h.delta_heads), name
    c = C.gpu_case(before=lambda m: made.update(before=m.scope(scopes["before"])))
    made["after"] = c.m.scope(scopes["after"])
    c.scopes, c.handles = scopes, made
    c.needles = C.find_needles(h)
    assert len(c.needles) == 10 + 15 + 1 + 2 + 2 + 2 + 40
    c.packed, c.offsets = _pack(c.needles)
    c.above_bars = ((1, 0), (3, 0)) + tuple((0, p) for p in c.floors) + ((0, 1000),)
    c.above = DT.ScopedAbove(DT.ArrayAbove(h.strings, h.refs, h.weights))
    c.similar = DT.ScopedSimilar(DT.FlooredSimilar(h.strings, h.refs, h.weights, DT.LEAST))
    # by reference: the delta families, the base families with their deleted twins (no rows, ntri 0) and their moved rows
    # (the new text's trigrams), and a reference that was never held
    c.by_ref = np.concatenate([h.delta_family, h.base_family, np.array([C.GONE_REF, ABSENT], dtype=np.uint32)])
    c.by_ref_strings = [h.held.get(int(r)) for r in c.by_ref]     # (None: not held)
    c.by_ref_ntri = [h.T(r) if int(r) in h.held else 0 for r in c.by_ref]
    assert c.by_ref_ntri.count(0) == len(h.twins) + 2
    yield c
    for sc in made.values():
        sc.close()
    c.m.close()


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
        if s is None:                                              # a reference that is not held: no rows
            assert int(row_off[i + 1]) == int(row_off[i]), (i, mm, mp)
            continue
        want = truth.rows(s, scope, mm, mp)
        assert int(row_off[i + 1]) - int(row_off[i]) == len(want), (i, s[:40], mm, mp, len(want))
        assert np.array_equal(rows[int(row_off[i]):int(row_off[i + 1])], want), (i, s[:40], mm, mp)


def _similar_lists(out):
    rows, counts, ntri = out[:3]
    return [[r + [t] for r, t in zip(rows[i, :c].tolist(), ntri[i, :c].tolist())] for i, c in enumerate(counts.tolist())]


def _similar_equal(out, needles, scopes, truth, limit, p):
    got = _similar_lists(out)
    for i, (s, scope) in enumerate(zip(needles, scopes)):
        assert got[i] == ([] if s is None else truth.rows(s, scope, limit, p)), (i, (s or b"")[:40], limit, p)
    return got


def _masked(m, fn):
    """fn under the mask strategy; the kernels of the last call in .names."""
    def call():
        out, call.names = _under(m, 1, fn)
        return out
    return call


_thrice = C.thrice


def test_the_log_is_as_the_host_books_it(case):
    C.assert_log(case.m, case.h)
    assert case.m.device_info()["n_windows"] == 2                 # (the base image's)


# ---- the threshold find and the similarity find --------------------------------------------------------------------------

def test_find_above_equals_the_truth_over_what_is_held_now(case):
    m, h, needles = case.m, case.h, case.needles
    whole = [None] * len(needles)
    for mm, mp in case.above_bars:
        one = _thrice(case, f"above {mm, mp}",
                      lambda mm=mm, mp=mp: m.find_batch_above_packed(case.packed, case.offsets, mm, mp))
        assert A_SWEEP in m.last_kernels()
        _above_equal(*one, needles, whole, case.above, mm, mp)
        print(f"above {mm, mp}: {len(one[0])} rows")
    rows, row_off = m.find_batch_above_packed(case.packed, case.offsets, 0, 600)
    of = lambda i: set(rows[int(row_off[i]):int(row_off[i + 1]), 0].tolist())
    # a delta head's rows are its family, rows of the delta image
    for i, head in enumerate(h.delta_heads):
        assert of(i) >= {head, head + 1, head + 2, head + 3}, head
    # a base head's rows: its family without the deleted twin, with the moved row where the head's text moved
    for i, head in enumerate(h.base_heads):
        got = of(len(h.delta_heads) + i)
        assert head in got and (head + 1 in got) == (head + 1 not in h.twins), head
        assert (head + 2 in got) or head not in h.moved_heads, head
    glued = of(needles.index(h.held[h.handmade.glued]))
    assert h.handmade.glued in glued and h.copy_deleted not in glued


def test_find_above_by_reference_equals_the_truth(case):
    m = case.m
    whole = [None] * len(case.by_ref)
    for mm, mp in ((0, 200), (0, 600), (0, case.p_star), (0, 1000)):
        rows, row_off, ntri = _thrice(case, f"above by reference {mm, mp}",
                                      lambda mm=mm, mp=mp: m.find_batch_by_reference_above(case.by_ref, mm, mp))
        assert A_SWEEP in m.last_kernels()
        assert ntri.tolist() == case.by_ref_ntri
        _above_equal(rows, row_off, case.by_ref_strings, whole, case.above, mm, mp)


def test_find_similar_equals_the_truth_over_what_is_held_now(case):
    m, needles = case.m, case.needles
    whole = [None] * len(needles)
    for limit in SIMILAR_LIMITS:
        for p in case.floors:
            one = _thrice(case, f"similar {limit, p}",
                          lambda limit=limit, p=p: m.find_batch_similar_packed(case.packed, case.offsets, limit, p))
            assert S_SWEEP in m.last_kernels()
            _similar_equal(one, needles, whole, case.similar, limit, p)


def test_find_similar_by_reference_equals_the_truth(case):
    m = case.m
    whole = [None] * len(case.by_ref)
    for limit, p in ((10, 350), (1000, 200), (1000, 600), (1000, case.p_star + 1)):
        rows, counts, ntri, nb = _thrice(case, f"similar by reference {limit, p}",
                                         lambda limit=limit, p=p: m.find_batch_by_reference_similar(case.by_ref, limit, p))
        assert S_SWEEP in m.last_kernels()
        assert nb.tolist() == case.by_ref_ntri
        _similar_equal((rows, counts, ntri), case.by_ref_strings, whole, case.similar, limit, p)


# ---- the scoped forms under the mask strategy ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["before", "after"])
def test_scoped_threshold_find_through_the_masks_equals_the_truth(case, name):
    m, sc, scope = case.m, case.handles[name], case.scopes[name]
    live = set(DT.live_of(case.above.above, scope).tolist())
    assert live & set(case.h.pending) and not live & (set(case.h.tombstones) - set(case.h.moved))
    n_rows = []
    for mm, mp in case.above_bars:
        call = _masked(m, lambda mm=mm, mp=mp: m.find_batch_above_in_packed(sc, case.packed, case.offsets, mm, mp))
        one = _thrice(case, f"above in {name} {mm, mp}", call)
        assert A_SWEEP in call.names and A_DIRECT not in call.names and A_EACH not in call.names, call.names
        _above_equal(*one, case.needles, [scope] * len(case.needles), case.above, mm, mp)
        n_rows.append(len(one[0]))
    print(f"{name}: rows per bar {n_rows}")
    assert n_rows[0] > n_rows[1] > 0 and n_rows[-2] > 0


@pytest.mark.parametrize("name", ["before", "after"])
def test_scoped_similarity_find_through_the_masks_equals_the_truth(case, name):
    m, sc, scope = case.m, case.handles[name], case.scopes[name]
    seen = 0
    for limit in (1,) + SIMILAR_LIMITS:
        for p in case.floors:
            call = _masked(m, lambda limit=limit, p=p: m.find_batch_similar_in_packed(sc, case.packed, case.offsets, limit, p))
            one = _thrice(case, f"similar in {name} {limit, p}", call)
            assert S_SWEEP in call.names and S_DIRECT not in call.names and S_EACH not in call.names, call.names
            seen += sum(map(len, _similar_equal(one, case.needles, [scope] * len(case.needles), case.similar, limit, p)))
    assert seen > 0


def _cycle(n):
    each = ("before", "after", None)
    which = [k % 3 if each[k % 3] is not None else None for k in range(n)]
    return which, [each[k % 3] for k in range(n)]


def test_a_scope_per_needle_under_the_mask_strategy_equals_the_truth(case):
    m = case.m
    handles = [case.handles["before"], case.handles["after"]]
    which, names_of = _cycle(len(case.needles))
    scopes = [None if name is None else case.scopes[name] for name in names_of]
    for mm, mp in ((3, 0), (0, 200), (0, 600), (0, case.p_star)):
        call = _masked(m, lambda mm=mm, mp=mp: m.find_batch_above_each_in(handles, which, case.packed, case.offsets, mm, mp))
        one = _thrice(case, f"above each in {mm, mp}", call)
        assert A_SWEEP in call.names and A_EACH not in call.names and A_DIRECT not in call.names, call.names
        _above_equal(*one, case.needles, scopes, case.above, mm, mp)
    for limit, p in ((1, 200), (10, 350), (1000, 200), (1000, 600), (1000, case.p_star + 1)):
        call = _masked(m, lambda limit=limit, p=p: m.find_batch_similar_each_in(handles, which, case.packed, case.offsets,
                                                                                 limit, p))
        one = _thrice(case, f"similar each in {limit, p}", call)
        assert S_SWEEP in call.names and S_EACH not in call.names and S_DIRECT not in call.names, call.names
        _similar_equal(one, case.needles, scopes, case.similar, limit, p)


# ---- the exact bar, in the delta ------------------------------------------------------------------------------------------

def test_the_copies_whose_matches_are_exactly_the_bar_are_rows_of_the_glued_string_at_500_and_not_at_501(case):
    m, h, g = case.m, case.h, case.h.handmade
    needles = [h.held[g.glued], C.WORD, C.OTHER]
    packed, offsets = _pack(needles)
    copies = set(g.held_copies.tolist())
    for p, n in ((500, len(copies) + 1), (501, 1)):
        assert len(case.above.rows(needles[0], None, 0, p)) == n
        one = m.find_batch_above_packed(packed, offsets, 0, p)
        _above_equal(*one, needles, [None] * 3, case.above, 0, p)
        _similar_equal(m.find_batch_similar_packed(packed, offsets, 1000, p), needles, [None] * 3, case.similar, 1000, p)
        rows, row_off, ntri = m.find_batch_by_reference_above(np.array([g.glued, h.copy_deleted], dtype=np.uint32), 0, p)
        assert ntri.tolist() == [12, 0] and np.array_equal(rows, case.above.rows(needles[0], None, 0, p))
        assert (set(rows[:, 0].tolist()) >= copies) == (p == 500) and h.copy_deleted not in rows[:, 0].tolist()
        for name in ("before", "after"):
            out, names = _under(m, 1, lambda: m.find_batch_above_in_packed(case.handles[name], packed, offsets, 0, p))
            assert A_SWEEP in names
            _above_equal(*out, needles, [case.scopes[name]] * 3, case.above, 0, p)


# ---- fold invariance (the last test: it changes the map) -----------------------------------------------------------------

def test_after_the_fold_one_image_answers_every_call_with_the_same_bytes(case):
    C.fold_and_compare(case, at_least=60)
