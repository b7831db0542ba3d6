"""tests/scope_boundary_case.py proven without a GPU: the numpy truth of the scoped find is the
oracle where the scope is the whole map, every scope has the property it was made for, and the small map of the direct
select holds its edge members and needles."""
import numpy as np
import pytest

import boundary_case as B
import scope_boundary_case as S
from helpers import Oracle
from scope_truth import Truth, c_prefix


@pytest.fixture(scope="module")
def case():
    return B.case()


@pytest.fixture(scope="module")
def truth_of(case):
    made = {}

    def get(which):
        if which not in made:
            made[which] = S.ScopedTruth(case, which)
        return made[which]
    return get


@pytest.mark.parametrize("limit", [10, 1025])
def test_the_truth_is_the_oracle_when_the_scope_is_the_whole_map(case, truth_of, limit):
    t = truth_of("a")
    want = case.oracle("a").batch(*case.pack(case.needles), limit=limit)
    rows, counts = t.batch("all", S.scope(case, "a", "all"), limit)
    assert np.array_equal(counts, want["counts"])
    live = np.arange(limit)[None, :] < counts[:, None].astype(np.int64)
    assert np.array_equal(np.where(live[:, :, None], rows, 0), np.where(live[:, :, None], want["rows"], 0))


def test_every_scope_has_the_property_it_was_made_for(case, truth_of):
    S.conditions(case, truth_of)


def test_the_scopes_are_sorted_distinct_references_of_their_map(case):
    for which, names in (("a", S.SCOPES_A), ("b", S.SCOPES_A), ("c", S.SCOPES_C)):
        held = set(S.view(case, which).refs.tolist())
        for name in names:
            refs = S.scope(case, which, name)
            assert refs.dtype == np.uint32 and len(refs) and (np.diff(refs.astype(np.int64)) > 0).all(), (which, name)
            assert set(refs.tolist()) <= held, (which, name)


def test_the_small_map_of_the_direct_select(case):
    d = S.direct_case()
    S.direct_conditions(d)
    o = Oracle()
    for s, r, w in zip(d.strings, d.refs.tolist(), d.weights.tolist()):
        o.put(s, r, w)
    mem = d.members(d.refs)
    for nd in d.needles + d.select_needles + [d.m255, d.super255, S.COPIED, S.COPIED_PREFIX]:
        for limit in (1, 10, 256):
            assert d.rows(mem, nd, limit) == o.find(c_prefix(nd), limit), nd[:20]
    # the 255 ceiling: the lighter of the two 255-members first, then the heavier, for the member's string and its superstring
    both = d.members([S.REF_255A, S.REF_255B])
    for nd in (d.m255, d.super255):
        assert d.rows(both, nd, 2) == [[S.REF_255A, 255, 7], [S.REF_255B, 255, 9]]
    # ties: the first `limit` copies in weight order; under the prefix needle the three prefix members come first
    ties, plus = d.members(d.ties), d.members(d.ties_plus)
    got = d.rows(ties, S.COPIED, 256)
    assert [r[0] for r in got] == list(range(S.COPY_REF0, S.COPY_REF0 + 256)) and {r[1] for r in got} == {B.T_of(S.COPIED)}
    got = d.rows(plus, S.COPIED_PREFIX, 256)
    tp = B.T_of(S.COPIED_PREFIX)
    assert got[:3] == [[S.PREFIX_REF0 + k, tp, 20 + k] for k in range(3)]
    assert [r[0] for r in got[3:]] == list(range(S.COPY_REF0, S.COPY_REF0 + 253)) and {r[1] for r in got[3:]} == {tp - 1}
    # the select's boundary: every needle has members that pass, and the count above the threshold value is below it
    fill = d.members(d.fill_refs)
    for nd in d.select_needles:
        m = Truth.matches(fill, nd)
        assert int((m >= 1).sum()) >= 2, nd
