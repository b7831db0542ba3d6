"""tests/boundary_case.py proven without a GPU: its own conditions, and what the oracle answers for its needles by
construction -- the facts tests/test_gpu_find_boundaries.py leans on when it compares the kernels with that oracle."""
import numpy as np
import pytest

import boundary_case as B


@pytest.fixture(scope="module")
def case():
    return B.case()                                             # (runs conditions())


def test_conditions_hold(case):
    B.conditions(case)
    assert len(case.needles) == len(B.CLASSES) + len(B.LENGTHS) == len(case.T)


@pytest.mark.parametrize("which", ["a", "b"])
def test_every_needle_finds_its_twin_on_the_counter_ceiling_and_its_near_twin_one_below(case, which):
    """Rows in result order: the twin (matches == T: the counter sits on `need` and, for T = 15 and T = 127, on the
    ceiling of its width), the superstring (T as well: its set contains the needle's), then the first row below T --
    T - 1 matches, the near twin's."""
    o = case.oracle(which)
    for t, i in case.classes.items():
        rows = o.find(case.needles[i], 10)
        twin, near, sup = case.ref_of(t, 0), case.ref_of(t, 1), case.ref_of(t, 2)
        assert rows[0][:2] == [twin, t], (t, rows[:3])
        full = [r for r in rows if r[1] == t]
        assert sorted(r[0] for r in full) == sorted([twin, sup]), (t, rows[:4])
        if t >= 2:
            below = rows[len(full)]
            assert below[1] == t - 1, (t, rows[:4])
            if t >= 3:                                          # (T = 2: thousands of strings share one trigram with b"a")
                assert near in [r[0] for r in rows if r[1] == t - 1], (t, rows[:6])
        if t >= 16:                                             # the 15-trigram prefix: 15 matches from a 4-bit window
            p = case.ref_of(t, 3)
            hit = [r for r in o.find(case.needles[i], 64) if r[0] == p]
            assert hit and hit[0][1] == 15 and hit[0][2] == 1, (t, hit)
    for j in range(len(B.LENGTHS)):
        i = case.n_class + j
        rows = o.find(case.needles[i], 10)
        assert rows[0][:2] == [case.ref_at(i, 0), case.T[i]], (j, rows[:2])


@pytest.mark.parametrize("which", ["a", "b"])
def test_some_needles_need_more_than_one_pass_and_the_pass_edge_lies_in_a_tie(case, which):
    """More than 1 024 rows (the needle-major pass of a needle of up to 127 trigrams) and more than 256 (a longer
    needle's): the rows on either side of the pass edge tie on (matches, weight), so only the floor key's rank
    separates the passes."""
    o = case.oracle(which)
    packed, off = case.pack(case.needles)
    got = o.batch(packed, off, limit=65535)
    counts = got["counts"]
    assert (counts > 1024).sum() >= 6 and (counts == 65535).any()    # (... and some fill the largest limit there is)
    for t, edge in ((15, 1024), (16, 1024), (64, 1024), (65, 1024), (127, 1024), (128, 256), (257, 256), (1200, 256)):
        rows = got["rows"][case.classes[t]]
        assert counts[case.classes[t]] > 2 * edge
        assert rows[edge - 1][1] == rows[edge][1] and rows[edge - 1][2] == rows[edge][2], (t, rows[edge - 1], rows[edge])


def test_the_maps_differ_in_one_weight_swap(case):
    diff = np.nonzero(case.weights_a != case.weights_b)[0]
    assert sorted(case.refs[diff].tolist()) == [case.last_filler, B.X_REF]
