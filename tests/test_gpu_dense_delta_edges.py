"""cluster_edges, cluster_edges(blocks=...), cluster_edges_extend and cluster_edges_between on
tests/dense_delta_case.py's map: a base image with tombstones behind its bitmaps and a delta image with dense slices of
its own.  cluster_edges_sweep_kernel (plain and blocked), cluster_edges_within_kernel and
cluster_edges_extend_sweep_kernel are further copies of the floor sweep, launched once per image by ClusterCall::sweep;
on the delta image their lists of 64 dense slices, the ranking of the L largest, the left-out slices' bitmaps read from
the delta's entries, the rank bound against the delta's n_refs and the positions from win0 run here for the first time,
and the base image is swept where its bitmaps still pass tombstoned ranks.  Every record carries its height
floor(1000 m / (T + R - m)), forest edge or not: an m that is off by one through a left-out bitmap changes a record where
every component stays the same.  The extending entry and ``between`` decide whose an edge is by absolute position
across the images, and a needle of the base image sweeps the delta image through the delta's bitmaps, which plain
``cluster`` never does: with the sides taken by image, ``between`` lets the delta's side sweep on `short` and the base's
on `long`.  `long` at floor 200 gives 26 tiles of the edge sort, at 350 one tile and 21 records.  Everything is compared
exactly with the host's truths over what is held now by the checkers of tests/test_gpu_cluster_edges.py and
tests/test_gpu_cluster_edges_extend.py; three calls give identical bytes, last_kernels() names one sweep per image, and
after the log is folded into a rebuilt base image every answer is the same bytes again.
tests/test_dense_delta_case.py proves the map's conditions on the host.

Not covered: a delta image of more than one window or with ranks of 32 768 and more (a base of millions of references);
DeviceInfo.n_bitmaps counts the base image's bitmaps only."""
import numpy as np
import pytest

import cluster_edges_truth as CE
import dense_delta_case as C
import dense_truths as DT
from test_gpu_cluster_edges import DIRECT, MERGE, SWEEP, TILE, check_blocked, check_plain
from test_gpu_cluster_edges_extend import SWEEP as EXTEND_SWEEP, check as check_extend

pytestmark = pytest.mark.gpu
LISTS = ["short", "long"]
KEYS = ["pairs", "families"]
FLOORS = range(5)                                              # indices into case.floors: 200, 350, 600, p*, p* + 1
DIRECT_ON = ("short", "long")                                  # the lists whose blocks are also scored directly (strategy 2)


@pytest.fixture(scope="module")
def case():
    c = C.gpu_case()
    c.keeping = C.keeping_truth(c.h)                           # (Split asks for three lists' pairs at every floor)
    assert len(c.floors) == len(FLOORS)
    yield c
    c.m.close()


def _images(m):
    """One sweep per image: two before the fold, one after."""
    return 2 if m.device_info()["n_pending"] else 1


def _plain(m, listed, p):
    edges = m.cluster_edges(listed, p)
    names = m.last_kernels()
    assert names.count(SWEEP) == _images(m) and DIRECT not in names, names
    assert (MERGE in names) == (len(edges) > TILE), names
    return (edges,)


def _blocked(m, listed, blocks, p, strategy):
    m.set_option("scope_strategy", strategy)
    try:
        edges = m.cluster_edges(listed, p, blocks=blocks)
        names = m.last_kernels()
    finally:
        m.set_option("scope_strategy", 0)
    if strategy == 1:
        assert names.count(SWEEP) == _images(m) and DIRECT not in names, names
    else:
        assert DIRECT in names and SWEEP not in names, names
    assert (MERGE in names) == (len(edges) > TILE), names
    return (edges,)


def _with_a_new_end(m, entry, old, new, p):
    edges = getattr(m, entry)(old, new, p)
    names = m.last_kernels()
    assert names.count(EXTEND_SWEEP) == _images(m) and SWEEP not in names, names
    assert (MERGE in names) == (len(edges) > TILE), names
    return (edges,)


def test_the_log_is_as_the_host_books_it(case):
    C.assert_log(case.m, case.h)


# ---- cluster_edges, unblocked ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", FLOORS)
@pytest.mark.parametrize("name", LISTS)
def test_cluster_edges_equals_the_truth_and_the_other_entries(case, name, k):
    m, h, truth, listed, p = case.m, case.h, case.truth(name), case.lists[name], case.floors[k]
    want = CE.records(truth, listed, p, DT.LEAST)
    edges = check_plain(m, listed, p, want)
    one = C.thrice(case, f"edges {name} {p}", lambda: _plain(m, listed, p))
    assert one[0].tobytes() == want.tobytes()
    kinds = C.kinds(h, edges)
    print(f"{name}, floor {p}: {len(edges)} records; delta-delta, base-delta, base-base {kinds}")
    assert min(kinds) >= 1, kinds
    # a listed reference that is not held -- a deleted twin, a deleted word, the deleted copy -- is nobody's end
    gone = np.array(h.twins + h.words_deleted.tolist() + [h.copy_deleted], dtype=np.uint32)
    assert np.isin(listed, gone).sum() >= 3 and not np.isin(edges[:, :2], gone).any()
    # a moved row, a node of the delta image now, has a record to a member of its base family
    rows = edges[:, :2].tolist()
    for r, x in zip(h.moved, h.moved_heads):
        family = set(h.family(x)) - {r}
        assert any((a == r and b in family) or (b == r and a in family) for a, b in rows), (r, p)
    if (name, p) == ("long", 200):
        assert len(edges) > 4 * TILE                              # several merge passes
    if (name, p) == ("long", 350):
        assert TILE < len(edges) < 2 * TILE                       # one tile and a few records


@pytest.mark.parametrize("name", LISTS)
def test_the_delta_pairs_record_is_there_at_p_star_and_gone_one_permille_above(case, name):
    """Both wide, both in the delta image: listed without the rest of their family, the record is written by the member
    at the higher delta position, in the delta's own sweep, or not at all."""
    m, h, listed = case.m, case.h, case.lists[name]
    low, high = case.pair
    alone = np.concatenate([listed[~np.isin(listed, h.delta_family)], np.array([low, high], dtype=np.uint32)])
    truth = case.truth(name + ", the pair alone")
    rows = {}
    for p in (case.p_star, case.p_star + 1):
        edges = check_plain(m, alone, p, CE.records(truth, alone, p, DT.LEAST))
        rows[p] = set(map(tuple, edges.tolist()))
    ends = (min(low, high), max(low, high))
    assert ends + (case.p_star,) in rows[case.p_star]
    assert not any(r[:2] == ends for r in rows[case.p_star + 1])
    assert rows[case.p_star + 1] == {r for r in rows[case.p_star] if r[2] > case.p_star}


# ---- cluster_edges(blocks=...) under auto, the sweep and the direct kernel ------------------------------------------------

@pytest.mark.parametrize("k", FLOORS)
@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("name", LISTS)
def test_the_blocked_records_equal_the_blocked_truth_under_every_strategy(case, name, keys, k):
    m, h, listed, p = case.m, case.h, case.lists[name], case.floors[k]
    blocks = C.keys_of(keys)(listed)
    want = CE.records(C.blocked_truth(case, name, keys), listed, p, DT.LEAST)
    strategies = (0, 1, 2) if name in DIRECT_ON else (0, 1)
    edges = check_blocked(m, listed, blocks, p, want, strategies=strategies)
    for s in strategies[1:]:
        one = C.thrice(case, f"edges within {name} {keys} {p} strategy {s}", lambda s=s: _blocked(m, listed, blocks, p, s))
        assert one[0].tobytes() == want.tobytes(), s
    # a record of a block that holds nodes of both images, one end in each
    across = C.across_in_a_block(h, edges, keys)
    print(f"{name}, {keys}, floor {p}: {len(edges)} records, {len(across)} of them base-delta")
    assert len(across) == int((C.delta_ends(h, edges) == 1).sum()) >= (len(h.moved) if keys == "families" else 1)


@pytest.mark.parametrize("name", LISTS)
def test_all_keys_equal_is_the_unblocked_call_byte_for_byte(case, name):
    m, listed = case.m, case.lists[name]
    blocks = np.full(len(listed), 7, dtype=np.uint32)
    for p in case.floors:
        DT._same_bytes(_blocked(m, listed, blocks, p, 1), _plain(m, listed, p))


# ---- cluster_edges_extend and cluster_edges_between ---------------------------------------------------------------------

def test_between_sweeps_from_the_deltas_side_on_short_and_from_the_bases_on_long(case):
    # cluster_edges_between lets the side of fewer references sweep.  Split by image that is the delta's on `short` (62
    # against about 800: needles of the delta image sweep the base through the base's bitmaps) and the base's on `long`
    # (about 800 against 3 062: needles of the base image sweep the delta through the delta's) -- whichever way round the
    # two lists are given, so the test below runs both directions of both.
    sizes = {name: tuple(len(x) for x in C.by_image(case.h, case.lists[name])) for name in LISTS}
    print(f"(in the base, in the delta) listed: {sizes}")
    assert sizes["short"][1] < sizes["short"][0] and sizes["long"][0] < sizes["long"][1]


@pytest.mark.parametrize("k", FLOORS)
@pytest.mark.parametrize("name", LISTS)
def test_extend_and_between_with_the_base_old_and_the_pending_new_and_the_other_way_round(case, name, k):
    m, h, p = case.m, case.h, case.floors[k]
    in_base, in_delta = C.by_image(h, case.lists[name])            # (the deleted, listed among the base's, are no nodes)
    for old, new, what in ((in_base, in_delta, "pending new"), (in_delta, in_base, "base new")):
        s, ext, btw = check_extend(m, case.keeping, old, new, p, least=DT.LEAST)
        for entry, want in (("cluster_edges_extend", ext), ("cluster_edges_between", btw)):
            one = C.thrice(case, f"{entry} {name} {what} {p}",
                           lambda entry=entry, old=old, new=new: _with_a_new_end(m, entry, old, new, p))
            assert one[0].tobytes() == want.tobytes(), (entry, what)
        old_old, old_new, new_new = s.figures()
        assert old_new >= 1 and new_new >= 1, (p, what, s.figures())
        assert (C.delta_ends(h, btw) == 1).all() and len(btw) == old_new   # between the images: an end in each


@pytest.mark.parametrize("at", ["200", "p_star"])
def test_a_split_by_seven_has_both_images_on_both_sides(case, at):
    """Not by image: every multiple of 7 on one side, the rest on the other, so both sides hold nodes of both images and
    the same-side rule, pos0 + r > qpos, is decided across the images.  Both ways round: with the multiples new their
    edges across the images are all old-new; with the rest new some are new-new (tests/test_dense_delta_case.py)."""
    m, h, listed = case.m, case.h, case.lists["short"]
    p = case.floors[0] if at == "200" else case.p_star
    rest, sevenths = C.by_seven(listed)
    for side in (rest, sevenths):
        assert {h.image(r) for r in side.tolist() if r in h.held} == {0, 1}
    for old, new, what in ((rest, sevenths, "sevenths new"), (sevenths, rest, "the rest new")):
        s, ext, btw = check_extend(m, case.keeping, old, new, p, least=DT.LEAST)
        for entry, want in (("cluster_edges_extend", ext), ("cluster_edges_between", btw)):
            one = C.thrice(case, f"{entry} short by seven, {what} {p}",
                           lambda entry=entry, old=old, new=new: _with_a_new_end(m, entry, old, new, p))
            assert one[0].tobytes() == want.tobytes(), (entry, what)
        assert s.figures()[1] >= 1 and (C.delta_ends(h, btw) == 1).any(), (what, s.figures())
    assert (C.delta_ends(h, s.new_new) == 1).any()                # (the rest new: an edge among the new across the images)


# ---- the exact bar, in the delta ------------------------------------------------------------------------------------------

def test_the_glued_strings_records_at_500_are_there_at_floor_500_and_not_at_501(case):
    m, h, g = case.m, case.h, case.h.handmade
    listed, truth = case.lists["handmade"], C.keeping_truth(case.h)
    copies = len(g.held_copies)
    glued = np.array([g.glued], dtype=np.uint32)
    assert copies == C.COPIES - 1 == 69
    for p in (500, 501):
        edges = check_plain(m, listed, p, CE.records(truth, listed, p))
        high, low = edges[edges[:, 2] == 1000], edges[edges[:, 2] == 500]
        assert len(high) == copies * (copies - 1) // 2 and len(low) == (copies if p == 500 else 0), p
        assert len(edges) == len(high) + len(low) and h.copy_deleted not in edges[:, :2]
        assert (low[:, :2] == g.glued).any(axis=1).all() and g.glued not in high[:, :2]
        # the copies against the glued string: the records at 500 and nothing else, whichever side sweeps
        s, ext, btw = check_extend(m, truth, g.held_copies, glued, p)
        assert btw.tobytes() == low.tobytes() and ext.tobytes() == low.tobytes(), p
        assert m.cluster_edges_between(glued, g.held_copies, p).tobytes() == low.tobytes(), p
        # the glued string old and the copies new: every edge has a new end
        s, ext, btw = check_extend(m, truth, glued, g.held_copies, p)
        assert btw.tobytes() == low.tobytes() and ext.tobytes() == edges.tobytes(), p
        for rows in (ext, btw):
            assert h.copy_deleted not in rows[:, :2]


# ---- fold invariance (the last test: it changes the map) -----------------------------------------------------------------

def test_after_the_fold_one_image_answers_every_call_with_the_same_bytes(case):
    C.fold_and_compare(case, at_least=98)
