"""tests/dense_delta_case.py proven without a GPU: the conditions tests/test_gpu_dense_delta_*.py lean on when they run
every sweep on a base image with tombstones behind its bitmaps and a delta image with dense slices of its own -- per
image, that the needles have more dense slices than a sweep lists and that the bars put L on all three sides of the list
of 64; that the truth has edges within the delta, from a wide delta node into the upper half of the base's window 0 and
into its window 1; that each deleted twin would be an edge and a row if it were still held, at the high floors through the
left-out bitmaps alone; and that a moved row lies elsewhere in the delta than in the base.  For the edge lists and the
newer blocked entries (tests/test_gpu_dense_delta_edges.py, tests/test_gpu_dense_delta_blocked.py): that the records of
`long` cross the edge sort's tile at floors 200 and 350 and are of every kind (within the delta, across the images,
within the base) at every floor; that under both key functions an edge across the images lies inside one block; that the
split by image has edges across and among the new either way round and makes the delta's side the smaller on `short` and
the base's on `long`; that the split by seven has both images on both sides and same-side edges across them; and that the
cores within blocks have borders and, at (p*, 5) under the family keys, a core.  The relations are asserted, not
figures (each is printed beside its relation): a re-seeded generator that empties a case fails here, and the remedy is
another seed.

Not covered by the map: a delta image of more than one window or with ranks of 32 768 and more (a base of millions of
references), and the delta's bitmaps as the device counts them (DeviceInfo.n_bitmaps is the base image's)."""
import numpy as np
import pytest

import cluster_edges_truth as CE
import dense_case as D
import dense_delta_case as C
import dense_truths as DT
from cluster_cores_truth import CORE
from cluster_cores_within_truth import CoresWithinEdges
from cluster_edges_extend_truth import Split
from cluster_truth import Truth


TILE = 4096                                                    # the edge sort's tile (cluster.h: kClusterEdgesTile)
LISTS = ("short", "long")
KEYS = ("pairs", "families")
MIN_DEGREES = (0, 2, 3, 5)                                     # tests/test_gpu_dense_delta_blocked.py's


@pytest.fixture(scope="module")
def case():
    h = C.host()
    c = C.inputs(h)
    c.h, c.truth = h, C.truths(h)
    return c


def _edges(h, listed, p):
    """The truth's edges of a list at floor p as (the end at the lower position, the end at the higher)."""
    nodes, a, b, m = h.truth.pairs(listed, DT.LEAST)
    edge = 1000 * m >= p * (h.truth.R[a] + h.truth.R[b] - m)
    pairs = zip(h.truth.refs[a[edge]].tolist(), h.truth.refs[b[edge]].tolist())
    return [(x, y) if h.position(x) < h.position(y) else (y, x) for x, y in pairs]


def test_the_host_books_the_log_as_the_map_does(case):
    h, base = case.h, case.h.base
    assert base is D.host() and h.base_windows == 2
    gone = set(h.twins) | set(h.words_deleted.tolist()) | {h.copy_deleted, C.GONE_REF}
    assert not gone & set(h.held) and set(h.moved) <= set(h.held)
    assert set(h.held) == (set(base.held) | set(h.pending)) - (gone - set(h.moved))
    assert h.tombstones == h.twins + h.words_deleted.tolist() + h.moved and len(h.words_deleted) >= 300
    assert len(h.pending) + len(h.tombstones) <= C.LOG_BUDGET
    assert all(h.held[r] == base.held[r] for r in base.held if r in h.held and r not in h.moved)
    assert all(h.held[r] == base.held[x] + b" moved" != base.held[r] for r, x in zip(h.moved, h.moved_heads))
    # the delta image is the pending puts alone, one window; the base image keeps every rank it was built with
    assert set(h.delta.loc) == set(h.pending) and all(w == 0 for w, _ in h.delta.loc.values())
    assert sorted(r for _, r in h.delta.loc.values()) == list(range(len(h.pending)))
    assert all(r in base.loc for r in h.tombstones)
    assert int(h.delta.postings.sum()) == sum(h.T(r) for r in h.pending)
    print(f"{len(h.pending)} pending, {len(h.tombstones)} tombstones; dense (code, window) pairs: base "
          f"{base.n_dense_pairs()}, delta {int(((h.delta.postings + 7) // 8 * 8 >= D.DENSE_MIN).sum())}")


def test_every_delta_head_has_more_dense_slices_than_the_list_holds_in_both_images(case):
    h = case.h
    assert len(h.delta_heads) == C.FAMILIES_EACH * len(D.FAMILY_WORDS)
    print([(h.T(x), h.dense(x, 1), h.dense(x, 0, 0), h.dense(x, 0, 1)) for x in h.delta_heads])
    assert all(h.dense(x, 1) > D.MAX_DENSE for x in h.delta_heads)             # in the delta's one window
    assert all(h.dense(x, 0, 0) > D.MAX_DENSE for x in h.delta_heads)          # and in the base's window 0, which they sweep
    narrow = [x for x in h.delta_heads if h.T(x) <= 255]
    wide = [x for x in h.delta_heads if h.T(x) > 255]
    assert len(narrow) >= 2 and len(wide) >= 3                    # both counter widths leave slices out
    # the moved rows: nodes of the delta whose base neighbours stand behind the base's bitmaps, one of each width
    assert sorted(h.T(r) > 255 for r in h.moved) == [False, True]
    assert all(h.image(r) == 1 and h.dense(r, 0, 0) > D.MAX_DENSE for r in h.moved)


def test_the_bars_put_L_on_all_three_sides_of_the_list_of_64_in_each_image(case):
    h = case.h
    delta_nodes = [int(r) for r in case.lists["long"] if int(r) in h.pending] + [h.handmade.glued]
    # the delta's nodes over the delta's one window, and over the base's two, which they sweep as well (the base's small
    # window 1 is where all of a delta needle's dense slices are left out)
    for image, windows, needles in ((1, (0,), delta_nodes), (0, (0, 1), h.delta_heads + h.moved)):
        sides = {"below": 0, "cap": 0, "all": 0}
        for x in needles:
            for window in windows:
                nd = h.dense(x, image, window)
                for p in case.floors:
                    t = DT.floor_bar(h.T(x), p)
                    sides["below"] += nd > D.MAX_DENSE and 1 < t and t - 1 < D.MAX_DENSE   # only the largest are left out
                    sides["cap"] += nd > D.MAX_DENSE < t - 1                               # L is capped at the 64 recorded
                    sides["all"] += 1 <= nd <= min(t - 1, D.MAX_DENSE)                     # nd <= t - 1: all are left out
        print(("base", "delta")[image], sides)
        assert min(sides.values()) >= 3, (image, sides)


def test_the_pair_of_p_star_is_a_wide_pair_of_the_delta(case):
    h = case.h
    low, high = case.pair
    assert h.image(low) == h.image(high) == 1 and h.position(low) < h.position(high)
    assert h.T(low) > 255 and h.T(high) > 255
    assert 350 <= case.p_star < 999 and not {case.p_star, case.p_star + 1} & set(DT.FIXED_FLOORS), case.p_star
    for name in ("short", "long"):
        assert (low, high) in _edges(h, case.lists[name], case.p_star)
        assert (low, high) not in _edges(h, case.lists[name], case.p_star + 1)


def test_edges_within_the_delta_and_from_a_wide_delta_node_into_both_base_windows(case):
    h = case.h
    for name in ("short", "long"):
        edges = _edges(h, case.lists[name], case.floors[0])
        kinds = {"delta-delta": 0, "base-delta": 0, "base-base": 0}
        upper = window1 = False
        for lo, hi in edges:
            images = (h.image(lo), h.image(hi))
            kinds[{(1, 1): "delta-delta", (0, 1): "base-delta", (0, 0): "base-base"}[images]] += 1
            if images == (0, 1):                                   # found from the delta node, through the base's bitmaps
                _, w, r = h.at(lo)
                upper |= h.T(hi) > 255 and w == 0 and r >= D.HALF
                window1 |= w == 1
        print(name, kinds)
        assert min(kinds.values()) >= 1, kinds
        assert upper, "no wide delta node has a base neighbour at a rank >= 32768 of window 0"
        assert window1, "no delta node has a neighbour in the base's window 1"
        # the moved rows keep their families: at every floor an edge to a member that is still in the base image
        for p in case.floors:
            at_p = set(_edges(h, case.lists[name], p))
            assert all(any((lo, r) in at_p for lo in h.family(x)) for r, x in zip(h.moved, h.moved_heads)), p
    # among the pending phrases alone the delta has edges at every fixed floor
    assert all(sum(h.image(lo) == 1 for lo, _ in _edges(h, case.lists["long"], p)) > 100 for p in DT.FIXED_FLOORS)


def test_each_deleted_twin_would_be_an_edge_and_a_row_at_every_floor_if_it_were_still_held(case):
    h, base = case.h, case.h.base
    still = dict(h.held)
    still.update({r: base.held[r] for r in h.twins})
    truth = Truth(still)
    listed = case.lists["short"]
    assert set(h.twins) <= set(listed.tolist())
    refs = np.array(sorted(still), dtype=np.uint32)
    weight_of = dict(h.weight_of)
    weight_of.update({r: int(base.weights[np.searchsorted(base.refs, r)]) for r in h.twins})
    above = DT.ArrayAbove([still[int(r)] for r in refs], refs, [weight_of[int(r)] for r in refs])
    now = DT.ArrayAbove(h.strings, h.refs, h.weights)
    through_bitmaps_alone = 0
    for x, twin in zip(h.twin_heads, h.twins):
        assert h.image(x) == 0 and base.loc[twin][0] == 0
        for p in case.floors:
            labels, _, _, of_ref = truth.cluster(listed, p, DT.LEAST)
            assert of_ref[twin] == of_ref[x], (x, p)               # held, the twin is the head's neighbour ...
            _, _, _, of_now = h.truth.cluster(listed, p, DT.LEAST)
            assert twin not in of_now                              # ... deleted, it is no node
            held_rows = above.rows(base.held[x], 0, p)[:, 0].tolist()
            assert twin in held_rows and x in held_rows and twin not in now.rows(base.held[x], 0, p)[:, 0].tolist()
            # its T matches are the head's own: with L slices left out it is counted T - L times, and below the bar
            # where that is less than t -- there the tombstone is all that keeps a rank the bitmaps pass from the rows
            T, nd = h.T(x), base.dense_padded(x, 0)
            t = DT.floor_bar(T, p)
            L = min(t - 1, nd, D.MAX_DENSE)
            through_bitmaps_alone += T - L < t
    assert through_bitmaps_alone >= 2 and sorted(h.T(x) > 255 for x in h.twin_heads) == [False, True]
    # the plain words deleted are held no more; a few of them are listed
    assert len(set(h.words_deleted.tolist()) & set(case.lists["short"].tolist())) >= 1


def test_a_moved_row_lies_elsewhere_in_the_delta_than_in_the_base(case):
    h = case.h
    for r in h.moved:
        (bw, br), (dw, dr) = h.base.loc[r], h.delta.loc[r]
        assert br != dr and h.at(r) == (1, dw, dr) and h.position(r) >= 2 * D.WINDOW_RANKS
        assert h.position(r) != bw * D.WINDOW_RANKS + br
    # the reference put and deleted again is nowhere; the deleted copy is of the delta alone
    assert C.GONE_REF not in h.delta.loc and C.GONE_REF not in h.base.loc and h.copy_deleted not in h.delta.loc


def test_the_exact_bar_in_the_delta(case):
    """The glued string's six dense slices in the delta are the word's; at floor 500 its bar is 6, five are left out, and a
    copy shares exactly those six: 69 held copies are its edges at 500 and none is at 501."""
    h, g = case.h, case.h.handmade
    assert len(g.held_copies) == C.COPIES - 1 and h.copy_deleted in g.listed.tolist()
    post = h.delta.postings[0]
    word_codes, glued_codes = h.codes(int(g.copies[0])), h.codes(g.glued)
    dense = (post[glued_codes] + 7) // 8 * 8 >= D.DENSE_MIN
    assert sorted(glued_codes[dense].tolist()) == sorted(word_codes.tolist()) and (post[word_codes] >= C.COPIES).all()
    assert DT.floor_bar(12, 500) == 6 and DT.floor_bar(12, 501) == 7
    for p, n in ((500, C.COPIES - 1), (501, 0)):
        mine = [e for e in _edges(h, g.listed, p) if g.glued in e]
        assert len(mine) == n and all(hi == g.glued for _, hi in mine), p


# ---- what tests/test_gpu_dense_delta_edges.py and tests/test_gpu_dense_delta_blocked.py lean on ---------------------------

def _records(case, name, p):
    return CE.records(case.truth(name), case.lists[name], p, DT.LEAST)


def test_the_edge_records_cross_the_sorts_tile_and_are_of_every_kind_at_every_floor(case):
    count = {}
    for name in LISTS:
        for p in case.floors:
            rows = _records(case, name, p)
            kinds = C.kinds(case.h, rows)
            count[name, p] = len(rows)
            print(f"{name}, floor {p}: {len(rows)} records; delta-delta, base-delta, base-base {kinds}")
            assert min(kinds) >= 1 and sum(kinds) == len(rows), (name, p, kinds)
    assert count["long", 200] > 4 * TILE                          # several merge passes of the sort
    assert TILE < count["long", 350] < 2 * TILE                   # one tile and a few records: the first merge pass
    assert all(count["short", p] < TILE for p in case.floors)     # and no merge at all


@pytest.mark.parametrize("keys", KEYS)
def test_every_list_and_floor_has_a_base_delta_edge_inside_one_block(case, keys):
    h = case.h
    for name in LISTS:
        blocks = C.keys_of(keys)(case.lists[name])
        key_of = dict(zip(case.lists[name].tolist(), blocks.tolist()))
        for p in case.floors:
            rows = _records(case, name, p)
            within = rows[[key_of[a] == key_of[b] for a, b, _ in rows.tolist()]]
            across = C.across_in_a_block(h, rows, keys)
            print(f"{name}, {keys}, floor {p}: {len(within)} within-block edges, {len(across)} of them base-delta")
            assert len(across) >= (len(h.moved) if keys == "families" else 1), (name, p)
    # under `families` a moved row's block is its base family's: a block of both images
    moved_keys = C.key_families(np.array(h.moved, dtype=np.uint32))
    assert moved_keys.tolist() == C.key_families(np.array(h.moved_heads, dtype=np.uint32)).tolist()


def test_the_split_by_image_has_edges_across_and_among_the_new_either_way_round(case):
    h, truth = case.h, C.keeping_truth(case.h)
    sizes = {}
    for name in LISTS:
        in_base, in_delta = C.by_image(h, case.lists[name])
        sizes[name] = (len(in_base), len(in_delta))
        assert set(h.moved) <= set(in_delta.tolist()) and set(h.twins) <= set(in_base.tolist())
        for p in case.floors:
            for old, new, what in ((in_base, in_delta, "pending new"), (in_delta, in_base, "base new")):
                figures = Split(truth, old, new, p, DT.LEAST).check_itself().figures()
                print(f"{name}, floor {p}, {what}: old-old, old-new, new-new {figures}")
                assert figures[1] >= 1 and figures[2] >= 1, (name, p, what)
    # cluster_edges_between lets the side of fewer references sweep: the delta's on `short`, the base's on `long`
    print(f"(in the base, in the delta) listed: {sizes}")
    assert sizes["short"][1] < sizes["short"][0] and sizes["long"][0] < sizes["long"][1]


def test_the_split_by_seven_has_both_images_on_both_sides_and_same_side_edges_across_them(case):
    h, listed = case.h, case.lists["short"]
    old, new = C.by_seven(listed)
    for side in (old, new):
        assert {h.image(r) for r in side.tolist() if r in h.held} == {0, 1}
    for p in (case.floors[0], case.p_star):
        rows = _records(case, "short", p)
        across = rows[C.delta_ends(h, rows) == 1]
        sides = (across[:, :2] % 7 == 0).sum(axis=1)
        print(f"short by seven, floor {p}: base-delta edges old-old, old-new, new-new "
              f"{[int((sides == k).sum()) for k in (0, 1, 2)]}")
        assert (sides != 1).sum() >= 1, p                          # a same-side edge whose ends lie in different images
        assert (sides == 1).sum() >= 1, p                          # and one across the sides as well
        # the GPU file runs the split with the sides exchanged too: the same-side edges between two references that are
        # no multiples of 7 are then edges among the new, which cluster_edges_extend's needles find from the higher end
        assert (sides == 0).sum() >= 1, p


@pytest.mark.parametrize("keys", KEYS)
def test_cores_within_blocks_have_borders_and_the_core_tree_a_core_at_p_star(case, keys):
    h = case.h
    for name in LISTS:
        listed = case.lists[name]
        blocks = C.keys_of(keys)(listed)
        borders = 0
        for p in case.floors:
            e = CoresWithinEdges(case.truth(name), listed, blocks, p, DT.LEAST)
            for k in MIN_DEGREES:
                t = e.cores(k)
                borders += t.n_borders
                if (p, k) == (case.p_star, 5):
                    cores = int((t.kinds == CORE).sum())
                    print(f"{name}, {keys}, floor {p}, min_degree {k}: {cores} cores, {t.n_core_edges} core edges")
                    assert cores >= 1 or keys != "families"       # the core tree's case (p*, 5) has a core height
        print(f"{name}, {keys}: {borders} borders over every floor and min_degree")
        assert borders >= 1
