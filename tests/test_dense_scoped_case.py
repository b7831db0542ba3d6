"""tests/dense_truths.py proven without a GPU: the conditions that tests/test_gpu_dense_cluster_within.py and
tests/test_gpu_dense_scoped_finds.py lean on when they put cluster_within and the scoped floor finds on
tests/dense_case.py's map -- the block keys and the family pair, the within-block edges of both lists at the five floors,
the six scopes and what they take from a family head's rows -- and the two scoped truths anchored once on the
ScopedTruth classes of tests/scope_above_truth.py and tests/scope_similar_truth.py.  The relations are asserted, not
figures: a re-seeded generator that empties a case fails here."""
import numpy as np
import pytest

import dense_case as D
import dense_truths as DT
import scope_above_truth
import scope_similar_truth
from cluster_truth import Truth
from cluster_within_truth import WithinTruth, telling

ABOVE_BARS = ((1, 0), (3, 0), (0, 200), (0, 600), (0, 1000))   # tests/test_gpu_dense_floor_sweeps.py's
WIDE_SCOPES = ("short", "nofirst", "half", "upper", "nolow")
MEMBER_CAP = 57344                                             # find_kernels.h: kScopeMaxMembers


@pytest.fixture(scope="module")
def case():
    h = D.host()
    c = DT.inputs(h)
    c.h = h
    c.within = WithinTruth(h.held)
    c.above = DT.ScopedAbove(DT.ArrayAbove(h.strings, h.refs, h.weights))
    c.similar = DT.ScopedSimilar(DT.FlooredSimilar(h.strings, h.refs, h.weights, DT.LEAST))
    return c


def _edges(truth, listed, blocks, p):
    return DT.within_edges(truth, listed, blocks, p)


def test_the_pair_lies_in_the_upper_half_of_window_0_is_wide_and_the_keys_split_it_one_way_only(case):
    h, (low, high) = case.h, case.pair
    assert h.loc[low][0] == h.loc[high][0] == 0 and D.HALF <= h.loc[low][1] < h.loc[high][1]
    assert h.T(low) > 255 and h.T(high) > 255
    assert case.p_star == h.permille(low, high) and 350 <= case.p_star < 999
    assert not {case.p_star, case.p_star + 1} & set(DT.FIXED_FLOORS)
    assert DT.key_pairs([low])[0] == DT.key_pairs([high])[0]
    assert DT.key_parity([low])[0] != DT.key_parity([high])[0]
    # a family's two identical strings share a key under (ref // 2) % 2: each family keeps its J = 1 edge
    assert all(DT.key_pairs([x])[0] == DT.key_pairs([x + 1])[0] and h.held[x] == h.held[x + 1] for x in h.heads)
    # the second set of keys: a key a family, three for the words, none shared between the two
    fam = DT.key_families(case.family)
    assert [len(set(fam[i:i + D.MEMBERS].tolist())) for i in range(0, len(fam), D.MEMBERS)] == [1] * len(h.heads)
    assert len(set(fam.tolist())) == len(h.heads)
    assert not set(fam.tolist()) & {0, 1, 2}
    for name in ("short", "long"):                                # (both lists' words take all three)
        assert set(DT.key_families(case.lists[name][:-len(fam)]).tolist()) == {0, 1, 2}


@pytest.mark.parametrize("name", ["short", "long"])
def test_every_floor_tells_blocked_from_plain_clustering_and_the_pair_is_an_edge_up_to_p_star(case, name):
    h, truth, listed = case.h, case.within, case.lists[name]
    blocks = DT.key_pairs(listed)
    pair = (min(case.pair), max(case.pair))
    family = set(case.family.tolist())
    n_edges = {}
    for p in case.floors:
        _, n_clusters, n_edges[p], blocked = truth.cluster_within(listed, blocks, p, DT.LEAST)
        _, plain_clusters, plain_edges, plain = truth.cluster(listed, p, DT.LEAST)
        print(f"{name}, floor {p}: within {n_edges[p]} edges, {n_clusters} clusters; plain {plain_edges}, {plain_clusters}")
        assert 0 < n_edges[p] < plain_edges and n_clusters > plain_clusters, p
        assert telling(blocked, plain), p
        within = _edges(truth, listed, blocks, p)
        assert len(within) == n_edges[p]
        assert (pair in within) == (p <= case.p_star), p
        # under ref % 2 the pair is an edge at no floor, though the floor passes up to p*
        assert pair not in _edges(truth, listed, DT.key_parity(listed), p), p
        assert (pair in _edges(truth, listed, None, p)) == (p <= case.p_star), p
        # each family under a key of its own keeps every edge inside a family (from 350 on there are no others, so
        # those floors tell nothing there); the words' three keys cut edges at the lowest floor
        _, _, fam_edges, fam_blocked = truth.cluster_within(listed, DT.key_families(listed), p, DT.LEAST)
        assert 0 < fam_edges <= plain_edges, p
        if p == DT.LEAST:
            assert fam_edges < plain_edges and telling(fam_blocked, plain)
        if name == "short":
            # family edges within a block that cross the two windows: the workgroup of window 0 finds them
            across = [e for e in within if e[0] in family and {h.loc[e[0]][0], h.loc[e[1]][0]} == {0, 1}]
            assert len(across) >= 1, p
    # the edge count falls with the floor, and by exactly the pair from p* to p* + 1
    assert [n_edges[p] for p in case.floors] == sorted((n_edges[p] for p in case.floors), reverse=True)
    assert n_edges[case.p_star] == n_edges[case.p_star + 1] + 1 and n_edges[200] > n_edges[600]


def test_the_scopes_sizes_their_wide_members_and_which_has_a_direct_form(case):
    h, scopes = case.h, case.scopes
    n_heads = len(h.heads)
    assert len(scopes["short"]) == len(case.lists["short"]) and len(scopes["nofirst"]) == len(scopes["short"]) - 2 * n_heads
    assert len(scopes["nolow"]) == len(scopes["short"]) - 1 and case.pair[0] not in scopes["nolow"].tolist()
    assert case.pair[1] in scopes["nolow"].tolist()
    for name in WIDE_SCOPES:                                      # a member of more than 255 trigrams: no direct form
        assert DT.wide_members(h, scopes[name]) >= 1, name
    # the whole-map scopes are under the member cap: only their wide members keep the direct form from them
    assert len(scopes["short"]) < len(scopes["half"]) < MEMBER_CAP and len(scopes["upper"]) < MEMBER_CAP
    assert len(scopes["half"]) > len(h.refs) // 3 and len(scopes["upper"]) > len(h.refs) // 3
    assert DT.wide_members(h, scopes["words97"]) == 0 and max(h.T(int(r)) for r in scopes["words97"]) <= 255
    assert not set(scopes["words97"].tolist()) & set(case.family.tolist())
    # `upper` holds nothing of the first half window
    assert all(h.loc[int(r)][0] == 1 or h.loc[int(r)][1] >= D.HALF for r in scopes["upper"])
    assert {h.loc[int(r)][0] for r in scopes["upper"]} == {0, 1}
    print({k: (len(v), DT.wide_members(h, v)) for k, v in scopes.items()})


def test_every_scope_takes_rows_from_a_head_and_leaves_it_some(case):
    """What can be asserted for every head: at the two match bars each of the six scopes keeps some of a head's rows and
    drops some; at every bar `nofirst` and `half` do (each family has members under both keys), the scopes that hold
    the families keep a row, and no scope has a row the whole map has not.  `short` cannot drop a row at the permille
    bars -- a head's rows there are its own family, all of it listed -- and `words97` holds none of them."""
    h, above, scopes = case.h, case.above, case.scopes
    for x in h.heads:
        s = h.held[x]
        for mm, mp in ABOVE_BARS:
            whole = above.rows(s, None, mm, mp)
            assert len(whole) > 0
            count = {}
            for name, scope in scopes.items():
                rows = above.rows(s, scope, mm, mp)
                count[name] = len(rows)
                assert set(rows[:, 0].tolist()) <= set(whole[:, 0].tolist())
            strictly = list(scopes) if mp == 0 else ["nofirst", "half"] + (["upper"] if mp < 1000 else [])
            for name in strictly:
                assert 0 < count[name] < len(whole), (x, mm, mp, name, count[name], len(whole))
            for name in ("short", "nofirst", "half", "nolow"):
                assert count[name] > 0, (x, mm, mp, name)
            # `nofirst` removes the head's two identical strings, rows of T matches at every bar
            full = set(whole[whole[:, 1] == h.T(x)][:, 0].tolist())
            assert {x, x + 1} <= full and not {x, x + 1} & set(above.rows(s, scopes["nofirst"], mm, mp)[:, 0].tolist())
        # ... which are its best two rows by similarity, J = 1000: the list of the scoped find fills from what remains
        best = case.similar.rows(s, None, 2, 600)
        assert sorted(r[0] for r in best) == [x, x + 1] and all(r[1] == r[3] == h.T(x) for r in best)
        left = case.similar.rows(s, scopes["nofirst"], 10, DT.LEAST)
        assert 1 <= len(left) < 10 and all(r[1] < r[3] or r[1] < h.T(x) for r in left)


def test_nolow_removes_exactly_the_pairs_lower_member_from_the_higher_members_rows(case):
    h, above, (low, high) = case.h, case.above, case.pair
    s = h.held[high]
    bar = DT.above_truth.bar(h.T(high), 0, 600)
    whole = above.rows(s, None, 0, 600)
    assert low in whole[:, 0].tolist() and int(whole[whole[:, 0] == low][0, 1]) >= bar
    short = above.rows(s, case.scopes["short"], 0, 600)
    nolow = above.rows(s, case.scopes["nolow"], 0, 600)
    assert low in short[:, 0].tolist()
    assert nolow.tolist() == [r for r in short.tolist() if r[0] != low] and len(nolow) == len(short) - 1


def test_the_scoped_truths_equal_the_scoped_truth_classes_on_a_one_window_prefix(case):
    """Two needles -- a wide family head and a word -- over the first 15 000 words and two families under their own
    weights (one window), two scopes and NO_SCOPE, every bar, limits 1, 10 and 1000 at the three fixed floors."""
    h = case.h
    refs = np.concatenate([h.refs[:15000], case.family[-2 * D.MEMBERS:]])
    where = {int(r): i for i, r in enumerate(h.refs)}
    strings = [h.held[int(r)] for r in refs]
    weights = [int(h.weights[where[int(r)]]) for r in refs]
    assert max(w for w, _ in D.locate(refs, weights).values()) == 0
    t_above, t_similar = scope_above_truth.ScopedTruth(), scope_similar_truth.ScopedTruth()
    for s, r, w in zip(strings, refs.tolist(), weights):
        t_above.put(s, r, w)
        t_similar.put(s, r, w)
    above = DT.ScopedAbove(DT.ArrayAbove(strings, refs, weights))
    similar = DT.ScopedSimilar(DT.FlooredSimilar(strings, refs, weights, DT.LEAST))
    # scopes that name references outside the prefix too: the live set is what the map holds
    scopes = {"half": case.scopes["half"], "nofirst": case.scopes["nofirst"], "whole": None}
    needles = [h.held[h.heads[-1]], h.strings[7]]
    assert h.T(h.heads[-1]) > 255
    seen = 0
    for s in needles:
        for name, scope in scopes.items():
            for mm, mp in ABOVE_BARS:
                want = t_above.rows(s, scope, mm, mp)
                assert above.rows(s, scope, mm, mp).tolist() == want, (name, mm, mp)
                seen += len(want)
            for limit in (1, 10, 1000):
                for p in DT.FIXED_FLOORS:
                    want = t_similar.rows(s, scope, limit, p)
                    assert similar.rows(s, scope, limit, p) == want, (name, limit, p)
                    seen += len(want)
    assert seen > 1000
    # filtering first matters: under `nofirst` the head's row at limit 1 is one the whole-map find cuts off
    head = needles[0]
    first = similar.rows(head, None, 1, 200)
    assert similar.rows(head, scopes["nofirst"], 1, 200) not in ([], first)
    assert first[0][0] not in case.scopes["nofirst"].tolist()


def test_the_blocked_truth_with_all_keys_equal_is_the_plain_truth(case):
    listed = case.lists["short"]
    for p in (200, case.p_star):
        got = case.within.cluster_within(listed, np.zeros(len(listed), dtype=np.uint32), p, DT.LEAST)
        want = Truth.cluster(case.within, listed, p, DT.LEAST)
        assert np.array_equal(got[0], want[0]) and got[1:3] == want[1:3]


def test_the_hand_made_case_has_its_seventy_edges_at_500_only_and_none_across_two_keys():
    c = DT.handmade()                                             # (asserts the bar, the six dense slices and the position)
    truth = WithinTruth(c.held)
    pairs = 70 * 69 // 2
    one_key, own_key = np.zeros(len(c.refs), dtype=np.uint32), (c.refs == 1).astype(np.uint32)
    for p, blocks, edges, clusters in ((500, one_key, pairs + 70, 3), (501, one_key, pairs, 4), (500, own_key, pairs, 4),
                                       (501, own_key, pairs, 4)):
        _, n_clusters, n_edges, _ = truth.cluster_within(c.refs, blocks, p)
        assert (n_clusters, n_edges) == (clusters, edges), p
