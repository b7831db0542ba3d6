"""tests/dense_tree_case.py proven without a GPU: the conditions tests/test_gpu_dense_cluster_trees.py leans on when it
puts cluster_tree, cluster_core_tree and cluster_tree_within on the dense-slice map with chain families -- that the
trees' later Boruvka rounds pick records whose higher end has slices left out, under both counter widths, across the
windows and in the upper half window; that an edge inside a component stands behind a bitmap probe; what the three sets
of block keys do to a chain; what the core tree's cases hold; and the hand-made case's figures.  The relations are
asserted, not figures: a re-seeded generator that empties a case fails here, and the remedy is another seed."""
import numpy as np
import pytest

import cluster_tree_truth as TT
import dense_case as D
import dense_tree_case as C
import dense_truths as DT
from cluster_core_tree_truth import NO_CORE, CoreTreeTruth, edges as core_edges
from cluster_tree_within_truth import blocked
from cluster_truth import Truth

BUCKETS = 32                                                   # cluster.h: kCoreBuckets


@pytest.fixture(scope="module")
def case():
    h = C.host()
    c = C.inputs(h)
    c.h, c.truth, c._rounds = h, C.truths(h, c), {}

    def rounds(name, p):
        if (name, p) not in c._rounds:
            c._rounds[name, p] = TT.boruvka_rounds(c.truth(name), c.lists[name], p, DT.LEAST)
        return c._rounds[name, p]

    c.rounds = rounds
    return c


def _ends(h, a, b):
    """(the end at the lower position, the end at the higher): an edge is found by the sweep of its higher end."""
    return (a, b) if C.position(h, a) < C.position(h, b) else (b, a)


def test_the_map_is_the_dense_map_with_sixty_chain_members_behind_it(case):
    h, base = case.h, D.host()
    assert len(h.chains) == len(D.FAMILY_WORDS) and len(h.members) == 60 and int(h.members[0]) == C.CHAIN_REF0
    assert all(h.held[r] == s for r, s in base.held.items()) and len(h.held) == len(base.held) + 60
    assert np.array_equal(h.weights[:len(base.weights)], base.weights)
    for name in ("short", "long"):
        assert np.array_equal(case.lists[name][:-60], DT.inputs(base).lists[name])
        assert np.array_equal(case.lists[name][-60:], h.members)
    # the pair of dense_truths is where it was: both wide, in the upper half of window 0
    low, high = case.pair
    assert h.loc[low][0] == h.loc[high][0] == 0 and D.HALF <= h.loc[low][1] < h.loc[high][1]
    assert h.T(low) > 255 and h.T(high) > 255 and case.p_star == DT.inputs(base).p_star
    assert 350 <= case.p_star < 999 and not {case.p_star, case.p_star + 1} & set(DT.FIXED_FLOORS)
    # every chain member has more dense slices in window 0 than a sweep lists, and the chain of 25 words has members on
    # both sides of the byte counters' bound
    assert all(h.dense(int(r), 0) > D.MAX_DENSE for r in h.members)
    T25 = [h.T(r) for r in h.chain(h.chains[1])]
    print("T of the chain of 25 words:", T25, "of the widest:", [h.T(r) for r in h.chain(h.chains[-1])])
    assert min(T25) <= 255 < max(T25)
    assert all(h.T(r) <= 255 for r in h.chain(h.chains[0])) and all(h.T(r) > 255 for f in h.chains[2:] for r in h.chain(f))
    # the chain's keys: one each, none shared with a family's or the words'
    keys = C.key_chains(h.members)
    assert [len(set(keys[i:i + C.CHAIN_MEMBERS].tolist())) for i in range(0, 60, C.CHAIN_MEMBERS)] == [1] * 5
    assert len(set(keys.tolist())) == 5 and not set(keys.tolist()) & set(DT.key_families(case.lists["long"][:-60]).tolist())
    assert np.array_equal(C.key_chains(case.lists["long"][:-60]), DT.key_families(case.lists["long"][:-60]))


def test_the_new_boruvka_is_the_old_one_with_its_rounds_told(case):
    for name, p in (("short", 200), ("long", 600)):
        picked_in, rounds, after = case.rounds(name, p)
        forest, old_rounds = TT.boruvka(case.truth(name), case.lists[name], p, DT.LEAST)
        assert set(picked_in) == forest and rounds == old_rounds == len(after) == max(picked_in.values())
        assert set(map(tuple, TT.kruskal(case.truth(name), case.lists[name], p, DT.LEAST).tolist())) == forest
        # the components after the last round are Truth.cluster's
        _, n_clusters, _, of_ref = case.truth(name).cluster(case.lists[name], p, DT.LEAST)
        refs = case.truth(name).refs
        assert all(int(refs[after[-1][i]]) == of_ref[int(refs[i])] for i in TT.nodes_of(case.truth(name), case.lists[name]))
        # each round's picked edges leave the components of the round before
        for (a, b, _), k in picked_in.items():
            if k >= 2:
                ia, ib = np.searchsorted(refs, [a, b])
                assert after[k - 2][ia] != after[k - 2][ib] and after[k - 1][ia] == after[k - 1][ib]


def test_every_chain_alone_needs_two_merging_rounds_wherever_it_is_connected(case):
    h = case.h
    for first in h.chains:
        chain = np.array(h.chain(first), dtype=np.uint32)
        for p in DT.FIXED_FLOORS:
            picked_in, rounds, _ = TT.boruvka_rounds(h.truth, chain, p)
            connected = len(picked_in) == len(chain) - 1
            print(f"chain {first} (T about {h.T(first)}) alone at floor {p}: {rounds} rounds, {len(picked_in)} records")
            if connected:
                assert rounds >= 2, (first, p)
        assert len(TT.boruvka_rounds(h.truth, chain, 200)[0]) == len(chain) - 1, first   # connected at the lowest at least


@pytest.mark.parametrize("name", ["short", "long"])
def test_the_later_rounds_pick_records_with_left_out_slices_of_both_widths_across_windows_and_in_the_upper_half(case, name):
    h = case.h
    chain = set(h.members.tolist())
    for p in case.floors:
        picked_in, rounds, _ = case.rounds(name, p)
        late = [_ends(h, a, b) for (a, b, _), k in picked_in.items() if k >= 2 and a in chain and b in chain]
        in0 = [(lo, hi) for lo, hi in late if h.loc[lo][0] == h.loc[hi][0] == 0 and h.dense(hi, 0) > D.MAX_DENSE]
        met = {
            "wide": [e for e in in0 if h.T(e[1]) > 255],
            "narrow": [e for e in in0 if h.T(e[1]) <= 255],
            "windows": [e for e in late if (h.loc[e[0]][0], h.loc[e[1]][0]) == (0, 1)],
            "upper": [e for e in in0 if h.T(e[1]) > 255 and h.loc[e[0]][1] >= D.HALF and h.loc[e[1]][1] >= D.HALF],
        }
        print(f"{name}, floor {p}: {rounds} rounds, {len(picked_in)} records, {len(late)} of the chains' after round 1: "
              + ", ".join(f"{k} {len(v)}" for k, v in met.items()))
        assert rounds >= 2, p
        if p in DT.FIXED_FLOORS:
            for k, v in met.items():
                assert v, (name, p, k)


@pytest.mark.parametrize("name", ["short", "long"])
def test_an_edge_inside_a_component_of_round_1_stands_behind_a_bitmap_probe(case, name):
    """Only this makes the `co == cq` skip of a sweep run, in a round that still merges, for a rank that slices left out
    of the count let through: an edge at the floor between two chain members of one component after round 1, both in
    window 0, the one at the higher position with more dense slices than the list holds."""
    h, truth, listed = case.h, case.truth(name), case.lists[name]
    refs = truth.refs
    for p in DT.FIXED_FLOORS:
        picked_in, rounds, after = case.rounds(name, p)
        lo, hi, _ = TT.edges(truth, listed, p, DT.LEAST)
        inside = [_ends(h, int(refs[a]), int(refs[b])) for a, b in zip(lo.tolist(), hi.tolist())
                  if refs[a] >= C.CHAIN_REF0 and refs[b] >= C.CHAIN_REF0 and after[0][a] == after[0][b]
                  and (int(refs[a]), int(refs[b])) not in {e[:2] for e in picked_in}]
        behind = [e for e in inside if h.loc[e[0]][0] == h.loc[e[1]][0] == 0 and h.dense(e[1], 0) > D.MAX_DENSE]
        print(f"{name}, floor {p}: {len(inside)} chain edges inside a component of round 1 and in no record, {len(behind)} "
              f"behind a bitmap probe, {sum(h.T(e[1]) > 255 for e in behind)} of them of a wide needle")
        assert rounds >= 2 and behind, p
        if p == 200:
            assert any(h.T(e[1]) > 255 for e in behind) and any(h.T(e[1]) <= 255 for e in behind)


@pytest.mark.parametrize("name", ["short", "long"])
def test_what_the_three_sets_of_keys_do_to_a_chain(case, name):
    h, listed = case.h, case.lists[name]
    plain = case.truth(name)
    chain_rows = lambda rows: [r for r in rows.tolist() if r[0] >= C.CHAIN_REF0 or r[1] >= C.CHAIN_REF0]
    pairs = blocked(h.held, listed, DT.key_pairs(listed))
    chains = blocked(h.held, listed, C.key_chains(listed))
    shared = C.blocked_on(h.truth, listed, DT.key_pairs(listed))   # (the GPU tests' way to the same truth)
    assert np.array_equal(shared.key, pairs.key)
    assert all(np.array_equal(x, y) for x, y in zip(shared.pairs(listed, DT.LEAST), pairs.pairs(listed, DT.LEAST)))
    a, b = case.parity_edge
    assert DT.key_parity([a])[0] != DT.key_parity([b])[0] and h.loc[a][0] == h.loc[b][0] == 0
    assert h.T(a) > 255 and h.dense(a, 0) > D.MAX_DENSE and h.dense(b, 0) > D.MAX_DENSE
    for p in case.floors:
        # key_pairs: the list's blocked forest takes several rounds, and at the fixed floors some chain's alone does
        _, rounds, _ = TT.boruvka_rounds(pairs, listed, p, DT.LEAST)
        alone = {first: TT.boruvka_rounds(pairs, np.array(h.chain(first), dtype=np.uint32), p)[1] for first in h.chains}
        # key_chains: a chain's records are the plain tree's
        want = chain_rows(TT.kruskal(plain, listed, p, DT.LEAST))
        got = chain_rows(TT.kruskal(chains, listed, p, DT.LEAST))
        c_rounds = TT.boruvka_rounds(chains, listed, p, DT.LEAST)[1]
        print(f"{name}, floor {p}: key_pairs {rounds} rounds (the chains alone {sorted(alone.values())}), key_chains "
              f"{c_rounds} rounds, {len(got)} chain records")
        assert rounds >= 2 and c_rounds >= 2, p
        assert got == want and len(got) >= 5, p
        if p in DT.FIXED_FLOORS:
            assert max(alone.values()) >= 2, p
        # key_parity: the chain edge passes the floor at every floor used and is an edge under no parity
        assert (min(a, b), max(a, b)) in DT.within_edges(plain, listed, None, p), p
        assert (min(a, b), max(a, b)) not in DT.within_edges(plain, listed, DT.key_parity(listed), p), p
    assert h.permille(a, b) >= case.floors[-1]


@pytest.mark.parametrize("name", ["short", "long"])
def test_what_the_core_trees_cases_hold(case, name):
    h, truth, listed = case.h, case.truth(name), case.lists[name]
    refs = truth.refs
    chain = refs >= C.CHAIN_REF0
    family = (refs >= D.FAMILY_REF0) & ~chain
    top = max(k for _, k in C.core_cases(case))
    second = False
    for p, k in C.core_cases(case):
        want = CoreTreeTruth(truth, listed, p, k, DT.LEAST if p >= DT.LEAST else None)
        lo, hi, ht = core_edges(truth, listed, p, DT.LEAST)
        best = np.full(len(refs), -1, dtype=np.int64)
        np.maximum.at(best, lo, ht)
        np.maximum.at(best, hi, ht)
        c = want.c
        capped = chain & (c >= 0) & (c < best)
        none = chain & want.node & (c < 0)
        width = (1001 - p + BUCKETS - 1) // BUCKETS
        other_bucket = chain & (c >= 0) & ((c - p) // width != (best - p) // width)
        print(f"{name}, ({p}, {k}): cores {int((c >= 0).sum())} ({int((chain & (c >= 0)).sum())} chain members, "
              f"{int((family & (c >= 0)).sum())} family members), {len(want.merges)} records, capped chain members "
              f"{int(capped.sum())}, chain members without a core height {int(none.sum())}, with the k-th edge in another "
              f"bucket than the best {int(other_bucket.sum())}")
        if k < top:
            assert (chain & (c >= 0)).any() and (family & (c >= 0)).any(), (p, k)
            assert capped.any(), (p, k)
            assert len(want.merges) >= 3
        else:
            assert none.any(), (p, k)
        if p <= 1000 - BUCKETS:
            second |= bool(other_bucket.any())
    assert second, "the second height sweep decides nothing for a chain member"
    assert any(p >= 1001 - BUCKETS for p, _ in C.core_cases(case)) and any(p <= 1000 - BUCKETS for p, _ in C.core_cases(case))


def test_the_hand_made_cases_expectations():
    """From m = 6, T = 12, R = 6: the glued string meets a copy at exactly 500."""
    c = DT.handmade()                                             # (asserts the bar, the six dense slices and the position)
    e = C.handmade_expectations(c)
    truth = Truth(c.held)
    copies = list(range(2, 72))
    for p, records in ((500, e.tree[500]), (501, e.tree[501])):
        assert TT.kruskal(truth, c.refs, p).tolist() == records
    assert e.tree[500] == [[2, r, 1000] for r in copies[1:]] + [[1, 2, 500]] and e.tree[501] == e.tree[500][:-1]
    assert len(e.tree[501]) == 69
    for (p, k), core_of in e.core.items():
        want = CoreTreeTruth(truth, c.refs, p, k)
        assert dict(zip(c.refs.tolist(), want.core_permille.tolist())) == core_of, (p, k)
    at = e.core
    assert all(at[500, 70][r] == 500 for r in [1] + copies) and at[500, 70][100] == at[500, 70][101] == NO_CORE
    # (the glued string's 69th largest of 70 edges at 500 is 500; one per mille up it has no edge and no core height)
    assert all(at[500, 69][r] == 1000 for r in copies) and at[500, 69][1] == 500
    assert all(at[501, 69][r] == 1000 for r in copies) and at[501, 69][1] == NO_CORE
    assert set(at[501, 70].values()) == {NO_CORE}
    own = blocked(c.held, c.refs, e.own_key)
    for p in (500, 501):
        assert TT.kruskal(own, c.refs, p).tolist() == e.tree[501]
