"""cluster_tree, cluster_core_tree and cluster_tree_within on the dense-slice map: cluster_tree_sweep_kernel, the two
endings of core_sweep (cluster_core_height_sweep_kernel, cluster_core_tree_sweep_kernel) and
cluster_tree_within_sweep_kernel are three more copies of the floor sweep (the list of at most 64 dense slices, the
L = min(t - 1, nd) largest left out and asked about in their bitmaps, 16-bit counters over two half windows for a needle
of more than 255 trigrams, a needle's windows shared among workgroups), and cluster_tree_within_kernel has its own copy
of the transposed-image scoring with byte counters emptied every 255 codes.  Their endings write the height
floor(1000 m / (T + R - m)) into the records, bin it into 32 counters a node and cap edges by it: an m that is off by one
moves a record, a core height or the order of two records where the components stay the same.

The map is tests/dense_tree_case.py's: tests/dense_case.py's with five chain families, whose members need two or three
Boruvka rounds to join, so that the code of round 2 onwards -- the closed component's return, the `co == cq` skip
behind the bitmap probes, the direct kernel's closed needle and member -- runs for needles with slices left out, of both
counter widths, across the windows and in the upper half window.  tests/test_dense_tree_case.py proves those conditions
on the host.  Everything is compared exactly with the host's truths (cluster_tree_truth.py, cluster_core_tree_truth.py,
cluster_tree_within_truth.py: numpy over the strings' tokenisations, nothing of the library) by the checkers of
tests/test_gpu_cluster_tree.py, tests/test_gpu_cluster_core_tree.py and tests/test_gpu_cluster_tree_within.py."""
import numpy as np
import pytest

import cluster_tree_truth as TT
import dense_case as D
import dense_tree_case as C
import dense_truths as DT
from blurrily_amd import RawMap
from blurrily_amd.map import _pack
from cluster_core_tree_truth import NO_CORE, CoreTreeTruth
from cluster_tree_within_truth import blocked
from cluster_truth import Truth
from dense_truths import _same_bytes
from test_gpu_cluster_core_tree import check_core_tree, height_sweeps, sweeps_for
from test_gpu_cluster_tree import check_tree, sweeps
from test_gpu_cluster_tree_within import DIRECT, SWEEP, check_tree as check_within, one_tree_per_block

pytestmark = pytest.mark.gpu
CUTS = 3                                                        # the core tree's (its cuts are proven on this kind of map by
TREE_CUTS = 1                                                   # tests/test_gpu_dense_floor_sweeps.py); the other two entries'
KEYS = {"pairs": DT.key_pairs, "chains": C.key_chains, "parity": DT.key_parity}
KERNELS = {1: (SWEEP, DIRECT), 2: (DIRECT, SWEEP), 0: (DIRECT, SWEEP)}   # strategy: (runs, does not); auto: every block is small


@pytest.fixture(scope="module")
def case():
    import torch
    m, h = C.build()
    c = C.inputs(h)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # windows_per_workgroup: per = max(1, n_windows * nodes / (8 CUs)), at most n_windows
    assert 2 * len(c.lists["short"]) < 8 * cus, (len(c.lists["short"]), cus)     # per == 1: two workgroups a needle
    assert len(c.lists["long"]) >= 8 * cus, (len(c.lists["long"]), cus)          # per == 2: one
    assert m.device_info()["n_pending"] == 0                      # (one image: a round is one sweep)
    c.m, c.h, c.truth, c._blocked = m, h, C.truths(h, c), {}

    def blocked_truth(name, keys):
        if (name, keys) not in c._blocked:
            c.truth(name).pairs(c.lists[name], DT.LEAST)            # (the list's pairs once: the blocked truths filter them)
            c._blocked[name, keys] = C.blocked_on(c.truth(name), c.lists[name], KEYS[keys](c.lists[name]))
        return c._blocked[name, keys]

    c.blocked = blocked_truth
    yield c
    m.close()


def rows_of(merges):
    return set(map(tuple, np.asarray(merges).tolist()))


def joined(merges, a, b):
    """Whether a record joins exactly these two references."""
    return any({r[0], r[1]} == {a, b} for r in np.asarray(merges).tolist())


# ---- cluster_tree ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["short", "long"])
def test_cluster_tree_equals_kruskal_and_the_cluster_truth_round_by_round_at_every_floor(case, name):
    m, truth, listed = case.m, case.truth(name), case.lists[name]
    for p in case.floors:
        labels, merges = check_tree(m, truth, listed, p, least=DT.LEAST, cuts=TREE_CUTS)
        w_labels, w_clusters, w_edges, _ = truth.cluster(listed, p, DT.LEAST)
        picked_in, rounds, _ = TT.boruvka_rounds(truth, listed, p, DT.LEAST)
        one, two, three = (m.cluster_tree(listed, p) for _ in range(3))
        assert rounds >= 2 and sweeps(m) == rounds + 1, (p, rounds, sweeps(m))
        assert m.last_kernels().count("cluster_tree_merge_kernel") == rounds + 1
        _same_bytes(one, two)
        _same_bytes(one, three)
        assert one[0].tobytes() == labels.tobytes() and one[1].tobytes() == merges.tobytes()
        assert np.array_equal(labels, w_labels) and one[2:] == (w_clusters, w_edges), p
        assert rows_of(merges) == set(picked_in), p
        chain_late = sum(1 for e, k in picked_in.items() if k >= 2 and e[0] >= C.CHAIN_REF0)
        print(f"{name}, floor {p}: {rounds} rounds, {len(merges)} records, {chain_late} of the chains' after round 1")
        assert chain_late >= 5, p


@pytest.mark.parametrize("name", ["short", "long"])
def test_the_pairs_record_disappears_from_p_star_to_p_star_plus_1_without_its_family(case, name):
    m, listed = case.m, case.lists[name]
    low, high = case.pair
    alone = np.concatenate([listed[~np.isin(listed, case.family)], np.array([low, high], dtype=np.uint32)])
    truth = case.truth(name + ", the pair alone")
    at = {}
    for p in (case.p_star, case.p_star + 1):
        labels, at[p] = check_tree(m, truth, alone, p, least=DT.LEAST, cuts=1)
        assert (labels[-2] == labels[-1]) == (p == case.p_star), p
    assert (min(low, high), max(low, high), case.p_star) in rows_of(at[case.p_star])
    assert not joined(at[case.p_star + 1], low, high)
    assert rows_of(at[case.p_star + 1]) == {r for r in rows_of(at[case.p_star]) if r[2] > case.p_star}


# ---- cluster_core_tree -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["short", "long"])
def test_cluster_core_tree_equals_the_truth_at_every_case_with_its_height_sweeps_counted(case, name):
    m, truth, listed = case.m, case.truth(name), case.lists[name]
    assert [sweeps_for(p) for p, _ in C.core_cases(case)] == [2, 2, 2, 2, 2, 1]
    for p, k in C.core_cases(case):
        labels, core, merges = check_core_tree(m, truth, listed, p, k, least=DT.LEAST, cuts=CUTS)
        one, two = (m.cluster_core_tree(listed, p, k) for _ in range(2))
        assert height_sweeps(m) == sweeps_for(p), (p, k)
        assert "cluster_core_tree_sweep_kernel" in m.last_kernels() and "cluster_tree_sweep_kernel" not in m.last_kernels()
        _same_bytes(one, two)
        assert one[1].tobytes() == core.tobytes() and one[2].tobytes() == merges.tobytes()
        chains = np.isin(listed, case.chains)
        if k < 5:
            assert (core[chains] != NO_CORE).any() and len(merges) >= 3, (p, k)
        else:
            assert (core[chains] == NO_CORE).any(), (p, k)


@pytest.mark.parametrize("name", ["short", "long"])
def test_min_degree_zero_and_one_give_the_cluster_trees_records_byte_for_byte(case, name):
    m, listed = case.m, case.lists[name]
    for p in case.floors:
        t_labels, t_merges, t_clusters, t_edges = m.cluster_tree(listed, p)   # (proven above)
        assert len(t_merges) >= 3
        labels, core, merges, n_clusters, n_edges, n_core_edges = m.cluster_core_tree(listed, p, 0)
        assert "cluster_core_height_sweep_kernel" not in m.last_kernels()
        assert merges.tobytes() == t_merges.tobytes() and labels.tobytes() == t_labels.tobytes(), p
        assert (n_clusters, n_edges, n_core_edges) == (t_clusters, t_edges, t_edges) and (core == 1000).all(), p
        labels, core, merges, n_clusters, n_edges, n_core_edges = m.cluster_core_tree(listed, p, 1)
        assert height_sweeps(m) == sweeps_for(p)
        assert merges.tobytes() == t_merges.tobytes() and labels.tobytes() == t_labels.tobytes(), p
        assert (n_edges, n_core_edges) == (t_edges, t_edges), p
        # a node's core height at min_degree 1 is its best edge: of a record's ends, at least the record's height
        of = dict(zip(listed.tolist(), core.tolist()))
        assert all(ht <= of[a] <= 1000 and ht <= of[b] <= 1000 for a, b, ht in merges.tolist()), p


# ---- cluster_tree_within -----------------------------------------------------------------------------------------------

def within(m, listed, blocks, p, strategy, rounds=None):
    """One call under `strategy`, the intended kernel named (once per round and once more) and the other not."""
    m.set_option("scope_strategy", strategy)
    try:
        out = m.cluster_tree_within(listed, blocks, p)
        names = m.last_kernels()
    finally:
        m.set_option("scope_strategy", 0)
    ran, idle = KERNELS[strategy]
    assert ran in names and idle not in names and "cluster_tree_sweep_kernel" not in names, (strategy, names)
    if rounds is not None:
        assert names.count(ran) == rounds + 1 and names.count("cluster_tree_merge_kernel") == rounds + 1, (strategy, names)
    return out


@pytest.mark.parametrize("keys", ["pairs", "chains"])
@pytest.mark.parametrize("name", ["short", "long"])
def test_cluster_tree_within_equals_the_blocked_truth_under_the_sweep_direct_and_auto(case, name, keys):
    m, listed, truth = case.m, case.lists[name], case.blocked(name, keys)
    blocks = KEYS[keys](listed)
    plain = case.truth(name)
    for p in case.floors:
        labels, merges = check_within(m, truth, listed, blocks, p, least=DT.LEAST, cuts=TREE_CUTS)
        picked_in, rounds, _ = TT.boruvka_rounds(truth, listed, p, DT.LEAST)
        assert rounds >= 2 and rows_of(merges) == set(picked_in), p
        for s in (1, 2, 0):
            got = within(m, listed, blocks, p, s, rounds)
            assert got[0].tobytes() == labels.tobytes() and got[1].tobytes() == merges.tobytes(), (p, s)
        chain_rows = [r for r in merges.tolist() if r[0] >= C.CHAIN_REF0]
        print(f"{name}, {keys}, floor {p}: {rounds} rounds, {len(merges)} records, {len(chain_rows)} of the chains")
        if keys == "chains":                                       # a chain under a key of its own: the plain tree's records
            want = [r for r in TT.kruskal(plain, listed, p, DT.LEAST).tolist() if r[0] >= C.CHAIN_REF0]
            assert chain_rows == want and len(want) == len(case.chains) - len(case.h.chains), p
        else:
            assert 0 < len(chain_rows) < len(case.chains) - len(case.h.chains), p


@pytest.mark.parametrize("name", ["short", "long"])
def test_under_different_parities_the_pair_and_the_chain_edge_are_in_no_record(case, name):
    """Both bitmap probes and the floor pass for them; only the key test behind them says no."""
    m, listed, truth = case.m, case.lists[name], case.blocked(name, "parity")
    blocks = DT.key_parity(listed)
    low, high = case.pair
    a, b = case.parity_edge
    for p in case.floors:
        labels, merges = check_within(m, truth, listed, blocks, p, least=DT.LEAST, cuts=1, strategies=(1, 2))
        assert not joined(merges, low, high) and not joined(merges, a, b), p
        assert joined(m.cluster_tree(listed, p)[1], a, b), p      # (the plain tree has the chain's edge)
        assert (merges[:, 0] % 2 == merges[:, 1] % 2).all() and len(merges) > 0, p


@pytest.mark.parametrize("name", ["short", "long"])
def test_all_keys_equal_is_the_cluster_tree_byte_for_byte(case, name):
    m, listed = case.m, case.lists[name]
    blocks = np.full(len(listed), 7, dtype=np.uint32)
    for p in case.floors:
        want = m.cluster_tree(listed, p)                          # (proven above)
        rounds = sweeps(m) - 1
        for strategy in (1, 2):
            _same_bytes(within(m, listed, blocks, p, strategy, rounds), want)


@pytest.mark.parametrize("name", ["short", "long"])
def test_one_cluster_tree_call_per_block_gives_the_same_under_a_key_per_chain(case, name):
    m, listed = case.m, case.lists[name]
    blocks = C.key_chains(listed)
    for p in (200, case.p_star):
        w_labels, w_merges, w_clusters, w_edges = one_tree_per_block(m, listed, blocks, p)
        for strategy in (1, 2):
            labels, merges, n_clusters, n_edges = within(m, listed, blocks, p, strategy)
            assert merges.tobytes() == w_merges.tobytes() and labels.tobytes() == w_labels.tobytes(), (p, strategy)
            assert (n_clusters, n_edges) == (w_clusters, w_edges), (p, strategy)


# ---- small cases -------------------------------------------------------------------------------------------------------

def _entries(m, blocks_of):
    """The three entries as (name, call(listed, floor) -> (labels, records, the counts))."""
    def tree(listed, p):
        out = m.cluster_tree(listed, p)
        return out[0], out[1], out[2:]

    def core_tree(listed, p):
        out = m.cluster_core_tree(listed, p, 2)
        return out[0], out[2], (out[1],) + out[3:]

    def tree_within(strategy):
        def call(listed, p):
            out = within(m, listed, blocks_of(listed), p, strategy)
            return out[0], out[1], out[2:]
        return call

    return (("tree", tree), ("core tree", core_tree), ("within, the sweep", tree_within(1)), ("within, direct", tree_within(2)))


def test_the_list_reversed_and_the_chains_listed_twice_give_the_same_label_per_reference_and_the_same_records(case):
    m, listed = case.m, case.lists["short"]
    others = (listed[::-1].copy(), np.concatenate([case.chains, listed]), np.concatenate([listed[::-1], case.chains[::-1]]))
    for what, call in _entries(m, C.key_chains):
        for p in (200, 600):
            labels, merges, counts = call(listed, p)
            label_of = dict(zip(listed.tolist(), labels.tolist()))
            assert len(merges) >= 60
            for other in others:
                o_labels, o_merges, o_counts = call(other, p)
                assert o_merges.tobytes() == merges.tobytes(), (what, p)
                assert o_labels.tolist() == [label_of[r] for r in other.tolist()], (what, p)
                if what == "core tree":                            # (its first count is the core heights, per element)
                    core_of = dict(zip(listed.tolist(), counts[0].tolist()))
                    assert o_counts[0].tolist() == [core_of[r] for r in other.tolist()] and o_counts[1:] == counts[1:], p
                else:
                    assert o_counts == counts, (what, p)


def test_every_second_chain_member_held_but_not_listed_is_no_node_behind_a_passed_probe(case):
    """The members left out pass the bitmap probes and the floor for their neighbours and are no nodes (kNoNode); the
    listed ones meet two apart, at other heights."""
    m, h, listed = case.m, case.h, case.lists["short"]
    odd = case.chains[1::2]
    fewer = listed[~np.isin(listed, odd)]
    truth = case.truth("short, every second")
    keys = C.key_chains(fewer)
    truth.pairs(fewer, DT.LEAST)
    within_truth = C.blocked_on(truth, fewer, keys)
    for p in (200, 600):
        full = TT.kruskal(case.truth("short"), listed, p, DT.LEAST)
        labels, merges = check_tree(m, truth, fewer, p, least=DT.LEAST, cuts=TREE_CUTS)
        assert not np.isin(merges[:, :2], odd).any()
        was = max(r[2] for r in full.tolist() if r[0] >= C.CHAIN_REF0 + 4 * C.CHAIN_MEMBERS)
        now = [r[2] for r in merges.tolist() if r[0] >= C.CHAIN_REF0 + 4 * C.CHAIN_MEMBERS]
        assert now and max(now) < was, p                           # the widest chain: joined still, lower
        for k in (2, 3):
            check_core_tree(m, truth, fewer, p, k, least=DT.LEAST, cuts=1)
        w_labels, w_merges = check_within(m, within_truth, fewer, keys, p, least=DT.LEAST, cuts=1)
        assert [r for r in w_merges.tolist() if r[0] >= C.CHAIN_REF0] == [r for r in merges.tolist() if r[0] >= C.CHAIN_REF0]


# ---- the hand-made case: exactly t matches, every one of them in the needle's largest dense slices -----------------------

def test_the_hand_made_case_under_the_three_entries():
    """L = t - 1 and not one more: the glued string's bar at floor 500 is 6 of its 12, a copy shares exactly the six that
    are its only dense slices, five are left out and the sixth is the one counted match that gets the copy asked about.
    tests/test_dense_tree_case.py asserts the same expectations on the truths."""
    c = DT.handmade()
    e = C.handmade_expectations(c)
    truth = Truth(c.held)
    strings = [c.held[int(r)] for r in c.refs]
    m = RawMap()
    m.set_option("dense_min", D.DENSE_MIN)
    m.put_many_packed(*_pack(strings), c.refs, c.weights)
    try:
        m.sync_device()
        assert m.device_info()["n_bitmaps"] == 6
        for p in (500, 501):
            labels, merges = check_tree(m, truth, c.refs, p)
            assert merges.tolist() == e.tree[p], p
        for (p, k), core_of in e.core.items():
            labels, core, merges = check_core_tree(m, truth, c.refs, p, k)
            assert dict(zip(c.refs.tolist(), core.tolist())) == core_of, (p, k)
            want = CoreTreeTruth(truth, c.refs, p, k)
            assert merges.tolist() == want.merges.tolist()
        one_key = np.zeros(len(c.refs), dtype=np.uint32)
        own = blocked(c.held, c.refs, e.own_key)
        for strategy in (1, 2):
            for p in (500, 501):
                labels, merges, n_clusters, n_edges = within(m, c.refs, one_key, p, strategy)
                assert merges.tolist() == e.tree[p] and n_clusters == len(c.refs) - len(e.tree[p]), (strategy, p)
                # under a key of its own the glued string joins nothing
                labels, merges, n_clusters, n_edges = within(m, c.refs, e.own_key, p, strategy)
                assert merges.tolist() == e.tree[501] and labels[c.refs == 1] == 1, (strategy, p)
                assert (n_clusters, n_edges) == (4, 70 * 69 // 2), (strategy, p)
                check_within(m, own, c.refs, e.own_key, p, strategies=(strategy,))
    finally:
        m.close()


# ---- every option at its default ---------------------------------------------------------------------------------------

def test_the_default_dense_min_where_every_dense_slice_of_a_family_is_left_out():
    m, h = D.build_default()
    try:
        family = np.array([r for head in h.heads for r in h.family(head)], dtype=np.uint32)
        listed = np.unique(np.concatenate([h.refs[::5], family]))
        blocks = DT.key_pairs(listed)
        floors = (350, 600)
        h.truth.pairs(listed, floors[0])
        within_truth = C.blocked_on(h.truth, listed, blocks)
        for p in floors:
            # every dense slice of a family's is left out: 1 <= nd <= t - 1
            assert all(1 <= h.dense_padded(x, 0) <= min(DT.floor_bar(h.T(x), p) - 1, D.MAX_DENSE) for x in h.heads)
            labels, merges = check_tree(m, h.truth, listed, p, least=floors[0], cuts=TREE_CUTS)
            of = dict(zip(listed.tolist(), labels.tolist()))
            for head in h.heads:                                   # joined within the upper half and across the halves
                assert len({of[r] for r in h.family(head)}) == 1, (p, head)
                assert sum(1 for r in merges.tolist() if head <= r[0] < head + D.MEMBERS) == D.MEMBERS - 1, (p, head)
            check_core_tree(m, h.truth, listed, p, 2, least=floors[0], cuts=TREE_CUTS)
            w_labels, w_merges = check_within(m, within_truth, listed, blocks, p, least=floors[0], cuts=TREE_CUTS, strategies=(1, 2))
            assert 0 < len(w_merges) < len(merges), p
            for s in (1, 2):
                within(m, listed, blocks, p, s)
    finally:
        m.close()
