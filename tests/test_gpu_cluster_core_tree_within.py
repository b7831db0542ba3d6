"""The cluster core tree within blocks on the GPU (cluster_core_tree_within.hip, cluster_core_tree_within_kernels.hip):
the merges, the core heights, the labels and the counts are compared byte for byte with the host's truth
(cluster_core_tree_within_truth.py: cluster_core_tree_truth's sorted heights and Kruskal over the pairs whose ends carry
one key, nothing of the library) under "scope_strategy" 0 (auto), 1 (every block swept) and 2 (every block scored
directly), and the tree cut at its floor and at its own heights (and one per mille above each) with
blurrily_storage_cluster_cores_within at those floors.  Over the oracle haystacks under interleaving keys with the
figures of DESIGN.md section 44, the identities (all keys equal, min_degree 0 and 1, all keys distinct, the counts of the
single-floor calls), built cases (the chain and its bridge under another key, ties at the k-th place in one block and
split, two triangles and a bridge, a core height that drops when a neighbour lies under another key, the counter widths
with a twin inside and one outside the block, the empty string, an unheld member), the floors at which the height
passes go from two to one, block sizes around the tile and the workgroup against one blurrily_storage_cluster_core_tree
call per block, a shuffled list, a haystack of more than one window, mutations, tests/dense_case.py's map, repeated
calls, the calls around a call, the kernels' names, and a block above the direct cap beside smaller ones."""
import numpy as np
import pytest

import dense_case as D
import dense_truths as DT
import workloads as W
from blurrily_amd import RawMap, _native
from blurrily_amd.map import _pack
from cluster_core_tree_truth import NO_CORE, CoreTreeTruth
from cluster_core_tree_within_truth import blocked, blocked_over
from cluster_tree_within_truth import BlockedTruth, per_block as merged_records
from cluster_truth import NO_CLUSTER
from helpers import oracle_case_inputs
from test_gpu_cluster import A, B, C, _j, _map_of, built_case
from test_gpu_cluster_cores import H, S, X1, X2, X3, _permille

pytestmark = pytest.mark.gpu
STRATEGIES = (0, 1, 2)                                        # "scope_strategy": auto, the sweep, the direct kernel
MAX_CUTS = 6
G = 16                                                        # the direct kernel's tile (cluster_plan.h: kClusterWithinTile)
BUCKETS = 32                                                  # kCoreBuckets of csrc/cluster.h
DIRECT = ["cluster_core_tree_within_kernel<height>", "cluster_core_tree_within_kernel<tree>"]
SWEEP = ["cluster_core_tree_within_sweep_kernel<height>", "cluster_core_tree_within_sweep_kernel<tree>"]
SETTLE = "cluster_core_height_settle_kernel"
OTHERS = ["cluster_tree_within_kernel", "cluster_tree_within_sweep_kernel", "cluster_core_tree_sweep_kernel",
          "cluster_core_height_sweep_kernel", "cluster_cores_within_kernel", "cluster_within_kernel", "cluster_sweep_kernel",
          "cluster_tree_sweep_kernel", "find_kernel"]


def passes_for(floor):
    """max(1, ceil(log_BUCKETS(1001 - floor))): the refinement's steps from a bracket of 1001 - floor heights."""
    s = 1
    while BUCKETS ** s < 1001 - floor:
        s += 1
    return s


def call(m, listed, blocks, p, min_degree, strategy=0):
    m.set_option("scope_strategy", strategy)
    try:
        return m.cluster_core_tree_within(listed, blocks, p, min_degree)
    finally:
        m.set_option("scope_strategy", 0)


def same_bytes(one, other, what=None):
    for k in range(3):
        assert one[k].dtype == other[k].dtype and one[k].tobytes() == other[k].tobytes(), (what, k)
    assert tuple(one[3:]) == tuple(other[3:]), (what, one[3:], other[3:])


def check(m, truth, listed, blocks, p, min_degree, least=None, cuts=MAX_CUTS, strategies=STRATEGIES):
    """One call per strategy against the truth (a blocked truth for this list's keys), everything exactly, and cuts at
    the tree's floor and at up to `cuts` of its heights spread over their range, each with the floor one per mille above
    it, against cluster_cores_within there.  Returns (the truth at (p, min_degree), (labels, core_permille, merges))."""
    listed, blocks = np.asarray(listed, dtype=np.uint32), np.asarray(blocks, dtype=np.uint32)
    want = CoreTreeTruth(truth, listed, p, min_degree, least)
    key_of = dict(zip(listed.tolist(), blocks.tolist()))
    for s in strategies:
        labels, core, merges, n_clusters, n_edges, n_core_edges = call(m, listed, blocks, p, min_degree, s)
        cores = len(np.unique(listed[core != NO_CORE]))
        print(f"floor {p}, min_degree {min_degree}, strategy {s}: {cores} cores, {len(merges)} merges (truth "
              f"{len(want.merges)}), clusters {n_clusters} (truth {want.n_clusters}), edges {n_edges} (truth {want.n_edges}), "
              f"core edges {n_core_edges} (truth {want.n_core_edges})")
        at = (p, min_degree, s)
        assert merges.dtype == np.uint32 and merges.shape == want.merges.shape, at
        assert merges.tobytes() == want.merges.tobytes(), at
        assert core.dtype == np.uint32 and core.tobytes() == want.core_permille.tobytes(), at
        assert labels.dtype == np.uint32 and labels.tobytes() == want.labels.tobytes(), at
        assert (n_clusters, n_edges, n_core_edges) == (want.n_clusters, want.n_edges, want.n_core_edges), at
        assert len(merges) == cores - n_clusters, at
        assert all(key_of[a] == key_of[b] for a, b, _ in merges.tolist()), at   # (no record joins two keys)
    if cuts:
        assert m.cluster_within(listed, blocks, p)[2] == n_edges
        heights = np.unique(merges[:, 2])
        if len(heights) > cuts:
            heights = heights[np.unique(np.linspace(0, len(heights) - 1, cuts).round().astype(int))]
        for f in [p] + [f for h in heights.tolist() for f in (h, h + 1)]:
            if f > 1000:
                continue
            c_labels, _, kinds, c_clusters, c_edges, c_core_edges = m.cluster_cores_within(listed, blocks, f, min_degree)
            cut, is_core = RawMap.cut_core_tree(listed, labels, core, merges, f, min_permille=p)
            assert np.array_equal(kinds == _native.KIND_CORE, (core != NO_CORE) & (core >= f)), f
            assert np.array_equal(kinds == _native.KIND_CORE, is_core), f
            assert c_labels[is_core].tobytes() == cut[is_core].tobytes(), f
            assert c_clusters == len(np.unique(cut[is_core])), f
            if f == p:
                assert (c_clusters, c_edges, c_core_edges) == (n_clusters, n_edges, n_core_edges)
    return want, (labels, core, merges)


_CASES = {}


def oracle_case(kind, n, modulus=3):
    """The map of one oracle haystack, made once, and per modulus the blocked truth under reference % modulus."""
    if (kind, n) not in _CASES:
        hay, off, needles = oracle_case_inputs(kind, n)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        _CASES[kind, n] = dict(m=_map_of(held), held=held, needles=needles, listed=np.arange(1, n + 1, dtype=np.uint32),
                               truths={})
    c = _CASES[kind, n]
    blocks = (c["listed"] % modulus).astype(np.uint32)
    if modulus not in c["truths"]:
        first = next(iter(c["truths"].values()), None)
        c["truths"][modulus] = (blocked_over(first, c["listed"], blocks) if first is not None else
                                blocked(c["held"], c["listed"], blocks))
    return dict(c, truth=c["truths"][modulus], blocks=blocks)


# (haystack, n, modulus, floor, {min_degree: (merges, heights, clusters, edges, core edges, cores)}): the figures of
# DESIGN.md section 44 for the first min_degree of each row, which tests/test_cluster_core_tree_within_abi.py asserts of
# the truth; the neighbouring min_degrees against the truth alone
TABLE = [("words", 5000, 3, 200, {2: (222, 9, 134, 873, 311, 356), 3: (71, 6, 55, 873, 102, 126), 4: None}),
         ("geonames", 8000, 3, 500, {5: (2780, 74, 74, 72710, 70270, 2854), 4: None, 6: None}),
         ("geonames", 8000, 64, 300, {3: (2687, 101, 168, 13206, 11624, 2855), 2: None, 4: None}),
         ("skewed", 6000, 3, 500, {3: (59, 4, 41, 640, 84, 100), 2: None, 4: None})]


@pytest.mark.parametrize("kind,n,modulus,p,figures", TABLE, ids=[f"{c[0]}-{c[2]}-{c[3]}" for c in TABLE])
def test_everything_equals_the_truth_and_every_cut_equals_the_cores_within_call(kind, n, modulus, p, figures):
    c = oracle_case(kind, n, modulus)
    m, listed, blocks = c["m"], c["listed"], c["blocks"]
    for min_degree, row in figures.items():
        want, (labels, core, merges) = check(m, c["truth"], listed, blocks, p, min_degree, least=p,
                                             cuts=MAX_CUTS if row else 0)
        if row:
            got = (len(merges), len(np.unique(merges[:, 2])), want.n_clusters, want.n_edges, want.n_core_edges,
                   int((core != NO_CORE).sum()))
            assert got == row
            assert (labels[core != NO_CORE] % modulus == listed[core != NO_CORE] % modulus).all()


def test_the_identities_equal_keys_min_degree_0_and_1_and_distinct_keys():
    c = oracle_case("words", 5000)
    m, everything, blocks = c["m"], c["listed"], c["blocks"]
    for s in STRATEGIES:
        # all keys equal: byte for byte the core tree
        for p, min_degree in ((200, 2), (300, 3)):
            plain = m.cluster_core_tree(everything, p, min_degree)
            got = call(m, everything, np.full(len(everything), 0xFFFFFFFF, dtype=np.uint32), p, min_degree, s)
            same_bytes(got, plain, (s, p))
            assert len(plain[2]) > 0
        # min_degree 0 and 1: the merges and labels of the cluster tree within blocks
        t_labels, t_merges, t_clusters, t_edges = m.cluster_tree_within(everything, blocks, 200)
        assert len(t_merges) >= 3
        labels, core, merges, n_clusters, n_edges, n_core_edges = call(m, everything, blocks, 200, 0, s)
        assert merges.tobytes() == t_merges.tobytes() and labels.tobytes() == t_labels.tobytes(), s
        assert (n_clusters, n_edges, n_core_edges) == (t_clusters, t_edges, t_edges) and (core == 1000).all()
        labels, core, merges, n_clusters, n_edges, n_core_edges = call(m, everything, blocks, 200, 1, s)
        assert merges.tobytes() == t_merges.tobytes() and labels.tobytes() == t_labels.tobytes(), s
        assert (n_edges, n_core_edges) == (t_edges, t_edges)
        assert n_clusters == t_clusters - int((core == NO_CORE).sum()) and (core == NO_CORE).any()
        # all keys distinct: no record, no core height, every held reference its own label
        some = np.concatenate([everything[:700], [888888]]).astype(np.uint32)
        for min_degree in (1, 3):
            labels, core, merges, n_clusters, n_edges, n_core_edges = call(m, some, some[::-1].copy(), 0, min_degree, s)
            assert labels.tolist() == some[:700].tolist() + [NO_CLUSTER] and (core == NO_CORE).all()
            assert (merges.shape, n_clusters, n_edges, n_core_edges) == ((0, 3), 0, 0, 0)
        labels, core, merges, n_clusters, n_edges, n_core_edges = call(m, some, some[::-1].copy(), 0, 0, s)
        assert core.tolist() == [1000] * 700 + [NO_CORE] and (merges.shape, n_clusters, n_edges) == ((0, 3), 700, 0)
        # the counts of the single-floor calls
        got = call(m, everything, blocks, 200, 3, s)
        assert got[4] == m.cluster_within(everything, blocks, 200)[2]
        assert got[3:] == m.cluster_cores_within(everything, blocks, 200, 3)[3:]


def plain_lists(result):
    return tuple(x.tolist() if isinstance(x, np.ndarray) else x for x in result)


def answers(m, listed, blocks, p, min_degree):
    """The call under every strategy, the three the same: as plain lists and numbers."""
    got = [plain_lists(call(m, listed, blocks, p, min_degree, s)) for s in STRATEGIES]
    assert got[0] == got[1] == got[2], (p, min_degree)
    return got[0]


def test_the_chain_in_one_block_and_with_its_bridge_under_another_key():
    held = built_case()
    m = _map_of(held)
    assert _j(A, B) == (8, 16) and _j(B, C) == (6, 17) and _j(A, C)[0] == 0
    chain = [5001, 5002, 5003]
    none = []
    # in one block: the core tree's answers (tests/test_gpu_cluster_core_tree.py)
    assert answers(m, chain, [4, 4, 4], 300, 2) == (chain, [NO_CORE, 352, NO_CORE], none, 1, 2, 0)
    assert answers(m, chain, [4, 4, 4], 300, 1) == ([5001] * 3, [500, 500, 352], [[5001, 5002, 500], [5002, 5003, 352]], 1, 2, 2)
    # B, the bridge, under another key: no edge is left, whatever the min_degree
    for min_degree in (1, 2):
        assert answers(m, chain, [1, 2, 1], 300, min_degree) == (chain, [NO_CORE] * 3, none, 0, 0, 0)
    assert answers(m, chain, [1, 2, 1], 0, 0) == (chain, [1000] * 3, none, 3, 0, 0)
    # C under another key: A - B alone, each the other's best edge
    assert answers(m, chain, [1, 1, 2], 300, 1) == ([5001, 5001, 5003], [500, 500, NO_CORE], [[5001, 5002, 500]], 1, 1, 1)
    assert answers(m, chain, [1, 1, 2], 300, 2) == (chain, [NO_CORE] * 3, none, 0, 1, 0)
    m.close()


def test_ties_at_the_kth_place_in_one_block_and_split_two_and_two():
    same = b"tied strings"
    m = _map_of({1: same, 2: same, 3: same, 4: same})
    four, star = [1, 2, 3, 4], [[1, 2, 1000], [1, 3, 1000], [1, 4, 1000]]
    assert answers(m, four, [9] * 4, 1000, 3) == ([1] * 4, [1000] * 4, star, 1, 6, 6)
    assert answers(m, four, [9] * 4, 1000, 4) == (four, [NO_CORE] * 4, [], 0, 6, 0)
    assert answers(m, [4, 2, 3, 1, 2], [9] * 5, 0, 3)[2] == star
    # split two and two: each has one edge; a core at min_degree 1 only
    split = [9, 9, 8, 8]
    assert answers(m, four, split, 1000, 1) == ([1, 1, 3, 3], [1000] * 4, [[1, 2, 1000], [3, 4, 1000]], 2, 2, 2)
    for min_degree in (2, 3, 4):
        assert answers(m, four, split, 1000, min_degree) == (four, [NO_CORE] * 4, [], 0, 2, 0)
    assert answers(m, [4, 2, 3, 1, 2], [8, 9, 8, 9, 9], 0, 1)[2] == [[1, 2, 1000], [3, 4, 1000]]
    m.close()


def test_two_triangles_and_a_bridge_and_a_core_height_that_drops_when_a_neighbour_lies_under_another_key():
    A1, A2, A3, Br, C1, C2, C3 = S[0], S[0] + b"z", S[0] + S[1], S[1] + S[2], S[2] + S[3], S[3], S[3] + b"pq"
    held = {i + 1: s for i, s in enumerate([A1, A2, A3, Br, C1, C2, C3])}
    m = _map_of(held)
    listed = [1, 2, 3, 4, 5, 6, 7]
    for blocks in ([1] * 7, [1, 1, 1, 2, 1, 1, 1], [1, 1, 1, 1, 2, 2, 2]):
        truth = blocked(held, listed, blocks)
        for min_degree in (0, 1, 2, 3, 4):
            want, (labels, core, merges) = check(m, truth, listed, blocks, 1, min_degree, cuts=4)
    # the bridge under another key: it has no edge, and each triangle is a tree of its own at min_degree 2
    labels, core, merges, n_clusters, n_edges, n_core_edges = call(m, listed, [1, 1, 1, 2, 1, 1, 1], 1, 2)
    assert labels.tolist() == [1, 1, 1, 4, 5, 5, 5] and core[3] == NO_CORE and (n_clusters, n_edges, n_core_edges) == (2, 6, 6)
    assert len(merges) == 4 and not (merges[:, :2] == 4).any()
    # all under one key the bridge joins them: one more record, and it names 4
    labels, core, merges, n_clusters, n_edges, n_core_edges = call(m, listed, [1] * 7, 1, 2)
    assert labels.tolist() == [1] * 7 and (n_clusters, n_edges, n_core_edges) == (1, 8, 8) and (merges[:, :2] == 4).any()
    m.close()
    # the hub: H has edges at 500, 384 and 666; its core height at min_degree 3 is the third, 384 -- and with X2 under
    # another key it has two edges and no core height, while at min_degree 2 its height is the second either way
    assert [_permille(*xy) for xy in ((H, X1), (H, X2), (H, X3), (X1, X3), (X2, X3))] == [500, 384, 666, 400, 235]
    held = {1: X1, 2: X2, 3: H, 4: X3}
    m = _map_of(held)
    four = [1, 2, 3, 4]
    assert answers(m, four, [5, 5, 5, 5], 300, 3)[1] == [NO_CORE, NO_CORE, 384, NO_CORE]
    assert answers(m, four, [5, 6, 5, 5], 300, 3)[1] == [NO_CORE] * 4
    assert answers(m, four, [5, 5, 5, 5], 300, 2) == ([1, 2, 1, 1], [400, NO_CORE, 500, 400], [[1, 3, 400], [1, 4, 400]], 1, 4, 3)
    assert answers(m, four, [5, 6, 5, 5], 300, 2) == ([1, 2, 1, 1], [400, NO_CORE, 500, 400], [[1, 3, 400], [1, 4, 400]], 1, 3, 3)
    # X3 under another key: H keeps 500 and 384, and its height drops from 500 to 384
    assert answers(m, four, [5, 5, 5, 6], 300, 2)[1] == [NO_CORE, NO_CORE, 384, NO_CORE]
    for blocks in ([5, 5, 5, 5], [5, 6, 5, 5], [5, 5, 5, 6], [5, 6, 6, 5]):
        truth = blocked(held, four, blocks)
        for min_degree in (1, 2, 3):
            check(m, truth, four, blocks, 300, min_degree, cuts=3)
    m.close()


def test_the_counter_widths_twins_inside_and_outside_a_block_the_empty_string_and_the_height_passes():
    held = built_case()
    sizes = (15, 16, 255, 256, 700)
    for i in range(len(sizes)):                               # a third twin of each sized node, and of the empty string
        held[6100 + i] = held[6000 + 4 * i]
    held[7003] = b""
    m = _map_of(held)
    # the words under three interleaving keys; the built nodes under key 7, the third twins under key 8
    everything = np.array(sorted(held), dtype=np.uint32)
    blocks = np.where(everything > 5000, 7, everything % 3).astype(np.uint32)
    blocks[np.isin(everything, [6100 + i for i in range(len(sizes))] + [7003])] = 8
    truth = blocked(held, everything, blocks)
    assert [passes_for(f) for f in (0, 968, 969, 1000)] == [2, 2, 1, 1]
    # (968 and 969: the equal strings' 1000 and their near copies' 990s on both sides of the step from two passes to one)
    for p in (0, 200, 1000 - BUCKETS, 1001 - BUCKETS, 1000):
        for min_degree in (1, 2):
            want, (labels, core, merges) = check(m, truth, everything, blocks, p, min_degree, cuts=2)
        for s, ran, idle in ((2, DIRECT, SWEEP), (1, SWEEP, DIRECT)):
            call(m, everything, blocks, p, 2, s)
            names = m.last_kernels()
            assert names.count(ran[0]) == passes_for(p) and idle[0] not in names, (p, s, names)
            assert names.count(SETTLE) == passes_for(p) + 1
        of = dict(zip(everything.tolist(), core.tolist()))
        rows = set(map(tuple, merges.tolist()))
        for i, t in enumerate(sizes):
            a, b, variant, away = 6000 + 4 * i, 6001 + 4 * i, 6002 + 4 * i, 6100 + i
            assert len(truth.codes[truth.refs.tolist().index(a)]) == t
            # (min_degree 2) the twins inside the block have each other at 1000 and their variants below: one core
            # height, under 1000, where a variant's edge is above the floor; the twin outside has no edge from 200 up
            assert of[a] == of[b] and (of[a] == NO_CORE or (of[a] < 1000 and (a, b, of[a]) in rows))
            assert p > 200 or of[a] != NO_CORE
            assert p == 0 or (of[away] == NO_CORE and away not in merges[:, :2])
        assert of[7003] == NO_CORE and of[7001] == of[7002] == NO_CORE    # (the empty strings: one edge each at most)
    # min_degree 1: the twins stand at 1000, the empty strings too, the ones outside alone
    want, (labels, core, merges) = check(m, truth, everything, blocks, 1000, 1, cuts=1)
    of, label = dict(zip(everything.tolist(), core.tolist())), dict(zip(everything.tolist(), labels.tolist()))
    for a, b, away in [(6000 + 4 * i, 6001 + 4 * i, 6100 + i) for i in range(len(sizes))] + [(7001, 7002, 7003)]:
        assert (of[a], of[b], of[away]) == (1000, 1000, NO_CORE) and (label[a], label[b], label[away]) == (a, a, away)
    # min_degree 0: no height pass at all
    for s, ran in ((2, DIRECT), (1, SWEEP)):
        call(m, everything, blocks, 200, 0, s)
        names = m.last_kernels()
        assert ran[0] not in names and ran[1] in names and names.count(SETTLE) == 1
    m.close()


def test_an_unheld_reference_in_the_middle_of_a_block():
    hay, off = W.words(600, seed=3)
    held = {10 * (i + 1): s for i, s in enumerate(W.unpack(hay, off))}
    m = _map_of(held)
    unheld = [15, 3005, 3015, 5995]
    listed = np.array(sorted(list(held) + unheld), dtype=np.uint32)
    blocks = ((listed // 10) % 2).astype(np.uint32)
    for lst, blk in ((listed, blocks), (listed[::-1].copy(), blocks[::-1].copy())):
        truth = blocked(held, lst, blk)
        for p, min_degree in ((0, 3), (200, 2)):
            want, (labels, core, merges) = check(m, truth, lst, blk, p, min_degree, cuts=2)
        gone = np.isin(lst, unheld)
        assert (labels[gone] == NO_CLUSTER).all() and (core[gone] == NO_CORE).all() and (labels[~gone] != NO_CLUSTER).all()
        assert not np.isin(merges[:, :2], unheld).any() and len(merges) > 0
    m.close()


def _sized_blocks(refs, sizes, rng):
    """Keys for a shuffled prefix of refs: blocks of the given sizes, their members anywhere among the references, the
    key values in no order."""
    picked = rng.permutation(refs)[:sum(sizes)]
    keys = rng.permutation(np.arange(1000, 1000 + len(sizes), dtype=np.uint32))
    return picked.astype(np.uint32), np.repeat(keys, sizes).astype(np.uint32)


def one_core_tree_per_block(m, listed, blocks, p, min_degree):
    """What one blurrily_storage_cluster_core_tree call per block gives: labels and core heights put back in place, the
    records merged into one list under the total order, the counts summed."""
    labels, core = np.zeros(len(listed), dtype=np.uint32), np.zeros(len(listed), dtype=np.uint32)
    records, sums = [], [0, 0, 0]
    for key in np.unique(blocks):
        own = blocks == key
        labels[own], core[own], rows, *counts = m.cluster_core_tree(listed[own], p, min_degree)
        records.append(rows)
        sums = [x + y for x, y in zip(sums, counts)]
    return (labels, core, merged_records(records), *sums)


def test_blocks_of_every_size_around_the_tile_and_the_workgroup_equal_one_core_tree_call_per_block():
    c = oracle_case("words", 5000)
    m = c["m"]
    sizes = [1, 2, G - 1, G, G + 1, 2 * G + 1, 255, 256, 257, 600]
    # (the seed: tests/test_gpu_cluster_cores_within.py's, under which there are cores and core edges at min_degree 3 too)
    listed, blocks = _sized_blocks(c["listed"], sizes, np.random.default_rng(78))
    truth = blocked_over(c["truth"], listed, blocks)
    for min_degree in (2, 3):
        want, (labels, core, merges) = check(m, truth, listed, blocks, 200, min_degree, cuts=3)
        assert want.n_core_edges >= 1 and len(merges) >= 1
        whole = one_core_tree_per_block(m, listed, blocks, 200, min_degree)
        for s in STRATEGIES:
            same_bytes(call(m, listed, blocks, 200, min_degree, s), whole, (s, min_degree))
        by_block = RawMap.tree_by_block(merges, listed, blocks)
        for key in np.unique(blocks).tolist():
            rows = m.cluster_core_tree(listed[blocks == key], 200, min_degree)[2]
            assert by_block.get(key, np.zeros((0, 3), dtype=np.uint32)).tobytes() == rows.tobytes(), key


def test_a_case_of_several_rounds_launches_each_kernel_once_per_pass_and_round():
    c = oracle_case("words", 5000)
    m, listed, blocks = c["m"], c["listed"], c["blocks"]
    rounds = 3                                                # (tests/test_cluster_core_tree_within_abi.py asserts it of the truth)
    assert m.device_info()["n_pending"] == 0 and len(listed) <= 1 << 20   # (one image, one chunk of needles)
    for s, ran, idle in ((2, DIRECT, SWEEP), (1, SWEEP, DIRECT), (0, DIRECT, SWEEP)):
        call(m, listed, blocks, 200, 2, s)
        names = m.last_kernels()
        # the beginning, the first settle, per height pass the pass and its settle, per round (and the one that finds
        # nothing) the offer, the merge and the flatten, the labels
        assert names == (["cluster_nodes_kernel", SETTLE] + [ran[0], SETTLE] * passes_for(200) +
                         ["cluster_tree_flatten_kernel"] +
                         [ran[1], "cluster_tree_merge_kernel", "cluster_tree_flatten_kernel"] * (rounds + 1) +
                         ["cluster_label_kernel"]), (s, names)
        assert not any(k in names for k in idle + OTHERS), (s, names)


def test_the_list_shuffled_with_repeats_and_absent_references_nothing_listed_and_nothing_held():
    c = oracle_case("words", 5000)
    m, everything = c["m"], c["listed"]
    rng = np.random.default_rng(31)
    absent = np.array([40000, 40001, 99999, 0xFFFFFFFF, 0], dtype=np.uint32)
    mixed = np.concatenate([everything, everything[::7], absent, absent[:2]])
    rng.shuffle(mixed)
    key = lambda refs: (refs % 3).astype(np.uint32)
    base = m.cluster_core_tree_within(everything, key(everything), 200, 2)
    for s in STRATEGIES:
        got = call(m, mixed, key(mixed), 200, 2, s)
        assert got[2].tobytes() == base[2].tobytes() and got[3:] == base[3:], s
        for k, nothing in ((0, NO_CLUSTER), (1, NO_CORE)):
            of = dict(zip(everything.tolist(), base[k].tolist()))
            assert got[k].tolist() == [of.get(int(r), nothing) for r in mixed]   # (repeats equal, absent ones nothing)
            assert (got[k][np.isin(mixed, absent)] == nothing).all()
        # nothing listed; nothing held
        out = call(m, [], [], 500, 2, s)
        assert [x.shape for x in out[:3]] == [(0,), (0,), (0, 3)] and out[3:] == (0, 0, 0)
        for min_degree in (0, 2):
            out = call(m, absent, [1, 1, 1, 2, 2], 0, min_degree, s)
            assert (out[0] == NO_CLUSTER).all() and (out[1] == NO_CORE).all() and out[2].shape == (0, 3)
            assert out[3:] == (0, 0, 0)
    check(m, c["truth"], mixed, key(mixed), 200, 2, least=200, cuts=2)
    assert NO_CLUSTER == _native.NO_CLUSTER and NO_CORE == _native.NO_CORE


def test_a_haystack_of_more_than_one_window_equals_one_core_tree_call_per_key():
    n = 70000
    hay, off = W.words(n, seed=17)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    weights = np.random.default_rng(23).integers(1, 1 << 20, size=n).astype(np.uint32)   # ranks unrelated to length
    m = _map_of(held, weights)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    blocks = (listed % 7).astype(np.uint32)
    whole = one_core_tree_per_block(m, listed, blocks, 300, 3)
    assert m.device_info()["n_windows"] >= 2 and whole[5] > 0
    assert len(whole[2]) >= 3 and len(np.unique(whole[2][:, 2])) >= 3
    for s in (1, 2):
        got = call(m, listed, blocks, 300, 3, s)
        print(f"strategy {s}: {len(got[2])} merges ({len(whole[2])}), clusters, edges, core edges {got[3:]} ({whole[3:]})")
        same_bytes(got, whole, s)
    m.close()


def test_mutations_a_deleted_core_pending_puts_a_reference_put_again_and_the_fold():
    assert [_permille(*xy) for xy in ((H, X1), (H, X2), (H, X3), (X1, X3), (X2, X3))] == [500, 384, 666, 400, 235]
    hay, off = W.words(5000, seed=7)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({9001: X1, 9002: X2, 9003: H, 9004: X3})
    key_of = {r: r % 3 for r in held}
    key_of.update({9001: 1, 9002: 1, 9003: 1, 9004: 1, 123456: 1})
    m = _map_of(held)
    m.sync_device()
    builds = m.device_info()["base_builds"]

    def verify(min_degree=2):
        listed = np.array(sorted(held) + [123456], dtype=np.uint32)
        blocks = np.array([key_of[int(r)] for r in listed], dtype=np.uint32)
        want, (labels, core, merges) = check(m, BlockedTruth(held, key_of), listed, blocks, 300, min_degree, cuts=2)
        return dict(zip(listed.tolist(), core.tolist())), set(map(tuple, merges.tolist())), listed, blocks

    of, rows, _, _ = verify()                                 # X1, H and X3 hang together at 400; X2 has one edge
    assert [of[r] for r in (9001, 9002, 9003, 9004, 123456)] == [400, NO_CORE, 500, 400, NO_CORE]
    assert (9001, 9003, 400) in rows and (9001, 9004, 400) in rows   # (three ties at 400: the first two)
    m.delete(9003)                                            # a core goes: X1 and X3 keep one edge, each other's
    del held[9003]
    of, rows, _, _ = verify()
    assert 9003 not in of and [of[r] for r in (9001, 9002, 9004)] == [NO_CORE] * 3
    assert not any(9003 in r[:2] for r in rows)
    m.put(H, 9500, 0)                                         # pending puts: H again under X1's key, in the delta image ...
    m.put(H + b"x", 9501, 0)                                  # ... with a neighbour there
    m.put(H, 9502, 0)                                         # and the same two under another key: these join nothing
    m.put(H + b"x", 9503, 0)                                  # there, and have each other alone
    held.update({9500: H, 9501: H + b"x", 9502: H, 9503: H + b"x"})
    key_of.update({9500: 1, 9501: 1, 9502: 2, 9503: 2})
    of, rows, listed, blocks = verify()
    assert m.device_info()["n_pending"] >= 4 and m.device_info()["base_builds"] == builds
    assert [of[r] for r in (9001, 9002, 9004, 9500, 9501, 9502, 9503)] == [461, NO_CORE, 625, 666, 625, NO_CORE, NO_CORE]
    assert not any((r[0] in (9502, 9503)) != (r[1] in (9502, 9503)) for r in rows)
    call(m, listed, blocks, 300, 2, 1)
    names = m.last_kernels()
    assert names.count(SWEEP[0]) == passes_for(300) * 2       # (two images: the base and the pending puts)
    assert names.count(SWEEP[1]) == names.count("cluster_tree_merge_kernel") * 2
    verify(min_degree=1)
    m.delete(16)                                              # deleted and put again with another text (16 % 3 == 1)
    m.put(X2 + b"u", 16, 0)
    held[16] = X2 + b"u"
    of, rows, _, _ = verify()
    assert of[16] == NO_CORE and of[9002] != NO_CORE          # (X2 has H's two copies' and this one's edges now)
    big, bo = W.words(9000, seed=34)                          # a log past its budget folds into a rebuilt base image
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    key_of.update({r: r % 3 for r in bulk.tolist()})
    again, _, _, _ = verify()
    info = m.device_info()
    assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    assert [again[r] for r in (9001, 9002, 9004, 9500, 16)] == [of[r] for r in (9001, 9002, 9004, 9500, 16)]
    m.close()


@pytest.fixture(scope="module")
def dense():
    m, h = D.build()
    c = DT.inputs(h)
    c.m, c.h = m, h
    yield c
    m.close()


@pytest.mark.parametrize("name", ["short", "long"])
def test_the_dense_slice_map_under_the_sweep_and_direct(dense, name):
    """tests/dense_case.py's map: more than 64 dense slices for a (needle, window), the largest left out of the count and
    asked about in their bitmaps, wide needles over two half windows.  The new sweep kernel leaves dense slices out as its
    parents do: strategy 1 against strategy 2 and both against the truth."""
    m, listed = dense.m, dense.lists[name]
    blocks = DT.key_pairs(listed)
    truth = blocked_over(dense.h.truth, listed, blocks)
    edges = []
    for p in (200, 350, 600):
        want, (labels, core, merges) = check(m, truth, listed, blocks, p, 2, least=DT.LEAST, cuts=0, strategies=(1, 2))
        edges.append(want.n_edges)
        for s, ran, idle in ((1, SWEEP, DIRECT), (2, DIRECT, SWEEP)):
            call(m, listed, blocks, p, 2, s)
            names = m.last_kernels()
            assert all(k in names for k in ran) and not any(k in names for k in idle), (s, names)
    assert edges[0] > edges[-1] > 0 and want.n_core_edges > 0 and len(merges) > 0


def test_three_calls_give_identical_bytes():
    c = oracle_case("words", 5000)
    m, listed, blocks = c["m"], c["listed"], c["blocks"]
    for s in STRATEGIES:
        for p, min_degree in ((100, 5), (200, 2)):
            one, two, three = (call(m, listed, blocks, p, min_degree, s) for _ in range(3))
            same_bytes(one, two, (s, p))
            same_bytes(one, three, (s, p))
            assert len(one[2]) >= 3


def test_the_calls_around_a_call_are_unchanged():
    c = oracle_case("words", 5000)
    m, listed, blocks = c["m"], c["listed"], c["blocks"]
    packed, offsets = _pack(c["needles"])
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    find_kernels = m.last_kernels()
    around = [(lambda: m.cluster_tree_within(listed, blocks, 200)), (lambda: m.cluster_cores_within(listed, blocks, 200, 3)),
              (lambda: m.cluster_core_tree(listed, 200, 2))]
    before = []
    for one in around:
        result = one()
        before.append((result, m.last_kernels()))
    for s in STRATEGIES:
        call(m, listed, blocks, 200, 2, s)
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == find_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    for one, (was, was_kernels) in zip(around, before):
        now = one()
        assert m.last_kernels() == was_kernels
        for x, y in zip(was, now):
            assert x.tobytes() == y.tobytes() if isinstance(x, np.ndarray) else x == y


def test_auto_sweeps_a_block_above_the_direct_cap_and_scores_the_others_into_the_same_words():
    cap = 100000                                              # cluster_plan.h: kClusterWithinDirectMax
    n = 2 * cap + 301
    hay, off = W.geonames(n, 2000, 41)
    m = _map_of({i + 1: s for i, s in enumerate(W.unpack(hay, off))})
    listed = np.arange(1, n + 1, dtype=np.uint32)
    # interleaving blocks of cap + 1 (swept), cap (the largest scored directly) and 300 members
    blocks = np.where(listed > 2 * cap + 1, 9, listed % 2).astype(np.uint32)
    assert [(blocks == k).sum() for k in (1, 0, 9)] == [cap + 1, cap, 300]
    results = {}
    for s, kernels in ((0, set(DIRECT + SWEEP)), (1, set(SWEEP)), (2, set(DIRECT))):
        results[s] = call(m, listed, blocks, 700, 3, s)
        assert {k for k in m.last_kernels() if k.startswith("cluster_core_tree_within")} == kernels, s
    for s in (1, 2):
        same_bytes(results[s], results[0], s)
    labels, core, merges, n_clusters, n_edges, n_core_edges = results[0]
    cores = int((core != NO_CORE).sum())
    assert n_edges > n_core_edges > 0 and 0 < n_clusters < cores < n and len(merges) == cores - n_clusters
    big = merges[:, 1] <= 2 * cap + 1                           # (the two large blocks are the odd and the even references)
    assert (merges[big, 0] % 2 == merges[big, 1] % 2).all() and (merges[~big, 0] > 2 * cap + 1).all()
    assert m.cluster_within(listed, blocks, 700)[2] == n_edges
    assert m.cluster_cores_within(listed, blocks, 700, 3)[3:] == (n_clusters, n_edges, n_core_edges)
    # one member fewer in the swept block: every block is scored directly
    m.cluster_core_tree_within(listed[2:], blocks[2:], 700, 3)
    assert not any(k in m.last_kernels() for k in SWEEP) and all(k in m.last_kernels() for k in DIRECT)
    m.close()
