"""Cluster cores within blocks on the GPU (cluster_cores_within.hip, cluster_cores_within_kernels.hip):
blurrily_storage_cluster_cores' labels, degrees, kinds and three counts where an edge also needs both ends under one
block key.  Everything is compared byte for byte with the host's truth (cluster_cores_within_truth.py: cluster_cores_truth's
edges kept where the keys agree, nothing of the library) under "scope_strategy" 0 (auto), 1 (every block swept) and 2
(every block scored directly): the oracle haystacks under interleaving keys with the figures of the issue, the
identities (all keys equal, min_degree 0, all keys distinct, one cluster_cores call per block, the degrees off the edge
records), built cases (a bridge in another block, a border between two clusters and its anchor moved away, a core that
loses neighbours to another key, edges exactly at their floor, the counter widths with twins inside and outside a block,
the empty string, an unheld member), block sizes around the direct kernel's tile and workgroup, a shuffled list, a
haystack of more than one window, mutations, tests/dense_case.py's map, repeated calls, the calls around a call, the
kernels' names, and a block above the direct cap beside smaller ones."""
import copy

import numpy as np
import pytest

import dense_case as D
import dense_truths as DT
import workloads as W
from blurrily_amd import _native
from cluster_cores_truth import BORDER, CORE, NOISE, NONE
from cluster_cores_within_truth import CoresWithinEdges, dense_lists
from cluster_truth import NO_CLUSTER
from cluster_within_truth import WithinTruth
from helpers import oracle_case_inputs
from test_gpu_cluster import A, B, _j, _map_of, built_case
from test_gpu_cluster_cores import H, N, S, X1, X2, X3, _permille

pytestmark = pytest.mark.gpu
STRATEGIES = (0, 1, 2)                                        # "scope_strategy": auto, the sweep, the direct kernel
G = 16                                                        # the direct kernel's tile (cluster_plan.h: kClusterWithinTile)
DIRECT = ["cluster_cores_within_kernel", "cluster_cores_within_kernel<unite>"]
SWEEP = ["cluster_cores_within_sweep_kernel", "cluster_cores_within_sweep_kernel<unite>"]


def edges_of(truth, listed, blocks, p, least=0):
    e = CoresWithinEdges(truth, listed, blocks, p, least)
    e.p, e.blocks = p, np.asarray(blocks, dtype=np.uint32)
    return e


def same_bytes(one, other, what=None):
    for k in range(3):
        assert one[k].dtype == other[k].dtype and one[k].tobytes() == other[k].tobytes(), (what, k)
    assert tuple(one[3:]) == tuple(other[3:]), (what, one[3:], other[3:])


def check(m, e, min_degree, strategies=STRATEGIES):
    """One call per strategy against the truth (`e`: the list, its keys and the floor), exactly.  Returns the truth."""
    listed, p = np.array(e.listed, dtype=np.uint32), e.p
    want = e.cores(min_degree)
    for s in strategies:
        m.set_option("scope_strategy", s)
        try:
            labels, degrees, kinds, n_clusters, n_edges, n_core_edges = m.cluster_cores_within(listed, e.blocks, p, min_degree)
        finally:
            m.set_option("scope_strategy", 0)
        print(f"floor {p}, min_degree {min_degree}, strategy {s}: {len(want.label_of)} nodes, clusters {n_clusters} "
              f"(truth {want.n_clusters}), edges {n_edges} (truth {want.n_edges}), core edges {n_core_edges} (truth "
              f"{want.n_core_edges}), cores, borders, noise {[int((kinds == k).sum()) for k in (CORE, BORDER, NOISE)]} "
              f"(truth {[int((want.kinds == k).sum()) for k in (CORE, BORDER, NOISE)]})")
        at = (p, min_degree, s)
        assert n_edges == want.n_edges, at
        assert n_core_edges == want.n_core_edges, at
        assert n_clusters == want.n_clusters, at
        assert degrees.dtype == np.uint32 and np.array_equal(degrees, want.degrees), at
        assert kinds.dtype == np.uint8 and np.array_equal(kinds, want.kinds), at
        assert labels.dtype == np.uint32 and np.array_equal(labels, want.labels), at
        _, first = np.unique(listed, return_index=True)         # (a reference listed twice is one node)
        assert int(degrees[first].sum(dtype=np.uint64)) == 2 * n_edges, at
    return want


def answers(m, listed, blocks, p, min_degree):
    """The call under every strategy, the three the same: as plain lists and numbers."""
    got = []
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        try:
            out = m.cluster_cores_within(listed, blocks, p, min_degree)
        finally:
            m.set_option("scope_strategy", 0)
        got.append((out[0].tolist(), out[1].tolist(), out[2].tolist(), out[3], out[4], out[5]))
    assert got[0] == got[1] == got[2], (p, min_degree)
    return got[0]


_CASES = {}


def oracle_case(kind, n):
    """The map and the truth of an oracle haystack, made once."""
    if (kind, n) not in _CASES:
        hay, off, needles = oracle_case_inputs(kind, n)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        _CASES[kind, n] = dict(m=_map_of(held), truth=WithinTruth(held), needles=needles,
                               listed=np.arange(1, n + 1, dtype=np.uint32))
    return _CASES[kind, n]


# (haystack, n, modulus, floor, min_degree: (edges, core edges, clusters)): the figures of the issue, which
# tests/test_cluster_cores_within_abi.py asserts of the truth with the rest of the table
TABLE = [("words", 5000, 3, 200, {3: (873, 102, 55), 2: (873, 311, 134)}),
         ("geonames", 8000, 3, 500, {5: (72710, 70270, 74), 2: (72710, 72060, 246), 3: (72710, 71434, 135)}),
         ("geonames", 8000, 64, 300, {3: (13206, 11624, 168)}),
         ("skewed", 6000, 3, 500, {3: (640, 84, 41)})]


@pytest.mark.parametrize("kind,n,modulus,p,figures", TABLE, ids=[f"{c[0]}-{c[2]}-{c[3]}" for c in TABLE])
def test_everything_equals_the_truth_on_the_oracle_haystacks_under_interleaving_keys(kind, n, modulus, p, figures):
    c = oracle_case(kind, n)
    m, listed = c["m"], c["listed"]
    e = edges_of(c["truth"], listed, listed % modulus, p, least=p)
    for min_degree, (edges, core_edges, clusters) in figures.items():
        want = check(m, e, min_degree)
        assert (want.n_edges, want.n_core_edges, want.n_clusters) == (edges, core_edges, clusters)
        if min_degree == next(iter(figures)):                   # (the table's row: a telling case)
            assert min(want.big_clusters, want.n_borders, want.noise_with_an_edge, want.torn_borders) >= 1
        member = want.kinds >= BORDER
        assert (want.labels[member] % modulus == listed[member] % modulus).all()   # (no cluster reaches across a key)


def test_the_identities_equal_keys_min_degree_0_distinct_keys_and_the_degrees_off_the_edge_records():
    c = oracle_case("words", 5000)
    m, everything = c["m"], c["listed"]
    blocks = everything % 3
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        for p, min_degree in ((200, 3), (300, 2)):
            # all keys equal: every output is cluster_cores' byte for byte
            want = m.cluster_cores(everything, p, min_degree)
            got = m.cluster_cores_within(everything, np.full(len(everything), 0xFFFFFFFF, dtype=np.uint32), p, min_degree)
            same_bytes(got, want, (s, p))
            assert want[5] > 0 and len({CORE, BORDER, NOISE} & set(want[2].tolist())) == 3
            # min_degree 0: cluster_within's labels, clusters and edges; every node a core
            w_labels, w_clusters, w_edges = m.cluster_within(everything, blocks, p)
            labels, degrees, kinds, n_clusters, n_edges, n_core_edges = m.cluster_cores_within(everything, blocks, p, 0)
            assert labels.tobytes() == w_labels.tobytes() and (n_clusters, n_edges) == (w_clusters, w_edges)
            assert n_core_edges == n_edges > 0 and (kinds == CORE).all()
            # the degrees read off cluster_edges_within's records at the same floor
            records = m.cluster_edges(everything, p, blocks=blocks)
            counted = np.bincount(records[:, :2].astype(np.int64).ravel(), minlength=len(everything) + 1)[1:]
            assert len(records) == n_edges and np.array_equal(degrees, counted.astype(np.uint32))
        # all keys distinct: every held reference its own label with degree 0
        some = np.concatenate([everything[:700], [888888]]).astype(np.uint32)
        for min_degree, kind, clusters in ((0, CORE, 700), (1, NOISE, 0), (3, NOISE, 0)):
            labels, degrees, kinds, n_clusters, n_edges, n_core_edges = m.cluster_cores_within(some, some[::-1].copy(), 0, min_degree)
            assert labels.tolist() == some[:700].tolist() + [NO_CLUSTER] and not degrees.any()
            assert kinds.tolist() == [kind] * 700 + [NONE] and (n_clusters, n_edges, n_core_edges) == (clusters, 0, 0)
    m.set_option("scope_strategy", 0)
    # nothing listed; nothing held
    out = m.cluster_cores_within([], [], 500, 3)
    assert [a.shape for a in out[:3]] == [(0,)] * 3 and out[3:] == (0, 0, 0)
    absent = np.array([40000, 40001, 99999, 0xFFFFFFFF, 0], dtype=np.uint32)
    out = m.cluster_cores_within(absent, [1, 1, 1, 2, 2], 0, 0)
    assert (out[0] == NO_CLUSTER).all() and not out[1].any() and (out[2] == NONE).all() and out[3:] == (0, 0, 0)


def test_a_bridge_in_another_block_and_a_core_that_loses_neighbours_to_another_key():
    A1, A2, A3, Br, C1, C2, C3 = S[0], S[0] + b"z", S[0] + S[1], S[1] + S[2], S[2] + S[3], S[3], S[3] + b"pq"
    held = {i + 1: s for i, s in enumerate([A1, A2, A3, Br, C1, C2, C3])}
    m, truth = _map_of(held), WithinTruth(held)
    listed = [1, 2, 3, 4, 5, 6, 7]
    one = [1] * 7
    # all under one key: cluster_cores' answers (tests/test_gpu_cluster_cores.py)
    assert answers(m, listed, one, 1, 3) == ([3, 3, 3, 3, 5, 5, 5], [2, 2, 3, 2, 3, 2, 2], [2, 2, 3, 2, 3, 2, 2], 2, 8, 0)
    assert answers(m, listed, one, 1, 2) == ([1] * 7, [2, 2, 3, 2, 3, 2, 2], [3] * 7, 1, 8, 8)
    # the bridge in another block: it joins nothing and adds to nobody's degree; each triangle is a cluster of its own
    away = [1, 1, 1, 2, 1, 1, 1]
    assert answers(m, listed, away, 1, 2) == ([1, 1, 1, 4, 5, 5, 5], [2, 2, 2, 0, 2, 2, 2], [3, 3, 3, 1, 3, 3, 3], 2, 6, 6)
    assert answers(m, listed, away, 1, 3) == (listed, [2, 2, 2, 0, 2, 2, 2], [1] * 7, 0, 6, 0)
    # the second triangle in another block: the bridge, a core of two edges at min_degree 2, keeps one and is a border
    split = [1, 1, 1, 1, 2, 2, 2]
    assert answers(m, listed, split, 1, 2) == ([1, 1, 1, 1, 5, 5, 5], [2, 2, 3, 1, 2, 2, 2], [3, 3, 3, 2, 3, 3, 3], 2, 7, 6)
    assert answers(m, listed, split, 1, 3) == ([3, 3, 3, 3, 5, 6, 7], [2, 2, 3, 1, 2, 2, 2], [2, 2, 3, 2, 1, 1, 1], 1, 7, 0)
    for blocks in (one, away, split):
        e = edges_of(truth, listed, blocks, 1)
        for min_degree in (0, 1, 2, 3, 4):
            check(m, e, min_degree)
    assert m.dense_duplicates_within([7, 6, 5, 4, 3, 2, 1, 1], [2, 2, 2, 1, 1, 1, 1, 1], 1, 3) == [[1, 2, 3, 4]]
    assert m.dense_duplicates_within(listed, split, 1, 2) == [[1, 2, 3, 4], [5, 6, 7]]
    m.close()
    # the hub: H has three edges at 300 and is the one core at min_degree 3; with X2 under another key it has two, nothing
    # is a core, and everything is noise
    assert [_permille(*xy) for xy in ((H, X1), (H, X2), (H, X3), (X1, X3), (X2, X3))] == [500, 384, 666, 400, 235]
    held = {1: X1, 2: X2, 3: H, 4: X3}
    m, truth = _map_of(held), WithinTruth(held)
    assert answers(m, [1, 2, 3, 4], [5, 5, 5, 5], 300, 3) == ([3, 3, 3, 3], [2, 1, 3, 2], [2, 2, 3, 2], 1, 4, 0)
    assert answers(m, [1, 2, 3, 4], [5, 6, 5, 5], 300, 3) == ([1, 2, 3, 4], [2, 0, 2, 2], [1, 1, 1, 1], 0, 3, 0)
    assert answers(m, [1, 2, 3, 4], [5, 6, 5, 5], 300, 2) == ([1, 2, 1, 1], [2, 0, 2, 2], [3, 1, 3, 3], 1, 3, 3)
    for blocks in ([5, 5, 5, 5], [5, 6, 5, 5], [5, 6, 6, 5]):
        for min_degree in (1, 2, 3):
            check(m, edges_of(truth, [1, 2, 3, 4], blocks, 300), min_degree)
    m.close()


def test_a_border_between_two_clusters_its_tie_and_its_better_anchor_moved_to_another_key():
    P1, P2, P3, X = S[0] + S[1], S[0], S[0] + b"z", S[1] + S[2]
    Q1, Q2, Q3, Q4 = S[2] + S[3], S[3], S[3] + b"pq", S[3] + b"rp"
    held = {i + 1: s for i, s in enumerate([P1, P2, P3, X, Q1, Q2, Q3, Q4])}
    m, truth = _map_of(held), WithinTruth(held)
    listed = sorted(held)
    # P1 has three edges, Q1 four: X, a border of degree 2, goes to Q1's cluster (label 5, its smallest core)
    one = [9] * 8
    assert answers(m, listed, one, 1, 3) == ([1, 1, 1, 5, 5, 5, 5, 5], [3, 2, 2, 2, 4, 3, 3, 3], [3, 2, 2, 2, 3, 3, 3, 3], 2, 11, 6)
    assert check(m, edges_of(truth, listed, one, 1), 3).torn_borders == 1
    # Q1 under another key: X keeps P1 alone and goes there; Q1 has no edge, and what it held together is noise
    moved = [9, 9, 9, 9, 4, 9, 9, 9]
    assert answers(m, listed, moved, 1, 3) == ([1, 1, 1, 1, 5, 6, 7, 8], [3, 2, 2, 1, 0, 2, 2, 2], [3, 2, 2, 2, 1, 1, 1, 1], 1, 7, 0)
    # Q4 under another key: P1 and Q1 tie at degree 3, and the smaller reference, P1, wins
    tie = [9, 9, 9, 9, 9, 9, 9, 4]
    assert answers(m, listed, tie, 1, 3) == ([1, 1, 1, 1, 5, 5, 5, 8], [3, 2, 2, 2, 3, 2, 2, 0], [3, 2, 2, 2, 3, 2, 2, 1], 2, 8, 0)
    for blocks in (moved, tie):
        for min_degree in (2, 3):
            check(m, edges_of(truth, listed, blocks, 1), min_degree)
    m.close()
    # the same strings with P1 and Q1 under each other's reference: the tie falls the other way
    held[1], held[5] = Q1, P1
    m, truth = _map_of(held), WithinTruth(held)
    assert answers(m, listed, tie, 1, 3) == ([1, 5, 5, 1, 5, 1, 1, 8], [3, 2, 2, 2, 3, 2, 2, 0], [3, 2, 2, 2, 3, 2, 2, 1], 2, 8, 0)
    check(m, edges_of(truth, listed, tie, 1), 3)
    m.close()


def test_edges_exactly_at_their_floor_the_counter_widths_twins_inside_and_outside_a_block_and_the_empty_string():
    held = built_case()
    held.update({5004: B[:-1], 5005: A[:-1]})                 # 7 / 15 against each other: 466 permille
    assert _j(A, B) == (8, 16) and _j(A[:-1], B[:-1]) == (7, 15)
    sizes = (15, 16, 255, 256, 700)
    for i in range(len(sizes)):                               # a third twin of each sized node, and of the empty string
        held[6100 + i] = held[6000 + 4 * i]
    held[7003] = b""
    m, truth = _map_of(held), WithinTruth(held)
    # exactly at the floor and one permille above, in one block and split across two, at min_degree 1
    for pair, at in (([5001, 5002], 500), ([5004, 5005], 466)):
        assert answers(m, pair, [3, 3], at, 1) == ([pair[0], pair[0]], [1, 1], [3, 3], 1, 1, 1)
        assert answers(m, pair, [3, 3], at + 1, 1) == (pair, [0, 0], [1, 1], 0, 0, 0)
        assert answers(m, pair, [3, 8], at, 1) == (pair, [0, 0], [1, 1], 0, 0, 0)
        assert answers(m, pair, [3, 8], at + 1, 1) == (pair, [0, 0], [1, 1], 0, 0, 0)
    # the words under three interleaving keys; the built nodes under key 7, the third twins under key 8
    everything = np.array(sorted(held), dtype=np.uint32)
    blocks = np.where(everything > 5000, 7, everything % 3).astype(np.uint32)
    blocks[np.isin(everything, [6100 + i for i in range(len(sizes))] + [7003])] = 8
    for p, min_degree in ((200, 2), (466, 1), (467, 1), (500, 1), (501, 1), (1000, 1), (1000, 2)):
        want = check(m, edges_of(truth, everything, blocks, p), min_degree)
    assert min_degree == 2 and p == 1000                      # (the last: equal strings alone are edges)
    for i, t in enumerate(sizes):
        a, b, away = 6000 + 4 * i, 6001 + 4 * i, 6100 + i
        assert len(truth.codes[truth.refs.tolist().index(a)]) == t
        assert (want.degree_of[a], want.degree_of[b], want.degree_of[away]) == (1, 1, 0)
        assert want.kind_of[away] == NOISE and want.label_of[away] == away
    want = check(m, edges_of(truth, everything, blocks, 1000), 1)
    for a, b, away in [(6000 + 4 * i, 6001 + 4 * i, 6100 + i) for i in range(len(sizes))] + [(7001, 7002, 7003)]:
        assert (want.label_of[a], want.label_of[b], want.label_of[away]) == (a, a, away)
        assert (want.kind_of[a], want.kind_of[b], want.kind_of[away]) == (CORE, CORE, NOISE)
    m.close()


def test_an_unheld_reference_in_the_middle_of_a_block():
    hay, off = W.words(600, seed=3)
    held = {10 * (i + 1): s for i, s in enumerate(W.unpack(hay, off))}
    m, truth = _map_of(held), WithinTruth(held)
    unheld = [15, 3005, 3015, 5995]
    listed = np.array(sorted(list(held) + unheld), dtype=np.uint32)
    blocks = ((listed // 10) % 2).astype(np.uint32)
    for lst, blk in ((listed, blocks), (listed[::-1].copy(), blocks[::-1].copy())):
        for p, min_degree in ((0, 3), (200, 2)):
            want = check(m, edges_of(truth, lst, blk, p), min_degree)
        gone = np.isin(lst, unheld)
        assert (want.labels[gone] == NO_CLUSTER).all() and (want.kinds[gone] == NONE).all() and not want.degrees[gone].any()
        assert (want.kinds != NONE).sum() == 600 and (want.kinds == CORE).any()
    m.close()


def _sized_blocks(refs, sizes, rng):
    """Keys for a shuffled prefix of refs: blocks of the given sizes, their members anywhere among the references, the
    key values in no order."""
    picked = rng.permutation(refs)[:sum(sizes)]
    keys = rng.permutation(np.arange(1000, 1000 + len(sizes), dtype=np.uint32))
    return picked.astype(np.uint32), np.repeat(keys, sizes).astype(np.uint32)


def test_blocks_of_every_size_around_the_tile_and_the_workgroup_equal_one_cores_call_per_block():
    c = oracle_case("words", 5000)
    m, truth = c["m"], c["truth"]
    sizes = [1, 2, G - 1, G, G + 1, 2 * G + 1, 255, 256, 257, 600]
    # (the seed: one of those under which the truth has cores, core edges and borders at min_degree 3 too)
    listed, blocks = _sized_blocks(c["listed"], sizes, np.random.default_rng(78))
    e = edges_of(truth, listed, blocks, 200)
    for min_degree in (2, 3):
        want = check(m, e, min_degree)
        assert want.n_core_edges >= 1 and want.n_borders >= 1
        # the direct kernel's tiles: G consecutive members of a block, ascending by reference.  In unite mode one of
        # them has needles of degree 0 only (it returns), one holds a core beside a needle that is none
        none_with_an_edge = mixed = 0
        for key in np.unique(blocks):
            members = np.sort(listed[blocks == key])
            for f in range(0, len(members), G):
                degrees = [want.degree_of[int(r)] for r in members[f:f + G]]
                cores = [d >= min_degree for d in degrees]
                none_with_an_edge += not any(degrees)
                mixed += any(cores) and not all(cores)
        print(f"min_degree {min_degree}: {none_with_an_edge} tiles without an edge, {mixed} with a core and a needle that is none")
        assert none_with_an_edge >= 1 and mixed >= 1
        # ... and equal to one cluster_cores call per block put back, the counts summed
        for s in STRATEGIES:
            m.set_option("scope_strategy", s)
            got = m.cluster_cores_within(listed, blocks, 200, min_degree)
            m.set_option("scope_strategy", 0)
            sums = [0, 0, 0]
            for key in np.unique(blocks):
                own = blocks == key
                one = m.cluster_cores(listed[own], 200, min_degree)
                for k in range(3):
                    assert np.array_equal(got[k][own], one[k]), (s, int(key), k)
                sums = [x + y for x, y in zip(sums, one[3:])]
            assert tuple(sums) == got[3:], s


def test_the_list_shuffled_with_repeats_and_absent_references_and_dense_duplicates_within():
    c = oracle_case("words", 5000)
    m, truth, everything = c["m"], c["truth"], c["listed"]
    rng = np.random.default_rng(31)
    absent = np.array([40000, 40001, 99999, 0xFFFFFFFF, 0], dtype=np.uint32)
    mixed = np.concatenate([everything, everything[::7], absent, absent[:2]])
    rng.shuffle(mixed)
    key = lambda refs: (refs % 5).astype(np.uint32)
    base = m.cluster_cores_within(everything, key(everything), 200, 3)
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        got = m.cluster_cores_within(mixed, key(mixed), 200, 3)
        m.set_option("scope_strategy", 0)
        assert got[3:] == base[3:]
        for k, nothing in ((0, NO_CLUSTER), (1, 0), (2, NONE)):
            of = dict(zip(everything.tolist(), base[k].tolist()))
            assert got[k].tolist() == [of.get(int(r), nothing) for r in mixed]   # (repeats equal, absent ones nothing)
            assert (got[k][np.isin(mixed, absent)] == nothing).all()
    want = check(m, edges_of(truth, mixed, key(mixed), 200), 3)
    lists = dense_lists(want)
    assert lists and any(len(g) >= 3 for g in lists) and all(len({r % 5 for r in g}) == 1 for g in lists)
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        assert m.dense_duplicates_within(mixed, key(mixed), 200, 3) == lists
        assert m.dense_duplicates_within(everything, key(everything), 200, 3) == lists
    m.set_option("scope_strategy", 0)


def test_a_haystack_of_more_than_one_window_equals_one_cores_call_per_key_and_crosses_the_window_boundary():
    n = 70000
    hay, off = W.words(n, seed=17)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    weights = np.random.default_rng(23).integers(1, 1 << 20, size=n).astype(np.uint32)   # ranks unrelated to length
    m = _map_of(held, weights)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    blocks = listed % 7
    p, min_degree = 300, 3
    want = [np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)]
    sums = [0, 0, 0]
    for key in range(7):
        own = blocks == key
        one = m.cluster_cores(listed[own], p, min_degree)
        for k in range(3):
            want[k][own] = one[k]
        sums = [x + y for x, y in zip(sums, one[3:])]
    assert m.device_info()["n_windows"] >= 2 and sums[2] > 0
    plain = m.cluster_cores(listed, p, min_degree)
    assert plain[4] > sums[1] and plain[5] > sums[2]             # (the keys cut edges)
    for s in (1, 2):
        m.set_option("scope_strategy", s)
        got = m.cluster_cores_within(listed, blocks, p, min_degree)
        m.set_option("scope_strategy", 0)
        print(f"strategy {s}: clusters, edges, core edges {got[3:]} ({sums})")
        same_bytes(got, (*want, *sums), s)
    # from the results and the edge records: core edges and anchors with their two ends in different windows, the end
    # at the higher reference (and the border) on either side
    labels, degrees, kinds = (x.astype(np.int64) for x in got[:3])
    loc = D.locate(listed, weights)
    window = np.array([loc[int(r)][0] for r in listed], dtype=np.int64)
    records = m.cluster_edges(listed, p, blocks=blocks).astype(np.int64)
    a, b = records[:, 0] - 1, records[:, 1] - 1                 # (reference r is element r - 1)
    both = (kinds[a] == CORE) & (kinds[b] == CORE)
    assert int(both.sum()) == got[5]
    assert ((window[a] == 0) & (window[b] == 1) & both).any() and ((window[a] == 1) & (window[b] == 0) & both).any()
    one = (kinds[a] == CORE) != (kinds[b] == CORE)
    x = np.where(kinds[a[one]] == CORE, b[one], a[one])           # the end that is no core
    core = np.where(kinds[a[one]] == CORE, a[one], b[one])
    best = np.zeros(n, dtype=np.int64)
    np.maximum.at(best, x, degrees[core] * (n + 1) + (n - core))
    border = np.flatnonzero(kinds == BORDER)
    anchor = n - best[border] % (n + 1)
    assert len(border) and (best[border] > 0).all() and np.array_equal(labels[border], labels[anchor])
    assert ((window[border] == 0) & (window[anchor] == 1)).any() and ((window[border] == 1) & (window[anchor] == 0)).any()
    m.close()


def test_mutations_a_deleted_core_pending_puts_a_reference_put_again_and_the_fold():
    assert [_permille(*xy) for xy in ((H, X1), (H, X2), (H, X3), (X1, X3), (X2, X3))] == [500, 384, 666, 400, 235]
    assert _j(X1, X2)[0] == 0 and [_permille(N, y) for y in (H, X2, X3, X1)] == [615, 416, 411, 214]
    hay, off = W.words(5000, seed=7)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({9001: X1, 9002: X2, 9003: H, 9004: X3})
    key_of = {r: r % 3 for r in held}
    key_of.update({9001: 1, 9002: 1, 9003: 1, 9004: 1, 123456: 1})
    m = _map_of(held)
    m.sync_device()
    builds = m.device_info()["base_builds"]
    ours = (9001, 9002, 9003, 9004, 9500, 9501, 9502, 9503)

    def verify():
        truth = WithinTruth(held)
        listed = np.array(sorted(held) + [123456], dtype=np.uint32)
        blocks = np.array([key_of[int(r)] for r in listed], dtype=np.uint32)
        want = check(m, edges_of(truth, listed, blocks, 300), 2)
        return want, [want.kind_of.get(r, NONE) for r in ours], [want.label_of.get(r) for r in ours]

    want, kinds, labels = verify()                            # X1, H and X3 are cores of one cluster, X2 its border
    assert [want.degree_of[r] for r in ours[:4]] == [2, 1, 3, 2]
    assert kinds[:4] == [CORE, BORDER, CORE, CORE] and labels[:4] == [9001] * 4
    m.delete(9003)                                            # a core goes: X1 and X3 keep one edge and are cores no more
    del held[9003]
    want, kinds, labels = verify()
    assert [want.degree_of[r] for r in (9001, 9002, 9004)] == [1, 0, 1]
    assert kinds[:4] == [NOISE, NOISE, NONE, NOISE] and labels[:4] == [9001, 9002, None, 9004]
    m.put(H, 9500, 0)                                         # pending puts under X2's key: a second edge makes it a core
    m.put(N, 9501, 0)
    m.put(H, 9502, 0)                                         # ... and under another key: they join nothing there and have
    m.put(N, 9503, 0)                                         # one edge, each other's, so they are noise
    held.update({9500: H, 9501: N, 9502: H, 9503: N})
    key_of.update({9500: 1, 9501: 1, 9502: 2, 9503: 2})
    want, kinds, labels = verify()
    assert m.device_info()["n_pending"] >= 4 and m.device_info()["base_builds"] == builds
    assert [want.degree_of[r] for r in (9001, 9002, 9004, 9500, 9501, 9502, 9503)] == [2, 2, 3, 4, 3, 1, 1]
    assert kinds == [CORE, CORE, NONE, CORE, CORE, CORE, NOISE, NOISE]
    assert labels == [9001, 9001, None, 9001, 9001, 9001, 9502, 9503]
    m.delete(16)                                              # deleted and put again with another text (16 % 3 == 1)
    m.put(X2 + b"u", 16, 0)
    held[16] = X2 + b"u"
    want, kinds, labels = verify()
    assert want.degree_of[16] == 1 and want.kind_of[16] == BORDER and want.label_of[16] == 9001   # (X2's, now of degree 3)
    assert want.degree_of[9002] == 3 and labels[:2] == [9001, 9001]
    big, bo = W.words(9000, seed=34)                          # a log past its budget folds into a rebuilt base image
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    key_of.update({r: r % 3 for r in bulk.tolist()})
    again, kinds_again, labels_again = verify()
    info = m.device_info()
    assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    assert kinds_again == kinds and labels_again == labels
    m.close()


@pytest.fixture(scope="module")
def dense():
    m, h = D.build()
    c = DT.inputs(h)
    base = WithinTruth(h.held)
    c.m, c._truth = m, {}

    def truth(name):
        """A truth per list (a Truth keeps one list's pairs), the tokenisation shared."""
        if name not in c._truth:
            c._truth[name] = copy.copy(base)
            c._truth[name]._pairs = {}
        return c._truth[name]

    c.truth = truth
    yield c
    m.close()


@pytest.mark.parametrize("name", ["short", "long"])
def test_the_dense_slice_map_under_the_sweep_and_direct(dense, name):
    """tests/dense_case.py's map: more than 64 dense slices for a (needle, window), the largest left out of the count and
    asked about in their bitmaps, wide needles over two half windows.  The new sweep kernel leaves dense slices out as its
    parents do: strategy 1 against strategy 2 and both against the truth."""
    m, listed = dense.m, dense.lists[name]
    blocks = DT.key_pairs(listed)
    edges = []
    for p in (200, 350, 600):
        e = edges_of(dense.truth(name), listed, blocks, p, least=DT.LEAST)
        want = check(m, e, 2, strategies=(1, 2))
        edges.append(want.n_edges)
        for s, ran, idle in ((1, SWEEP, DIRECT), (2, DIRECT, SWEEP)):
            m.set_option("scope_strategy", s)
            m.cluster_cores_within(listed, blocks, p, 2)
            names = m.last_kernels()
            m.set_option("scope_strategy", 0)
            assert all(k in names for k in ran) and not any(k in names for k in idle), (s, names)
    assert edges[0] > edges[-1] > 0 and want.n_core_edges > 0


def test_three_calls_give_identical_bytes():
    c = oracle_case("words", 5000)
    m, listed = c["m"], c["listed"]
    blocks = listed % 3
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        for p, min_degree in ((100, 5), (200, 2)):
            one, two, three = (m.cluster_cores_within(listed, blocks, p, min_degree) for _ in range(3))
            same_bytes(one, two, (s, p))
            same_bytes(one, three, (s, p))
            assert len({CORE, BORDER, NOISE} & set(one[2].tolist())) == 3
    m.set_option("scope_strategy", 0)


def test_the_calls_around_a_call_are_unchanged_and_the_kernels_are_named():
    c = oracle_case("words", 5000)
    m, listed = c["m"], c["listed"]
    blocks = listed % 3
    packed, offsets = _native_pack(c["needles"])
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    find_kernels = m.last_kernels()
    before_within = m.cluster_within(listed, blocks, 200)
    within_kernels = m.last_kernels()
    before_cores = m.cluster_cores(listed, 200, 3)
    cores_kernels = m.last_kernels()
    for s, ran, idle in ((2, DIRECT, SWEEP), (1, SWEEP, DIRECT), (0, DIRECT, SWEEP)):
        m.set_option("scope_strategy", s)
        got = m.cluster_cores_within(listed, blocks, 200, 3)
        names = m.last_kernels()
        assert names == ["cluster_nodes_kernel", *ran, "cluster_cores_label_kernel"], (s, names)
        assert not any(k in names for k in idle + ["cluster_within_kernel", "cluster_cores_sweep_kernel", "cluster_sweep_kernel",
                                                   "cluster_within_sweep_kernel", "cluster_label_kernel"])
        assert got[4] == before_within[2]
    m.set_option("scope_strategy", 0)
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == find_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    after_within = m.cluster_within(listed, blocks, 200)
    assert m.last_kernels() == within_kernels and "cluster_within_kernel" in within_kernels
    assert after_within[0].tobytes() == before_within[0].tobytes() and after_within[1:] == before_within[1:]
    after_cores = m.cluster_cores(listed, 200, 3)
    assert m.last_kernels() == cores_kernels and "cluster_cores_sweep_kernel" in cores_kernels
    same_bytes(after_cores, before_cores)
    assert _native.NO_CLUSTER == NO_CLUSTER
    assert (_native.KIND_NONE, _native.KIND_NOISE, _native.KIND_BORDER, _native.KIND_CORE) == (NONE, NOISE, BORDER, CORE)


def _native_pack(needles):
    from blurrily_amd.map import _pack
    return _pack(needles)


def test_auto_sweeps_a_block_above_the_direct_cap_and_scores_the_others_into_the_same_words():
    """Strategies 0, 1 and 2 all run at the full size -- blocks of 100 001, 100 000 and 300 members: strategy 2 scores
    the 100 001-member block directly twice, which cluster_within's test of the same shape does once."""
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
        m.set_option("scope_strategy", s)
        results[s] = m.cluster_cores_within(listed, blocks, 700, 3)
        assert {k for k in m.last_kernels() if k.startswith("cluster_cores_within")} == kernels, s
    m.set_option("scope_strategy", 0)
    for s in (1, 2):
        same_bytes(results[s], results[0], s)
    labels, degrees, kinds, n_clusters, n_edges, n_core_edges = results[0]
    assert n_edges > n_core_edges > 0 and 0 < n_clusters < n and int(degrees.sum(dtype=np.uint64)) == 2 * n_edges
    member = (kinds >= BORDER) & (listed <= 2 * cap + 1)        # (the two large blocks are the odd and the even references)
    assert len({CORE, BORDER, NOISE} & set(kinds.tolist())) == 3 and (labels[member] % 2 == listed[member] % 2).all()
    assert (labels[(kinds >= BORDER) & (blocks == 9)] > 2 * cap + 1).all()
    assert m.cluster_within(listed, blocks, 700)[2] == n_edges
    # one member fewer in the swept block: every block is scored directly
    m.cluster_cores_within(listed[2:], blocks[2:], 700, 3)
    assert not any(k in m.last_kernels() for k in SWEEP) and all(k in m.last_kernels() for k in DIRECT)
    m.close()
