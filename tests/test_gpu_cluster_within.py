"""Clusters within blocks on the GPU (cluster_within.hip, cluster_within_kernels.hip): blurrily_storage_cluster's
components where an edge also needs both ends under one block key.  Labels, components and edges equal the host's
truth (cluster_within_truth.py: cluster_truth's pairs kept where the keys agree, nothing of the library) exactly, under
"scope_strategy" 0 (auto), 1 (every block swept) and 2 (every block scored directly) on the same inputs: over the
oracle haystacks with interleaving keys at floors that tell blocked from plain clustering, built cases (a bridge in
another block, pairs exactly at their floor, the counter widths, block sizes around the direct kernel's tile and
workgroup, an unheld member, equal keys, distinct keys, a shuffled list with repeats and absent references), a haystack
of more than one window against one plain cluster call per block, mutations, repeated calls, and beside the other
entries, which it leaves as they were."""
import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, _native
from blurrily_amd.map import _pack
from cluster_truth import NO_CLUSTER
from cluster_within_truth import WithinTruth, telling
from helpers import oracle_case_inputs
from test_gpu_cluster import A, B, C, _j, _map_of, built_case

pytestmark = pytest.mark.gpu
FLOORS = (0, 200, 300, 500, 700, 1000)
STRATEGIES = (0, 1, 2)                                        # "scope_strategy": auto, the sweep, the direct kernel
G = 16                                                        # the direct kernel's tile (cluster.h: kClusterWithinTile)


def check(m, truth, listed, blocks, p, least=0, strategies=STRATEGIES):
    """One floor under every strategy against the truth: labels, components and edges, exactly.  Returns the truth's
    {reference: label}."""
    w_labels, w_clusters, w_edges, of_ref = truth.cluster_within(listed, blocks, p, least)
    for s in strategies:
        m.set_option("scope_strategy", s)
        labels, n_clusters, n_edges = m.cluster_within(listed, blocks, p)
        print(f"floor {p} strategy {s}: {len(of_ref)} nodes, clusters {n_clusters} (truth {w_clusters}), "
              f"edges {n_edges} (truth {w_edges})")
        assert n_edges == w_edges, (p, s)
        assert n_clusters == w_clusters, (p, s)
        assert labels.dtype == np.uint32 and np.array_equal(labels, w_labels), (p, s)
    m.set_option("scope_strategy", 0)
    return of_ref


_CASES = {}


def oracle_case(kind, n):
    """The map and the truth of an oracle haystack, made once."""
    if (kind, n) not in _CASES:
        hay, off, needles = oracle_case_inputs(kind, n)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        _CASES[kind, n] = dict(m=_map_of(held), truth=WithinTruth(held), needles=needles,
                               listed=np.arange(1, n + 1, dtype=np.uint32))
    return _CASES[kind, n]


# (with these keys a block's members interleave with the other blocks' in reference order and in position)
@pytest.mark.parametrize("kind,n,modulus,telling_floors", [("words", 5000, 3, (200, 300)),
                                                           ("geonames", 8000, 3, (200, 300, 500, 700)),
                                                           ("geonames", 8000, 64, (200, 300, 500, 700)),
                                                           ("skewed", 6000, 3, (200, 300, 500))])
def test_labels_components_and_edges_equal_the_truth_at_every_floor(kind, n, modulus, telling_floors):
    c = oracle_case(kind, n)
    m, truth, listed = c["m"], c["truth"], c["listed"]
    blocks = listed % modulus
    tells = []
    for p in FLOORS:
        blocked = check(m, truth, listed, blocks, p)
        if telling(blocked, truth.cluster(listed, p)[3]):
            tells.append(p)
        assert all(blocked[r] % modulus == r % modulus for r in blocked)   # (no component spans two blocks)
    print("telling floors:", tells)
    assert len(tells) >= 2 and set(telling_floors) <= set(tells)


def _plain(result):
    return result[0].tolist(), result[1], result[2]


def test_built_cases_a_bridge_in_another_block_the_exact_floor_and_the_counter_widths():
    held = built_case()
    short = B[:-1]
    held.update({5004: short, 5005: A[:-1]})                  # 7 / 15 against each other: 466 permille
    assert _j(A, B) == (8, 16) and _j(B, C) == (6, 17) and _j(A, C)[0] == 0 and _j(A[:-1], short) == (7, 15)
    m, truth = _map_of(held), WithinTruth(held)
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        # B, the bridge between A and C, in another block: nothing joins; all in one block: the chain
        assert _plain(m.cluster_within([5001, 5002, 5003], [1, 2, 1], 350)) == ([5001, 5002, 5003], 3, 0)
        labels, n_clusters, n_edges = m.cluster_within([5001, 5002, 5003], [4, 4, 4], 350)
        assert (labels.tolist(), n_clusters, n_edges) == ([5001, 5001, 5001], 1, 2)
        # exactly at the floor and one permille above, in one block and split across two
        for pair, at in (([5001, 5002], 500), ([5004, 5005], 466)):
            assert _plain(m.cluster_within(pair, [3, 3], at)) == ([pair[0], pair[0]], 1, 1)
            assert _plain(m.cluster_within(pair, [3, 3], at + 1)) == (pair, 2, 0)
            assert _plain(m.cluster_within(pair, [3, 8], at)) == (pair, 2, 0)
            assert _plain(m.cluster_within(pair, [3, 8], at + 1)) == (pair, 2, 0)
    m.set_option("scope_strategy", 0)
    # the words under three interleaving keys; A, B, C and the nodes of T = 1, 15, 16, 255, 256 and 700 with their
    # variants in one block of their own
    everything = np.array(sorted(held), dtype=np.uint32)
    blocks = np.where(everything > 5000, 7, everything % 3).astype(np.uint32)
    for p in (0, 200, 466, 467, 500, 501, 1000):
        of_ref = check(m, truth, everything, blocks, p)
    assert of_ref[6000] == of_ref[6001] == 6000 and of_ref[7002] == 7001 and of_ref[6017] == 6016
    # ... and split from their variants: equal strings under two keys stay apart
    blocks = np.where(everything > 5000, everything % 2 + 7, everything % 3).astype(np.uint32)
    of_ref = check(m, truth, everything, blocks, 1000)
    assert of_ref[6001] == 6001 and of_ref[7002] == 7002
    m.close()


def _sized_blocks(refs, sizes, rng):
    """Keys for a shuffled prefix of refs: blocks of the given sizes, their members anywhere among the references, the
    key values in no order."""
    picked = rng.permutation(refs)[:sum(sizes)]
    keys = rng.permutation(np.arange(1000, 1000 + len(sizes), dtype=np.uint32))
    return picked.astype(np.uint32), np.repeat(keys, sizes).astype(np.uint32)


def test_blocks_of_every_size_around_the_tile_and_the_workgroup():
    c = oracle_case("words", 5000)
    m, truth = c["m"], c["truth"]
    sizes = [1, 2, G - 1, G, G + 1, 2 * G + 1, 255, 256, 257, 600]
    listed, blocks = _sized_blocks(c["listed"], sizes, np.random.default_rng(29))
    for p in (200, 300):
        blocked = check(m, truth, listed, blocks, p)
        assert any(v != r for r, v in blocked.items())        # (some edge exists)
    # ... and equal to one plain cluster call per block, the counts summed
    labels, n_clusters, n_edges = m.cluster_within(listed, blocks, 200)
    sum_clusters = sum_edges = 0
    for key in np.unique(blocks):
        own = blocks == key
        one, k, e = m.cluster(listed[own], 200)
        assert np.array_equal(labels[own], one), int(key)
        sum_clusters, sum_edges = sum_clusters + k, sum_edges + e
    assert (n_clusters, n_edges) == (sum_clusters, sum_edges)


def test_an_unheld_member_equal_keys_distinct_keys_and_the_list_shuffled():
    # blocks with references the map does not hold in their middle, in reference order and in the list
    hay, off = W.words(600, seed=3)
    held = {10 * (i + 1): s for i, s in enumerate(W.unpack(hay, off))}
    own, own_truth = _map_of(held), WithinTruth(held)
    listed = np.array(sorted(list(held) + [15, 3005, 3015, 5995]), dtype=np.uint32)
    blocks = ((listed // 10) % 2).astype(np.uint32)
    rng = np.random.default_rng(31)
    for lst, blk in ((listed, blocks), (listed[::-1].copy(), blocks[::-1].copy())):
        for p in (0, 200):
            of_ref = check(own, own_truth, lst, blk, p)
        labels, _, _ = own.cluster_within(lst, blk, 200)
        assert (labels[np.isin(lst, [15, 3005, 3015, 5995])] == NO_CLUSTER).all() and 3005 not in of_ref
        assert (labels != NO_CLUSTER).sum() == 600
    own.close()
    c = oracle_case("words", 5000)
    m, truth = c["m"], c["truth"]
    everything = c["listed"]
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        # all keys equal: byte for byte the plain call
        for p in (200, 300):
            want = m.cluster(everything, p)
            got = m.cluster_within(everything, np.full(len(everything), 0xFFFFFFFF, dtype=np.uint32), p)
            assert got[0].tobytes() == want[0].tobytes() and got[1:] == want[1:]
        # all keys distinct: every held reference is its own label
        some = np.concatenate([everything[:700], [888888]]).astype(np.uint32)
        labels, n_clusters, n_edges = m.cluster_within(some, some[::-1].copy(), 0)
        assert labels.tolist() == some[:700].tolist() + [NO_CLUSTER] and (n_clusters, n_edges) == (700, 0)
    m.set_option("scope_strategy", 0)
    # the list shuffled, with repeats under consistent keys and absent references: the same label per reference
    absent = np.array([40000, 40001, 99999, 0xFFFFFFFF, 0], dtype=np.uint32)
    mixed = np.concatenate([everything, everything[::7], absent, absent[:2]])
    rng.shuffle(mixed)
    key = lambda refs: (refs % 5).astype(np.uint32)
    base_labels, base_clusters, base_edges = m.cluster_within(everything, key(everything), 200)
    want = dict(zip(everything.tolist(), base_labels.tolist()))
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        labels, n_clusters, n_edges = m.cluster_within(mixed, key(mixed), 200)
        assert (n_clusters, n_edges) == (base_clusters, base_edges)
        assert labels.tolist() == [want.get(int(r), NO_CLUSTER) for r in mixed]
    m.set_option("scope_strategy", 0)
    assert (labels[np.isin(mixed, absent)] == NO_CLUSTER).all() and NO_CLUSTER == _native.NO_CLUSTER
    check(m, truth, mixed, key(mixed), 200)
    # nothing listed; nothing held
    labels, n_clusters, n_edges = m.cluster_within([], [], 500)
    assert (labels.shape, n_clusters, n_edges) == ((0,), 0, 0)
    labels, n_clusters, n_edges = m.cluster_within(absent, [1, 1, 1, 2, 2], 0)
    assert ((labels == NO_CLUSTER).all(), n_clusters, n_edges) == (True, 0, 0)


def test_a_haystack_of_more_than_one_window_equals_one_plain_call_per_block():
    n = 70000
    hay, off = W.words(n, seed=17)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    weights = np.random.default_rng(23).integers(1, 1 << 20, size=n).astype(np.uint32)   # ranks unrelated to length
    m = _map_of(held, weights)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    blocks = listed % 7
    p = 300
    want = np.zeros(n, dtype=np.uint32)
    sum_clusters = sum_edges = 0
    for key in range(7):                                      # (a node's neighbours lie in the windows on both sides of its own)
        own = blocks == key
        want[own], k, e = m.cluster(listed[own], p)
        sum_clusters, sum_edges = sum_clusters + k, sum_edges + e
    assert m.device_info()["n_windows"] >= 2 and sum_edges > 0
    _, plain_clusters, plain_edges = m.cluster(listed, p)
    assert plain_edges > sum_edges and plain_clusters < sum_clusters   # (the keys cut edges)
    for s in (1, 2):
        m.set_option("scope_strategy", s)
        labels, n_clusters, n_edges = m.cluster_within(listed, blocks, p)
        print(f"strategy {s}: clusters {n_clusters} ({sum_clusters}), edges {n_edges} ({sum_edges})")
        assert np.array_equal(labels, want), s
        assert (n_clusters, n_edges) == (sum_clusters, sum_edges), s
    m.close()


def test_mutations_deleted_bridges_pending_puts_a_reference_put_again_and_the_fold():
    hay, off = W.words(5000, seed=7)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({9001: A, 9002: B, 9003: C})
    key_of = {r: r % 3 for r in held}
    key_of.update({9001: 1, 9002: 1, 9003: 1, 123456: 1})
    m = _map_of(held)
    m.sync_device()
    builds = m.device_info()["base_builds"]

    def verify():
        truth = WithinTruth(held)
        listed = np.array(sorted(held) + [123456], dtype=np.uint32)
        blocks = np.array([key_of[int(r)] for r in listed], dtype=np.uint32)
        return [check(m, truth, listed, blocks, p) for p in (200, 350)][1]

    of_ref = verify()
    assert of_ref[9001] == of_ref[9003]
    m.delete(9002)                                            # the within-block bridge goes: the component splits
    del held[9002]
    of_ref = verify()
    assert of_ref[9001] != of_ref[9003]
    m.put(B, 9500, 0)                                         # a pending put bridges two base components of its block
    m.put(B + b"x", 9501, 0)                                  # ... and has a neighbour in the delta image
    m.put(B, 9502, 0)                                         # pending puts that neighbour them from other blocks:
    m.put(B + b"x", 9503, 0)                                  # these join nothing there, and each other
    held.update({9500: B, 9501: B + b"x", 9502: B, 9503: B + b"x"})
    key_of.update({9500: 1, 9501: 1, 9502: 2, 9503: 2})
    of_ref = verify()
    assert of_ref[9001] == of_ref[9003] == of_ref[9500] == of_ref[9501]
    assert of_ref[9502] == of_ref[9503] == 9502
    assert m.device_info()["n_pending"] >= 4 and m.device_info()["base_builds"] == builds
    m.delete(16)                                              # deleted and put again with another text (16 % 3 == 1)
    m.put(C + b"x", 16, 0)
    held[16] = C + b"x"
    of_ref = verify()
    assert of_ref[16] == of_ref[9003] == 16
    big, bo = W.words(9000, seed=34)                          # a log past its budget folds into a rebuilt base image
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    key_of.update({r: r % 3 for r in bulk.tolist()})
    of_ref = verify()
    info = m.device_info()
    assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    assert of_ref[16] == of_ref[9003] == of_ref[9001] == of_ref[9500] == 16 and of_ref[9502] == of_ref[9503] == 9502
    m.close()


def test_three_calls_give_identical_bytes():
    c = oracle_case("words", 5000)
    m, listed = c["m"], c["listed"]
    blocks = listed % 3
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        for p in (100, 200):
            one, two, three = (m.cluster_within(listed, blocks, p) for _ in range(3))
            assert one[0].tobytes() == two[0].tobytes() == three[0].tobytes()
            assert one[1:] == two[1:] == three[1:]
    m.set_option("scope_strategy", 0)


def test_the_calls_around_a_cluster_within_call_are_unchanged_and_the_kernels_are_named():
    c = oracle_case("words", 5000)
    m, listed = c["m"], c["listed"]
    blocks = listed % 3
    packed, offsets = _pack(c["needles"])
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    before_kernels = m.last_kernels()
    plain = m.cluster(listed, 200)
    plain_kernels = m.last_kernels()
    for s, ran, idle in ((2, "cluster_within_kernel", "cluster_within_sweep_kernel"),
                         (1, "cluster_within_sweep_kernel", "cluster_within_kernel"),
                         (0, "cluster_within_kernel", "cluster_within_sweep_kernel")):
        m.set_option("scope_strategy", s)
        labels, _, _ = m.cluster_within(listed, blocks, 200)
        names = m.last_kernels()
        for name in ("cluster_nodes_kernel", ran, "cluster_label_kernel"):
            assert name in names, (s, names)
        assert idle not in names and "cluster_sweep_kernel" not in names and "find_kernel" not in names
    m.set_option("scope_strategy", 0)
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == before_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    again = m.cluster(listed, 200)
    assert m.last_kernels() == plain_kernels
    assert again[0].tobytes() == plain[0].tobytes() and again[1:] == plain[1:]
    # duplicates_within: the within-block components of two or more, each ascending, ordered by label
    groups = {}
    for r, lab in zip(listed.tolist(), labels.tolist()):
        groups.setdefault(lab, []).append(r)
    want = [groups[k] for k in sorted(groups) if len(groups[k]) >= 2]
    assert want and m.duplicates_within(listed, blocks, 200) == want
    mixed = np.concatenate([listed[::-1], listed[:50], [77777]]).astype(np.uint32)
    assert m.duplicates_within(mixed, mixed % 3, 200) == want
    mp = Map()
    mp.put("San José", 1)
    mp.put("san jose", 2)
    mp.put("san jose", 3)
    mp.put("london", 4)
    assert mp.duplicates_within([4, 3, 2, 1, 5], [0, 1, 0, 0, 0], 900) == [[1, 2]]
    assert mp.cluster_within([4, 3, 2, 1, 5], [0, 1, 0, 0, 0], 900)[0].tolist() == [4, 3, 1, 1, NO_CLUSTER]
    mp.close()


def test_auto_sweeps_a_block_above_the_direct_cap_and_scores_the_others_into_the_same_forest():
    cap = 100000                                              # cluster_plan.h: kClusterWithinDirectMax
    n = 2 * cap + 301
    hay, off = W.geonames(n, 2000, 41)
    m = _map_of({i + 1: s for i, s in enumerate(W.unpack(hay, off))})
    listed = np.arange(1, n + 1, dtype=np.uint32)
    # interleaving blocks of cap + 1 (swept), cap (the largest scored directly) and 300 members
    blocks = np.where(listed > 2 * cap + 1, 9, listed % 2).astype(np.uint32)
    assert [(blocks == k).sum() for k in (1, 0, 9)] == [cap + 1, cap, 300]
    results = {}
    for s, kernels in ((0, {"cluster_within_kernel", "cluster_within_sweep_kernel"}), (1, {"cluster_within_sweep_kernel"}),
                       (2, {"cluster_within_kernel"})):
        m.set_option("scope_strategy", s)
        results[s] = m.cluster_within(listed, blocks, 700)
        assert {k for k in m.last_kernels() if k.startswith("cluster_within")} == kernels, s
    m.set_option("scope_strategy", 0)
    for s in (1, 2):
        assert results[s][0].tobytes() == results[0][0].tobytes() and results[s][1:] == results[0][1:], s
    labels, n_clusters, n_edges = results[0]
    assert n_edges > 0 and n_clusters < n and (labels % 2 == listed % 2)[:2 * cap + 1].all()
    # one member fewer in the swept block: every block is scored directly
    m.cluster_within(listed[2:], blocks[2:], 700)
    assert "cluster_within_sweep_kernel" not in m.last_kernels() and "cluster_within_kernel" in m.last_kernels()
    m.close()
