"""The cluster tree within blocks on the GPU (cluster_tree_within.hip, cluster_tree_within_kernels.hip): the merges are
compared byte for byte with the host's maximum spanning forest of the within-block edges (cluster_tree_within_truth.py:
cluster_tree_truth's Kruskal over the pairs whose ends carry one key, nothing of the library), the labels, components
and edges with a separate blurrily_storage_cluster_within call at the tree's floor, and the tree cut at its own heights
(and one per mille above each) with blurrily_storage_cluster_within at those floors -- under "scope_strategy" 0 (auto),
1 (every block swept) and 2 (every block scored directly) on the same inputs.  Over the oracle haystacks under
interleaving keys at four floors, a case of several Boruvka rounds with the launches counted, block sizes around the
direct kernel's tile and workgroup against one blurrily_storage_cluster_tree call per block, test_gpu_cluster_levels.py's
built cases and ties, equal keys, distinct keys, a shuffled list, a haystack of more than one window, mutations,
repeated calls, the direct cap, and beside the other entries, which it leaves as they were."""
import numpy as np
import pytest

import workloads as W
from blurrily_amd import RawMap, _native
from blurrily_amd.map import _pack
import cluster_tree_truth as TT
from cluster_tree_within_truth import BlockedTruth, blocked, per_block, unblocked
from cluster_truth import NO_CLUSTER
from helpers import oracle_case_inputs
from test_gpu_cluster_levels import A, B, C, SHORT, _j, _map_of, built_case

pytestmark = pytest.mark.gpu
FLOORS = (200, 300, 500, 700)
STRATEGIES = (0, 1, 2)                                        # "scope_strategy": auto, the sweep, the direct kernel
MAX_CUTS = 12
G = 16                                                        # the direct kernel's tile (cluster.h: kClusterWithinTile)
DIRECT, SWEEP = "cluster_tree_within_kernel", "cluster_tree_within_sweep_kernel"


def check_tree(m, truth, listed, blocks, floor, least=None, cuts=MAX_CUTS, strategies=STRATEGIES):
    """One call under every strategy against the blocked truth's records, the separate cluster_within call at its floor,
    and cuts at up to `cuts` of its heights spread over their range, each with the floor one per mille above it;
    everything exactly.  Returns (labels, merges)."""
    listed, blocks = np.asarray(listed, dtype=np.uint32), np.asarray(blocks, dtype=np.uint32)
    want = TT.kruskal(truth, listed, floor, least)
    m.set_option("scope_strategy", 0)
    s_labels, s_clusters, s_edges = m.cluster_within(listed, blocks, floor)
    key_of = dict(zip(listed.tolist(), blocks.tolist()))
    for s in strategies:
        m.set_option("scope_strategy", s)
        labels, merges, n_clusters, n_edges = m.cluster_tree_within(listed, blocks, floor)
        nodes = len(np.unique(listed[labels != NO_CLUSTER]))
        print(f"floor {floor} strategy {s}: {nodes} nodes, {len(merges)} merges (truth {len(want)}), clusters {n_clusters} "
              f"(separate call {s_clusters}), edges {n_edges} (separate call {s_edges})")
        assert merges.dtype == np.uint32 and merges.shape == want.shape, (floor, s)
        assert merges.tobytes() == want.tobytes(), (floor, s)
        assert labels.dtype == np.uint32 and labels.tobytes() == s_labels.tobytes(), (floor, s)
        assert (n_clusters, n_edges) == (s_clusters, s_edges), (floor, s)
        assert len(merges) == nodes - n_clusters, (floor, s)
        assert len(TT.nodes_of(truth, listed)) == nodes
        assert all(key_of[a] == key_of[b] for a, b, _ in merges.tolist())   # (no record joins two keys)
    m.set_option("scope_strategy", 0)
    # (the records are the same bytes under every strategy: one round of cuts serves all)
    heights = np.unique(merges[:, 2])
    if len(heights) > cuts:
        heights = heights[np.unique(np.linspace(0, len(heights) - 1, cuts).round().astype(int))]
    for h in heights.tolist():
        for f in (h, h + 1):
            if f > 1000:
                continue
            at = m.cluster_within(listed, blocks, f)[0]
            assert RawMap.cut_tree(listed, labels, merges, f, min_permille=floor).tobytes() == at.tobytes(), f
    return labels, merges


_ORACLE = {}


def oracle_case(kind, n, modulus=3):
    """The map and the blocked truth (keys: reference % modulus) of one oracle haystack, made once."""
    if (kind, n) not in _ORACLE:
        hay, off, needles = oracle_case_inputs(kind, n)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        listed = np.arange(1, n + 1, dtype=np.uint32)
        _ORACLE[kind, n] = dict(m=_map_of(held), held=held, truth=blocked(held, listed, listed % modulus),
                                needles=needles, listed=listed, blocks=(listed % modulus).astype(np.uint32))
    return _ORACLE[kind, n]


# (with these keys a block's members interleave with the other blocks' in reference order and in position)
@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("kind,n", [("words", 5000), ("geonames", 8000), ("skewed", 6000)])
def test_the_merges_equal_the_blocked_truth_and_every_cut_equals_the_cluster_within_call(kind, n, floor):
    c = oracle_case(kind, n)
    labels, merges = check_tree(c["m"], c["truth"], c["listed"], c["blocks"], floor, least=FLOORS[0])
    # the keys tell: the plain tree over the same list has other records wherever there are edges at all
    plain = TT.kruskal(unblocked(c["truth"]), c["listed"], floor, FLOORS[0])
    print(f"{kind} at {floor}: {len(merges)} blocked records against {len(plain)} plain")
    if len(plain):
        assert len(merges) < len(plain) and merges.tobytes() != plain.tobytes()
    if (kind, floor) == ("geonames", 700):
        assert len(plain) > 0


def test_a_case_of_several_rounds_launches_each_kernel_once_per_round_and_one_more():
    c = oracle_case("words", 5000)
    m, listed, blocks = c["m"], c["listed"], c["blocks"]
    forest, rounds = TT.boruvka(c["truth"], listed, 200, FLOORS[0])
    assert rounds >= 3, "this case no longer needs several merging rounds: the test shows nothing"
    assert m.device_info()["n_pending"] == 0 and len(listed) <= 1 << 20   # (one image, one chunk of needles)
    for s, ran, idle in ((2, DIRECT, SWEEP), (1, SWEEP, DIRECT)):
        m.set_option("scope_strategy", s)
        labels, merges, _, _ = m.cluster_tree_within(listed, blocks, 200)
        assert set(map(tuple, merges.tolist())) == forest
        kernels = m.last_kernels()
        assert kernels.count(ran) == rounds + 1, (s, kernels)    # (the last round finds nothing to merge)
        assert kernels.count("cluster_tree_merge_kernel") == rounds + 1
        assert kernels.count("cluster_tree_flatten_kernel") == rounds + 2
        assert kernels.count("cluster_nodes_kernel") == 1 and kernels[-1] == "cluster_label_kernel"
        for name in (idle, "cluster_tree_sweep_kernel", "cluster_within_kernel", "cluster_within_sweep_kernel",
                     "cluster_sweep_kernel"):
            assert name not in kernels, (s, name)
        # no edges at all: one round, which finds nothing
        labels, merges, n_clusters, n_edges = m.cluster_tree_within(listed, blocks, 1000)
        assert TT.boruvka(c["truth"], listed, 1000, FLOORS[0])[1] == 0
        assert m.last_kernels().count(ran) == 1 and m.last_kernels().count("cluster_tree_merge_kernel") == 1
        assert (merges.shape, n_clusters, n_edges) == ((0, 3), len(listed), 0)
    m.set_option("scope_strategy", 0)


def _sized_blocks(refs, sizes, rng):
    """Keys for a shuffled prefix of refs: blocks of the given sizes, their members anywhere among the references, the
    key values in no order (as tests/test_gpu_cluster_within.py's)."""
    picked = rng.permutation(refs)[:sum(sizes)]
    keys = rng.permutation(np.arange(1000, 1000 + len(sizes), dtype=np.uint32))
    return picked.astype(np.uint32), np.repeat(keys, sizes).astype(np.uint32)


def one_tree_per_block(m, listed, blocks, floor):
    """What one blurrily_storage_cluster_tree call per block gives: the labels put back in place, the records merged
    into one list under the total order, the counts summed."""
    labels = np.zeros(len(listed), dtype=np.uint32)
    records, sum_clusters, sum_edges = [], 0, 0
    for key in np.unique(blocks):
        own = blocks == key
        labels[own], rows, k, e = m.cluster_tree(listed[own], floor)
        records.append(rows)
        sum_clusters, sum_edges = sum_clusters + k, sum_edges + e
    return labels, per_block(records), sum_clusters, sum_edges


def test_blocks_of_every_size_around_the_tile_and_the_workgroup():
    c = oracle_case("words", 5000)
    m = c["m"]
    sizes = [1, 2, G - 1, G, G + 1, 2 * G + 1, 255, 256, 257, 600]
    listed, blocks = _sized_blocks(c["listed"], sizes, np.random.default_rng(29))
    truth = blocked(c["held"], listed, blocks)
    rounds = TT.boruvka(truth, listed, 100)[1]
    assert rounds >= 3, "this case no longer needs several merging rounds"
    labels, merges = check_tree(m, truth, listed, blocks, 100, cuts=6)
    assert len(merges) > 0
    # ... and equal to one cluster_tree call per block
    w_labels, w_merges, w_clusters, w_edges = one_tree_per_block(m, listed, blocks, 100)
    for s in (1, 2):
        m.set_option("scope_strategy", s)
        labels, merges, n_clusters, n_edges = m.cluster_tree_within(listed, blocks, 100)
        assert merges.tobytes() == w_merges.tobytes() and labels.tobytes() == w_labels.tobytes(), s
        assert (n_clusters, n_edges) == (w_clusters, w_edges), s
        assert m.last_kernels().count(SWEEP if s == 1 else DIRECT) == rounds + 1
    m.set_option("scope_strategy", 0)
    by_block = RawMap.tree_by_block(merges, listed, blocks)
    for key in np.unique(blocks).tolist():
        rows = m.cluster_tree(listed[blocks == key], 100)[1]
        assert by_block.get(key, np.zeros((0, 3), dtype=np.uint32)).tobytes() == rows.tobytes(), key


def _plain(result):
    return result[0].tolist(), result[1].tolist(), result[2], result[3]


def test_built_cases_the_chain_a_bridge_in_another_block_the_exact_floor_and_the_counter_widths():
    held = built_case()
    held.update({5004: SHORT, 5005: A[:-1]})                  # 7 / 15 against each other: 466 permille
    assert _j(A, B) == (8, 16) and _j(B, C) == (6, 17) and _j(A, C)[0] == 0 and _j(A[:-1], SHORT) == (7, 15)
    m = _map_of(held)
    chain = [5001, 5002, 5003]
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        # the chain in one block: two merges at their whole per mille; with B, the bridge, under another key: none
        labels, merges, n_clusters, n_edges = m.cluster_tree_within(chain, [4, 4, 4], 300)
        assert merges.tolist() == [[5001, 5002, 500], [5002, 5003, 352]]
        assert (labels.tolist(), n_clusters, n_edges) == ([5001] * 3, 1, 2)
        assert _plain(m.cluster_tree_within(chain, [1, 2, 1], 300)) == (chain, [], 3, 0)
        assert _plain(m.cluster_tree_within(chain, [1, 2, 1], 0)) == (chain, [], 3, 0)
        # exactly at the floor and one per mille above, in one block and split across two
        for pair, at in (([5001, 5002], 500), ([5004, 5005], 466)):
            assert _plain(m.cluster_tree_within(pair, [3, 3], at)) == ([pair[0]] * 2, [pair + [at]], 1, 1)
            assert _plain(m.cluster_tree_within(pair, [3, 3], at + 1)) == (pair, [], 2, 0)
            assert _plain(m.cluster_tree_within(pair, [3, 8], at)) == (pair, [], 2, 0)
            assert _plain(m.cluster_tree_within(pair, [3, 8], at + 1)) == (pair, [], 2, 0)
    m.set_option("scope_strategy", 0)
    # everything listed: the words under three interleaving keys; A, B, C and the nodes of T = 1, 15, 16, 255, 256 and 700
    # with their variants in one block of their own
    everything = np.array(sorted(held), dtype=np.uint32)
    blocks = np.where(everything > 5000, 7, everything % 3).astype(np.uint32)
    truth = blocked(held, everything, blocks)
    for floor in (0, 200, 352, 500, 1000):
        labels, merges = check_tree(m, truth, everything, blocks, floor, cuts=4)
        of = dict(zip(everything.tolist(), labels.tolist()))
        assert of[6000] == of[6001] and of[7002] == of[7001] and of[6017] == of[6016]   # (equal strings)
        rows = set(map(tuple, merges.tolist()))
        assert (6000, 6001, 1000) in rows and (7001, 7002, 1000) in rows and (6016, 6017, 1000) in rows
    # ... and split from their variants: equal strings under two keys stay apart
    blocks = np.where(everything > 5000, everything % 2 + 7, everything % 3).astype(np.uint32)
    labels, merges = check_tree(m, blocked(held, everything, blocks), everything, blocks, 1000)
    of = dict(zip(everything.tolist(), labels.tolist()))
    assert of[6001] == 6001 and of[7002] == 7002 and 6001 not in merges[:, :2]
    m.close()


def test_ties_are_settled_by_the_total_order_inside_a_block_and_never_across_two():
    same = b"tied strings"
    m = _map_of({1: same, 2: same, 3: same, 4: same})
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        labels, merges, n_clusters, n_edges = m.cluster_tree_within([1, 2, 3, 4], [9, 9, 9, 9], 1000)
        assert merges.tolist() == [[1, 2, 1000], [1, 3, 1000], [1, 4, 1000]]
        assert (labels.tolist(), n_clusters, n_edges) == ([1] * 4, 1, 6)
        labels, merges, n_clusters, n_edges = m.cluster_tree_within([1, 2, 3, 4], [9, 9, 8, 8], 1000)
        assert merges.tolist() == [[1, 2, 1000], [3, 4, 1000]]
        assert (labels.tolist(), n_clusters, n_edges) == ([1, 1, 3, 3], 2, 2)
        assert m.cluster_tree_within([4, 2, 3, 1, 2], [8, 9, 8, 9, 9], 0)[1].tolist() == [[1, 2, 1000], [3, 4, 1000]]
    m.close()


def test_equal_keys_distinct_keys_the_list_shuffled_nothing_listed_and_nothing_held():
    c = oracle_case("words", 5000)
    m, everything = c["m"], c["listed"]
    key = lambda refs: (refs % 3).astype(np.uint32)
    rng = np.random.default_rng(31)
    absent = np.array([40000, 40001, 99999, 0xFFFFFFFF, 0], dtype=np.uint32)
    mixed = np.concatenate([everything, everything[::7], absent, absent[:2]])
    rng.shuffle(mixed)
    base = m.cluster_tree_within(everything, key(everything), 200)
    want = dict(zip(everything.tolist(), base[0].tolist()))
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        # all keys equal: byte for byte the plain tree
        for p in (200, 300):
            plain = m.cluster_tree(everything, p)
            got = m.cluster_tree_within(everything, np.full(len(everything), 0xFFFFFFFF, dtype=np.uint32), p)
            assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes(), (s, p)
            assert got[2:] == plain[2:] and len(got[1]) > 0
        # all keys distinct: no records, every held reference its own label
        some = np.concatenate([everything[:700], [888888]]).astype(np.uint32)
        labels, merges, n_clusters, n_edges = m.cluster_tree_within(some, some[::-1].copy(), 0)
        assert labels.tolist() == some[:700].tolist() + [NO_CLUSTER]
        assert (merges.shape, n_clusters, n_edges) == ((0, 3), 700, 0)
        # the list shuffled, with repeats under consistent keys and absent references: the same records, the same label
        # per reference
        labels, merges, n_clusters, n_edges = m.cluster_tree_within(mixed, key(mixed), 200)
        assert merges.tobytes() == base[1].tobytes() and (n_clusters, n_edges) == base[2:], s
        assert labels.tolist() == [want.get(int(r), NO_CLUSTER) for r in mixed]
        assert (labels[np.isin(mixed, absent)] == NO_CLUSTER).all() and NO_CLUSTER == _native.NO_CLUSTER
        # nothing listed; nothing held
        labels, merges, n_clusters, n_edges = m.cluster_tree_within([], [], 500)
        assert (labels.shape, merges.shape, n_clusters, n_edges) == ((0,), (0, 3), 0, 0)
        labels, merges, n_clusters, n_edges = m.cluster_tree_within(absent, [1, 1, 1, 2, 2], 0)
        assert ((labels == NO_CLUSTER).all(), merges.shape, n_clusters, n_edges) == (True, (0, 3), 0, 0)
    m.set_option("scope_strategy", 0)
    check_tree(m, c["truth"], mixed, key(mixed), 200, least=FLOORS[0], cuts=3)


def test_a_haystack_of_more_than_one_window_equals_one_tree_call_per_block():
    n = 70000
    hay, off = W.words(n, seed=17)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    weights = np.random.default_rng(23).integers(1, 1 << 20, size=n).astype(np.uint32)   # ranks unrelated to length
    m = _map_of(held, weights)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    blocks = listed % 7
    p = 300
    w_labels, w_merges, w_clusters, w_edges = one_tree_per_block(m, listed, blocks, p)
    assert m.device_info()["n_windows"] >= 2 and w_edges > 0
    assert len(w_merges) >= 3 and len(np.unique(w_merges[:, 2])) >= 3
    for s in (1, 2):
        m.set_option("scope_strategy", s)
        labels, merges, n_clusters, n_edges = m.cluster_tree_within(listed, blocks, p)
        print(f"strategy {s}: {len(merges)} merges ({len(w_merges)}), clusters {n_clusters} ({w_clusters}), "
              f"edges {n_edges} ({w_edges})")
        assert merges.tobytes() == w_merges.tobytes() and labels.tobytes() == w_labels.tobytes(), s
        assert (n_clusters, n_edges) == (w_clusters, w_edges), s
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
        listed = np.array(sorted(held) + [123456], dtype=np.uint32)
        blocks = np.array([key_of[int(r)] for r in listed], dtype=np.uint32)
        truth = BlockedTruth(held, key_of)
        labels, merges = check_tree(m, truth, listed, blocks, 200, cuts=3)
        return dict(zip(listed.tolist(), labels.tolist())), set(map(tuple, merges.tolist())), truth, listed, blocks

    of, rows, _, _, _ = verify()
    assert (9001, 9002, 500) in rows and (9002, 9003, 352) in rows
    m.delete(9002)                                            # the within-block bridge goes: both of its merges go with it
    del held[9002]
    of, rows, _, _, _ = verify()
    assert not any(9002 in r[:2] for r in rows) and of[9001] != of[9003]
    m.put(B, 9500, 0)                                         # a pending put bridges two base components of its block
    m.put(B + b"x", 9501, 0)                                  # ... and has a neighbour in the delta image
    m.put(B, 9502, 0)                                         # pending puts that neighbour them from another block:
    m.put(B + b"x", 9503, 0)                                  # these join nothing there, and each other
    held.update({9500: B, 9501: B + b"x", 9502: B, 9503: B + b"x"})
    key_of.update({9500: 1, 9501: 1, 9502: 2, 9503: 2})
    of, rows, truth, listed, blocks = verify()
    assert (9001, 9500, 500) in rows and (9003, 9500, 352) in rows and of[9001] == of[9003] == of[9500] == of[9501]
    assert of[9502] == of[9503] == 9502 and not any((r[0] in (9502, 9503)) != (r[1] in (9502, 9503)) for r in rows)
    assert m.device_info()["n_pending"] >= 4 and m.device_info()["base_builds"] == builds
    truth_rounds = TT.boruvka(truth, listed, 200)[1]
    m.set_option("scope_strategy", 1)
    m.cluster_tree_within(listed, blocks, 200)
    assert m.last_kernels().count(SWEEP) == (truth_rounds + 1) * 2   # (two images: the base and the pending puts)
    m.set_option("scope_strategy", 0)
    m.delete(16)                                              # deleted and put again with another text (16 % 3 == 1)
    m.put(C + b"x", 16, 0)
    held[16] = C + b"x"
    of, rows, _, _, _ = verify()
    assert of[16] == of[9003] == 16
    big, bo = W.words(9000, seed=34)                          # a log past its budget folds into a rebuilt base image
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    key_of.update({r: r % 3 for r in bulk.tolist()})
    of, rows, _, _, _ = verify()
    info = m.device_info()
    assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    assert of[16] == of[9003] == of[9001] == of[9500] == 16 and of[9502] == of[9503] == 9502
    m.close()


def test_three_calls_give_identical_bytes():
    c = oracle_case("words", 5000)
    m, listed, blocks = c["m"], c["listed"], c["blocks"]
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        for p in (100, 200):
            one, two, three = (m.cluster_tree_within(listed, blocks, p) for _ in range(3))
            for x, y, z in zip(one[:2], two[:2], three[:2]):
                assert x.tobytes() == y.tobytes() == z.tobytes()
            assert one[2:] == two[2:] == three[2:] and len(one[1]) > 0
    m.set_option("scope_strategy", 0)


def test_the_calls_around_a_cluster_tree_within_call_are_unchanged_and_the_kernels_are_named():
    c = oracle_case("words", 5000)
    m, listed, blocks = c["m"], c["listed"], c["blocks"]
    packed, offsets = _pack(c["needles"])
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    around = [(lambda: m.cluster(listed, 200)), (lambda: m.cluster_within(listed, blocks, 200)),
              (lambda: m.cluster_tree(listed, 200))]
    before_kernels = m.last_kernels()
    before = []
    for call in around:
        result = call()
        before.append((result, m.last_kernels()))
    for s, ran, idle in ((2, DIRECT, SWEEP), (1, SWEEP, DIRECT), (0, DIRECT, SWEEP)):
        m.set_option("scope_strategy", s)
        m.cluster_tree_within(listed, blocks, 200)
        names = m.last_kernels()
        for name in ("cluster_nodes_kernel", ran, "cluster_tree_merge_kernel", "cluster_tree_flatten_kernel",
                     "cluster_label_kernel"):
            assert name in names, (s, names)
        for name in (idle, "cluster_sweep_kernel", "cluster_within_kernel", "cluster_within_sweep_kernel",
                     "cluster_tree_sweep_kernel", "find_kernel"):
            assert name not in names, (s, name)
    m.set_option("scope_strategy", 0)
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == before_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    for call, (was, was_kernels) in zip(around, before):
        now = call()
        assert m.last_kernels() == was_kernels
        for x, y in zip(was, now):
            assert x.tobytes() == y.tobytes() if isinstance(x, np.ndarray) else x == y


def test_auto_sweeps_a_block_above_the_direct_cap_and_scores_the_others_into_the_same_best():
    cap = 100000                                              # cluster_plan.h: kClusterWithinDirectMax
    n = 2 * cap + 301
    hay, off = W.geonames(n, 2000, 41)
    m = _map_of({i + 1: s for i, s in enumerate(W.unpack(hay, off))})
    listed = np.arange(1, n + 1, dtype=np.uint32)
    # interleaving blocks of cap + 1 (swept), cap (the largest scored directly) and 300 members
    blocks = np.where(listed > 2 * cap + 1, 9, listed % 2).astype(np.uint32)
    assert [(blocks == k).sum() for k in (1, 0, 9)] == [cap + 1, cap, 300]
    results = {}
    for s, kernels in ((0, {DIRECT, SWEEP}), (1, {SWEEP}), (2, {DIRECT})):
        m.set_option("scope_strategy", s)
        results[s] = m.cluster_tree_within(listed, blocks, 700)
        assert {k for k in m.last_kernels() if k.startswith("cluster_tree_within")} == kernels, s
    m.set_option("scope_strategy", 0)
    for s in (1, 2):
        assert results[s][0].tobytes() == results[0][0].tobytes() and results[s][1].tobytes() == results[0][1].tobytes(), s
        assert results[s][2:] == results[0][2:], s
    labels, merges, n_clusters, n_edges = results[0]
    assert n_edges > 0 and n_clusters < n and len(merges) == n - n_clusters
    assert (labels % 2 == listed % 2)[:2 * cap + 1].all() and (merges[:, 0] % 2 == merges[:, 1] % 2)[merges[:, 1] <= 2 * cap + 1].all()
    within = m.cluster_within(listed, blocks, 700)
    assert within[0].tobytes() == labels.tobytes() and within[1:] == (n_clusters, n_edges)
    # one member fewer in the swept block: every block is scored directly
    m.cluster_tree_within(listed[2:], blocks[2:], 700)
    assert SWEEP not in m.last_kernels() and DIRECT in m.last_kernels()
    m.close()
