"""The cluster tree on the GPU (cluster_tree.hip, cluster_tree_kernels.hip): the merges are compared byte for byte with
the host's maximum spanning forest under the total order (cluster_tree_truth.py: Kruskal over cluster_truth.py's pairs,
nothing of the library), the labels, components and edges with a separate blurrily_storage_cluster call at the tree's
floor, and the tree cut at its own heights (and one per mille above each) with blurrily_storage_cluster at those
floors.  Over the oracle haystacks at four floors, a case that needs several Boruvka rounds (asserted from the
truth, with the launches counted), ties that only the total order settles, test_gpu_cluster_levels.py's built cases,
a haystack of more than one window, mutations, repeated calls, and beside the find and the single-floor call, which a
tree call leaves as they were."""
import numpy as np
import pytest

import workloads as W
from blurrily_amd import RawMap
from blurrily_amd.map import _pack
import cluster_tree_truth as TT
from cluster_truth import NO_CLUSTER, Truth
from helpers import ORACLE_CASES, oracle_case_inputs
from test_gpu_cluster_levels import A, B, C, SHORT, _j, _map_of, built_case

pytestmark = pytest.mark.gpu
FLOORS = (200, 300, 500, 1000)
MAX_CUTS = 12


def sweeps(m):
    return m.last_kernels().count("cluster_tree_sweep_kernel")


def check_tree(m, truth, listed, floor, least=None, cuts=MAX_CUTS):
    """One tree call against the truth's records, the separate cluster call at its floor, and cuts at up to `cuts` of
    its heights spread over their range, each with the floor one per mille above it; everything exactly.  Returns
    (labels, merges)."""
    listed = np.asarray(listed, dtype=np.uint32)
    labels, merges, n_clusters, n_edges = m.cluster_tree(listed, floor)
    want = TT.kruskal(truth, listed, floor, least)
    s_labels, s_clusters, s_edges = m.cluster(listed, floor)
    nodes = len(np.unique(listed[labels != NO_CLUSTER]))
    print(f"floor {floor}: {nodes} nodes, {len(merges)} merges (truth {len(want)}), clusters {n_clusters} (separate call "
          f"{s_clusters}), edges {n_edges} (separate call {s_edges})")
    assert merges.dtype == np.uint32 and merges.shape == want.shape
    assert merges.tobytes() == want.tobytes()
    assert labels.tobytes() == s_labels.tobytes() and (n_clusters, n_edges) == (s_clusters, s_edges)
    assert len(merges) == nodes - n_clusters
    assert len(TT.nodes_of(truth, listed)) == nodes
    heights = np.unique(merges[:, 2])
    if len(heights) > cuts:
        heights = heights[np.unique(np.linspace(0, len(heights) - 1, cuts).round().astype(int))]
    for h in heights.tolist():
        for f in (h, h + 1):
            if f > 1000:
                continue
            at = m.cluster(listed, f)[0]
            assert RawMap.cut_tree(listed, labels, merges, f, min_permille=floor).tobytes() == at.tobytes(), f
    return labels, merges


_ORACLE = {}


def oracle_case(kind, n):
    """The map and the truth of one oracle haystack, made once (the truth keeps the pairs at the lowest floor)."""
    if kind not in _ORACLE:
        hay, off, needles = oracle_case_inputs(kind, n)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        _ORACLE[kind] = dict(m=_map_of(held), truth=Truth(held), needles=needles)
    return _ORACLE[kind]


@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("kind,n,_limit", ORACLE_CASES)
def test_the_merges_equal_the_truth_and_every_cut_equals_the_cluster_call(kind, n, _limit, floor):
    c = oracle_case(kind, n)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    check_tree(c["m"], c["truth"], listed, floor, least=FLOORS[0])


def test_a_case_of_several_rounds_launches_one_sweep_per_round_and_one_more():
    kind, n, _ = ORACLE_CASES[0]
    c = oracle_case(kind, n)
    m, listed = c["m"], np.arange(1, n + 1, dtype=np.uint32)
    forest, rounds = TT.boruvka(c["truth"], listed, 200, FLOORS[0])
    assert rounds >= 3, "this case no longer needs several merging rounds: the test shows nothing"
    labels, merges, _, _ = m.cluster_tree(listed, 200)
    assert set(map(tuple, merges.tolist())) == forest
    images = 1 + (m.device_info()["n_pending"] > 0)
    assert images == 1 and n <= 1 << 20                       # (one image, one chunk of needles)
    kernels = m.last_kernels()
    assert sweeps(m) == rounds + 1                            # (the last round finds nothing to merge)
    assert kernels.count("cluster_tree_merge_kernel") == rounds + 1
    assert kernels.count("cluster_tree_flatten_kernel") == rounds + 2
    assert kernels.count("cluster_nodes_kernel") == 1 and kernels[-1] == "cluster_label_kernel"
    assert "cluster_sweep_kernel" not in kernels
    # no edges at all: one round, which finds nothing
    m.cluster_tree(listed, 1000)
    assert TT.boruvka(c["truth"], listed, 1000, FLOORS[0])[1] == 0 and sweeps(m) == 1


def test_ties_are_settled_by_the_total_order():
    same, other = b"tied strings", b"another group"
    held = {1: same, 2: same, 3: same, 4: same}
    m = _map_of(held)
    labels, merges, n_clusters, n_edges = m.cluster_tree([1, 2, 3, 4], 1000)
    assert merges.tolist() == [[1, 2, 1000], [1, 3, 1000], [1, 4, 1000]]
    assert (labels.tolist(), n_clusters, n_edges) == ([1] * 4, 1, 6)
    assert m.cluster_tree([4, 2, 3, 1, 2], 0)[1].tolist() == [[1, 2, 1000], [1, 3, 1000], [1, 4, 1000]]
    m.close()
    # two such groups joined by one weaker edge through a string that holds both
    held.update({11: other, 12: other, 13: other, 14: other, 5: same + b" another"})
    m, truth = _map_of(held), Truth(held)
    for floor in (0, 300, 1000):
        labels, merges = check_tree(m, truth, sorted(held), floor)
        assert merges.tolist()[:6] == [[1, 2, 1000], [1, 3, 1000], [1, 4, 1000], [11, 12, 1000], [11, 13, 1000],
                                       [11, 14, 1000]]
    assert len(m.cluster_tree(sorted(held), 0)[1]) == 8
    m.close()


def test_built_cases_chain_unlisted_bridge_the_exact_floor_counter_widths_and_list_shape():
    held = built_case()
    m = _map_of(held)
    assert _j(A, B) == (8, 16) and _j(B, C) == (6, 17) and _j(A, C)[0] == 0
    # the chain: two merges at their whole per mille, the cuts on both sides of both
    labels, merges, n_clusters, n_edges = m.cluster_tree([5001, 5002, 5003], 300)
    assert merges.tolist() == [[5001, 5002, 500], [5002, 5003, 352]]
    assert (labels.tolist(), n_clusters, n_edges) == ([5001] * 3, 1, 2)
    for floor, want in ((352, [5001] * 3), (353, [5001, 5001, 5003]), (500, [5001, 5001, 5003]), (501, [5001, 5002, 5003])):
        assert RawMap.cut_tree([5001, 5002, 5003], labels, merges, floor, min_permille=300).tolist() == want
        assert m.cluster([5001, 5002, 5003], floor)[0].tolist() == want
    assert RawMap.merge_profile(merges) == [{"permille": 500, "merges": 1, "n_clusters": 2},
                                            {"permille": 352, "merges": 2, "n_clusters": 1}]
    # an edge below the floor does not exist
    assert m.cluster_tree([5001, 5002, 5003], 353)[1].tolist() == [[5001, 5002, 500]]
    assert m.cluster_tree([5001, 5002, 5003], 501)[1].shape == (0, 3)
    # ... joined only through B: with B held but not listed they stay apart
    labels, merges, n_clusters, n_edges = m.cluster_tree([5001, 5003], 0)
    assert (labels.tolist(), merges.shape, n_clusters, n_edges) == ([5001, 5003], (0, 3), 2, 0)
    # a pair exactly at a floor and one per mille above it
    assert m.cluster_tree([5001, 5002], 500)[1].tolist() == [[5001, 5002, 500]]
    assert m.cluster_tree([5001, 5002], 501)[1].tolist() == []
    assert _j(A[:-1], SHORT) == (7, 15)
    m.put(SHORT, 5004, 0)
    m.put(A[:-1], 5005, 0)
    assert m.cluster_tree([5004, 5005], 466)[1].tolist() == [[5004, 5005, 466]]
    assert m.cluster_tree([5004, 5005], 467)[1].tolist() == []
    held.update({5004: SHORT, 5005: A[:-1]})
    truth = Truth(held)
    everything = np.array(sorted(held), dtype=np.uint32)
    # everything listed -- the nodes of 1, 15, 16, 255, 256 and 700 trigrams among them -- from 0 to 1000
    for floor in (0, 200, 352, 500, 1000):
        labels, merges = check_tree(m, truth, everything, floor)
        of = dict(zip(everything.tolist(), labels.tolist()))
        assert of[6000] == of[6001] and of[7002] == of[7001] and of[6017] == of[6016]   # (equal strings)
        rows = set(map(tuple, merges.tolist()))
        assert (6000, 6001, 1000) in rows and (7001, 7002, 1000) in rows and (6016, 6017, 1000) in rows
    base_labels, base_merges, base_clusters, base_edges = m.cluster_tree(everything, 200)
    without = everything[everything != 5002]
    labels, merges = check_tree(m, truth, without, 300)
    assert 5002 not in merges[:, :2] and labels[without == 5001] != labels[without == 5003]
    # the list shuffled, with repeats and absent references mixed in: the same records, the same label per reference
    rng = np.random.default_rng(5)
    absent = np.array([4000, 4001, 9999, 0xFFFFFFFF, 0], dtype=np.uint32)
    mixed = np.concatenate([everything, everything[::7], absent, absent[:2]])
    rng.shuffle(mixed)
    labels, merges = check_tree(m, truth, mixed, 200)
    assert merges.tobytes() == base_merges.tobytes()
    assert m.cluster_tree(mixed, 200)[2:] == (base_clusters, base_edges)
    want = dict(zip(everything.tolist(), base_labels.tolist()))
    assert labels.tolist() == [want.get(int(r), NO_CLUSTER) for r in mixed]
    assert (labels[np.isin(mixed, absent)] == NO_CLUSTER).all()
    # nothing listed; nothing held
    labels, merges, n_clusters, n_edges = m.cluster_tree([], 300)
    assert (labels.shape, merges.shape, n_clusters, n_edges) == ((0,), (0, 3), 0, 0)
    labels, merges, n_clusters, n_edges = m.cluster_tree(absent, 0)
    assert ((labels == NO_CLUSTER).all(), merges.shape, n_clusters, n_edges) == (True, (0, 3), 0, 0)
    m.close()


_TWO_WINDOWS = {}
N_TWO = 70000


def two_windows_case():
    if not _TWO_WINDOWS:
        hay, off = W.words(N_TWO, seed=17)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        weights = np.random.default_rng(23).integers(1, 1 << 20, size=N_TWO).astype(np.uint32)   # ranks unrelated to length
        _TWO_WINDOWS.update(m=_map_of(held, weights), truth=Truth(held))
    return _TWO_WINDOWS


@pytest.mark.parametrize("which", ["all", "every_third", "shuffled_30000"])
def test_a_haystack_of_more_than_one_window(which):
    c = two_windows_case()
    m = c["m"]
    listed = np.arange(1, N_TWO + 1, dtype=np.uint32)
    if which == "every_third":
        listed = listed[::3]
    elif which == "shuffled_30000":
        listed = np.random.default_rng(2).permutation(listed)[:30000]
    labels, merges = check_tree(m, c["truth"], listed, 300, cuts=4)   # (all the pairs sharing a trigram do not fit the host)
    assert m.device_info()["n_windows"] >= 2
    assert len(merges) >= 3 and len(np.unique(merges[:, 2])) >= 3


def test_mutations_deleted_bridges_pending_puts_a_reference_put_again_and_the_fold():
    hay, off = W.words(5000, seed=7)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({9001: A, 9002: B, 9003: C})
    m = _map_of(held)
    m.sync_device()
    builds = m.device_info()["base_builds"]

    def verify():
        truth = Truth(held)
        listed = np.array(sorted(held) + [123456], dtype=np.uint32)
        labels, merges = check_tree(m, truth, listed, 200, cuts=3)
        return dict(zip(listed.tolist(), labels.tolist())), set(map(tuple, merges.tolist()))

    of, rows = verify()
    assert (9001, 9002, 500) in rows and (9002, 9003, 352) in rows
    m.delete(9002)                                            # the bridge goes: both of its merges go with it
    del held[9002]
    of, rows = verify()
    assert not any(9002 in r[:2] for r in rows) and of[9001] != of[9003]
    m.put(B, 9500, 0)                                         # a pending put bridges two base components
    m.put(B + b"x", 9501, 0)                                  # ... and has a neighbour in the delta image
    held.update({9500: B, 9501: B + b"x"})
    of, rows = verify()
    assert (9001, 9500, 500) in rows and (9003, 9500, 352) in rows and of[9001] == of[9003] == of[9501]
    assert m.device_info()["n_pending"] >= 2 and m.device_info()["base_builds"] == builds
    truth_rounds = TT.boruvka(Truth(held), sorted(held), 200)[1]
    m.cluster_tree(sorted(held), 200)
    assert sweeps(m) == (truth_rounds + 1) * 2                # (two images: the base and the pending puts)
    m.delete(17)                                              # deleted and put again with another text
    m.put(C + b"x", 17, 0)
    held[17] = C + b"x"
    of, rows = verify()
    assert of[17] == of[9003] == 17
    big, bo = W.words(9000, seed=34)                          # a log past its budget folds into a rebuilt base image
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    of, rows = verify()
    info = m.device_info()
    assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    assert of[17] == of[9003] == of[9001] == of[9500] == 17
    m.close()


def test_three_calls_give_identical_bytes():
    m = oracle_case(*ORACLE_CASES[0][:2])["m"]
    listed = np.arange(1, 5001, dtype=np.uint32)
    one, two, three = (m.cluster_tree(listed, 200) for _ in range(3))
    for x, y, z in zip(one[:2], two[:2], three[:2]):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert one[2:] == two[2:] == three[2:]


def test_the_finds_and_the_single_floor_call_around_a_tree_call_are_unchanged():
    c = oracle_case(*ORACLE_CASES[0][:2])
    m = c["m"]
    packed, offsets = _pack(c["needles"])
    listed = np.arange(1, 5001, dtype=np.uint32)
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    before_kernels = m.last_kernels()
    before_cluster = m.cluster(listed, 200)
    cluster_kernels = m.last_kernels()
    m.cluster_tree(listed, 200)
    for name in ("cluster_nodes_kernel", "cluster_tree_sweep_kernel", "cluster_tree_merge_kernel",
                 "cluster_tree_flatten_kernel", "cluster_label_kernel"):
        assert name in m.last_kernels()
    assert "cluster_sweep_kernel" not in m.last_kernels() and "find_kernel" not in m.last_kernels()
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == before_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    after_cluster = m.cluster(listed, 200)
    assert m.last_kernels() == cluster_kernels
    assert before_cluster[0].tobytes() == after_cluster[0].tobytes() and before_cluster[1:] == after_cluster[1:]
