"""The cluster core tree on the GPU (cluster_core_tree.hip, cluster_core_tree_kernels.hip): the merges, the core
heights, the labels and the four counts are compared byte for byte with the host's truth (cluster_core_tree_truth.py:
sorted heights and Kruskal over cluster_truth.py's pairs, nothing of the library), and the tree cut at its own heights
(and one per mille above each) with blurrily_storage_cluster_cores at those floors: the cores, their labels, the
clusters.  Over the oracle haystacks at five (floor, min_degree), the degenerate min_degree 0 and 1 against the
cluster tree, the chain that single linkage bridges and the cores do not, ties at the k-th place, the floors at which
the height sweeps go from two to one, test_gpu_cluster_levels.py's built case, a haystack of more than one window,
mutations, the list's shape, repeated calls, and beside the find, the single-floor call and the tree call, which a
core-tree call leaves as they were."""
import numpy as np
import pytest

import workloads as W
from blurrily_amd import RawMap, _native
from blurrily_amd.map import _pack
from cluster_core_tree_truth import NO_CORE, CoreTreeTruth, edges
from cluster_truth import NO_CLUSTER, Truth
from test_gpu_cluster_levels import A, B, C, _j, _map_of, built_case
from test_gpu_cluster_tree import N_TWO, oracle_case, two_windows_case
from helpers import ORACLE_CASES

pytestmark = pytest.mark.gpu
CASES = ((200, 2), (200, 4), (500, 2), (500, 4), (1000, 2))
LEAST = 200                                                   # (the floor test_gpu_cluster_tree.py's truths keep their pairs at)
MAX_CUTS = 6
BUCKETS = 32                                                  # kCoreBuckets of csrc/cluster.h


def height_sweeps(m):
    return m.last_kernels().count("cluster_core_height_sweep_kernel")


def sweeps_for(floor):
    """max(1, ceil(log_BUCKETS(1001 - floor))): the refinement's steps from a bracket of 1001 - floor heights."""
    s = 1
    while BUCKETS ** s < 1001 - floor:
        s += 1
    return s


def check_core_tree(m, truth, listed, floor, min_degree, least=None, cuts=MAX_CUTS):
    """One core-tree call against the truth, everything exactly, and cuts at the tree's floor and at up to `cuts` of
    its heights spread over their range, each with the floor one per mille above it, against cluster_cores there.
    Returns (labels, core_permille, merges)."""
    listed = np.asarray(listed, dtype=np.uint32)
    labels, core, merges, n_clusters, n_edges, n_core_edges = m.cluster_core_tree(listed, floor, min_degree)
    want = CoreTreeTruth(truth, listed, floor, min_degree, least)
    cores = len(np.unique(listed[core != NO_CORE]))
    print(f"floor {floor}, min_degree {min_degree}: {cores} cores, {len(merges)} merges (truth {len(want.merges)}), clusters "
          f"{n_clusters} (truth {want.n_clusters}), edges {n_edges} (truth {want.n_edges}), core edges {n_core_edges} "
          f"(truth {want.n_core_edges})")
    assert merges.dtype == np.uint32 and merges.shape == want.merges.shape
    assert merges.tobytes() == want.merges.tobytes()
    assert core.dtype == np.uint32 and core.tobytes() == want.core_permille.tobytes()
    assert labels.dtype == np.uint32 and labels.tobytes() == want.labels.tobytes()
    assert (n_clusters, n_edges, n_core_edges) == (want.n_clusters, want.n_edges, want.n_core_edges)
    assert len(merges) == cores - n_clusters
    heights = np.unique(merges[:, 2])
    if len(heights) > cuts:
        heights = heights[np.unique(np.linspace(0, len(heights) - 1, cuts).round().astype(int))]
    for f in [floor] + [f for h in heights.tolist() for f in (h, h + 1)]:
        if f > 1000:
            continue
        c_labels, _, kinds, c_clusters, c_edges, c_core_edges = m.cluster_cores(listed, f, min_degree)
        at, is_core = RawMap.cut_core_tree(listed, labels, core, merges, f, min_permille=floor)
        assert np.array_equal(kinds == _native.KIND_CORE, (core != NO_CORE) & (core >= f)), f
        assert np.array_equal(kinds == _native.KIND_CORE, is_core), f
        assert c_labels[is_core].tobytes() == at[is_core].tobytes(), f
        assert c_clusters == len(np.unique(at[is_core])), f
        if f == floor:
            assert (c_clusters, c_edges, c_core_edges) == (n_clusters, n_edges, n_core_edges)
    return labels, core, merges


@pytest.mark.parametrize("floor,min_degree", CASES)
@pytest.mark.parametrize("kind,n,_limit", ORACLE_CASES)
def test_everything_equals_the_truth_and_every_cut_equals_the_cores_call(kind, n, _limit, floor, min_degree):
    c = oracle_case(kind, n)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    check_core_tree(c["m"], c["truth"], listed, floor, min_degree, least=LEAST)


def test_min_degree_zero_and_one_are_the_cluster_tree():
    kind, n, _ = ORACLE_CASES[0]
    c = oracle_case(kind, n)
    m, listed = c["m"], np.arange(1, n + 1, dtype=np.uint32)
    t_labels, t_merges, t_clusters, t_edges = m.cluster_tree(listed, 200)
    assert len(t_merges) >= 3
    # min_degree 0: every node is a core at every floor, nothing is capped, and no height is sought
    labels, core, merges, n_clusters, n_edges, n_core_edges = m.cluster_core_tree(listed, 200, 0)
    kernels = m.last_kernels()
    assert merges.tobytes() == t_merges.tobytes() and labels.tobytes() == t_labels.tobytes()
    assert (n_clusters, n_edges, n_core_edges) == (t_clusters, t_edges, t_edges)
    assert (core == 1000).all()
    assert "cluster_core_height_sweep_kernel" not in kernels and "cluster_core_tree_sweep_kernel" in kernels
    assert "cluster_tree_sweep_kernel" not in kernels and "cluster_sweep_kernel" not in kernels
    # min_degree 1: the core height is the node's best edge, which caps no edge of its own
    labels, core, merges, n_clusters, n_edges, n_core_edges = m.cluster_core_tree(listed, 200, 1)
    assert merges.tobytes() == t_merges.tobytes() and labels.tobytes() == t_labels.tobytes()
    assert (n_edges, n_core_edges) == (t_edges, t_edges)
    lo, hi, h = edges(c["truth"], listed, 200, LEAST)
    best = np.full(len(c["truth"].refs), -1, dtype=np.int64)
    np.maximum.at(best, lo, h)
    np.maximum.at(best, hi, h)
    assert core.tolist() == [NO_CORE if b < 0 else b for b in best.tolist()]      # (refs are 1 .. n: index i holds i + 1)
    assert n_clusters == t_clusters - int((best < 0).sum())
    assert height_sweeps(m) == 2


def test_a_chain_that_single_linkage_bridges_has_no_cores_to_bridge():
    held = built_case()
    m = _map_of(held)
    assert _j(A, B) == (8, 16) and _j(B, C) == (6, 17) and _j(A, C)[0] == 0
    chain = [5001, 5002, 5003]
    labels, core, merges, n_clusters, n_edges, n_core_edges = m.cluster_core_tree(chain, 300, 2)
    assert merges.shape == (0, 3)
    assert core.tolist() == [NO_CORE, 352, NO_CORE]
    assert labels.tolist() == chain
    assert (n_clusters, n_edges, n_core_edges) == (1, 2, 0)
    assert m.cluster_tree(chain, 300)[1].tolist() == [[5001, 5002, 500], [5002, 5003, 352]]
    # with min_degree 1 the chain is there, the lower edge capped by nothing: B's core height is its best edge
    labels, core, merges, n_clusters, n_edges, n_core_edges = m.cluster_core_tree(chain, 300, 1)
    assert (core.tolist(), merges.tolist()) == ([500, 500, 352], [[5001, 5002, 500], [5002, 5003, 352]])
    assert (labels.tolist(), n_clusters, n_edges, n_core_edges) == ([5001] * 3, 1, 2, 2)
    m.close()


def test_ties_at_the_kth_place_and_the_exact_degree():
    same, other = b"tied strings", b"another group"
    held = {1: same, 2: same, 3: same, 4: same}
    m = _map_of(held)
    labels, core, merges, n_clusters, n_edges, n_core_edges = m.cluster_core_tree([1, 2, 3, 4], 1000, 3)
    assert core.tolist() == [1000] * 4
    assert merges.tolist() == [[1, 2, 1000], [1, 3, 1000], [1, 4, 1000]]
    assert (labels.tolist(), n_clusters, n_edges, n_core_edges) == ([1] * 4, 1, 6, 6)
    labels, core, merges, n_clusters, n_edges, n_core_edges = m.cluster_core_tree([1, 2, 3, 4], 1000, 4)
    assert core.tolist() == [NO_CORE] * 4 and merges.shape == (0, 3)
    assert (labels.tolist(), n_clusters, n_edges, n_core_edges) == ([1, 2, 3, 4], 0, 6, 0)
    assert m.cluster_core_tree([4, 2, 3, 1, 2], 0, 3)[2].tolist() == [[1, 2, 1000], [1, 3, 1000], [1, 4, 1000]]
    m.close()
    # two such groups joined by one weaker edge through a string that holds both
    held.update({11: other, 12: other, 13: other, 14: other, 5: same + b" another"})
    m, truth = _map_of(held), Truth(held)
    for floor in (0, 300):
        for min_degree in (3, 4):
            labels, core, merges = check_core_tree(m, truth, sorted(held), floor, min_degree)
            if min_degree == 3:                               # three equal strings each: the groups stand at 1000
                assert merges.tolist()[:6] == [[1, 2, 1000], [1, 3, 1000], [1, 4, 1000], [11, 12, 1000], [11, 13, 1000],
                                               [11, 14, 1000]]
            else:                                             # the fourth edge is the bridge's: it caps the three
                assert len(set(core[:4].tolist())) == 1 and core[0] == merges[0, 2] < 1000
                assert merges.tolist()[0][:2] == [1, 2]
    m.close()


@pytest.mark.parametrize("floor", [0, 1000 - BUCKETS, 1001 - BUCKETS, 1000])
def test_the_bracket_edges_and_the_count_of_height_sweeps(floor):
    assert [sweeps_for(f) for f in (0, 968, 969, 1000)] == [2, 2, 1, 1]
    kind, n, _ = ORACLE_CASES[0]
    c = oracle_case(kind, n)
    m, listed = c["m"], np.arange(1, n + 1, dtype=np.uint32)
    check_core_tree(m, c["truth"], listed, floor, 2, least=LEAST if floor >= LEAST else None, cuts=2)
    m.cluster_core_tree(listed, floor, 2)
    images = 1 + (m.device_info()["n_pending"] > 0)
    assert images == 1 and n <= 1 << 20                       # (one image, one chunk of needles)
    assert height_sweeps(m) == sweeps_for(floor) * images
    assert m.last_kernels().count("cluster_core_height_settle_kernel") == sweeps_for(floor) + 1


def test_the_built_case_with_every_counter_width():
    held = built_case()
    m, truth = _map_of(held), Truth(held)
    everything = np.array(sorted(held), dtype=np.uint32)
    # (968 and 969: the equal strings' 1000 and their near copies' 990s on both sides of the step from two sweeps to one)
    for floor in (0, 352, 353, 500, 1000 - BUCKETS, 1001 - BUCKETS):
        for min_degree in (1, 2):
            labels, core, merges = check_core_tree(m, truth, everything, floor, min_degree, cuts=3)
        m.cluster_core_tree(everything, floor, 2)
        assert height_sweeps(m) == sweeps_for(floor)
        of = dict(zip(everything.tolist(), core.tolist()))
        # (min_degree 2) equal strings have equal edges but for each other: one core height, under their 1000 ...
        assert of[6000] == of[6001] != 1000 and of[6016] == of[6017] < 1000
        # ... and the chain's middle is a core through both its edges only at or below the lower one
        assert of[5002] == (352 if floor <= 352 else NO_CORE)
    m.close()


@pytest.mark.parametrize("which", ["all", "every_third"])
def test_a_haystack_of_more_than_one_window(which):
    c = two_windows_case()
    m = c["m"]
    listed = np.arange(1, N_TWO + 1, dtype=np.uint32)
    if which == "every_third":
        listed = listed[::3]
    labels, core, merges = check_core_tree(m, c["truth"], listed, 300, 3, cuts=3)
    assert m.device_info()["n_windows"] >= 2
    if which == "all":
        assert len(merges) >= 3 and (core != NO_CORE).sum() > len(merges)


def test_mutations_deleted_bridges_pending_puts_a_reference_put_again_and_the_fold():
    hay, off = W.words(5000, seed=7)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({9001: A, 9002: B, 9003: C})
    m = _map_of(held)
    m.sync_device()
    builds = m.device_info()["base_builds"]

    def verify(min_degree=2):
        truth = Truth(held)
        listed = np.array(sorted(held) + [123456], dtype=np.uint32)
        labels, core, merges = check_core_tree(m, truth, listed, 200, min_degree, cuts=2)
        return dict(zip(listed.tolist(), core.tolist())), set(map(tuple, merges.tolist()))

    of, rows = verify()
    assert of[9002] == 352 and of[123456] == NO_CORE
    m.delete(9002)                                            # the bridge goes: its neighbours lose an edge each
    del held[9002]
    of, rows = verify()
    assert not any(9002 in r[:2] for r in rows) and 9002 not in of
    m.put(B, 9500, 0)                                         # a pending put bridges two base components
    m.put(B + b"x", 9501, 0)                                  # ... and has a neighbour in the delta image
    held.update({9500: B, 9501: B + b"x"})
    of, rows = verify()
    assert m.device_info()["n_pending"] >= 2 and m.device_info()["base_builds"] == builds
    # 9500's edges: 9501 in its own image, 9001 and 9003 across the two images, each counted once at both ends
    assert _j(B, B + b"x") == (14, 17) and of[9500] == 500 and of[9501] >= 200
    m.cluster_core_tree(sorted(held), 200, 2)
    assert height_sweeps(m) == sweeps_for(200) * 2            # (two images: the base and the pending puts)
    verify(min_degree=1)
    m.delete(17)                                              # deleted and put again with another text
    m.put(C + b"x", 17, 0)
    held[17] = C + b"x"
    of, rows = verify()
    assert of[17] != NO_CORE
    big, bo = W.words(9000, seed=34)                          # a log past its budget folds into a rebuilt base image
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    of, rows = verify()
    info = m.device_info()
    assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    m.close()


def test_the_lists_shape_does_not_matter():
    held = built_case()
    m, truth = _map_of(held), Truth(held)
    everything = np.array(sorted(held), dtype=np.uint32)
    base = m.cluster_core_tree(everything, 200, 2)
    rng = np.random.default_rng(5)
    absent = np.array([4000, 4001, 9999, 0xFFFFFFFF, 0], dtype=np.uint32)
    mixed = np.concatenate([everything, everything[::7], absent, absent[:2]])
    rng.shuffle(mixed)
    labels, core, merges = check_core_tree(m, truth, mixed, 200, 2, cuts=2)
    assert merges.tobytes() == base[2].tobytes()
    assert m.cluster_core_tree(mixed, 200, 2)[3:] == base[3:]
    want_label, want_core = dict(zip(everything.tolist(), base[0].tolist())), dict(zip(everything.tolist(), base[1].tolist()))
    assert labels.tolist() == [want_label.get(int(r), NO_CLUSTER) for r in mixed]
    assert core.tolist() == [want_core.get(int(r), NO_CORE) for r in mixed]
    assert (labels[np.isin(mixed, absent)] == NO_CLUSTER).all() and (core[np.isin(mixed, absent)] == NO_CORE).all()
    # a bridge held but not listed: its neighbours lose the edge, here the only one each has
    without = everything[everything != 5002]
    labels, core, merges = check_core_tree(m, truth, without, 300, 1, cuts=2)
    assert 5002 not in merges[:, :2] and core[without == 5001] == NO_CORE and core[without == 5003] == NO_CORE
    # nothing listed; nothing held
    out = m.cluster_core_tree([], 300, 2)
    assert [x.shape for x in out[:3]] == [(0,), (0,), (0, 3)] and out[3:] == (0, 0, 0)
    for min_degree in (0, 2):
        labels, core, merges, n_clusters, n_edges, n_core_edges = m.cluster_core_tree(absent, 0, min_degree)
        assert (labels == NO_CLUSTER).all() and (core == NO_CORE).all() and merges.shape == (0, 3)
        assert (n_clusters, n_edges, n_core_edges) == (0, 0, 0)
    m.close()


def test_three_calls_give_identical_bytes():
    m = oracle_case(*ORACLE_CASES[0][:2])["m"]
    listed = np.arange(1, 5001, dtype=np.uint32)
    one, two, three = (m.cluster_core_tree(listed, 200, 2) for _ in range(3))
    assert len(one[2]) >= 3
    for x, y, z in zip(one[:3], two[:3], three[:3]):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert one[3:] == two[3:] == three[3:]


def test_the_finds_the_single_floor_call_and_the_tree_call_around_a_core_tree_call_are_unchanged():
    c = oracle_case(*ORACLE_CASES[0][:2])
    m = c["m"]
    packed, offsets = _pack(c["needles"])
    listed = np.arange(1, 5001, dtype=np.uint32)
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    find_kernels = m.last_kernels()
    before_cluster = m.cluster(listed, 200)
    cluster_kernels = m.last_kernels()
    before_tree = m.cluster_tree(listed, 200)
    tree_kernels = m.last_kernels()
    m.cluster_core_tree(listed, 200, 2)
    for name in ("cluster_nodes_kernel", "cluster_core_height_settle_kernel", "cluster_core_height_sweep_kernel",
                 "cluster_core_tree_sweep_kernel", "cluster_tree_merge_kernel", "cluster_tree_flatten_kernel",
                 "cluster_label_kernel"):
        assert name in m.last_kernels()
    for name in ("cluster_sweep_kernel", "cluster_tree_sweep_kernel", "find_kernel"):
        assert name not in m.last_kernels()
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == find_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    after_cluster = m.cluster(listed, 200)
    assert m.last_kernels() == cluster_kernels
    assert before_cluster[0].tobytes() == after_cluster[0].tobytes() and before_cluster[1:] == after_cluster[1:]
    after_tree = m.cluster_tree(listed, 200)
    assert m.last_kernels() == tree_kernels
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before_tree[:2], after_tree[:2])) and before_tree[2:] == after_tree[2:]
