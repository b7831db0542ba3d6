"""Cluster levels on the GPU (cluster_levels.hip, cluster_levels_kernels.hip): one call, several floors.  Level k's
labels, components and edges are compared exactly with two independent truths: the host's (cluster_truth.py: numpy
over the strings' tokenisations, nothing of the library) and a separate blurrily_storage_cluster call at floors[k].
Over the oracle haystacks at three floor sets (the cap of eight among them; the levels must be telling and differ
from each other: asserted), the nesting of adjacent levels, test_gpu_cluster.py's built cases rebuilt here with floors
that straddle their edges, a haystack of more than one window, mutations, repeated calls, and beside the find and
the single-floor call, which a levels call leaves as they were."""
import numpy as np
import pytest

import workloads as W
from blurrily_amd import RawMap, _native
from blurrily_amd.map import _pack
from cluster_truth import NO_CLUSTER, Truth, shape
from helpers import ORACLE_CASES, Oracle, oracle_case_inputs

pytestmark = pytest.mark.gpu
FLOOR_SETS = ((0, 1, 200, 300, 500, 700, 999, 1000), (200, 300, 500), (1000,))


def nested(labels, n_edges):
    """Adjacent levels nest: one label at the higher floor means one label at the lower; the edges and every
    element's component do not grow with the floor."""
    for lo, hi in zip(labels, labels[1:]):
        held = hi != NO_CLUSTER
        assert np.array_equal(held, lo != NO_CLUSTER)
        pairs = np.unique(np.stack([hi[held], lo[held]]), axis=1)
        assert pairs.shape[1] == len(np.unique(hi[held]))     # every higher component lies in ONE lower component

        def size_of_own(level):
            _, inverse, counts = np.unique(level[held], return_inverse=True, return_counts=True)
            return counts[inverse]
        assert (size_of_own(hi) <= size_of_own(lo)).all()
    assert all(a >= b for a, b in zip(n_edges.tolist(), n_edges.tolist()[1:]))


def check_levels(m, truth, listed, floors, least=0):
    """One levels call against both truths, level by level, exactly.  Returns (labels, the truth's {reference: label}
    per level)."""
    labels, n_clusters, n_edges = m.cluster_levels(listed, floors)
    assert labels.dtype == np.uint32 and labels.shape == (len(floors), len(listed))
    assert len(n_clusters) == len(n_edges) == len(floors)
    of_refs = []
    for k, p in enumerate(floors):
        w_labels, w_clusters, w_edges, of_ref = truth.cluster(listed, p, least)
        s_labels, s_clusters, s_edges = m.cluster(listed, p)
        print(f"floor {p}: {len(of_ref)} nodes, clusters {n_clusters[k]} (truth {w_clusters}, separate call {s_clusters}), "
              f"edges {n_edges[k]} (truth {w_edges}, separate call {s_edges})")
        assert n_edges[k] == w_edges == s_edges, p
        assert n_clusters[k] == w_clusters == s_clusters, p
        assert np.array_equal(labels[k], w_labels), p
        assert labels[k].tobytes() == s_labels.tobytes(), p
        of_refs.append(of_ref)
    nested(labels, n_edges)
    return labels, of_refs


def _map_of(held, weights=None):
    refs = np.array(sorted(held), dtype=np.uint32)
    m = RawMap()
    m.put_many_packed(*_pack([held[int(r)] for r in refs]), refs,
                      np.zeros(len(refs), dtype=np.uint32) if weights is None else weights)
    return m


_ORACLE = {}


def oracle_case(kind, n):
    """The map and the truth of one oracle haystack, made once (the truth keeps the pairs of the one list asked)."""
    if kind not in _ORACLE:
        hay, off, needles = oracle_case_inputs(kind, n)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        _ORACLE[kind] = dict(m=_map_of(held), truth=Truth(held), needles=needles)
    return _ORACLE[kind]


@pytest.mark.parametrize("floors", FLOOR_SETS, ids=lambda f: "-".join(map(str, f)))
@pytest.mark.parametrize("kind,n,_limit", ORACLE_CASES)
def test_every_level_equals_the_truth_and_the_separate_call(kind, n, _limit, floors):
    c = oracle_case(kind, n)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    labels, of_refs = check_levels(c["m"], c["truth"], listed, floors)
    if len(floors) == 1:
        return
    # which floors leave a haystack non-degenerate was worked out from the truth on the CPU (test_gpu_cluster.py: words
    # 200 and 300; geonames 300, 500, 999, 1000; skewed 200, 300, 500, 999, 1000): both longer sets hold two for each
    telling = 0
    for of_ref in of_refs:
        components, three_or_more, singletons = shape(of_ref)
        telling += components > 1 and three_or_more >= 1 and singletons >= 1
    assert telling >= 2, "fewer than two levels leave this haystack with several components, a large one and a singleton"
    assert len({level.tobytes() for level in labels}) >= 2, "all levels coincide: the test shows nothing"


def _needle_of(rng, t):
    """A string of exactly t distinct trigrams."""
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz ", dtype=np.uint8)
    while True:
        s = bytes(rng.choice(letters, size=t + 40).tolist())
        if len(Oracle.tokenise(s)) >= t:
            for k in range(0, len(s) + 1):
                if len(Oracle.tokenise(s[:k])) == t:
                    return s[:k]


def _j(a, b):
    """(m, union) of two strings."""
    A, B = set(Oracle.tokenise(a)), set(Oracle.tokenise(b))
    return len(A & B), len(A | B)


A, B, C = b"qxzqvwkj", b"qxzqvwkjxqzzvk", b"jxqzzvk"           # J(A, B) = 8 / 16, J(B, C) = 6 / 17, J(A, C) = 0
SHORT = B[:-1]                                                # J(A[:-1], SHORT) = 7 / 15: 466 per mille, not 467
STRADDLE = (300, 352, 353, 500, 501)                          # 6 / 17 is 352.9 per mille, 8 / 16 is 500


def built_case():
    hay, off = W.words(3000, seed=5)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({5001: A, 5002: B, 5003: C})
    rng = np.random.default_rng(47)
    ref = 6000
    for t in (15, 16, 255, 256, 700):                         # the counters' widths: 4 bits, bytes, 16 bits
        s = _needle_of(rng, t)
        assert len(Oracle.tokenise(s)) == t
        for variant in (s, s, s + b" zq", s[:-1]):
            held[ref] = variant
            ref += 1
    held[7001] = held[7002] = b""                             # T == 1
    assert len(Oracle.tokenise(b"")) == 1
    return held


def test_built_cases_chain_unlisted_bridge_the_exact_floor_counter_widths_and_list_shape():
    held = built_case()
    m = _map_of(held)
    assert _j(A, B) == (8, 16) and _j(B, C) == (6, 17) and _j(A, C)[0] == 0
    # the chain at floors on both sides of both edges: all three, then A - B alone, then nothing
    labels, n_clusters, n_edges = m.cluster_levels([5001, 5002, 5003], STRADDLE)
    assert labels.tolist() == [[5001] * 3, [5001] * 3, [5001, 5001, 5003], [5001, 5001, 5003], [5001, 5002, 5003]]
    assert (n_clusters.tolist(), n_edges.tolist()) == ([1, 1, 2, 2, 3], [2, 2, 1, 1, 0])
    # ... joined only through B: with B held but not listed they stay apart at every level
    labels, n_clusters, n_edges = m.cluster_levels([5001, 5003], STRADDLE)
    assert labels.tolist() == [[5001, 5003]] * 5 and n_clusters.tolist() == [2] * 5 and n_edges.tolist() == [0] * 5
    # a pair exactly at a floor and one per mille above it, as adjacent levels
    assert m.cluster_levels([5001, 5002], (500, 501))[0].tolist() == [[5001, 5001], [5001, 5002]]
    assert _j(A[:-1], SHORT) == (7, 15)
    m.put(SHORT, 5004, 0)
    m.put(A[:-1], 5005, 0)
    assert m.cluster_levels([5004, 5005], (466, 467))[0].tolist() == [[5004, 5004], [5004, 5005]]
    held.update({5004: SHORT, 5005: A[:-1]})
    truth = Truth(held)
    everything = np.array(sorted(held), dtype=np.uint32)
    # everything listed -- the nodes of 1, 15, 16, 255, 256 and 700 trigrams among them -- at the straddling floors and
    # from 0 to 1000
    _, of_refs = check_levels(m, truth, everything, STRADDLE)
    assert of_refs[0][5001] == of_refs[0][5003] and of_refs[2][5001] == of_refs[2][5002] != of_refs[2][5003]
    assert of_refs[4][5001] != of_refs[4][5003]                # (A and B still meet through SHORT: 8 / 15 and 13 / 16)
    _, of_refs = check_levels(m, truth, everything, (0, 200, 466, 467, 500, 501, 1000))
    for of_ref in of_refs:                                    # (equal strings: together at every floor)
        assert of_ref[6000] == of_ref[6001] and of_ref[7002] == of_ref[7001] and of_ref[6017] == of_ref[6016]
    assert of_refs[-1][6000] == 6000 and of_refs[-1][7002] == 7001 and of_refs[-1][6017] == 6016
    without = everything[everything != 5002]
    _, of_refs = check_levels(m, truth, without, (300, 352))
    assert of_refs[0][5001] != of_refs[0][5003]
    # the list shuffled, with repeats and absent references mixed in: the same label per reference at every level
    rng = np.random.default_rng(5)
    absent = np.array([4000, 4001, 9999, 0xFFFFFFFF, 0], dtype=np.uint32)
    mixed = np.concatenate([everything, everything[::7], absent, absent[:2]])
    rng.shuffle(mixed)
    floors = (200, 350, 500)
    base_labels, base_clusters, base_edges = m.cluster_levels(everything, floors)
    labels, _ = check_levels(m, truth, mixed, floors)
    _, n_clusters, n_edges = m.cluster_levels(mixed, floors)
    assert np.array_equal(n_clusters, base_clusters) and np.array_equal(n_edges, base_edges)
    for k in range(len(floors)):
        want = dict(zip(everything.tolist(), base_labels[k].tolist()))
        assert labels[k].tolist() == [want.get(int(r), NO_CLUSTER) for r in mixed]
    assert (labels[:, np.isin(mixed, absent)] == NO_CLUSTER).all() and NO_CLUSTER == _native.NO_CLUSTER
    # nothing listed; nothing held
    labels, n_clusters, n_edges = m.cluster_levels([], (300, 500))
    assert (labels.shape, n_clusters.tolist(), n_edges.tolist()) == ((2, 0), [0, 0], [0, 0])
    labels, n_clusters, n_edges = m.cluster_levels(absent, (0, 500))
    assert ((labels == NO_CLUSTER).all(), n_clusters.tolist(), n_edges.tolist()) == (True, [0, 0], [0, 0])
    # the profile a caller picks a floor by
    profile = m.cluster_profile(mixed, floors)
    for k, row in enumerate(profile):
        _, sizes = np.unique(base_labels[k], return_counts=True)
        assert row == {"floor": floors[k], "n_clusters": int(base_clusters[k]), "n_edges": int(base_edges[k]),
                       "largest": int(sizes.max()), "singletons": int((sizes == 1).sum())}
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
    floors = (300, 400, 600)                                  # (all the pairs sharing a trigram do not fit the host)
    labels, of_refs = check_levels(m, c["truth"], listed, floors, least=floors[0])
    assert m.device_info()["n_windows"] >= 2
    if which == "all":
        for of_ref in of_refs[:2]:
            components, three_or_more, singletons = shape(of_ref)
            assert components > 1 and three_or_more >= 1 and singletons >= 1
    assert len({level.tobytes() for level in labels}) >= 2


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
        return check_levels(m, truth, listed, (200, 350, 500))[1]

    low, mid, high = verify()
    assert mid[9001] == mid[9003] and high[9001] == high[9002] != high[9003]
    m.delete(9002)                                            # the bridge goes: the component splits
    del held[9002]
    low, mid, high = verify()
    assert mid[9001] != mid[9003]
    m.put(B, 9500, 0)                                         # a pending put bridges two base components
    m.put(B + b"x", 9501, 0)                                  # ... and has a neighbour in the delta image
    held.update({9500: B, 9501: B + b"x"})
    low, mid, high = verify()
    assert mid[9001] == mid[9003] == mid[9500] == mid[9501] and high[9001] == high[9500] != high[9003]
    assert m.device_info()["n_pending"] >= 2 and m.device_info()["base_builds"] == builds
    m.delete(17)                                              # deleted and put again with another text
    m.put(C + b"x", 17, 0)
    held[17] = C + b"x"
    low, mid, high = verify()
    assert mid[17] == mid[9003] == 17
    big, bo = W.words(9000, seed=34)                          # a log past its budget folds into a rebuilt base image
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    low, mid, high = verify()
    info = m.device_info()
    assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    assert mid[17] == mid[9003] == mid[9001] == mid[9500] == 17
    m.close()


def test_three_calls_give_identical_bytes():
    m = oracle_case(*ORACLE_CASES[0][:2])["m"]
    listed = np.arange(1, 5001, dtype=np.uint32)
    one, two, three = (m.cluster_levels(listed, (100, 200, 300)) for _ in range(3))
    for x, y, z in zip(one, two, three):
        assert x.tobytes() == y.tobytes() == z.tobytes()


def test_the_finds_and_the_single_floor_call_around_a_levels_call_are_unchanged():
    c = oracle_case(*ORACLE_CASES[0][:2])
    m = c["m"]
    packed, offsets = _pack(c["needles"])
    listed = np.arange(1, 5001, dtype=np.uint32)
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    before_kernels = m.last_kernels()
    before_cluster = m.cluster(listed, 200)
    cluster_kernels = m.last_kernels()
    m.cluster_levels(listed, (100, 200, 300))
    for name in ("cluster_nodes_kernel", "cluster_levels_sweep_kernel", "cluster_label_kernel"):
        assert name in m.last_kernels()
    assert "cluster_sweep_kernel" not in m.last_kernels() and "find_kernel" not in m.last_kernels()
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == before_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    after_cluster = m.cluster(listed, 200)
    assert m.last_kernels() == cluster_kernels
    assert before_cluster[0].tobytes() == after_cluster[0].tobytes() and before_cluster[1:] == after_cluster[1:]
