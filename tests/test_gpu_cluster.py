"""Clusters on the GPU (cluster.hip, cluster_kernels.hip): the connected components of "J(a, b) >= min_permille / 1000"
over a list of stored references, one label per reference (the smallest reference of its component), the number of
components and the number of edges -- all three equal to the host's truth (cluster_truth.py: numpy over the strings'
tokenisations, nothing of the library), over the oracle cases at degenerate and non-degenerate floors, built cases (a
chain, an unlisted bridge, the list shuffled with duplicates and absent references, a pair exactly at the floor, the
counter-width boundaries), a haystack of more than one window, mutations, repeated calls, the similarity find's
workaround, and beside the top-k find, which it leaves as it was."""
import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, RawMap, _native
from blurrily_amd.map import _pack
from cluster_truth import NO_CLUSTER, Truth, shape
from helpers import ORACLE_CASES, Oracle, oracle_case_inputs

pytestmark = pytest.mark.gpu
# 0 and 1 (every pair sharing a trigram), mid values, 999 and 1000 (equal trigram sets only).  Which of them leave a
# haystack non-degenerate was worked out from the truth on the CPU: words 200 and 300; geonames 300, 500, 999, 1000;
# skewed 200, 300, 500, 999, 1000 -- the test asserts at least two for each.
FLOORS = (0, 1, 200, 300, 500, 999, 1000)


def check(m, truth, listed, p, least=0):
    """One call against the truth: labels, components and edges, exactly.  Returns the truth's {reference: label}."""
    labels, n_clusters, n_edges = m.cluster(listed, p)
    w_labels, w_clusters, w_edges, of_ref = truth.cluster(listed, p, least)
    print(f"floor {p}: {len(of_ref)} nodes, clusters {n_clusters} (truth {w_clusters}), edges {n_edges} (truth {w_edges})")
    assert n_edges == w_edges, p
    assert n_clusters == w_clusters, p
    assert labels.dtype == np.uint32 and np.array_equal(labels, w_labels), p
    return of_ref


def _map_of(held, weights=None):
    refs = np.array(sorted(held), dtype=np.uint32)
    m = RawMap()
    m.put_many_packed(*_pack([held[int(r)] for r in refs]), refs,
                      np.zeros(len(refs), dtype=np.uint32) if weights is None else weights)
    return m


@pytest.mark.parametrize("kind,n,_limit", ORACLE_CASES)
def test_labels_components_and_edges_equal_the_truth_at_every_floor(kind, n, _limit):
    hay, off, _ = oracle_case_inputs(kind, n)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    m, truth = _map_of(held), Truth(held)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    telling = 0
    for p in FLOORS:
        components, three_or_more, singletons = shape(check(m, truth, listed, p))
        telling += components > 1 and three_or_more >= 1 and singletons >= 1
    assert telling >= 2, "fewer than two floors leave this haystack with several components, a large one and a singleton"
    m.close()


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


def test_built_cases_chain_unlisted_bridge_list_shape_and_the_exact_floor():
    held = built_case()
    m, truth = _map_of(held), Truth(held)
    assert _j(A, B) == (8, 16) and _j(B, C) == (6, 17) and _j(A, C)[0] == 0
    everything = np.array(sorted(held), dtype=np.uint32)
    # the chain: A - B and B - C are edges at 350, A - C is not; together all the same
    of_ref = check(m, truth, everything, 350)
    assert of_ref[5001] == of_ref[5002] == of_ref[5003] == 5001
    labels, _, _ = m.cluster([5001, 5002, 5003], 350)
    assert labels.tolist() == [5001, 5001, 5001]
    # ... joined only through B: with B held but not listed they stay apart
    labels, n_clusters, n_edges = m.cluster([5001, 5003], 350)
    assert (labels.tolist(), n_clusters, n_edges) == ([5001, 5003], 2, 0)
    without = everything[everything != 5002]
    of_ref = check(m, truth, without, 350)
    assert of_ref[5001] != of_ref[5003]
    # exactly at the floor (8 / 16 at 500), above it by one permille, and a pair one trigram short of it
    assert m.cluster([5001, 5002], 500)[0].tolist() == [5001, 5001]
    assert m.cluster([5001, 5002], 501)[0].tolist() == [5001, 5002]
    short = B[:-1]
    assert _j(A, short) == (8, 15) and _j(A + b"r", short)[0] == 8 and _j(A[:-1], short) == (7, 15)
    m.put(short, 5004, 0)
    m.put(A[:-1], 5005, 0)                                    # 7 / 15 against `short`: 466 permille
    assert m.cluster([5004, 5005], 466)[0].tolist() == [5004, 5004]
    assert m.cluster([5004, 5005], 467)[0].tolist() == [5004, 5005]
    held.update({5004: short, 5005: A[:-1]})
    truth = Truth(held)
    everything = np.array(sorted(held), dtype=np.uint32)
    for p in (0, 200, 466, 467, 500, 501, 1000):              # the counter-width nodes among them, at every floor
        of_ref = check(m, truth, everything, p)
    assert of_ref[6000] == of_ref[6001] == 6000 and of_ref[7002] == 7001 and of_ref[6017] == 6016
    # the list shuffled, with duplicates and absent references mixed in: the same label per reference
    rng = np.random.default_rng(5)
    absent = np.array([4000, 4001, 9999, 0xFFFFFFFF, 0], dtype=np.uint32)
    mixed = np.concatenate([everything, everything[::7], absent, absent[:2]])
    rng.shuffle(mixed)
    base_labels, base_clusters, base_edges = m.cluster(everything, 200)
    labels, n_clusters, n_edges = m.cluster(mixed, 200)
    assert (n_clusters, n_edges) == (base_clusters, base_edges)
    want = dict(zip(everything.tolist(), base_labels.tolist()))
    assert labels.tolist() == [want.get(int(r), NO_CLUSTER) for r in mixed]
    assert (labels[np.isin(mixed, absent)] == NO_CLUSTER).all() and NO_CLUSTER == _native.NO_CLUSTER
    check(m, truth, mixed, 200)
    # nothing listed; nothing held
    labels, n_clusters, n_edges = m.cluster([], 500)
    assert (labels.shape, n_clusters, n_edges) == ((0,), 0, 0)
    labels, n_clusters, n_edges = m.cluster(absent, 0)
    assert ((labels == NO_CLUSTER).all(), n_clusters, n_edges) == (True, 0, 0)
    m.close()


def test_a_haystack_of_more_than_one_window_all_references_and_a_strided_subset():
    n = 70000
    hay, off = W.words(n, seed=17)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    weights = np.random.default_rng(23).integers(1, 1 << 20, size=n).astype(np.uint32)   # ranks unrelated to length
    m, truth = _map_of(held, weights), Truth(held)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    for p in (300, 400):                                      # (all the pairs sharing a trigram do not fit the host)
        components, three_or_more, singletons = shape(check(m, truth, listed, p, least=300))
        assert components > 1 and three_or_more >= 1 and singletons >= 1
    assert m.device_info()["n_windows"] >= 2
    # (references and ranks are unrelated: a node's neighbours lie in the windows on both sides of its own, and the
    # subsets below leave held references that are no nodes between them)
    check(m, truth, listed[::3], 300, least=300)
    rng = np.random.default_rng(2)
    check(m, truth, rng.permutation(listed)[:30000], 300, least=300)
    m.close()


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
        return [check(m, truth, listed, p) for p in (200, 350)][1]

    of_ref = verify()
    assert of_ref[9001] == of_ref[9003]
    m.delete(9002)                                            # the bridge goes: the component splits
    del held[9002]
    of_ref = verify()
    assert of_ref[9001] != of_ref[9003]
    m.put(B, 9500, 0)                                         # a pending put bridges two base components
    m.put(B + b"x", 9501, 0)                                  # ... and has a neighbour in the delta image
    held.update({9500: B, 9501: B + b"x"})
    of_ref = verify()
    assert of_ref[9001] == of_ref[9003] == of_ref[9500] == of_ref[9501]
    assert m.device_info()["n_pending"] >= 2 and m.device_info()["base_builds"] == builds
    m.delete(17)                                              # deleted and put again with another text
    m.put(C + b"x", 17, 0)
    held[17] = C + b"x"
    of_ref = verify()
    assert of_ref[17] == of_ref[9003] == 17
    big, bo = W.words(9000, seed=34)                          # a log past its budget folds into a rebuilt base image
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    of_ref = verify()
    info = m.device_info()
    assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    assert of_ref[17] == of_ref[9003] == of_ref[9001] == of_ref[9500] == 17
    m.close()


_WORDS = {}


def words_case():
    if not _WORDS:
        hay, off, needles = oracle_case_inputs("words", 5000)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        _WORDS.update(m=_map_of(held), held=held, needles=needles)
    return _WORDS


def test_three_calls_give_identical_bytes():
    m = words_case()["m"]
    listed = np.arange(1, 5001, dtype=np.uint32)
    for p in (100, 200):
        one, two, three = (m.cluster(listed, p) for _ in range(3))
        assert one[0].tobytes() == two[0].tobytes() == three[0].tobytes()
        assert one[1:] == two[1:] == three[1:]


def test_the_similarity_find_workaround_gives_the_same_labels():
    m = words_case()["m"]
    listed = np.arange(1, 5001, dtype=np.uint32)
    p = 200
    rows, counts, _, _ = m.find_batch_by_reference_similar(listed, 65535, p)
    assert counts.max() < 65535                               # (no node's neighbours were cut)
    parent = list(range(5001))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    edges = set()
    for i, ref in enumerate(listed.tolist()):
        for other in rows[i, :counts[i], 0].tolist():
            if other != ref:
                edges.add((min(ref, other), max(ref, other)))
                a, b = find(ref), find(other)
                parent[max(a, b)] = min(a, b)
    want = np.array([find(r) for r in listed.tolist()], dtype=np.uint32)
    labels, n_clusters, n_edges = m.cluster(listed, p)
    assert np.array_equal(labels, want)
    assert n_clusters == len(set(want.tolist())) and n_edges == len(edges)


def test_the_finds_around_a_cluster_call_are_unchanged_and_the_map_surface_groups():
    c = words_case()
    m = c["m"]
    packed, offsets = _pack(c["needles"])
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    before_kernels = m.last_kernels()
    sim = m.find_batch_similar_packed(packed, offsets, 10, 300)
    sim_kernels = m.last_kernels()
    listed = np.arange(1, 5001, dtype=np.uint32)
    labels, _, _ = m.cluster(listed, 200)
    for name in ("cluster_sweep_kernel", "cluster_label_kernel"):
        assert name in m.last_kernels()
    assert "similar_sweep_kernel" not in m.last_kernels() and "find_kernel" not in m.last_kernels()
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == before_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    again = m.find_batch_similar_packed(packed, offsets, 10, 300)
    assert m.last_kernels() == sim_kernels and all(np.array_equal(x, y) for x, y in zip(sim, again))
    # duplicates: the components of two or more, each ascending, ordered by label
    groups = {}
    for r, lab in zip(listed.tolist(), labels.tolist()):
        groups.setdefault(lab, []).append(r)
    want = [groups[k] for k in sorted(groups) if len(groups[k]) >= 2]
    assert want and m.duplicates(listed, 200) == want
    assert m.duplicates(np.concatenate([listed[::-1], listed[:50], [77777]]), 200) == want
    mp = Map()
    mp.put("San José", 1)
    mp.put("san jose", 2)
    mp.put("london", 3)
    assert mp.duplicates([3, 2, 1, 4], 900) == [[1, 2]]
    assert mp.cluster([3, 2, 1, 4], 900)[0].tolist() == [3, 1, 1, NO_CLUSTER]
    mp.close()
