"""Cluster cores on the GPU (cluster_cores.hip, cluster_cores_kernels.hip): per reference its label, its degree and its
kind (core, border, noise); the clusters, the edges and the edges between cores.  Everything is compared exactly with
the host's truth (cluster_cores_truth.py over cluster_truth.py: numpy over the strings' tokenisations, nothing of the
library), and the degrees must sum to twice the edges.  Over hand-made graphs (two triangles and a bridge, a border
between two clusters with the tie falling either way, a noise pair, a bridge held but not listed, an edge exactly at
the floor, the counter widths' node sizes, a shuffled list with repeats and absent references, min_degree 0, 1 and
beyond every degree), the oracle haystacks at the floors and degrees that leave them clusters, borders and noise
(asserted), a haystack of more than one window, mutations, repeated calls, and beside the find and the other cluster
calls, which it leaves as they were."""
import numpy as np
import pytest

import workloads as W
from blurrily_amd import RawMap, _native
from blurrily_amd.map import _pack
from cluster_cores_truth import BORDER, CORE, NOISE, NONE, CoresEdges
from cluster_truth import NO_CLUSTER, Truth
from helpers import Oracle, oracle_case_inputs

pytestmark = pytest.mark.gpu
KERNELS = ["cluster_nodes_kernel", "cluster_cores_sweep_kernel", "cluster_cores_sweep_kernel<unite>",
           "cluster_cores_label_kernel"]


def check(m, edges, min_degree):
    """One call against the truth (`edges`: a CoresEdges, the list and the floor), exactly.  Returns the truth."""
    listed, p = np.array(edges.listed, dtype=np.uint32), edges.p
    labels, degrees, kinds, n_clusters, n_edges, n_core_edges = m.cluster_cores(listed, p, min_degree)
    want = edges.cores(min_degree)
    print(f"floor {p}, min_degree {min_degree}: {len(want.label_of)} nodes, clusters {n_clusters} (truth "
          f"{want.n_clusters}), edges {n_edges} (truth {want.n_edges}), core edges {n_core_edges} (truth "
          f"{want.n_core_edges}), degrees' sum {int(degrees.sum(dtype=np.uint64))}, cores, borders, noise "
          f"{[int((kinds == k).sum()) for k in (CORE, BORDER, NOISE)]} (truth "
          f"{[int((want.kinds == k).sum()) for k in (CORE, BORDER, NOISE)]})")
    assert n_edges == want.n_edges, (p, min_degree)
    assert n_core_edges == want.n_core_edges, (p, min_degree)
    assert n_clusters == want.n_clusters, (p, min_degree)
    assert degrees.dtype == np.uint32 and np.array_equal(degrees, want.degrees), (p, min_degree)
    assert kinds.dtype == np.uint8 and np.array_equal(kinds, want.kinds), (p, min_degree)
    assert labels.dtype == np.uint32 and np.array_equal(labels, want.labels), (p, min_degree)
    _, first = np.unique(listed, return_index=True)             # (a reference listed twice is one node)
    assert int(degrees[first].sum(dtype=np.uint64)) == 2 * n_edges, (p, min_degree)
    return want


def edges_of(truth, listed, p, least=0):
    e = CoresEdges(truth, listed, p, least)
    e.p = p
    return e


def _map_of(held, weights=None):
    refs = np.array(sorted(held), dtype=np.uint32)
    m = RawMap()
    m.put_many_packed(*_pack([held[int(r)] for r in refs]), refs,
                      np.zeros(len(refs), dtype=np.uint32) if weights is None else weights)
    return m


def _j(a, b):
    """(m, union) of two strings."""
    A, B = set(Oracle.tokenise(a)), set(Oracle.tokenise(b))
    return len(A & B), len(A | B)


def _permille(a, b):
    return 1000 * _j(a, b)[0] // _j(a, b)[1]


def _answers(m, listed, p, min_degree):
    labels, degrees, kinds, n_clusters, n_edges, n_core_edges = m.cluster_cores(listed, p, min_degree)
    return labels.tolist(), degrees.tolist(), kinds.tolist(), n_clusters, n_edges, n_core_edges


def _adjacency(strings):
    return [[int(x is not y and _j(x, y)[0] >= 1) for y in strings] for x in strings]


# five parts without a letter in common: strings share trigrams exactly when they share a part
S = [b"abcde", b"fghij", b"klmno", b"pqrst", b"uvwxy"]


def test_two_triangles_joined_through_a_bridge():
    A1, A2, A3, B, C1, C2, C3 = S[0], S[0] + b"z", S[0] + S[1], S[1] + S[2], S[2] + S[3], S[3], S[3] + b"pq"
    strings = [A1, A2, A3, B, C1, C2, C3]
    assert _adjacency(strings) == [[0, 1, 1, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0, 0], [1, 1, 0, 1, 0, 0, 0],
                                   [0, 0, 1, 0, 1, 0, 0],                          # the bridge: degree 2
                                   [0, 0, 0, 1, 0, 1, 1], [0, 0, 0, 0, 1, 0, 1], [0, 0, 0, 0, 1, 1, 0]]
    held = {i + 1: s for i, s in enumerate(strings)}
    m, truth = _map_of(held), Truth(held)
    listed = [1, 2, 3, 4, 5, 6, 7]
    degrees = [2, 2, 3, 2, 3, 2, 2]
    # min_degree 3: the two corners the bridge touches are the only cores; the bridge is a border (its two anchors tie
    # at degree 3: the smaller reference), the clusters stay two
    assert _answers(m, listed, 1, 3) == ([3, 3, 3, 3, 5, 5, 5], degrees, [2, 2, 3, 2, 3, 2, 2], 2, 8, 0)
    # min_degree 2: everything is a core, the bridge unites: one cluster, as cluster's one component
    assert _answers(m, listed, 1, 2) == ([1] * 7, degrees, [3] * 7, 1, 8, 8)
    assert m.cluster(listed, 1)[1:] == (1, 8)
    # the bridge held but not listed: it joins nothing and adds to nobody's degree
    without = [1, 2, 3, 5, 6, 7]
    assert _answers(m, without, 1, 2) == ([1, 1, 1, 5, 5, 5], [2] * 6, [3] * 6, 2, 6, 6)
    assert _answers(m, without, 1, 3) == (without, [2] * 6, [1] * 6, 0, 6, 0)
    for listed in (listed, without):
        e = edges_of(truth, listed, 1)
        for min_degree in (0, 1, 2, 3, 4):
            check(m, e, min_degree)
    assert m.dense_duplicates([7, 6, 5, 4, 3, 2, 1, 1], 1, 3) == [[1, 2, 3, 4], [5, 6, 7]]
    m.close()


def test_a_border_between_two_clusters_goes_to_the_higher_degree_and_a_tie_to_the_smaller_reference():
    P1, P2, P3, X = S[0] + S[1], S[0], S[0] + b"z", S[1] + S[2]
    Q1, Q2, Q3, Q4 = S[2] + S[3], S[3], S[3] + b"pq", S[3] + b"rp"
    strings = [P1, P2, P3, X, Q1, Q2, Q3, Q4]
    assert _adjacency(strings) == [[0, 1, 1, 1, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0, 0],
                                   [1, 0, 0, 0, 1, 0, 0, 0],                       # X touches P1 and Q1 only
                                   [0, 0, 0, 1, 0, 1, 1, 1], [0, 0, 0, 0, 1, 0, 1, 1], [0, 0, 0, 0, 1, 1, 0, 1],
                                   [0, 0, 0, 0, 1, 1, 1, 0]]
    # P1 has three edges, Q1 four: X, a border of degree 2, goes to Q1's cluster (label 5, its smallest core)
    held = {i + 1: s for i, s in enumerate(strings)}
    m, truth = _map_of(held), Truth(held)
    listed = sorted(held)
    assert _answers(m, listed, 1, 3) == ([1, 1, 1, 5, 5, 5, 5, 5], [3, 2, 2, 2, 4, 3, 3, 3], [3, 2, 2, 2, 3, 3, 3, 3], 2, 11, 6)
    want = check(m, edges_of(truth, listed, 1), 3)
    assert want.torn_borders == 1
    m.close()
    # without Q4 both have three edges: the smaller reference, P1, wins
    del held[8]
    m, truth = _map_of(held), Truth(held)
    listed = sorted(held)
    assert _answers(m, listed, 1, 3) == ([1, 1, 1, 1, 5, 5, 5], [3, 2, 2, 2, 3, 2, 2], [3, 2, 2, 2, 3, 2, 2], 2, 8, 0)
    assert check(m, edges_of(truth, listed, 1), 3).torn_borders == 1
    m.close()
    # the same strings with P1 and Q1 under each other's reference: the tie falls the other way
    held[1], held[5] = Q1, P1
    m, truth = _map_of(held), Truth(held)
    assert _answers(m, listed, 1, 3) == ([1, 5, 5, 1, 5, 1, 1], [3, 2, 2, 2, 3, 2, 2], [3, 2, 2, 2, 3, 2, 2], 2, 8, 0)
    assert check(m, edges_of(truth, listed, 1), 3).torn_borders == 1
    assert m.dense_duplicates(listed, 1, 3) == [[1, 4, 6, 7], [2, 3, 5]]
    m.close()


def test_a_pair_below_min_degree_is_noise_and_min_degree_beyond_every_degree_leaves_only_noise():
    held = {3: S[0], 9: S[0] + b"z", 11: S[4]}
    m, truth = _map_of(held), Truth(held)
    assert _answers(m, [3, 9, 11], 1, 2) == ([3, 9, 11], [1, 1, 0], [1, 1, 1], 0, 1, 0)
    assert _answers(m, [3, 9, 11], 1, 1) == ([3, 3, 11], [1, 1, 0], [3, 3, 1], 1, 1, 1)
    assert _answers(m, [3, 9, 11], 1, 0) == ([3, 3, 11], [1, 1, 0], [3, 3, 3], 2, 1, 1)
    assert _answers(m, [3, 9, 11], 1, 0xFFFFFFFF) == ([3, 9, 11], [1, 1, 0], [1, 1, 1], 0, 1, 0)
    e = edges_of(truth, [3, 9, 11], 1)
    for min_degree in (0, 1, 2, 0xFFFFFFFF):
        check(m, e, min_degree)
    assert m.dense_duplicates([3, 9, 11], 1, 2) == [] and m.dense_duplicates([3, 9, 11], 1, 1) == [[3, 9]]
    m.close()


# J(A, B) = 8 / 16, J(B, C) = 6 / 17, J(A, C) = 0; D shares A's trigrams and too few of B's
A, B, C, D = b"qxzqvwkj", b"qxzqvwkjxqzzvk", b"jxqzzvk", b"nmqxzqvwkj"


def test_an_edge_exactly_at_the_floor_makes_a_core_and_one_permille_above_a_border():
    assert _j(A, B) == (8, 16) and _j(B, C) == (6, 17) and _j(A, C)[0] == 0 and _j(D, C)[0] == 0
    assert _permille(B, C) == 352 and _permille(D, A) >= 353 and _permille(D, B) < 352
    # three copies of A, each with edges to the two others, B and D; B: the copies and, at 352 and no higher, C
    held = {1: A, 2: A, 3: A, 4: B, 5: C, 6: D}
    m, truth = _map_of(held), Truth(held)
    listed = sorted(held)
    assert _answers(m, listed, 352, 4) == ([1, 1, 1, 1, 1, 1], [4, 4, 4, 4, 1, 3], [3, 3, 3, 3, 2, 2], 1, 10, 6)
    assert _answers(m, listed, 353, 4) == ([1, 1, 1, 1, 5, 1], [4, 4, 4, 3, 0, 3], [3, 3, 3, 2, 1, 2], 1, 9, 3)
    for p in (352, 353, 500, 501):
        e = edges_of(truth, listed, p)
        for min_degree in (2, 3, 4):
            check(m, e, min_degree)
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


def test_node_sizes_of_both_counter_widths_the_shape_of_the_list_and_the_two_identities():
    hay, off = W.words(3000, seed=5)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    rng = np.random.default_rng(47)
    ref = 6000
    sized = {}
    for t in (15, 16, 255, 256, 700):                         # both counter widths and their boundaries
        s = _needle_of(rng, t)
        assert len(Oracle.tokenise(s)) == t
        sized[t] = ref
        for variant in (s, s, s + b" zq", s[:-1]):               # four of a kind: three edges each where the floor lets them
            held[ref] = variant
            ref += 1
    held[7001] = held[7002] = held[7003] = b""                # T == 1
    assert len(Oracle.tokenise(b"")) == 1
    m, truth = _map_of(held), Truth(held)
    everything = np.array(sorted(held), dtype=np.uint32)
    for p in (200, 500):
        e = edges_of(truth, everything, p)
        for min_degree in (0, 1, 2, 3):
            want = check(m, e, min_degree)
            # the two identities, against a separate cluster call
            if min_degree <= 1:
                labels, degrees, kinds, n_clusters, n_edges, n_core_edges = m.cluster_cores(everything, p, min_degree)
                s_labels, s_clusters, s_edges = m.cluster(everything, p)
                assert n_edges == s_edges == n_core_edges
                if min_degree == 0:
                    assert labels.tobytes() == s_labels.tobytes() and n_clusters == s_clusters and (kinds == CORE).all()
                else:
                    alone = degrees == 0
                    assert alone.any() and not alone.all()
                    assert np.array_equal(labels[~alone], s_labels[~alone]) and (kinds[~alone] == CORE).all()
                    assert (kinds[alone] == NOISE).all() and np.array_equal(labels[alone], everything[alone])
                    assert n_clusters == s_clusters - int(alone.sum())
        assert all(want.kind_of[sized[t]] == CORE and want.degree_of[sized[t]] >= 3 for t in (15, 16, 255, 256, 700)), p
        assert want.degree_of[7001] == 2 and want.kind_of[7001] == NOISE and want.label_of[7002] == 7002   # (T == 1: a triangle below 3)
    # min_degree larger than any degree: everything is noise
    top = int(want.degrees.max())
    out = m.cluster_cores(everything, 500, top + 1)
    assert (out[2] == NOISE).all() and np.array_equal(out[0], everything) and (out[3], out[5]) == (0, 0)
    assert out[4] == want.n_edges and m.cluster_cores(everything, 500, top)[3] >= 1
    # the list shuffled, with repeats and absent references mixed in
    rng = np.random.default_rng(5)
    absent = np.array([4000, 4001, 9999, 0xFFFFFFFF, 0], dtype=np.uint32)
    mixed = np.concatenate([everything, everything[::7], absent, absent[:2]])
    rng.shuffle(mixed)
    base = m.cluster_cores(everything, 200, 3)
    got = m.cluster_cores(mixed, 200, 3)
    assert got[3:] == base[3:]
    for k, nothing in ((0, NO_CLUSTER), (1, 0), (2, NONE)):
        of = dict(zip(everything.tolist(), base[k].tolist()))
        assert got[k].tolist() == [of.get(int(r), nothing) for r in mixed]   # (repeats equal, absent ones nothing)
        assert (got[k][np.isin(mixed, absent)] == nothing).all()
    check(m, edges_of(truth, mixed, 200), 3)
    assert m.dense_duplicates(mixed, 200, 3) == m.dense_duplicates(everything, 200, 3) != []
    # nothing listed; nothing held
    out = m.cluster_cores([], 500, 3)
    assert [a.shape for a in out[:3]] == [(0,)] * 3 and out[3:] == (0, 0, 0)
    out = m.cluster_cores(absent, 0, 0)
    assert (out[0] == NO_CLUSTER).all() and not out[1].any() and (out[2] == NONE).all() and out[3:] == (0, 0, 0)
    m.close()


# (haystack, n, floor, the min_degrees, and where the issue gives them: the min_degree at which the haystack must have
# (clusters of three or more cores, borders, noise nodes with an edge) and borders between two clusters)
ORACLE_FLOORS = [("words", 5000, 300, (2, 3), (2, (4, 59, 190), None)),
                 ("geonames", 30000, 500, (3, 5), (5, (150, 3094, 2675), 55)),
                 ("geonames", 30000, 700, (2,), None),
                 ("skewed", 20000, 500, (2, 3, 5), (3, (31, 2084, 3061), 34))]


@pytest.mark.parametrize("kind,n,p,min_degrees,telling", ORACLE_FLOORS, ids=[f"{c[0]}-{c[2]}" for c in ORACLE_FLOORS])
def test_everything_equals_the_truth_on_the_oracle_haystacks(kind, n, p, min_degrees, telling):
    hay, off, _ = oracle_case_inputs(kind, n)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    m, truth = _map_of(held), Truth(held)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    e = edges_of(truth, listed, p, least=p)
    for min_degree in min_degrees:
        want = check(m, e, min_degree)
        if telling and telling[0] == min_degree:
            has = (want.big_clusters, want.n_borders, want.noise_with_an_edge)
            print(f"clusters of three or more cores, borders, noise with an edge: {has}; borders between two clusters: "
                  f"{want.torn_borders}")
            assert has == telling[1] and min(has) >= 1
            if telling[2] is not None:
                assert want.torn_borders == telling[2] >= 1
    m.close()


def test_a_haystack_of_more_than_one_window_all_references_and_every_third():
    n = 70000
    hay, off = W.words(n, seed=17)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    weights = np.random.default_rng(23).integers(1, 1 << 20, size=n).astype(np.uint32)   # ranks unrelated to length
    m, truth = _map_of(held, weights), Truth(held)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    # (references and ranks are unrelated: a node's neighbours and its anchor lie in the windows on both sides of its
    # own, so core edges and anchors are found from either end; the subset leaves held references that are no nodes)
    want = check(m, edges_of(truth, listed, 300, least=300), 3)
    assert want.big_clusters >= 1 and want.n_borders >= 1 and want.noise_with_an_edge >= 1
    assert m.device_info()["n_windows"] >= 2
    check(m, edges_of(truth, listed[::3], 300, least=300), 3)
    m.close()


# a hub and what hangs on it, in trigrams that English words hardly have.  Per mille: H - X1 500, H - X2 384, H - X3 666,
# X1 - X3 400, X2 - X3 235, X1 - X2 nothing; N (put later) - H 615, N - X2 416, N - X3 411, N - X1 214; Y (put later)
# - X3 alone
H, X1, X2, X3, N, Y = b"klmnopqrst", b"klmnop", b"opqrst", b"klmnopqrstuvw", b"lmnopqrst", b"qrstuvw"


def test_mutations_a_deleted_core_pending_puts_a_reference_put_again_and_the_fold():
    assert [_permille(*xy) for xy in ((H, X1), (H, X2), (H, X3), (X1, X3), (X2, X3))] == [500, 384, 666, 400, 235]
    assert _j(X1, X2)[0] == 0 and [_permille(N, y) for y in (H, X2, X3, X1)] == [615, 416, 411, 214]
    assert _permille(Y, X3) >= 300 and max(_permille(Y, y) for y in (H, X1, X2, N)) < 300
    hay, off = W.words(5000, seed=7)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({9001: X1, 9002: X2, 9003: H, 9004: X3})
    m = _map_of(held)
    m.sync_device()
    builds = m.device_info()["base_builds"]
    ours = (9001, 9002, 9003, 9004, 9500, 9501, 9502)

    def verify():
        truth = Truth(held)
        listed = np.array(sorted(held) + [123456], dtype=np.uint32)
        want = check(m, edges_of(truth, listed, 300), 3)
        return want, [want.kind_of.get(r, NONE) for r in ours], [want.label_of.get(r) for r in ours]

    want, kinds, labels = verify()                            # H alone has three edges: a core with three borders
    assert [want.degree_of[r] for r in ours[:4]] == [2, 1, 3, 2]
    assert kinds[:4] == [BORDER, BORDER, CORE, BORDER] and labels[:4] == [9003] * 4
    m.delete(9003)                                            # the core goes: its neighbours are noise
    del held[9003]
    want, kinds, labels = verify()
    assert [want.degree_of[r] for r in (9001, 9002, 9004)] == [1, 0, 1]
    assert kinds[:4] == [NOISE, NOISE, NONE, NOISE] and labels[:4] == [9001, 9002, None, 9004]
    m.put(H, 9500, 0)                                         # pending puts become cores, from the delta image
    m.put(N, 9501, 0)
    m.put(Y, 9502, 0)                                         # ... and one a border of a core of the base image
    held.update({9500: H, 9501: N, 9502: Y})
    want, kinds, labels = verify()
    assert m.device_info()["n_pending"] >= 3 and m.device_info()["base_builds"] == builds
    assert [want.degree_of[r] for r in (9001, 9002, 9004, 9500, 9501, 9502)] == [2, 2, 4, 4, 3, 1]
    assert kinds == [BORDER, BORDER, NONE, CORE, CORE, CORE, BORDER]
    assert labels == [9004, 9004, None, 9004, 9004, 9004, 9004]   # (X2's anchor is H, 9500; Y's is X3, as X1's: the tie with H)
    m.delete(17)                                              # deleted and put again with another text
    m.put(X2 + b"u", 17, 0)
    held[17] = X2 + b"u"
    want, kinds, labels = verify()
    assert want.degree_of[17] == 1 and want.kind_of[17] == BORDER and want.label_of[17] == 9002   # (a third edge for X2: a core)
    assert kinds == [BORDER, CORE, NONE, CORE, CORE, CORE, BORDER] and labels == [9002, 9002, None, 9002, 9002, 9002, 9002]
    big, bo = W.words(9000, seed=34)                          # a log past its budget folds into a rebuilt base image
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    again, kinds_again, labels_again = verify()
    info = m.device_info()
    assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    assert kinds_again == kinds and labels_again == labels
    m.close()


@pytest.fixture(scope="module")
def words_case():
    """The words oracle haystack in a map of its own, shared by the tests below and closed behind them."""
    hay, off, needles = oracle_case_inputs("words", 5000)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    m = _map_of(held)
    yield dict(m=m, held=held, needles=needles)
    m.close()


def test_three_calls_give_identical_bytes_and_last_kernels_names_the_four(words_case):
    m = words_case["m"]
    listed = np.arange(1, 5001, dtype=np.uint32)
    for p, min_degree in ((100, 5), (300, 2)):
        one, two, three = (m.cluster_cores(listed, p, min_degree) for _ in range(3))
        assert m.last_kernels() == KERNELS
        for k in range(3):
            assert one[k].tobytes() == two[k].tobytes() == three[k].tobytes()
        assert one[3:] == two[3:] == three[3:]
        assert len({CORE, BORDER, NOISE} & set(one[2].tolist())) == 3


def test_the_calls_around_a_cores_call_are_unchanged(words_case):
    c = words_case
    m = c["m"]
    packed, offsets = _pack(c["needles"])
    listed = np.arange(1, 5001, dtype=np.uint32)
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    find_kernels = m.last_kernels()
    before_cluster = m.cluster(listed, 300)
    cluster_kernels = m.last_kernels()
    before_centres = m.cluster_centres(listed, 300)
    centres_kernels = m.last_kernels()
    cores = m.cluster_cores(listed, 300, 2)
    assert m.last_kernels() == KERNELS
    assert np.array_equal(cores[1], before_centres[1]) and cores[4] == before_centres[5] == before_cluster[2]
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == find_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    after_cluster = m.cluster(listed, 300)
    assert m.last_kernels() == cluster_kernels and "cluster_sweep_kernel" in cluster_kernels
    assert after_cluster[0].tobytes() == before_cluster[0].tobytes() and after_cluster[1:] == before_cluster[1:]
    after_centres = m.cluster_centres(listed, 300)
    assert m.last_kernels() == centres_kernels and "cluster_centres_sweep_kernel" in centres_kernels
    assert all(np.array_equal(x, y) for x, y in zip(before_centres[:4], after_centres[:4]))
    assert before_centres[4:] == after_centres[4:]
    assert _native.NO_CLUSTER == NO_CLUSTER
    assert (_native.KIND_NONE, _native.KIND_NOISE, _native.KIND_BORDER, _native.KIND_CORE) == (NONE, NOISE, BORDER, CORE)
