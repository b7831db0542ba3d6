"""Cluster centres on the GPU (cluster_centres.hip, cluster_centres_kernels.hip): per reference its label, its degree,
its component's centre and whether it is attached to that centre; the components and the edges.  Everything is
compared exactly with the host's truth (cluster_centres_truth.py over cluster_truth.py: numpy over the strings'
tokenisations, nothing of the library), labels and counts also with a separate blurrily_storage_cluster call, and the
degrees must sum to twice the edges.  Over the oracle haystacks at six floors (at least one floor per haystack has a
chain with an unattached member, a star and a singleton: asserted), hand-made chains, a triangle with a pendant, a
bridge held but not listed, a pair at its floor, the counter widths' node sizes, a shuffled list with repeats and
absent references, a haystack of more than one window, mutations, repeated calls, the call without `attached`, and
beside the find and the other cluster calls, which it leaves as they were."""
import numpy as np
import pytest

import workloads as W
from blurrily_amd import RawMap, _native
from blurrily_amd.map import _pack
from cluster_centres_truth import CentresTruth
from cluster_truth import NO_CLUSTER, Truth
from helpers import ORACLE_CASES, Oracle, oracle_case_inputs

pytestmark = pytest.mark.gpu
FLOORS = (0, 1, 300, 500, 700, 1000)
MARK = "cluster_centres_sweep_kernel<mark>"


def check(m, truth, listed, p, least=0):
    """One call against the truth and the separate cluster call, exactly.  Returns the truth."""
    labels, degrees, centres, attached, n_clusters, n_edges = m.cluster_centres(listed, p)
    want = CentresTruth(truth, listed, p, least)
    s_labels, s_clusters, s_edges = m.cluster(listed, p)
    print(f"floor {p}: {len(want.label_of)} nodes, clusters {n_clusters} (truth {want.n_clusters}, cluster {s_clusters}), "
          f"edges {n_edges} (truth {want.n_edges}, cluster {s_edges}), degrees' sum {int(degrees.sum(dtype=np.uint64))}, "
          f"unattached {int((attached == 0).sum())} (truth {int((want.attached == 0).sum())})")
    assert n_edges == want.n_edges == s_edges, p
    assert n_clusters == want.n_clusters == s_clusters, p
    assert labels.dtype == np.uint32 and np.array_equal(labels, want.labels) and labels.tobytes() == s_labels.tobytes(), p
    assert degrees.dtype == np.uint32 and np.array_equal(degrees, want.degrees), p
    assert centres.dtype == np.uint32 and np.array_equal(centres, want.centres), p
    assert attached.dtype == np.uint8 and np.array_equal(attached, want.attached), p
    _, first = np.unique(np.asarray(listed), return_index=True)  # (a reference listed twice is one node)
    assert int(degrees[first].sum(dtype=np.uint64)) == 2 * n_edges, p
    return want


def _map_of(held, weights=None):
    refs = np.array(sorted(held), dtype=np.uint32)
    m = RawMap()
    m.put_many_packed(*_pack([held[int(r)] for r in refs]), refs,
                      np.zeros(len(refs), dtype=np.uint32) if weights is None else weights)
    return m


@pytest.mark.parametrize("kind,n,_limit", ORACLE_CASES)
def test_everything_equals_the_truth_at_every_floor(kind, n, _limit):
    hay, off, _ = oracle_case_inputs(kind, n)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    m, truth = _map_of(held), Truth(held)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    # (worked out from the truth on the CPU: 300 has all three on every haystack; geonames and skewed also at 500)
    telling = [p for p in FLOORS if all(check(m, truth, listed, p).telling())]
    assert telling, "no floor leaves this haystack a chain with an unattached member, a star and a singleton"
    m.close()


def _j(a, b):
    """(m, union) of two strings."""
    A, B = set(Oracle.tokenise(a)), set(Oracle.tokenise(b))
    return len(A & B), len(A | B)


# five parts without a letter in common: strings made of two neighbouring parts share trigrams exactly when they share
# a part
S = [b"abcde", b"fghij", b"klmno", b"pqrst", b"uvwxy"]
CA, CB, CC, CD = S[0] + S[1], S[1] + S[2], S[2] + S[3], S[3] + S[4]


def _answers(m, listed, p):
    labels, degrees, centres, attached, n_clusters, n_edges = m.cluster_centres(listed, p)
    return labels.tolist(), degrees.tolist(), centres.tolist(), attached.tolist(), n_clusters, n_edges


def test_hand_made_chains_and_where_the_tie_falls():
    for x, y in ((CA, CB), (CB, CC), (CC, CD)):
        assert _j(x, y)[0] >= 1
    for x, y in ((CA, CC), (CA, CD), (CB, CD)):
        assert _j(x, y)[0] == 0
    low = min(1000 * _j(x, y)[0] // _j(x, y)[1] for x, y in ((CA, CB), (CB, CC), (CC, CD)))   # every link holds up to here
    assert low >= 2
    # A - B - C, the ends not similar: B is the centre and touches both
    held = {1: CA, 2: CB, 3: CC}
    m, truth = _map_of(held), Truth(held)
    for p in (1, low):
        assert _answers(m, [1, 2, 3], p) == ([1, 1, 1], [1, 2, 1], [2, 2, 2], [1, 1, 1], 1, 2)
        check(m, truth, [1, 2, 3], p)
    m.close()
    # A - B - C - D: B and C tie at two edges, the smaller reference is the centre, the far end is unattached
    held = {1: CA, 2: CB, 3: CC, 4: CD}
    m, truth = _map_of(held), Truth(held)
    for p in (1, low):
        assert _answers(m, [1, 2, 3, 4], p) == ([1, 1, 1, 1], [1, 2, 2, 1], [2, 2, 2, 2], [1, 1, 1, 0], 1, 3)
        check(m, truth, [1, 2, 3, 4], p)
    high = max(1000 * _j(x, y)[0] // _j(x, y)[1] for x, y in ((CA, CB), (CB, CC), (CC, CD)))
    assert _answers(m, [1, 2, 3, 4], high + 1) == ([1, 2, 3, 4], [0] * 4, [1, 2, 3, 4], [1] * 4, 4, 0)   # no link holds
    m.close()
    # the same four strings under other references: A 1, B 3, C 2, D 4 -- now C wins the tie and A is the far end
    held = {1: CA, 3: CB, 2: CC, 4: CD}
    m, truth = _map_of(held), Truth(held)
    for p in (1, low):
        assert _answers(m, [1, 2, 3, 4], p) == ([1, 1, 1, 1], [1, 2, 2, 1], [2, 2, 2, 2], [0, 1, 1, 1], 1, 3)
        check(m, truth, [1, 2, 3, 4], p)
    # the bridge B (3) held but not listed: A alone, C - D a pair; B adds to nobody's degree
    assert _answers(m, [1, 2, 4], 1) == ([1, 2, 2], [0, 1, 1], [1, 2, 2], [1, 1, 1], 2, 1)
    check(m, truth, [1, 2, 4], 1)
    m.close()


def test_a_triangle_with_a_pendant():
    core = S[0] + S[1] + S[2]
    X, Y, Z, P = core, core + b"z", core + S[3], S[3] + S[4]
    for x, y in ((X, Y), (X, Z), (Y, Z), (Z, P)):
        assert _j(x, y)[0] >= 1
    assert _j(X, P)[0] == 0 and _j(Y, P)[0] == 0
    held = {10: X, 20: Y, 30: Z, 40: P}
    m, truth = _map_of(held), Truth(held)
    listed = [10, 20, 30, 40]
    assert _answers(m, listed, 1) == ([10] * 4, [2, 2, 3, 1], [30] * 4, [1, 1, 1, 1], 1, 4)   # a star around Z
    check(m, truth, listed, 1)
    pendant = 1000 * _j(Z, P)[0] // _j(Z, P)[1]
    assert pendant < min(1000 * _j(x, y)[0] // _j(x, y)[1] for x, y in ((X, Y), (X, Z), (Y, Z)))
    check(m, truth, listed, pendant)
    # one permille above the pendant's edge: the triangle alone, all of degree two, the smallest reference its centre
    assert _answers(m, listed, pendant + 1) == ([10, 10, 10, 40], [2, 2, 2, 0], [10, 10, 10, 40], [1, 1, 1, 1], 2, 3)
    check(m, truth, listed, pendant + 1)
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


A, B, C = b"qxzqvwkj", b"qxzqvwkjxqzzvk", b"jxqzzvk"           # J(A, B) = 8 / 16, J(B, C) = 6 / 17, J(A, C) = 0


def test_the_exact_floor_node_sizes_and_the_shape_of_the_list():
    hay, off = W.words(3000, seed=5)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({5001: A, 5002: B, 5003: C})
    rng = np.random.default_rng(47)
    ref = 6000
    for t in (15, 16, 255, 256, 700):                         # both counter widths and their boundaries
        s = _needle_of(rng, t)
        assert len(Oracle.tokenise(s)) == t
        for variant in (s, s, s + b" zq", s[:-1]):
            held[ref] = variant
            ref += 1
    held[7001] = held[7002] = b""                             # T == 1
    assert len(Oracle.tokenise(b"")) == 1
    m, truth = _map_of(held), Truth(held)
    # a pair exactly at its floor (8 / 16 at 500) and one permille above
    assert _j(A, B) == (8, 16)
    assert _answers(m, [5001, 5002], 500) == ([5001, 5001], [1, 1], [5001, 5001], [1, 1], 1, 1)
    assert _answers(m, [5001, 5002], 501) == ([5001, 5002], [0, 0], [5001, 5002], [1, 1], 2, 0)
    everything = np.array(sorted(held), dtype=np.uint32)
    for p in (0, 200, 352, 353, 500, 501, 1000):              # the counter-width nodes among them, at every floor
        want = check(m, truth, everything, p)
    assert want.degree_of[6000] == want.degree_of[6001] == 1 and want.centre_of[6001] == 6000   # (equal strings at 1000)
    assert want.degree_of[7001] == 1 and want.centre_of[7002] == 7001
    # the list shuffled, with repeats and absent references mixed in
    rng = np.random.default_rng(5)
    absent = np.array([4000, 4001, 9999, 0xFFFFFFFF, 0], dtype=np.uint32)
    mixed = np.concatenate([everything, everything[::7], absent, absent[:2]])
    rng.shuffle(mixed)
    base = m.cluster_centres(everything, 200)
    got = m.cluster_centres(mixed, 200)
    assert got[4:] == base[4:]
    for k, nothing in ((0, NO_CLUSTER), (1, 0), (2, NO_CLUSTER), (3, 0)):
        of = dict(zip(everything.tolist(), base[k].tolist()))
        assert got[k].tolist() == [of.get(int(r), nothing) for r in mixed]   # (repeats equal, absent ones nothing)
        assert (got[k][np.isin(mixed, absent)] == nothing).all()
    check(m, truth, mixed, 200)
    # nothing listed; nothing held
    out = m.cluster_centres([], 500)
    assert [a.shape for a in out[:4]] == [(0,)] * 4 and out[4:] == (0, 0)
    out = m.cluster_centres(absent, 0)
    assert (out[0] == NO_CLUSTER).all() and (out[2] == NO_CLUSTER).all() and not out[1].any() and not out[3].any()
    assert out[4:] == (0, 0)
    m.close()


def test_a_haystack_of_more_than_one_window_all_references_a_strided_subset_and_a_shuffled_one():
    n = 70000
    hay, off = W.words(n, seed=17)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    weights = np.random.default_rng(23).integers(1, 1 << 20, size=n).astype(np.uint32)   # ranks unrelated to length
    m, truth = _map_of(held, weights), Truth(held)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    # (references and ranks are unrelated: a node's neighbours and its centre lie in the windows on both sides of its
    # own, so the marks are found from either end, and the subsets leave held references that are no nodes between them)
    want = check(m, truth, listed, 300, least=300)
    assert all(want.telling())
    assert m.device_info()["n_windows"] >= 2
    check(m, truth, listed[::3], 300, least=300)
    check(m, truth, np.random.default_rng(2).permutation(listed)[:30000], 300, least=300)
    m.close()


# a hub and what hangs on it, in trigrams that English words hardly have.  Per mille: H - X1 500, H - X2 384, H - X3 666,
# X1 - X3 400, X2 - X3 235, X1 - X2 nothing; N (put later) - H 615, N - X2 416, N - X3 411, N - X1 214
H, X1, X2, X3, N = b"klmnopqrst", b"klmnop", b"opqrst", b"klmnopqrstuvw", b"lmnopqrst"


def test_mutations_a_deleted_centre_a_pending_centre_a_reference_put_again_and_the_fold():
    permille = lambda x, y: 1000 * _j(x, y)[0] // _j(x, y)[1]
    assert [permille(*xy) for xy in ((H, X1), (H, X2), (H, X3), (X1, X3), (X2, X3))] == [500, 384, 666, 400, 235]
    assert _j(X1, X2)[0] == 0 and [permille(N, y) for y in (H, X2, X3, X1)] == [615, 416, 411, 214]
    hay, off = W.words(5000, seed=7)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({9001: X1, 9002: X2, 9003: H, 9004: X3})
    m = _map_of(held)
    m.sync_device()
    builds = m.device_info()["base_builds"]

    def verify():
        truth = Truth(held)
        listed = np.array(sorted(held) + [123456], dtype=np.uint32)
        return [check(m, truth, listed, p) for p in (400, 300)][1]

    want = verify()                                           # at 300: a star around H
    assert [want.degree_of[r] for r in (9001, 9002, 9003, 9004)] == [2, 1, 3, 2]
    assert [want.centre_of[r] for r in (9001, 9002, 9003, 9004)] == [9003] * 4
    m.delete(9003)                                            # the centre goes: the centre moves, X2 is alone
    del held[9003]
    want = verify()
    assert want.centre_of[9001] == want.centre_of[9004] == 9001 and want.centre_of[9002] == 9002
    m.put(H, 9500, 0)                                         # a pending put becomes the centre, from the delta image
    m.put(N, 9501, 0)                                         # ... and has a neighbour there
    held.update({9500: H, 9501: N})
    want = verify()
    assert m.device_info()["n_pending"] >= 2 and m.device_info()["base_builds"] == builds
    assert [want.degree_of[r] for r in (9001, 9002, 9004, 9500, 9501)] == [2, 2, 3, 4, 3]
    assert [want.centre_of[r] for r in (9001, 9002, 9004, 9500, 9501)] == [9500] * 5
    assert [want.attached_of[r] for r in (9001, 9002, 9004, 9500, 9501)] == [1] * 5
    m.delete(17)                                              # deleted and put again with another text
    m.put(X2 + b"u", 17, 0)
    held[17] = X2 + b"u"
    want = verify()
    assert want.label_of[17] == want.label_of[9002] == 17 and want.degree_of[17] >= 1 and want.centre_of[17] == 9500
    big, bo = W.words(9000, seed=34)                          # a log past its budget folds into a rebuilt base image
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    want = verify()
    info = m.device_info()
    assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    assert want.label_of[9500] == 17 and want.centre_of[9001] == 9500
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
    for p in (100, 300):
        one, two, three = (m.cluster_centres(listed, p) for _ in range(3))
        for k in range(4):
            assert one[k].tobytes() == two[k].tobytes() == three[k].tobytes()
        assert one[4:] == two[4:] == three[4:]


def test_without_attached_the_rest_is_the_same_and_the_second_sweep_is_not_run():
    m = words_case()["m"]
    listed = np.arange(1, 5001, dtype=np.uint32)
    full = m.cluster_centres(listed, 300)
    with_mark = m.last_kernels()
    assert with_mark == ["cluster_nodes_kernel", "cluster_centres_sweep_kernel", "cluster_label_kernel",
                         "cluster_centres_kernel", MARK]
    assert (full[3] == 0).any() and (full[3] == 1).any()
    lean = m.cluster_centres(listed, 300, attached=False)
    assert m.last_kernels() == with_mark[:-1]
    assert lean[3] is None and lean[4:] == full[4:]
    for k in range(3):
        assert lean[k].tobytes() == full[k].tobytes()
    # the shapes: numpy over the same call
    shapes = m.cluster_shapes(listed, 300)
    labels, degrees, centres, attached = full[:4]
    sizes = {}
    for lab in labels.tolist():
        sizes[lab] = sizes.get(lab, 0) + 1
    assert [s["label"] for s in shapes] == sorted(k for k, v in sizes.items() if v >= 2)
    for s in shapes:
        own = labels == s["label"]
        assert s == dict(label=s["label"], size=int(own.sum()), edges=int(degrees[own].sum()) // 2,
                         centre=int(centres[own][0]), attached=int(attached[own].sum()),
                         star=bool(attached[own].all()))
    assert sum(s["edges"] for s in shapes) == full[5]
    assert any(s["star"] for s in shapes) and not all(s["star"] for s in shapes)
    assert m.cluster_shapes(np.concatenate([listed[::-1], listed[:50], [77777]]), 300) == shapes


def test_the_calls_around_a_centres_call_are_unchanged():
    c = words_case()
    m = c["m"]
    packed, offsets = _pack(c["needles"])
    listed = np.arange(1, 5001, dtype=np.uint32)
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    find_kernels = m.last_kernels()
    before_cluster = m.cluster(listed, 300)
    cluster_kernels = m.last_kernels()
    before_levels = m.cluster_levels(listed, (200, 300))
    levels_kernels = m.last_kernels()
    m.cluster_centres(listed, 300)
    for name in ("cluster_sweep_kernel", "cluster_levels_sweep_kernel", "similar_sweep_kernel", "find_kernel"):
        assert name not in m.last_kernels()
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == find_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    after_cluster = m.cluster(listed, 300)
    assert m.last_kernels() == cluster_kernels and "cluster_sweep_kernel" in cluster_kernels
    assert after_cluster[0].tobytes() == before_cluster[0].tobytes() and after_cluster[1:] == before_cluster[1:]
    after_levels = m.cluster_levels(listed, (200, 300))
    assert m.last_kernels() == levels_kernels
    assert all(np.array_equal(x, y) for x, y in zip(before_levels, after_levels))
    assert _native.NO_CLUSTER == NO_CLUSTER
