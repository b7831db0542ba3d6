"""Cluster extend on the GPU (cluster_extend.hip, cluster_extend_kernels.hip): the clusters of old and new references
together, from the labels the caller holds for the old ones and a sweep of the new ones alone.  Both label arrays, the
components and the edges are compared exactly, every time, with the host's truth (cluster_extend_truth.py over
cluster_truth.py: numpy over the strings' tokenisations, nothing of the library) and, where the seeds are
``cluster``'s own labels, with ``cluster`` over the two lists in one: over the oracle haystacks split mod 7 at floors
where the split is telling (asserted), test_gpu_cluster.py's built case (the chain, twins of every counter width, the
exact floor), seeds that are no labels of ``cluster``, a haystack of two windows, both images either way round and the
fold, deletes and the documented recipe, dense_case.py's map, outputs fed back as inputs, repeated calls, and beside
the find and ``cluster``, which it leaves as they were."""
import numpy as np
import pytest

import dense_case as D
import workloads as W
from blurrily_amd import RawMap, _native
from blurrily_amd.map import _pack
from cluster_extend_truth import ExtendTruth
from cluster_truth import NO_CLUSTER, Truth
from helpers import ORACLE_CASES, Oracle, oracle_case_inputs

pytestmark = pytest.mark.gpu
KERNELS = ["cluster_nodes_kernel", "cluster_extend_seed_kernel", "cluster_extend_sweep_kernel", "cluster_label_kernel"]


def check(m, truth, old, seeds, new, p, least=0):
    """One call against the truth: both label arrays, components and edges, exactly.  Returns the truth."""
    old, seeds, new = (np.asarray(x, dtype=np.uint32) for x in (old, seeds, new))
    labels_old, labels_new, n_clusters, n_edges = m.cluster_extend(old, seeds, new, p)
    want = ExtendTruth(truth, old, seeds, new, p, least)
    print(f"floor {p}: {len(old)} old, {len(new)} new, {len(want.of_ref)} nodes, {want.n_seeds} seeds; clusters "
          f"{n_clusters} (truth {want.n_clusters}), edges {n_edges} (truth {want.n_edges}: {want.old_new_edges} old-new, "
          f"{want.new_new_edges} new-new)")
    assert n_edges == want.n_edges, p
    assert n_clusters == want.n_clusters, p
    assert labels_old.dtype == np.uint32 and np.array_equal(labels_old, want.labels_old), p
    assert labels_new.dtype == np.uint32 and np.array_equal(labels_new, want.labels_new), p
    return want


def check_contract(m, truth, old, new, p, least=0):
    """The contract: seeds from a separate ``cluster(old)``, the lists disjoint -- the extend equals ``cluster`` over
    both lists byte for byte, and the truth.  Returns (the truth, the seeds, the extend's answer)."""
    old, new = np.asarray(old, dtype=np.uint32), np.asarray(new, dtype=np.uint32)
    seeds, _, old_edges = m.cluster(old, p)
    want = check(m, truth, old, seeds, new, p, least)
    got = m.cluster_extend(old, seeds, new, p)
    whole, whole_clusters, whole_edges = m.cluster(np.concatenate([old, new]), p)
    assert np.concatenate([got[0], got[1]]).tobytes() == whole.tobytes(), p
    assert got[2] == whole_clusters and got[3] == whole_edges - old_edges, p
    return want, seeds, got


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


def _answers(m, old, seeds, new, p):
    labels_old, labels_new, n_clusters, n_edges = m.cluster_extend(old, seeds, new, p)
    return labels_old.tolist(), labels_new.tolist(), n_clusters, n_edges


def telling(old, seeds, labels_old):
    """(components that merge two or more old groups, old labels that change) of an extend over held old references."""
    pairs = np.unique(np.stack([np.asarray(labels_old, dtype=np.int64), np.asarray(seeds, dtype=np.int64)], axis=1), axis=0)
    _, groups = np.unique(pairs[:, 0], return_counts=True)
    return int((groups >= 2).sum()), int((np.asarray(seeds) != np.asarray(labels_old)).sum())


# (haystack, n, the floors, and per floor what a CPU run of the truth gave: components that merge two or more old
# groups, old labels that change, new-new edges)
ORACLE_FLOORS = {"words": ((200, 300), ((28, 1103, 63), (5, 25, 5))),
                 "geonames": ((500, 700), ((19, 869, 67597), (25, 1848, 26229))),
                 "skewed": ((500,), ((56, 626, 403),))}


@pytest.mark.parametrize("kind,n,_limit", ORACLE_CASES)
def test_the_oracle_haystacks_split_mod_seven_equal_cluster_and_the_truth(kind, n, _limit):
    hay, off, _ = oracle_case_inputs(kind, n)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    m, truth = _map_of(held), Truth(held)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    old, new = listed[listed % 7 != 0], listed[listed % 7 == 0]
    floors, figures = ORACLE_FLOORS[kind]
    for p, figure in zip(floors, figures):
        want, seeds, got = check_contract(m, truth, old, new, p, least=floors[0])
        has = telling(old, seeds, want.labels_old) + (want.new_new_edges,)
        print(f"{kind} at {p}: components that merge old groups, old labels that change, new-new edges: {has}")
        assert min(has) >= 1 and has == figure, (p, has)
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
SHORT, A_SHORT = B[:-1], A[:-1]                                # J = 7 / 15: 466 per mille
WIDTHS = (15, 16, 255, 256, 700)                               # both counter widths and their boundaries
TWIN0 = {t: 6000 + 4 * k for k, t in enumerate(WIDTHS)}        # reference of s; s again, s + " zq" and s[:-1] behind it


@pytest.fixture(scope="module")
def built():
    """test_gpu_cluster.py's built case in a map of its own: 3 000 words, the chain A - B - C, the pair one trigram
    short of it, nodes of 15, 16, 255, 256 and 700 trigrams with their twins, two empty strings.  Left unchanged."""
    hay, off = W.words(3000, seed=5)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({5001: A, 5002: B, 5003: C, 5004: SHORT, 5005: A_SHORT})
    rng = np.random.default_rng(47)
    for t in WIDTHS:
        s = _needle_of(rng, t)
        assert len(Oracle.tokenise(s)) == t
        for k, variant in enumerate((s, s, s + b" zq", s[:-1])):
            held[TWIN0[t] + k] = variant
    held[7001] = held[7002] = b""                             # T == 1
    assert len(Oracle.tokenise(b"")) == 1
    assert _j(A, B) == (8, 16) and _j(B, C) == (6, 17) and _j(A, C)[0] == 0 and _j(A_SHORT, SHORT) == (7, 15)
    m = _map_of(held)
    yield dict(m=m, held=held, truth=Truth(held), everything=np.array(sorted(held), dtype=np.uint32))
    m.close()


def test_the_chain_b_between_a_and_c_either_way_round_and_b_not_listed(built):
    m, truth, everything = built["m"], built["truth"], built["everything"]
    # B arrives between A and C at 350 and joins their two groups
    assert m.cluster([5001, 5003], 350)[0].tolist() == [5001, 5003]
    assert _answers(m, [5001, 5003], [5001, 5003], [5002], 350) == ([5001, 5001], [5001], 1, 2)
    # A and C arrive with B old
    assert _answers(m, [5002], [5002], [5001, 5003], 350) == ([5001], [5001, 5001], 1, 2)
    # B is held but not listed: nothing joins A and C, whichever of them is new
    assert _answers(m, [5001], [5001], [5003], 350) == ([5001], [5003], 2, 0)
    assert _answers(m, [5003], [5003], [5001], 350) == ([5003], [5001], 2, 0)
    assert _answers(m, [], [], [5001, 5003], 350) == ([], [5001, 5003], 2, 0)
    # ... and among everything else: B alone new, A and C new, B left out
    for new in ([5002], [5001, 5003]):
        old = everything[~np.isin(everything, new)]
        want, _, _ = check_contract(m, truth, old, new, 350)
        assert want.of_ref[5001] == want.of_ref[5002] == want.of_ref[5003] == 5001
    old = everything[~np.isin(everything, [5001, 5002, 5003, 5004, 5005])]   # (B's shortened copy would bridge them too)
    want, _, _ = check_contract(m, truth, old, [5001, 5003], 350)
    assert want.of_ref[5001] != want.of_ref[5003]


def test_twins_new_together_and_one_old_one_new_at_every_counter_width(built):
    m, truth, everything = built["m"], built["truth"], built["everything"]
    for t, ref in TWIN0.items():
        # s twice, both new: the pair at J = 1 is counted once, and no needle counts itself
        assert _answers(m, [], [], [ref, ref + 1], 1000) == ([], [ref, ref], 1, 1), t
        assert _answers(m, [], [], [ref], 1000) == ([], [ref], 1, 0), t
        assert _answers(m, [], [], [ref], 0) == ([], [ref], 1, 0), t
        # one old and one new, either way round: the new one finds the old one wherever it lies
        assert _answers(m, [ref], [ref], [ref + 1], 1000) == ([ref], [ref], 1, 1), t
        assert _answers(m, [ref + 1], [ref + 1], [ref], 1000) == ([ref], [ref], 1, 1), t
    twins = np.array([r + k for r in TWIN0.values() for k in (0, 1)], dtype=np.uint32)
    firsts, seconds = twins[::2], twins[1::2]
    for p in (200, 1000):
        for new in (twins, firsts, seconds):
            want, _, _ = check_contract(m, truth, everything[~np.isin(everything, new)], new, p)
            assert all(want.of_ref[r] == want.of_ref[r + 1] for r in TWIN0.values())
    # the empty strings: T == 1, equal sets
    assert _answers(m, [7001], [7001], [7002], 1000) == ([7001], [7001], 1, 1)
    assert _answers(m, [7002], [7002], [7001], 1000) == ([7001], [7001], 1, 1)


def test_a_pair_exactly_at_its_floor_and_one_permille_above_it(built):
    m, truth, everything = built["m"], built["truth"], built["everything"]
    for a, b, p in ((5001, 5002, 500), (5004, 5005, 466)):
        for old, new in ((a, b), (b, a)):
            assert _answers(m, [old], [old], [new], p) == ([a], [a], 1, 1), (old, new, p)
            assert _answers(m, [old], [old], [new], p + 1) == ([old], [new], 2, 0), (old, new, p)
        assert _answers(m, [], [], [a, b], p) == ([], [a, a], 1, 1)
        assert _answers(m, [], [], [a, b], p + 1) == ([], [a, b], 2, 0)
    # the whole case split mod 7, the counter-width nodes among old and new, at every floor
    old, new = everything[everything % 7 != 0], everything[everything % 7 == 0]
    assert any((r % 7 == 0) != ((r + 1) % 7 == 0) for r in TWIN0.values())   # (a twin on either side of the split)
    for p in (0, 200, 466, 467, 500, 501, 1000):
        check_contract(m, truth, old, new, p)


# five parts without a letter in common: strings share trigrams exactly when they share a part
S = [b"abcde", b"fghij", b"klmno", b"pqrst", b"uvwxy"]


def test_seeds_that_are_not_clusters_labels():
    held = {1: S[0] + b"z", 2: S[1], 5: S[0], 7: S[2], 8: S[3], 9: S[4], 12: S[3] + b"pq"}
    assert _j(held[1], held[5])[0] >= 1 and _j(held[8], held[12])[0] >= 1
    unrelated = [(2, 5), (2, 1), (7, 8), (8, 9), (7, 9), (2, 7), (5, 7)]
    assert all(_j(held[a], held[b])[0] == 0 for a, b in unrelated)
    m, truth = _map_of(held), Truth(held)

    def both(old, seeds, new, p=1):
        check(m, truth, old, seeds, new, p)
        return _answers(m, old, seeds, new, p)

    # two unrelated words are must-linked and stay together, the label either of them
    assert both([2, 5], [2, 2], []) == ([2, 2], [], 1, 0)
    assert both([2, 5], [5, 5], []) == ([2, 2], [], 1, 0)
    assert both([2, 5], [2, 5], []) == ([2, 5], [], 2, 0)
    # a new node similar to one of them labels all three with the smallest
    assert both([2, 5], [5, 5], [1]) == ([1, 1], [1], 1, 1)
    assert both([2, 5], [2, 5], [1]) == ([2, 1], [1], 2, 1)
    # a chain a -> b, b -> c
    assert both([7, 8, 9], [8, 9, 9], []) == ([7, 7, 7], [], 1, 0)
    assert both([9, 8, 7], [8, 7, 7], [12]) == ([7, 7, 7], [7], 1, 1)
    # a label that is not listed (8 is held): no seed
    assert both([7], [8], []) == ([7], [], 1, 0)
    assert both([7, 9], [8, 8], []) == ([7, 9], [], 2, 0)
    # a label that is listed but not held, and an element that is not held
    assert both([7, 100, 9], [100, 100, 100], []) == ([7, NO_CLUSTER, 9], [], 2, 0)
    assert both([100, 7], [7, 7], [101]) == ([NO_CLUSTER, 7], [NO_CLUSTER], 1, 0)
    # a reference in both lists is new, and its seed -- and a seed that points at it -- is ignored
    assert both([2, 5], [2, 2], [5]) == ([2, 5], [5], 2, 0)
    assert both([2, 5], [5, 5], [5]) == ([2, 5], [5], 2, 0)
    assert both([2, 5, 7], [7, 7, 7], [5, 1]) == ([2, 1, 2], [1, 1], 2, 1)
    # nothing listed, nothing held
    assert _answers(m, [], [], [], 500) == ([], [], 0, 0)
    assert both([100], [100], [101, 0xFFFFFFFF]) == ([NO_CLUSTER], [NO_CLUSTER] * 2, 0, 0)
    m.close()


def test_both_lists_shuffled_with_repeats_and_either_list_empty(built):
    m, truth, everything = built["m"], built["truth"], built["everything"]
    p = 200
    old, new = everything[everything % 7 != 0], everything[everything % 7 == 0]
    want, seeds, base = check_contract(m, truth, old, new, p)
    label_of = dict(zip(np.concatenate([old, new]).tolist(), np.concatenate([base[0], base[1]]).tolist()))
    seed_of = dict(zip(old.tolist(), seeds.tolist()))
    rng = np.random.default_rng(5)
    absent = np.array([4000, 4001, 9999, 0xFFFFFFFF, 0], dtype=np.uint32)
    old_mixed = np.concatenate([old, old[::7], absent[:3]])
    new_mixed = np.concatenate([new, new[::3], absent[2:], absent[3:]])
    rng.shuffle(old_mixed)
    rng.shuffle(new_mixed)
    seeds_mixed = np.array([seed_of.get(int(r), NO_CLUSTER) for r in old_mixed], dtype=np.uint32)
    got = m.cluster_extend(old_mixed, seeds_mixed, new_mixed, p)
    assert got[2:] == base[2:]
    assert got[0].tolist() == [label_of.get(int(r), NO_CLUSTER) for r in old_mixed]   # (repeats equal, absent ones nothing)
    assert got[1].tolist() == [label_of.get(int(r), NO_CLUSTER) for r in new_mixed]
    assert (got[1][np.isin(new_mixed, absent)] == NO_CLUSTER).all() and NO_CLUSTER == _native.NO_CLUSTER
    check(m, truth, old_mixed, seeds_mixed, new_mixed, p)
    # n_new == 0: the components of the seeds alone -- with cluster's labels, those labels again
    labels, n_clusters, _ = m.cluster(everything, p)
    got = m.cluster_extend(everything, labels, [], p)
    assert got[0].tobytes() == labels.tobytes() and got[1].shape == (0,) and got[2:] == (n_clusters, 0)
    assert "cluster_extend_sweep_kernel" not in m.last_kernels() and "cluster_extend_seed_kernel" in m.last_kernels()
    check(m, truth, everything, labels, [], p)
    # n_old == 0: cluster(new_refs)
    for listed in (everything, new_mixed):
        labels, n_clusters, n_edges = m.cluster(listed, p)
        got = m.cluster_extend([], [], listed, p)
        assert got[1].tobytes() == labels.tobytes() and got[0].shape == (0,) and got[2:] == (n_clusters, n_edges)
        assert "cluster_extend_seed_kernel" not in m.last_kernels() and "cluster_extend_sweep_kernel" in m.last_kernels()
    check(m, truth, [], [], everything, p)


def test_a_haystack_of_two_windows_every_seventh_reference_new_and_fifty_new():
    n, p = 70000, 300
    hay, off = W.words(n, seed=17)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    weights = np.random.default_rng(23).integers(1, 1 << 20, size=n).astype(np.uint32)   # ranks unrelated to length
    m, truth = _map_of(held, weights), Truth(held)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    loc = D.locate(listed, weights)
    position = lambda r: loc[int(r)][0] * D.WINDOW_RANKS + loc[int(r)][1]

    def sides(want):
        """(new nodes with an old neighbour at a higher position, ... at a lower one, edges across the windows)."""
        higher, lower, across = set(), set(), 0
        for a, b in zip(*(x.tolist() for x in want.edge_refs)):
            across += loc[a][0] != loc[b][0]
            for x, y in ((a, b), (b, a)):
                if x in want.is_new_ref and y not in want.is_new_ref:
                    (higher if position(y) > position(x) else lower).add(x)
        return len(higher), len(lower), across

    # (all the pairs sharing a trigram do not fit the host: the truth keeps the pairs at or above the floor)
    want, _, _ = check_contract(m, truth, listed[listed % 7 != 0], listed[listed % 7 == 0], p, least=p)
    assert m.device_info()["n_windows"] >= 2
    has = sides(want)
    print(f"new nodes with an old neighbour at a higher position, at a lower one, edges across the windows: {has}")
    assert min(has) >= 1 and want.new_new_edges >= 1
    # fifty new references that have an edge (by the truth): tasks = n_windows, each needle gets many workgroups
    ends = np.stack(want.edge_refs, axis=1).reshape(-1)
    new = np.sort(ends[np.sort(np.unique(ends, return_index=True)[1])][:50]).astype(np.uint32)
    assert len(new) == 50
    want, _, _ = check_contract(m, truth, listed[~np.isin(listed, new)], new, p, least=p)
    has = sides(want)
    print(f"fifty new: {has}")
    assert min(has) >= 1
    m.close()


def test_both_images_either_way_round_the_fold_a_deleted_member_and_the_recipe():
    p = 350
    hay, off = W.words(5000, seed=7)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({9001: A, 9002: B, 9003: C})
    m = _map_of(held)
    m.sync_device()
    builds = m.device_info()["base_builds"]
    everything = lambda: np.array(sorted(held), dtype=np.uint32)
    old = everything()
    stale, _, _ = m.cluster(old, p)                           # the job's labels, B joining A and C
    assert stale[-3:].tolist() == [9001, 9001, 9001]

    # a deleted old member gets NO_CLUSTER; its group is taken on trust: the stale seeds keep A and C together
    m.delete(9002)
    del held[9002]
    truth = Truth(held)
    want = check(m, truth, old, stale, [], p)
    assert want.labels_old[-3:].tolist() == [9001, NO_CLUSTER, 9001]
    assert m.cluster([9001, 9003], p)[0].tolist() == [9001, 9003]
    # the documented recipe: cluster over the group's remaining members, its labels into old_labels, then extend
    old = everything()
    seeds = stale[np.isin(np.arange(1, 5001).tolist() + [9001, 9002, 9003], old)].copy()
    group = old[seeds == 9001]
    seeds[seeds == 9001] = m.cluster(group, p)[0]
    new = np.array([9500, 9501, 9502], dtype=np.uint32)

    # old nodes in the base image, new ones as pending puts: one bridges two base groups, one has a neighbour in the delta image
    m.put(B, 9500, 0)
    m.put(B + b"x", 9501, 0)
    m.put(b"zzkkqqvv", 9502, 0)
    held.update({9500: B, 9501: B + b"x", 9502: b"zzkkqqvv"})
    truth = Truth(held)
    info = m.device_info()
    assert info["n_pending"] >= 3 and info["base_builds"] == builds
    want = check(m, truth, old, seeds, new, p)
    assert want.of_ref[9001] == want.of_ref[9003] == want.of_ref[9500] == want.of_ref[9501] == 9001
    assert want.new_new_edges >= 1 and want.old_new_edges >= 2
    got = m.cluster_extend(old, seeds, new, p)
    whole = m.cluster(np.concatenate([old, new]), p)
    assert np.concatenate([got[0], got[1]]).tobytes() == whole[0].tobytes() and got[2] == whole[1]
    want, _, _ = check_contract(m, truth, old, new, p)
    # old nodes pending, new nodes in the base image: the pending ones alone, and with a seventh of the base image
    want, _, _ = check_contract(m, truth, new, old, p)
    assert want.of_ref[9001] == want.of_ref[9500] == 9001 and want.old_new_edges >= 2
    pending_old = np.concatenate([old[old % 7 == 0], new])
    base_new = old[old % 7 != 0]
    assert {9001, 9003} <= set(base_new.tolist())
    want, _, _ = check_contract(m, truth, pending_old, base_new, p)
    assert want.of_ref[9001] == want.of_ref[9500] == 9001
    # a reference deleted and put again with another text: a node of the delta image, its base rank no node
    m.delete(17)
    m.put(C + b"x", 17, 0)
    held[17] = C + b"x"
    truth = Truth(held)
    for o, w in ((old, new), (pending_old, base_new), (old[old != 17], np.concatenate([new, [17]]))):
        want, _, _ = check_contract(m, truth, o, w, p)
        assert want.of_ref[9003] == want.of_ref[17] == 17
    # the same after the log folds into a rebuilt base image
    big, bo = W.words(9000, seed=34)
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    truth = Truth(held)
    for o, w in ((old, new), (pending_old, base_new), (np.concatenate([old, new]), bulk)):
        want, _, _ = check_contract(m, truth, o, w, p)
        assert want.of_ref[9003] == want.of_ref[9500] == want.of_ref[17] == 17
        info = m.device_info()                                # (the first call after the bulk put folds the log)
        assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    m.close()


PAIR_FAMILY, PAIR_MEMBERS = 12, (4, 5)                         # the family pair whose permille p* gives the last two floors


def test_dense_slices_left_out_and_sixteen_bit_halves_on_the_dense_map():
    m, h = D.build()
    family = np.array([r for head in h.heads for r in h.family(head)], dtype=np.uint32)
    listed = np.concatenate([h.refs[:D.N_WORDS][::97], family])
    assert len(listed) == 812
    old, new = listed[listed % 5 != 1], listed[listed % 5 == 1]
    head = h.heads[PAIR_FAMILY]
    low, high = (head + k for k in PAIR_MEMBERS)
    p_star = h.permille(low, high)
    # a wide pair in the upper half of window 0, one of them new: an edge up to p*, none at p* + 1
    assert 350 <= p_star < 999 and (low % 5 == 1) != (high % 5 == 1) and h.T(low) > 255 and h.T(high) > 255
    assert all(h.loc[r][0] == 0 and h.loc[r][1] >= D.HALF for r in (low, high))
    # among the needles and among the old nodes: both counter widths with more dense slices than the list of 64 holds
    for side in (new, old):
        fam = [int(r) for r in side if r >= D.FAMILY_REF0]
        assert any(h.T(r) > 255 and h.dense(r, 0) > D.MAX_DENSE for r in fam)
        assert any(h.T(r) <= 255 and h.dense(r, 0) > D.MAX_DENSE for r in fam)
    # a wide new needle with a neighbour in the upper half window, and one in the other window
    new_set = set(new.tolist())
    for p in sorted((200, 350, 600, p_star, p_star + 1)):
        want, _, _ = check_contract(m, h.truth, old, new, p, least=200)
        pairs = {(min(a, b), max(a, b)) for a, b in zip(*(x.tolist() for x in want.edge_refs))}
        assert ((low, high) in pairs) == (p <= p_star), p
        if p == 350:
            upper = windows = False
            for a, b in zip(*(x.tolist() for x in want.edge_refs)):
                for x, y in ((a, b), (b, a)):
                    if x in new_set and h.T(x) > 255:
                        upper |= h.loc[y][0] == 0 and h.loc[y][1] >= D.HALF
                        windows |= h.loc[x][0] != h.loc[y][0]
            assert upper and windows and want.new_new_edges >= 1 and want.old_new_edges >= 1
    m.close()


def test_four_extends_each_fed_the_previous_outputs_equal_one_cluster_call(built):
    m, truth, everything = built["m"], built["truth"], built["everything"]
    for p in (200, 350):
        refs, labels = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
        edges = 0
        for k in range(4):
            part = everything[everything % 4 == k]
            want = check(m, truth, refs, labels, part, p)
            labels_old, labels_new, n_clusters, n_edges = m.cluster_extend(refs, labels, part, p)
            refs, labels = np.concatenate([refs, part]), np.concatenate([labels_old, labels_new])
            edges += n_edges
        whole, whole_clusters, whole_edges = m.cluster(refs, p)
        assert labels.tobytes() == whole.tobytes() and n_clusters == whole_clusters and edges == whole_edges
        moved, now = m.cluster_changes(refs, labels, whole)
        assert len(moved) == 0 and len(now) == 0


@pytest.fixture(scope="module")
def words_case():
    """The words oracle haystack in a map of its own, shared by the tests below and closed behind them."""
    hay, off, needles = oracle_case_inputs("words", 5000)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    m = _map_of(held)
    listed = np.arange(1, 5001, dtype=np.uint32)
    yield dict(m=m, needles=needles, old=listed[listed % 7 != 0], new=listed[listed % 7 == 0])
    m.close()


def test_three_calls_give_identical_bytes_and_last_kernels_names_the_four(words_case):
    m, old, new = words_case["m"], words_case["old"], words_case["new"]
    for p in (200, 300):
        seeds, _, _ = m.cluster(old, p)
        one = m.cluster_extend(old, seeds, new, p)
        two, three = (m.cluster_extend(old, seeds, new, p) for _ in range(2))
        assert m.last_kernels() == KERNELS
        for k in range(2):
            assert one[k].tobytes() == two[k].tobytes() == three[k].tobytes()
        assert one[2:] == two[2:] == three[2:]
        moved, now = m.cluster_changes(old, seeds, one[0])
        assert len(moved) >= 1 and np.array_equal(now, one[0][np.isin(old, moved)]) and (now < moved).all()


def test_a_fresh_maps_first_extend_names_the_per_rank_table_kernel_too():
    m = _map_of({1: S[0], 2: S[0] + b"z", 3: S[1]})
    assert _answers(m, [1, 3], [1, 3], [2], 1) == ([1, 3], [1], 2, 1)
    names = m.last_kernels()                                  # (a map's first floor sweep builds its per-rank table)
    assert "similar_ntri_kernel" in names and [k for k in names if k in KERNELS] == KERNELS
    assert _answers(m, [1, 3], [1, 3], [2], 1) == ([1, 3], [1], 2, 1)
    assert m.last_kernels() == KERNELS
    m.close()


def test_the_calls_around_an_extend_are_unchanged(words_case):
    c = words_case
    m, old, new = c["m"], c["old"], c["new"]
    packed, offsets = _pack(c["needles"])
    listed = np.concatenate([old, new])
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    find_kernels = m.last_kernels()
    before_cluster = m.cluster(listed, 300)
    cluster_kernels = m.last_kernels()
    seeds, _, old_edges = m.cluster(old, 300)
    got = m.cluster_extend(old, seeds, new, 300)
    assert m.last_kernels() == KERNELS
    assert np.concatenate([got[0], got[1]]).tobytes() == before_cluster[0].tobytes()
    assert got[2] == before_cluster[1] and got[3] == before_cluster[2] - old_edges
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == find_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    after_cluster = m.cluster(listed, 300)
    assert m.last_kernels() == cluster_kernels and "cluster_sweep_kernel" in cluster_kernels
    assert "cluster_extend_sweep_kernel" not in cluster_kernels and "cluster_extend_seed_kernel" not in cluster_kernels
    assert after_cluster[0].tobytes() == before_cluster[0].tobytes() and after_cluster[1:] == before_cluster[1:]
