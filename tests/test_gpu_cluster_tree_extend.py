"""Cluster tree extend on the GPU (cluster_tree_extend.hip, cluster_tree_extend_kernels.hip): the tree of old and new
references together, from the records the caller holds for the old ones and sweeps of the new ones alone.  In every
test the ``cluster_tree`` call over the old list feeds the extend, and the extend's records, both label arrays, the
components and the edges are compared exactly with ``cluster_tree`` over the two lists in one (the edges as that call's
minus the old call's) and with the host's truth (cluster_tree_extend_truth.py: Kruskal over the old records and the
pairs with a new end, nothing of the library).  Over the oracle haystacks split mod 7, records of a lower floor, the
displacement case built by hand and its mirror, twins of every counter width, the exact floor, ties, shuffled lists,
either list empty, a reference in both lists, records that are no tree's, a haystack of two windows, both images and
the fold, a deleted member, dense_case.py's map, a chain of extends, the launches of a case of several rounds, repeated
calls, and beside the find, ``cluster_tree`` and ``cluster_extend``, which it leaves as they were."""
import numpy as np
import pytest

import dense_case as D
import workloads as W
from blurrily_amd import RawMap
from blurrily_amd.map import _pack
from cluster_tree_extend_truth import TreeExtendTruth, boruvka_rounds
from cluster_truth import NO_CLUSTER, Truth
from helpers import ORACLE_CASES
from test_gpu_cluster_extend import A, A_SHORT, B, C, S, SHORT, TWIN0, WIDTHS, _j, _map_of, _needle_of
from test_gpu_cluster_tree import oracle_case, two_windows_case, N_TWO

pytestmark = pytest.mark.gpu
SWEEP, OFFER, RESOLVE = ("cluster_tree_extend_sweep_kernel", "cluster_tree_extend_offer_kernel",
                         "cluster_tree_extend_resolve_kernel")
NONE = np.zeros((0, 3), dtype=np.uint32)


def check(m, truth, old, held, new, floor, least=None):
    """One call against the truth: the records, both label arrays, components and edges, exactly.  Returns (the truth,
    the call's answer)."""
    old, new = np.asarray(old, dtype=np.uint32), np.asarray(new, dtype=np.uint32)
    got = m.cluster_tree_extend(old, held, new, floor)
    labels_old, labels_new, merges, n_clusters, n_edges = got
    want = TreeExtendTruth(truth, old, held, new, floor, least)
    print(f"floor {floor}: {len(old)} old, {len(new)} new, {len(want.of_ref)} nodes, {want.n_old_candidates} old records of "
          f"which {len(want.dropped)} displaced; merges {len(merges)} (truth {len(want.records)}), clusters {n_clusters} "
          f"(truth {want.n_clusters}), edges {n_edges} (truth {want.n_edges}: {want.old_new_edges} old-new, "
          f"{want.new_new_edges} new-new)")
    assert merges.dtype == np.uint32 and merges.shape == want.records.shape, floor
    assert merges.tobytes() == want.records.tobytes(), floor
    assert (n_clusters, n_edges) == (want.n_clusters, want.n_edges), floor
    assert labels_old.dtype == np.uint32 and labels_old.tobytes() == want.labels_old.tobytes(), floor
    assert labels_new.dtype == np.uint32 and labels_new.tobytes() == want.labels_new.tobytes(), floor
    assert len(merges) == len(want.of_ref) - n_clusters
    return want, got


def check_contract(m, truth, old, new, floor, f_old=None, least=None):
    """The contract: records from a separate ``cluster_tree(old)`` at f_old <= floor, the lists disjoint -- the extend
    equals ``cluster_tree`` over both lists byte for byte, and the truth.  Returns (the truth, the old records, the
    extend's answer)."""
    old, new = np.asarray(old, dtype=np.uint32), np.asarray(new, dtype=np.uint32)
    held = m.cluster_tree(old, floor if f_old is None else f_old)[1]
    old_edges = m.cluster_tree(old, floor)[3]
    want, got = check(m, truth, old, held, new, floor, least)
    labels, merges, n_clusters, n_edges = m.cluster_tree(np.concatenate([old, new]), floor)
    assert got[2].tobytes() == merges.tobytes(), floor
    assert np.concatenate([got[0], got[1]]).tobytes() == labels.tobytes(), floor
    assert got[3] == n_clusters and got[4] == n_edges - old_edges, floor
    return want, held, got


def _answers(m, old, held, new, floor):
    labels_old, labels_new, merges, n_clusters, n_edges = m.cluster_tree_extend(old, held, new, floor)
    return labels_old.tolist(), labels_new.tolist(), merges.tolist(), n_clusters, n_edges


@pytest.mark.parametrize("floor", (200, 500, 1000))
@pytest.mark.parametrize("kind,n,_limit", ORACLE_CASES)
def test_the_oracle_haystacks_with_every_seventh_reference_new(kind, n, _limit, floor):
    c = oracle_case(kind, n)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    check_contract(c["m"], c["truth"], listed[listed % 7 != 0], listed[listed % 7 == 0], floor, least=200)


def test_old_records_made_at_200_serve_a_call_at_500_and_displaced_records_are_told():
    kind, n, _ = ORACLE_CASES[0]
    c = oracle_case(kind, n)
    m, listed = c["m"], np.arange(1, n + 1, dtype=np.uint32)
    old, new = listed[listed % 7 != 0], listed[listed % 7 == 0]
    want, held, got = check_contract(m, c["truth"], old, new, 500, f_old=200, least=200)
    assert 0 < want.n_old_candidates < len(held)              # (the records below the floor are passed over)
    for kind, n, _ in ORACLE_CASES[1:]:
        c = oracle_case(kind, n)
        listed = np.arange(1, n + 1, dtype=np.uint32)
        check_contract(c["m"], c["truth"], listed[listed % 7 != 0], listed[listed % 7 == 0], 500, f_old=200, least=200)
    # at 200 the split displaces old records (the CPU test of the truth asserts as much): tree_changes names them
    c = oracle_case(*ORACLE_CASES[0][:2])
    want, held, got = check_contract(m, c["truth"], old, new, 200, least=200)
    assert len(want.dropped) >= 1
    removed, added = RawMap.tree_changes(held, got[2])
    assert removed.tolist() == [list(r) for r in sorted(want.dropped, key=lambda r: (-r[2], r[0], r[1]))]
    assert len(added) == len(got[2]) - len(held) + len(removed) and np.isin(added[:, :2], new).any(axis=1).all()


# the displacement case: A and B share 3 of 15 trigrams (200 per mille); N shares 5 of 14 with each (357); M shares 8 of
# 11 with B (727) and 3 of 16 with A (187)
D_A, D_B, D_N, D_M = b"abcdefgh", b"defghijk", b"bcdefghij", b"defghijkl"


def test_a_new_reference_displaces_an_old_record_and_the_mirror_case_keeps_it():
    assert _j(D_A, D_B) == (3, 15) and _j(D_A, D_N) == (5, 14) and _j(D_B, D_N) == (5, 14)
    assert _j(D_B, D_M) == (8, 11) and _j(D_A, D_M) == (3, 16)
    held = {10: D_A, 20: D_B, 30: D_N, 40: D_M}
    m, truth = _map_of(held), Truth(held)
    old_tree = m.cluster_tree([10, 20], 0)[1]
    assert old_tree.tolist() == [[10, 20, 200]]
    # N is closer to both: (A, N) and (B, N) are in, (A, B) is out
    want, _, got = check_contract(m, truth, [10, 20], [30], 0)
    assert got[2].tolist() == [[10, 30, 357], [20, 30, 357]]
    assert (got[0].tolist(), got[1].tolist(), got[3], got[4]) == ([10, 10], [10], 1, 2)
    assert want.dropped == [(10, 20, 200)]
    removed, added = RawMap.tree_changes(old_tree, got[2])
    assert removed.tolist() == [[10, 20, 200]] and added.tolist() == [[10, 30, 357], [20, 30, 357]]
    # the mirror: M is close to B alone -- (A, M) is the worst of its cycle, the old record survives
    want, _, got = check_contract(m, truth, [10, 20], [40], 0)
    assert got[2].tolist() == [[20, 40, 727], [10, 20, 200]] and got[4] == 2 and want.dropped == []
    removed, added = RawMap.tree_changes(old_tree, got[2])
    assert removed.shape == (0, 3) and added.tolist() == [[20, 40, 727]]
    # a floor above the old record, and one above the new edges too
    assert _answers(m, [10, 20], old_tree, [30], 201) == ([10, 10], [10], [[10, 30, 357], [20, 30, 357]], 1, 2)
    assert _answers(m, [10, 20], old_tree, [30], 358) == ([10, 20], [30], [], 3, 0)
    m.close()


@pytest.fixture(scope="module")
def built():
    """test_gpu_cluster_extend.py's built case in a map of its own: 3 000 words, the chain A - B - C, the pair one
    trigram short of it, nodes of 15, 16, 255, 256 and 700 trigrams with their twins, two empty strings.  Left unchanged."""
    hay, off = W.words(3000, seed=5)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({5001: A, 5002: B, 5003: C, 5004: SHORT, 5005: A_SHORT})
    rng = np.random.default_rng(47)
    for t in WIDTHS:
        s = _needle_of(rng, t)
        for k, variant in enumerate((s, s, s + b" zq", s[:-1])):
            held[TWIN0[t] + k] = variant
    held[7001] = held[7002] = b""                             # T == 1
    m = _map_of(held)
    yield dict(m=m, held=held, truth=Truth(held), everything=np.array(sorted(held), dtype=np.uint32))
    m.close()


def test_twins_both_new_and_one_old_one_new_at_every_counter_width(built):
    m, truth, everything = built["m"], built["truth"], built["everything"]
    for ref in list(TWIN0.values()) + [7001]:
        # both ends new: the pair at J = 1 is found once, and no needle finds itself
        assert _answers(m, [], NONE, [ref, ref + 1], 1000) == ([], [ref, ref], [[ref, ref + 1, 1000]], 1, 1), ref
        assert _answers(m, [], NONE, [ref], 0) == ([], [ref], [], 1, 0), ref
        # one old and one new, either way round: the new one finds the old one wherever it lies
        assert _answers(m, [ref], NONE, [ref + 1], 1000) == ([ref], [ref], [[ref, ref + 1, 1000]], 1, 1), ref
        assert _answers(m, [ref + 1], NONE, [ref], 1000) == ([ref], [ref], [[ref, ref + 1, 1000]], 1, 1), ref
    twins = np.array([r + k for r in TWIN0.values() for k in (0, 1)], dtype=np.uint32)
    for floor in (200, 1000):
        for new in (twins, twins[::2], twins[1::2]):
            want, _, got = check_contract(m, truth, everything[~np.isin(everything, new)], new, floor)
            rows = set(map(tuple, got[2].tolist()))
            assert all((r, r + 1, 1000) in rows for r in TWIN0.values())


def test_a_pair_exactly_at_its_floor_and_one_permille_above_it(built):
    m, truth, everything = built["m"], built["truth"], built["everything"]
    for a, b, p in ((5001, 5002, 500), (5004, 5005, 466)):
        for old, new in ((a, b), (b, a)):
            assert _answers(m, [old], NONE, [new], p) == ([a], [a], [[a, b, p]], 1, 1), (old, new, p)
            assert _answers(m, [old], NONE, [new], p + 1) == ([old], [new], [], 2, 0), (old, new, p)
        # ... and as an old record: in at its height, passed over one per mille above it
        assert _answers(m, [a, b], [(a, b, p)], [], p) == ([a, a], [], [[a, b, p]], 1, 0)
        assert _answers(m, [a, b], [(a, b, p)], [], p + 1) == ([a, b], [], [], 2, 0)
    old, new = everything[everything % 7 != 0], everything[everything % 7 == 0]
    for p in (0, 466, 467, 500, 501):
        check_contract(m, truth, old, new, p)


def test_four_identical_strings_split_two_old_two_new_follow_the_total_order():
    same = b"tied strings"
    held = {1: same, 2: same, 3: same, 4: same}
    m, truth = _map_of(held), Truth(held)
    star = [[1, 2, 1000], [1, 3, 1000], [1, 4, 1000]]
    for old, new in (([1, 2], [3, 4]), ([3, 4], [1, 2]), ([1, 4], [2, 3]), ([2, 3], [4, 1]), ([2, 3, 4], [1]), ([1], [4, 3, 2])):
        want, held_records, got = check_contract(m, truth, old, new, 1000)
        assert got[2].tolist() == star and got[3] == 1, (old, new)
        assert got[4] == 6 - len(old) * (len(old) - 1) // 2   # (the old ones' pairs are not looked at)
    # (3, 4) is the old tree; 1 and 2 arrive and every record of the new tree names 1: the old record is displaced
    removed, added = RawMap.tree_changes([(3, 4, 1000)], m.cluster_tree_extend([3, 4], [(3, 4, 1000)], [1, 2], 1000)[2])
    assert removed.tolist() == [[3, 4, 1000]] and added.tolist() == star
    m.close()


def test_both_lists_shuffled_with_repeats_and_absent_references_and_either_list_empty(built):
    m, truth, everything = built["m"], built["truth"], built["everything"]
    floor = 200
    old, new = everything[everything % 7 != 0], everything[everything % 7 == 0]
    want, held, base = check_contract(m, truth, old, new, floor)
    label_of = dict(zip(np.concatenate([old, new]).tolist(), np.concatenate([base[0], base[1]]).tolist()))
    rng = np.random.default_rng(5)
    absent = np.array([4000, 4001, 9999, 0xFFFFFFFF, 0], dtype=np.uint32)
    old_mixed = np.concatenate([old, old[::7], absent[:3]])
    new_mixed = np.concatenate([new, new[::3], absent[2:], absent[3:]])
    rng.shuffle(old_mixed)
    rng.shuffle(new_mixed)
    shuffled = held[rng.permutation(len(held))]               # (the records in any order)
    want, got = check(m, truth, old_mixed, shuffled, new_mixed, floor)
    assert got[2].tobytes() == base[2].tobytes() and got[3:] == base[3:]
    assert got[0].tolist() == [label_of.get(int(r), NO_CLUSTER) for r in old_mixed]   # (repeats equal, absent ones nothing)
    assert got[1].tolist() == [label_of.get(int(r), NO_CLUSTER) for r in new_mixed]
    assert (got[1][np.isin(new_mixed, absent)] == NO_CLUSTER).all()
    # new empty: the old records at or above the floor, and no sweep at all
    labels, merges, n_clusters, _ = m.cluster_tree(everything, floor)
    got = m.cluster_tree_extend(everything, merges, [], floor)
    assert got[0].tobytes() == labels.tobytes() and got[1].shape == (0,) and got[2].tobytes() == merges.tobytes()
    assert got[3:] == (n_clusters, 0)
    assert SWEEP not in m.last_kernels() and RESOLVE in m.last_kernels() and OFFER in m.last_kernels()
    check(m, truth, everything, merges, [], floor)
    want, got = check(m, truth, everything, merges, [], 350)
    assert got[2].tobytes() == merges[merges[:, 2] >= 350].tobytes() == m.cluster_tree(everything, 350)[1].tobytes()
    # old empty: cluster_tree(new_refs)
    for listed in (everything, new_mixed):
        labels, merges, n_clusters, n_edges = m.cluster_tree(listed, floor)
        got = m.cluster_tree_extend([], NONE, listed, floor)
        assert got[1].tobytes() == labels.tobytes() and got[0].shape == (0,) and got[2].tobytes() == merges.tobytes()
        assert got[3:] == (n_clusters, n_edges)
        assert SWEEP in m.last_kernels() and RESOLVE not in m.last_kernels() and OFFER not in m.last_kernels()
    check(m, truth, [], NONE, everything, floor)
    # nothing listed; nothing held
    got = m.cluster_tree_extend([], NONE, [], 300)
    assert (got[0].shape, got[1].shape, got[2].shape, got[3], got[4]) == ((0,), (0,), (0, 3), 0, 0)
    got = m.cluster_tree_extend(absent[:2], NONE, absent[2:], 0)
    assert (got[0] == NO_CLUSTER).all() and (got[1] == NO_CLUSTER).all() and got[2].shape == (0, 3) and got[3:] == (0, 0)


def test_a_reference_in_both_lists_is_new_and_its_old_records_are_dropped(built):
    m, truth = built["m"], built["truth"]
    # B is listed as old too: its records do not exist, its edges are found again from it as a new node
    want, got = check(m, truth, [5001, 5002, 5003], [(5001, 5002, 500), (5002, 5003, 352)], [5002], 300)
    assert want.n_old_candidates == 0 and got[2].tolist() == [[5001, 5002, 500], [5002, 5003, 352]] and got[4] == 2
    assert (got[0].tolist(), got[1].tolist(), got[3]) == ([5001, 5001, 5001], [5001], 1)
    # made-up heights on such records change nothing
    want, got = check(m, truth, [5001, 5002, 5003], [(5001, 5002, 900), (5002, 5003, 900)], [5002], 300)
    assert got[2].tolist() == [[5001, 5002, 500], [5002, 5003, 352]]
    everything = built["everything"]
    old = everything[everything % 7 != 0]
    both = np.concatenate([everything[everything % 7 == 0], old[::50]])
    held = m.cluster_tree(old, 200)[1]
    want, got = check(m, truth, old, held, both, 200)
    assert want.n_old_candidates < len(held)


def test_records_that_are_no_trees_a_cycle_a_duplicate_an_end_not_listed_and_an_end_deleted():
    # five parts without a letter in common: no similarity edge at all, whatever the records claim
    held = {1: S[0], 2: S[1], 3: S[2], 4: S[3], 5: S[4], 6: S[0] + b"z"}
    m, truth = _map_of(held), Truth(held)
    old = [1, 2, 3, 4, 5]
    # a cycle of made-up heights: its worst edge stays out
    cycle = [(1, 2, 700), (2, 3, 600), (1, 3, 650)]
    want, got = check(m, truth, old, cycle, [], 0)
    assert got[2].tolist() == [[1, 2, 700], [1, 3, 650]] and got[3] == 3 and want.dropped == [(2, 3, 600)]
    # a duplicate, and the same pair at two heights: one record, the higher
    want, got = check(m, truth, old, [(1, 2, 700), (1, 2, 700), (4, 5, 300), (4, 5, 900)], [], 0)
    assert got[2].tolist() == [[4, 5, 900], [1, 2, 700]]
    # an end not listed (7 is not held either; 6 is held) and a record between two such ends
    want, got = check(m, truth, [1, 2, 3], [(1, 6, 800), (2, 7, 800), (1, 2, 100)], [], 0)
    assert got[2].tolist() == [[1, 2, 100]] and want.n_old_candidates == 1
    # with a new reference that does have an edge: 6 joins 1 at its true height, the made-up cycle beside it
    want, got = check(m, truth, old, cycle, [6], 0)
    assert [6 in r[:2] for r in got[2].tolist()].count(True) == 1 and got[4] == 1 and got[3] == 3
    # an end deleted: its records are dropped, and what they held together falls apart
    m.delete(2)
    del held[2]
    truth = Truth(held)
    want, got = check(m, truth, old, [(1, 2, 700), (2, 3, 600), (4, 5, 500)], [6], 0)
    assert got[0].tolist() == [1, NO_CLUSTER, 3, 4, 4] and got[2].tolist()[-1] == [4, 5, 500] and want.n_old_candidates == 1
    m.close()


@pytest.mark.parametrize("which", ["every_seventh", "fifty"])
def test_a_haystack_of_two_windows(which):
    c = two_windows_case()
    m, truth, floor = c["m"], c["truth"], 300
    listed = np.arange(1, N_TWO + 1, dtype=np.uint32)
    if which == "every_seventh":
        new = listed[listed % 7 == 0]
    else:                                                     # fifty references that have an edge (by the truth)
        _, a, b, _ = truth.pairs(listed, floor)
        ends = truth.refs[np.stack([a, b], axis=1).reshape(-1)]
        new = np.sort(ends[np.sort(np.unique(ends, return_index=True)[1])][:50]).astype(np.uint32)
        assert len(new) == 50
    # (all the pairs sharing a trigram do not fit the host: the truth keeps the pairs at or above the floor)
    want, held, got = check_contract(m, truth, listed[~np.isin(listed, new)], new, floor, least=floor)
    assert m.device_info()["n_windows"] >= 2
    assert want.old_new_edges >= 1 and len(got[2]) > len(held) - len(want.dropped)


def test_both_images_either_way_round_the_fold_and_a_deleted_old_member():
    floor = 300
    hay, off = W.words(5000, seed=7)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({9001: A, 9002: B, 9003: C})
    m = _map_of(held)
    m.sync_device()
    builds = m.device_info()["base_builds"]
    old = np.array(sorted(held), dtype=np.uint32)
    stale = m.cluster_tree(old, floor)[1]                     # the caller's tree, B joining A and C
    assert [9001, 9002, 500] in stale.tolist() and [9002, 9003, 352] in stale.tolist()
    new = np.array([9500, 9501, 9502], dtype=np.uint32)
    # old nodes in the base image, new ones as pending puts: one repeats B, one has a neighbour in the delta image
    m.put(B, 9500, 0)
    m.put(B + b"x", 9501, 0)
    m.put(b"zzkkqqvv", 9502, 0)
    held.update({9500: B, 9501: B + b"x", 9502: b"zzkkqqvv"})
    truth = Truth(held)
    info = m.device_info()
    assert info["n_pending"] >= 3 and info["base_builds"] == builds
    want, held_records, got = check_contract(m, truth, old, new, floor)
    m.cluster_tree_extend(old, held_records, new, floor)
    kernels = m.last_kernels()                                # (two images: the base and the pending puts)
    assert kernels.count(SWEEP) == 2 * kernels.count(OFFER) == 2 * kernels.count("cluster_tree_merge_kernel") >= 4
    rows = got[2].tolist()
    assert [9002, 9500, 1000] in rows and want.new_new_edges >= 1 and want.old_new_edges >= 2
    # old nodes pending, new nodes in the base image: the pending ones alone, and with a seventh of the base image
    check_contract(m, truth, new, old, floor)
    pending_old, base_new = np.concatenate([old[old % 7 == 0], new]), old[old % 7 != 0]
    check_contract(m, truth, pending_old, base_new, floor)
    # a deleted old member: its records are dropped, the rest of the stale tree is taken on trust
    m.delete(9002)
    del held[9002]
    truth = Truth(held)
    want, got = check(m, truth, old, stale, new, floor)
    assert got[0][-3:].tolist() == [9001, NO_CLUSTER, 9001]   # (9500 repeats B and bridges them now)
    assert not any(9002 in r[:2] for r in got[2].tolist()) and want.n_old_candidates == len(stale) - 2
    # the same after the log folds into a rebuilt base image
    big, bo = W.words(9000, seed=34)
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    truth = Truth(held)
    old = old[old != 9002]
    for o, w in ((old, new), (pending_old[pending_old != 9002], base_new[base_new != 9002]), (np.concatenate([old, new]), bulk)):
        check_contract(m, truth, o, w, floor)
        info = m.device_info()                                # (the first call after the bulk put folds the log)
        assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    m.close()


def test_dense_slices_left_out_and_sixteen_bit_halves_on_the_dense_map():
    m, h = D.build()
    family = np.array([r for head in h.heads for r in h.family(head)], dtype=np.uint32)
    listed = np.concatenate([h.refs[:D.N_WORDS][::97], family])
    old, new = listed[listed % 5 != 1], listed[listed % 5 == 1]
    for side in (new, old):                                   # both counter widths, more dense slices than the list of 64 holds
        fam = [int(r) for r in side if r >= D.FAMILY_REF0]
        assert any(h.T(r) > 255 and h.dense(r, 0) > D.MAX_DENSE for r in fam)
        assert any(h.T(r) <= 255 and h.dense(r, 0) > D.MAX_DENSE for r in fam)
    for floor in (200, 350, 600):
        want, _, _ = check_contract(m, h.truth, old, new, floor, least=200)
        assert want.new_new_edges >= 1 and want.old_new_edges >= 1
    check_contract(m, h.truth, old, new, 600, f_old=200, least=200)
    m.close()


def test_four_extends_in_a_chain_equal_one_cluster_tree_call(built):
    m, truth, everything = built["m"], built["truth"], built["everything"]
    for floor in (200, 350):
        refs, labels, records = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), NONE
        edges = 0
        for k in range(4):
            part = everything[everything % 4 == k]
            want, got = check(m, truth, refs, records, part, floor)
            refs, labels, records = np.concatenate([refs, part]), np.concatenate([got[0], got[1]]), got[2]
            edges += got[4]
        whole = m.cluster_tree(refs, floor)
        assert labels.tobytes() == whole[0].tobytes() and records.tobytes() == whole[1].tobytes()
        assert got[3] == whole[2] and edges == whole[3]
        removed, added = RawMap.tree_changes(records, whole[1])
        assert len(removed) == 0 and len(added) == 0
        assert RawMap.cut_tree(refs, labels, records, 500, min_permille=floor).tobytes() == m.cluster(refs, 500)[0].tobytes()
        assert RawMap.merge_profile(records) == RawMap.merge_profile(whole[1])


def test_a_case_of_several_rounds_names_every_launch():
    kind, n, _ = ORACLE_CASES[0]
    c = oracle_case(kind, n)
    m, listed = c["m"], np.arange(1, n + 1, dtype=np.uint32)
    old, new = listed[listed % 7 != 0], listed[listed % 7 == 0]
    held = m.cluster_tree(old, 200)[1]
    want, got = check(m, c["truth"], old, held, new, 200, least=200)
    kernels = m.last_kernels()
    rounds, forest = boruvka_rounds(*want.candidates)
    refs = c["truth"].refs
    assert {(int(refs[a]), int(refs[b]), p) for a, b, p in forest} == set(map(tuple, got[2].tolist()))
    assert rounds >= 3, "this case no longer needs several merging rounds: the test shows nothing"
    images = 1 + (m.device_info()["n_pending"] > 0)
    assert images == 1 and len(new) <= 1 << 20                # (one image, one chunk of needles)
    launched = rounds + 1                                     # (the last round finds nothing to merge)
    assert kernels.count(SWEEP) == launched * images * 1
    assert kernels.count(OFFER) == launched and kernels.count(RESOLVE) == 1
    assert kernels.count("cluster_tree_merge_kernel") == launched
    assert kernels.count("cluster_tree_flatten_kernel") == launched + 1
    assert kernels.count("cluster_nodes_kernel") == 1 and kernels[-1] == "cluster_label_kernel"
    assert "cluster_tree_sweep_kernel" not in kernels and "cluster_extend_sweep_kernel" not in kernels
    assert kernels.index(RESOLVE) < kernels.index(SWEEP) < kernels.index(OFFER) < kernels.index("cluster_tree_merge_kernel")


def test_three_calls_give_identical_bytes():
    m = oracle_case(*ORACLE_CASES[0][:2])["m"]
    listed = np.arange(1, 5001, dtype=np.uint32)
    old, new = listed[listed % 7 != 0], listed[listed % 7 == 0]
    held = m.cluster_tree(old, 200)[1]
    one, two, three = (m.cluster_tree_extend(old, held, new, 200) for _ in range(3))
    for x, y, z in zip(one[:3], two[:3], three[:3]):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert one[3:] == two[3:] == three[3:]


def test_the_calls_around_a_tree_extend_are_unchanged():
    c = oracle_case(*ORACLE_CASES[0][:2])
    m = c["m"]
    packed, offsets = _pack(c["needles"])
    listed = np.arange(1, 5001, dtype=np.uint32)
    old, new = listed[listed % 7 != 0], listed[listed % 7 == 0]
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    find_kernels = m.last_kernels()
    before_tree = m.cluster_tree(listed, 200)
    tree_kernels = m.last_kernels()
    seeds = m.cluster(old, 200)[0]
    before_extend = m.cluster_extend(old, seeds, new, 200)
    extend_kernels = m.last_kernels()
    held = m.cluster_tree(old, 200)[1]
    m.cluster_tree_extend(old, held, new, 200)
    for name in ("cluster_nodes_kernel", RESOLVE, SWEEP, OFFER, "cluster_tree_merge_kernel", "cluster_tree_flatten_kernel",
                 "cluster_label_kernel"):
        assert name in m.last_kernels()
    assert "find_kernel" not in m.last_kernels()
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == find_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    after_tree = m.cluster_tree(listed, 200)
    assert m.last_kernels() == tree_kernels and not any("extend" in k for k in tree_kernels)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before_tree[:2], after_tree[:2])) and before_tree[2:] == after_tree[2:]
    after_extend = m.cluster_extend(old, seeds, new, 200)
    assert m.last_kernels() == extend_kernels and not any("tree" in k for k in extend_kernels)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before_extend[:2], after_extend[:2]))
    assert before_extend[2:] == after_extend[2:]
