"""Cluster extend within blocks on the GPU (cluster_extend_within.hip, cluster_extend_within_kernels.hip): the clusters
of old and new references together inside caller-given blocks, from the labels the caller holds for the old ones, only
the new members of a block scored against it.  Both label arrays, the components and the edges are compared exactly,
every time, under "scope_strategy" 0 (auto), 1 (every such block swept) and 2 (every such block scored directly) unless
a strategy is named: with the host's truth (cluster_extend_within_truth.py: numpy over the strings' tokenisations,
nothing of the library) and, where the seeds are ``cluster_within``'s own labels, with ``cluster_within`` over the two
lists in one.  Over the oracle haystacks split mod 7 under interleaving keys at floors where the split is telling
(asserted), test_gpu_cluster.py's built case (a bridge under another key, the exact floor, twins of every counter
width inside a block and outside), blocks of every size of new and old members around the tile and the workgroup, seeds
that are no labels of ``cluster_within``, a haystack of two windows, both images either way round, the fold, a delete
and the documented recipe, dense_case.py's map, outputs fed back as inputs, the degenerate forms, auto's choice at the
cap, repeated calls, and beside the find, ``cluster_within`` and ``cluster_extend``, which it leaves as they were."""
import numpy as np
import pytest

import dense_case as D
import workloads as W
from blurrily_amd import _native
from blurrily_amd.map import _pack
from cluster_extend_within_truth import ORACLE_TABLE, ExtendWithinTruth
from cluster_truth import NO_CLUSTER
from cluster_within_truth import WithinTruth
from helpers import oracle_case_inputs
from test_gpu_cluster import A, B, C, _j, _map_of, built_case

pytestmark = pytest.mark.gpu
STRATEGIES = (0, 1, 2)                                        # "scope_strategy": auto, the sweep, the direct kernel
G = 16                                                        # the direct kernel's tile (cluster_plan.h: kClusterWithinTile)
SEED, DIRECT, SWEEP = ("cluster_extend_within_seed_kernel", "cluster_extend_within_kernel",
                       "cluster_extend_within_sweep_kernel")
SEQUENCE = {2: ["cluster_nodes_kernel", SEED, DIRECT, "cluster_label_kernel"],
            1: ["cluster_nodes_kernel", SEED, SWEEP, "cluster_label_kernel"],
            0: ["cluster_nodes_kernel", SEED, DIRECT, "cluster_label_kernel"]}   # (auto below the cap: direct)


def _u32(x):
    return np.asarray(x, dtype=np.uint32)


def check(m, truth, old, okeys, seeds, new, nkeys, p, least=0, strategies=STRATEGIES):
    """One call under every strategy against the truth: both label arrays, components and edges, exactly.  Returns
    the truth."""
    old, okeys, seeds, new, nkeys = (_u32(x) for x in (old, okeys, seeds, new, nkeys))
    want = ExtendWithinTruth(truth, old, okeys, seeds, new, nkeys, p, least)
    for s in strategies:
        m.set_option("scope_strategy", s)
        labels_old, labels_new, n_clusters, n_edges = m.cluster_extend_within(old, okeys, seeds, new, nkeys, p)
        print(f"floor {p} strategy {s}: {len(old)} old, {len(new)} new, {len(want.of_ref)} nodes, {want.n_seeds} seeds; "
              f"clusters {n_clusters} (truth {want.n_clusters}), edges {n_edges} (truth {want.n_edges}: "
              f"{want.old_new_edges} old-new, {want.new_new_edges} new-new; {want.cross_key_edges} cut by the keys)")
        assert n_edges == want.n_edges, (p, s)
        assert n_clusters == want.n_clusters, (p, s)
        assert labels_old.dtype == np.uint32 and np.array_equal(labels_old, want.labels_old), (p, s)
        assert labels_new.dtype == np.uint32 and np.array_equal(labels_new, want.labels_new), (p, s)
    m.set_option("scope_strategy", 0)
    return want


def against_within(m, old, okeys, new, nkeys, p, strategies=STRATEGIES):
    """The contract without a truth: seeds from a separate ``cluster_within(old)``, the lists disjoint -- the extend
    equals ``cluster_within`` over both lists byte for byte under every strategy, n_edges the difference of the two
    counts.  Returns (the seeds, the last answer)."""
    old, okeys, new, nkeys = (_u32(x) for x in (old, okeys, new, nkeys))
    m.set_option("scope_strategy", 0)
    seeds, _, old_edges = m.cluster_within(old, okeys, p)
    whole, whole_clusters, whole_edges = m.cluster_within(np.concatenate([old, new]), np.concatenate([okeys, nkeys]), p)
    for s in strategies:
        m.set_option("scope_strategy", s)
        got = m.cluster_extend_within(old, okeys, seeds, new, nkeys, p)
        print(f"floor {p} strategy {s}: clusters {got[2]} ({whole_clusters}), edges {got[3]} ({whole_edges} - {old_edges})")
        assert np.concatenate([got[0], got[1]]).tobytes() == whole.tobytes(), (p, s)
        assert got[2] == whole_clusters and got[3] == whole_edges - old_edges, (p, s)
    m.set_option("scope_strategy", 0)
    return seeds, got


def check_contract(m, truth, old, okeys, new, nkeys, p, least=0, strategies=STRATEGIES):
    """The contract against ``cluster_within`` over both lists and against the truth.  Returns (the truth, the seeds,
    the extend's answer)."""
    seeds, got = against_within(m, old, okeys, new, nkeys, p, strategies)
    return check(m, truth, old, okeys, seeds, new, nkeys, p, least, strategies), seeds, got


def _answers(m, old, okeys, seeds, new, nkeys, p):
    """The four outputs as plain values, the same under the three strategies (asserted)."""
    out = []
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        labels_old, labels_new, n_clusters, n_edges = m.cluster_extend_within(old, okeys, seeds, new, nkeys, p)
        out.append((labels_old.tolist(), labels_new.tolist(), n_clusters, n_edges))
    m.set_option("scope_strategy", 0)
    assert out[0] == out[1] == out[2], out
    return out[0]


def telling(seeds, labels_old):
    """(components that merge two or more old groups, old labels that change) of an extend over old references."""
    held = np.asarray(seeds) != NO_CLUSTER
    pairs = np.unique(np.stack([np.asarray(labels_old, dtype=np.int64)[held], np.asarray(seeds, dtype=np.int64)[held]],
                               axis=1), axis=0)
    _, groups = np.unique(pairs[:, 0], return_counts=True)
    return int((groups >= 2).sum()), int((np.asarray(seeds) != np.asarray(labels_old)).sum())


_CASES = {}


def oracle_case(kind, n):
    """The map and the truth of an oracle haystack, made once."""
    if (kind, n) not in _CASES:
        hay, off, needles = oracle_case_inputs(kind, n)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        _CASES[kind, n] = dict(m=_map_of(held), truth=WithinTruth(held), needles=needles,
                               listed=np.arange(1, n + 1, dtype=np.uint32))
    return _CASES[kind, n]


# 1 ---- the oracle haystacks

@pytest.mark.parametrize("kind,n,modulus,p,figures", ORACLE_TABLE, ids=[f"{c[0]}-{c[2]}-{c[3]}" for c in ORACLE_TABLE])
def test_the_oracle_haystacks_split_mod_seven_equal_cluster_within_and_the_truth(kind, n, modulus, p, figures):
    c = oracle_case(kind, n)
    m, truth, listed = c["m"], c["truth"], c["listed"]
    old, new = listed[listed % 7 != 0], listed[listed % 7 == 0]
    want, seeds, got = check_contract(m, truth, old, old % modulus, new, new % modulus, p, least=p)
    has = telling(seeds, want.labels_old) + (want.new_new_edges, want.cross_key_edges)
    print(f"{kind} % {modulus} at {p}: components that merge old groups, old labels that change, new-new edges, "
          f"cross-key edges with a new end: {has}")
    assert min(has) >= 1 and has == figures, (p, has)
    assert not want.spans_two_keys()
    both = np.concatenate([old, new])
    labels = np.concatenate([got[0], got[1]])
    assert (labels % modulus == both % modulus).all()           # (every reference is held: no component spans two keys)


# 2 ---- built cases

@pytest.fixture(scope="module")
def built():
    """test_gpu_cluster.py's built case in a map of its own, with the pair one trigram short of A - B and a copy of
    the bridge B below A and C.  Left unchanged."""
    held = built_case()
    held.update({5004: B[:-1], 5005: A[:-1], 4000: B})          # 7 / 15 against each other: 466 per mille
    assert _j(A, B) == (8, 16) and _j(B, C) == (6, 17) and _j(A, C)[0] == 0 and _j(A[:-1], B[:-1]) == (7, 15)
    m = _map_of(held)
    yield dict(m=m, held=held, truth=WithinTruth(held), everything=np.array(sorted(held), dtype=np.uint32))
    m.close()


def test_a_bridge_under_another_key_the_exact_floor_and_twins_inside_and_outside_the_block(built):
    m, truth, everything = built["m"], built["truth"], built["everything"]
    ans = lambda *a: _answers(m, *a)
    # the bridge B new under another key than old A and C: nothing joins; under theirs: the chain
    assert ans([5001, 5003], [1, 1], [5001, 5003], [5002], [2], 350) == ([5001, 5003], [5002], 3, 0)
    assert ans([5001, 5003], [1, 1], [5001, 5003], [5002], [1], 350) == ([5001, 5001], [5001], 1, 2)
    # ... and the bridge with the lowest reference: both old labels move
    assert ans([5001, 5003], [1, 1], [5001, 5003], [4000], [2], 350) == ([5001, 5003], [4000], 3, 0)
    got = m.cluster_extend_within([5001, 5003], [1, 1], [5001, 5003], [4000], [1], 350)
    assert (got[0].tolist(), got[1].tolist(), got[2], got[3]) == ([4000, 4000], [4000], 1, 2)
    moved, now = m.cluster_changes([5001, 5003], [5001, 5003], got[0])
    assert (moved.tolist(), now.tolist()) == ([5001, 5003], [4000, 4000])
    # A and C new with B old, under one key and with C under another
    assert ans([5002], [1], [5002], [5001, 5003], [1, 1], 350) == ([5001], [5001, 5001], 1, 2)
    assert ans([5002], [1], [5002], [5001, 5003], [1, 2], 350) == ([5001], [5001, 5003], 2, 1)
    # pairs exactly at their floor and one per mille above with one end new, under one key and split
    for a, b, p in ((5001, 5002, 500), (5004, 5005, 466)):
        for old, new in ((a, b), (b, a)):
            assert ans([old], [3], [old], [new], [3], p) == ([a], [a], 1, 1), (old, new, p)
            assert ans([old], [3], [old], [new], [3], p + 1) == ([old], [new], 2, 0), (old, new, p)
            assert ans([old], [3], [old], [new], [8], p) == ([old], [new], 2, 0), (old, new, p)
            assert ans([old], [3], [old], [new], [8], p + 1) == ([old], [new], 2, 0), (old, new, p)
    # twins of T = 1, 15, 16, 255, 256 and 700, one old and one new either way round, inside the block and outside
    for t, ref in ((1, 7001), (15, 6000), (16, 6004), (255, 6008), (256, 6012), (700, 6016)):
        assert truth.R[np.searchsorted(truth.refs, ref)] == t
        for old, new in ((ref, ref + 1), (ref + 1, ref)):
            assert ans([old], [4], [old], [new], [4], 1000) == ([ref], [ref], 1, 1), t
            assert ans([old], [4], [old], [new], [5], 1000) == ([old], [new], 2, 0), t
            assert ans([old], [4], [old], [new], [5], 0) == ([old], [new], 2, 0), t
        assert ans([], [], [], [ref, ref + 1], [4, 4], 1000) == ([], [ref, ref], 1, 1), t
        assert ans([], [], [], [ref], [4], 0) == ([], [ref], 1, 0), t      # (no needle counts itself)
    # the whole case split mod 7: the words under three interleaving keys, everything built in a block of its own;
    # then the built nodes split from their variants by a second key
    old, new = everything[everything % 7 != 0], everything[everything % 7 == 0]
    assert any((r % 7 == 0) != ((r + 1) % 7 == 0) for r in (6000, 6004, 6008, 6012, 6016))
    key = lambda refs: np.where(refs >= 4000, 7, refs % 3).astype(np.uint32)
    for p in (0, 200, 466, 467, 500, 501, 1000):
        want, _, _ = check_contract(m, truth, old, key(old), new, key(new), p)
    assert want.of_ref[6000] == want.of_ref[6001] == 6000 and want.of_ref[7002] == 7001 and want.of_ref[6017] == 6016
    key = lambda refs: np.where(refs >= 4000, refs % 2 + 7, refs % 3).astype(np.uint32)
    want, _, _ = check_contract(m, truth, old, key(old), new, key(new), 1000)
    assert want.of_ref[6001] == 6001 and want.of_ref[7002] == 7002 and want.cross_key_edges >= 1


# 3 ---- tile geometry

@pytest.fixture(scope="module")
def words10000():
    hay, off = W.words(10000, seed=11)
    m = _map_of({i + 1: s for i, s in enumerate(W.unpack(hay, off))})
    yield m, np.arange(1, 10001, dtype=np.uint32)
    m.close()


def test_blocks_of_every_size_of_new_and_old_members_around_the_tile_and_the_workgroup(words10000):
    m, refs = words10000
    news, olds = (0, 1, G - 1, G, G + 1, 2 * G + 1), (0, 1, G - 1, G, 255, 256, 257, 600)
    shapes = [(a, b) for a in news for b in olds]
    rng = np.random.default_rng(29)
    picked = rng.permutation(refs)[:sum(a + b for a, b in shapes)].astype(np.uint32)   # the members anywhere
    keys = rng.permutation(np.arange(1000, 1000 + len(shapes), dtype=np.uint32))       # the key values in no order
    old, okeys, new, nkeys, at = [], [], [], [], 0
    for (a, b), k in zip(shapes, keys.tolist()):
        new += picked[at:at + a].tolist()
        old += picked[at + a:at + a + b].tolist()
        nkeys += [k] * a
        okeys += [k] * b
        at += a + b
    assert len(old) + len(new) == len(picked) == 9056
    p = 200
    seeds, got = against_within(m, old, okeys, new, nkeys, p)
    assert got[3] >= 1 and (seeds != got[0]).any()              # (edges with a new end exist, and an old label moves)
    # the lists shuffled: the same label per reference
    po, pn = rng.permutation(len(old)), rng.permutation(len(new))
    again = m.cluster_extend_within(_u32(old)[po], _u32(okeys)[po], seeds[po], _u32(new)[pn], _u32(nkeys)[pn], p)
    assert np.array_equal(again[0], got[0][po]) and np.array_equal(again[1], got[1][pn]) and again[2:] == got[2:]
    # no block has a new member: neither the direct nor the sweep kernel is launched, under any strategy
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        only = m.cluster_extend_within(old, okeys, seeds, [], [], p)
        assert m.last_kernels() == ["cluster_nodes_kernel", SEED, "cluster_label_kernel"], s
        assert only[0].tobytes() == seeds.tobytes() and only[3] == 0
    m.set_option("scope_strategy", 0)


# 4 ---- seeds that are no labels of cluster_within

# five parts without a letter in common: strings share trigrams exactly when they share a part
S = [b"abcde", b"fghij", b"klmno", b"pqrst", b"uvwxy"]


def test_seeds_that_are_not_cluster_withins_labels():
    held = {1: S[0] + b"z", 2: S[1], 5: S[0], 7: S[2], 8: S[3], 9: S[4], 12: S[3] + b"pq"}
    assert _j(held[1], held[5])[0] >= 1 and _j(held[8], held[12])[0] >= 1
    unrelated = [(2, 5), (2, 1), (7, 8), (8, 9), (7, 9), (2, 7), (5, 7)]
    assert all(_j(held[a], held[b])[0] == 0 for a, b in unrelated)
    m, truth = _map_of(held), WithinTruth(held)

    def both(old, okeys, seeds, new, nkeys, p=1):
        check(m, truth, old, okeys, seeds, new, nkeys, p)
        return _answers(m, old, okeys, seeds, new, nkeys, p)

    # two unrelated words under one key are must-linked and stay together; under two keys the seed does not exist
    assert both([2, 5], [1, 1], [2, 2], [], []) == ([2, 2], [], 1, 0)
    assert both([2, 5], [1, 1], [5, 5], [], []) == ([2, 2], [], 1, 0)
    assert both([2, 5], [1, 2], [5, 5], [], []) == ([2, 5], [], 2, 0)
    assert both([2, 5], [1, 2], [2, 2], [], []) == ([2, 5], [], 2, 0)
    # a new node similar to one of them labels all three with the smallest -- under the one key only
    assert both([2, 5], [1, 1], [5, 5], [1], [1]) == ([1, 1], [1], 1, 1)
    assert both([2, 5], [1, 1], [5, 5], [1], [2]) == ([2, 2], [1], 2, 0)
    assert both([2, 5], [1, 2], [5, 5], [1], [2]) == ([2, 1], [1], 2, 1)
    # a must-link chain a -> b, b -> c inside a key, and cut where the keys change
    assert both([7, 8, 9], [3, 3, 3], [8, 9, 9], [], []) == ([7, 7, 7], [], 1, 0)
    assert both([9, 8, 7], [3, 3, 3], [8, 7, 7], [12], [3]) == ([7, 7, 7], [7], 1, 1)
    assert both([7, 8, 9], [3, 3, 4], [8, 9, 9], [12], [3]) == ([7, 7, 9], [7], 2, 1)
    assert both([7, 8, 9], [3, 4, 4], [8, 9, 9], [12], [3]) == ([7, 8, 8], [12], 3, 0)
    # a label that is not listed (8 is held): no seed
    assert both([7], [3], [8], [], []) == ([7], [], 1, 0)
    assert both([7, 9], [3, 3], [8, 8], [], []) == ([7, 9], [], 2, 0)
    # a label that is listed but not held, and an element that is not held, in the middle of a block
    assert both([7, 100, 9], [3, 3, 3], [100, 100, 100], [], []) == ([7, NO_CLUSTER, 9], [], 2, 0)
    assert both([100, 7], [3, 3], [7, 7], [101], [3]) == ([NO_CLUSTER, 7], [NO_CLUSTER], 1, 0)
    assert both([7, 8, 9], [3, 3, 3], [7, 7, 7], [10, 12, 13], [3, 3, 3]) == ([7, 7, 7], [NO_CLUSTER, 7, NO_CLUSTER], 1, 1)
    # a reference in both lists is new, and its seed -- and a seed that points at it -- is ignored
    assert both([2, 5], [1, 1], [2, 2], [5], [1]) == ([2, 5], [5], 2, 0)
    assert both([2, 5], [1, 1], [5, 5], [5], [1]) == ([2, 5], [5], 2, 0)
    assert both([2, 5, 7], [1, 1, 1], [7, 7, 7], [5, 1], [1, 1]) == ([2, 1, 2], [1, 1], 2, 1)
    # nothing listed, nothing held
    assert _answers(m, [], [], [], [], [], 500) == ([], [], 0, 0)
    assert both([100], [1], [100], [101, 0xFFFFFFFF], [1, 1]) == ([NO_CLUSTER], [NO_CLUSTER] * 2, 0, 0)
    m.close()


def test_both_lists_shuffled_with_repeats_and_absent_references(built):
    m, truth, everything = built["m"], built["truth"], built["everything"]
    p = 200
    key = lambda refs: (refs % 5).astype(np.uint32)
    old, new = everything[everything % 7 != 0], everything[everything % 7 == 0]
    want, seeds, base = check_contract(m, truth, old, key(old), new, key(new), p)
    label_of = dict(zip(np.concatenate([old, new]).tolist(), np.concatenate([base[0], base[1]]).tolist()))
    seed_of = dict(zip(old.tolist(), seeds.tolist()))
    rng = np.random.default_rng(5)
    absent = np.array([4001, 4002, 9999, 0xFFFFFFFF, 0], dtype=np.uint32)
    old_mixed = np.concatenate([old, old[::7], absent[:3]])
    new_mixed = np.concatenate([new, new[::3], absent[2:], absent[3:], old[::11]])   # (a repeat across the lists: new)
    rng.shuffle(old_mixed)
    rng.shuffle(new_mixed)
    seeds_mixed = np.array([seed_of.get(int(r), NO_CLUSTER) for r in old_mixed], dtype=np.uint32)
    check(m, truth, old_mixed, key(old_mixed), seeds_mixed, new_mixed, key(new_mixed), p)
    # without the repeat across the lists: the contract's labels, per reference
    new_mixed = new_mixed[~np.isin(new_mixed, old)]
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        got = m.cluster_extend_within(old_mixed, key(old_mixed), seeds_mixed, new_mixed, key(new_mixed), p)
        assert got[2:] == base[2:]
        assert got[0].tolist() == [label_of.get(int(r), NO_CLUSTER) for r in old_mixed]   # (repeats equal, absent ones nothing)
        assert got[1].tolist() == [label_of.get(int(r), NO_CLUSTER) for r in new_mixed]
    m.set_option("scope_strategy", 0)
    assert (got[1][np.isin(new_mixed, absent)] == NO_CLUSTER).all() and NO_CLUSTER == _native.NO_CLUSTER


# 5 ---- more than one window

def test_a_haystack_of_two_windows_a_thousand_new_references_spread_over_both():
    n, p = 70000, 300
    hay, off = W.words(n, seed=17)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    weights = np.random.default_rng(23).integers(1, 1 << 20, size=n).astype(np.uint32)   # ranks unrelated to length
    m = _map_of(held, weights)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    new = np.sort(np.random.default_rng(3).permutation(listed)[:1000])
    old = listed[~np.isin(listed, new)]
    loc = D.locate(listed, weights)
    m.sync_device()
    assert m.device_info()["n_windows"] >= 2 and {loc[int(r)][0] for r in new} >= {0, 1}
    assert {loc[int(r)][0] for r in old[::97]} >= {0, 1}
    seeds, got = against_within(m, old, old % 7, new, new % 7, p, strategies=(1, 2))
    assert got[3] >= 1 and (seeds != got[0]).any()
    m.close()


# 6 ---- mutations

def test_both_images_either_way_round_the_fold_a_deleted_member_the_recipe_and_a_reference_put_again():
    p = 350
    hay, off = W.words(5000, seed=7)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({9001: A, 9002: B, 9003: C})
    m = _map_of(held)
    m.sync_device()
    builds = m.device_info()["base_builds"]
    everything = lambda: np.array(sorted(held), dtype=np.uint32)
    key = lambda refs: np.where((refs > 9000) & (refs < 9502), 1, np.where((refs == 9502) | (refs == 9503), 2, refs % 3)
                                ).astype(np.uint32)
    old = everything()
    stale, _, _ = m.cluster_within(old, key(old), p)          # the job's labels, B joining A and C inside key 1
    assert stale[-3:].tolist() == [9001, 9001, 9001]

    # a deleted old member gets NO_CLUSTER; its group is taken on trust: the stale seeds keep A and C together
    m.delete(9002)
    del held[9002]
    truth = WithinTruth(held)
    want = check(m, truth, old, key(old), stale, [], [], p)
    assert want.labels_old[-3:].tolist() == [9001, NO_CLUSTER, 9001]
    assert m.cluster_within([9001, 9003], [1, 1], p)[0].tolist() == [9001, 9003]
    # the documented recipe: cluster_within over the group's remaining members, its labels into old_labels, then extend
    seeds = stale[old != 9002].copy()
    old = everything()
    group = old[seeds == 9001]
    seeds[seeds == 9001] = m.cluster_within(group, key(group), p)[0]
    new = np.array([9500, 9501, 9502, 9503], dtype=np.uint32)

    # old nodes in the base image, new ones as pending puts: one bridges two base groups of its block and has a
    # neighbour in the delta image; their copies under another key join nothing there, and each other
    m.put(B, 9500, 0)
    m.put(B + b"x", 9501, 0)
    m.put(B, 9502, 0)
    m.put(B + b"x", 9503, 0)
    held.update({9500: B, 9501: B + b"x", 9502: B, 9503: B + b"x"})
    assert key(new).tolist() == [1, 1, 2, 2]
    truth = WithinTruth(held)
    info = m.device_info()
    assert info["n_pending"] >= 4 and info["base_builds"] == builds
    want = check(m, truth, old, key(old), seeds, new, key(new), p)
    assert want.of_ref[9001] == want.of_ref[9003] == want.of_ref[9500] == want.of_ref[9501] == 9001
    assert want.of_ref[9502] == want.of_ref[9503] == 9502
    assert want.new_new_edges >= 2 and want.old_new_edges >= 2 and want.cross_key_edges >= 4
    check_contract(m, truth, old, key(old), new, key(new), p)
    # old nodes pending, new nodes in the base image: the pending ones alone, and with a seventh of the base image
    want, _, _ = check_contract(m, truth, new, key(new), old, key(old), p)
    assert want.of_ref[9001] == want.of_ref[9500] == 9001 and want.old_new_edges >= 2
    pending_old = np.concatenate([old[old % 7 == 0], new])
    base_new = old[old % 7 != 0]
    assert {9001, 9003} <= set(base_new.tolist())
    want, _, _ = check_contract(m, truth, pending_old, key(pending_old), base_new, key(base_new), p)
    assert want.of_ref[9001] == want.of_ref[9500] == 9001
    # a reference deleted and put again with another text (16 % 3 == 1): a node of the delta image, its base rank none
    m.delete(16)
    m.put(C + b"x", 16, 0)
    held[16] = C + b"x"
    truth = WithinTruth(held)
    for o, w in ((old, new), (pending_old, base_new), (old[old != 16], np.concatenate([new, [16]]).astype(np.uint32))):
        want, _, _ = check_contract(m, truth, o, key(o), w, key(w), p)
        assert want.of_ref[9003] == want.of_ref[16] == 16
    # the same after the log folds into a rebuilt base image
    big, bo = W.words(9000, seed=34)
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    truth = WithinTruth(held)
    for o, w in ((old, new), (np.concatenate([old, new]), bulk)):
        want, _, _ = check_contract(m, truth, o, key(o), w, key(w), p)
        assert want.of_ref[9003] == want.of_ref[9500] == want.of_ref[16] == 16
        info = m.device_info()                                # (the first call after the bulk put folds the log)
        assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    m.close()


# 7 ---- the dense-slice map

def test_dense_slices_left_out_and_sixteen_bit_halves_on_the_dense_map():
    m, h = D.build()
    family = np.array([r for head in h.heads for r in h.family(head)], dtype=np.uint32)
    listed = np.concatenate([h.refs[:D.N_WORDS][::97], family]).astype(np.uint32)
    assert len(listed) == 812
    old, new = listed[listed % 5 != 1], listed[listed % 5 == 1]
    new_set = set(new.tolist())
    for p in (200, 350, 600):
        m.set_option("scope_strategy", 0)
        seeds, _, _ = m.cluster_within(old, old % 2, p)
        want = check(m, h.truth, old, old % 2, seeds, new, new % 2, p, least=200, strategies=(1, 2))
        assert want.old_new_edges >= 1 and want.cross_key_edges >= 1, p   # (the keys mod 2 part a family's new pairs)
        one, two = [], []
        for s, out in ((1, one), (2, two)):
            m.set_option("scope_strategy", s)
            out += m.cluster_extend_within(old, old % 2, seeds, new, new % 2, p)
        assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes() and one[2:] == two[2:]
    # a wide new needle is among the new ones, with more dense slices than the sweep's list holds
    assert any(h.T(int(r)) > 255 and h.dense(int(r), 0) > D.MAX_DENSE for r in new_set if r >= D.FAMILY_REF0)
    m.set_option("scope_strategy", 0)
    m.close()


# 8 ---- chained extends

def test_four_extends_each_fed_the_previous_outputs_equal_one_cluster_within_call(built):
    m, truth, everything = built["m"], built["truth"], built["everything"]
    key = lambda refs: np.where(refs >= 4000, 7, refs % 3).astype(np.uint32)
    for p in (200, 350):
        for s in STRATEGIES:
            refs, labels = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
            edges = 0
            for k in range(4):
                part = everything[everything % 4 == k]
                if s == 0:
                    check(m, truth, refs, key(refs), labels, part, key(part), p, strategies=(0,))
                m.set_option("scope_strategy", s)
                labels_old, labels_new, n_clusters, n_edges = m.cluster_extend_within(refs, key(refs), labels, part,
                                                                                      key(part), p)
                refs, labels = np.concatenate([refs, part]), np.concatenate([labels_old, labels_new])
                edges += n_edges
            m.set_option("scope_strategy", 0)
            whole, whole_clusters, whole_edges = m.cluster_within(refs, key(refs), p)
            assert labels.tobytes() == whole.tobytes() and n_clusters == whole_clusters and edges == whole_edges, (p, s)
            moved, now = m.cluster_changes(refs, labels, whole)
            assert len(moved) == 0 and len(now) == 0


# 9 ---- degenerate forms

def test_all_keys_equal_is_cluster_extend_no_old_is_cluster_within_and_no_new_is_the_seeds_alone():
    c = oracle_case("words", 5000)
    m, listed = c["m"], c["listed"]
    old, new = listed[listed % 7 != 0], listed[listed % 7 == 0]
    same = lambda refs: np.full(len(refs), 0xFFFFFFFF, dtype=np.uint32)
    for p in (200, 300):
        m.set_option("scope_strategy", 0)
        seeds, _, _ = m.cluster(old, p)
        plain = m.cluster_extend(old, seeds, new, p)
        stars = np.where(old % 2 == 0, old[0], seeds).astype(np.uint32)   # (must-links that are no labels of cluster)
        plain_stars = m.cluster_extend(old, stars, new, p)
        within = m.cluster_within(new, new % 3, p)
        blocked_seeds, n_blocked, _ = m.cluster_within(old, old % 3, p)
        for s in STRATEGIES:
            m.set_option("scope_strategy", s)
            # all keys equal: cluster_extend byte for byte
            for want, sd in ((plain, seeds), (plain_stars, stars)):
                got = m.cluster_extend_within(old, same(old), sd, new, same(new), p)
                assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (p, s)
                assert got[2:] == want[2:] and got[3] >= 1, (p, s)
            # n_old == 0: cluster_within(new_refs, new_blocks) byte for byte
            got = m.cluster_extend_within([], [], [], new, new % 3, p)
            assert got[0].shape == (0,) and got[1].tobytes() == within[0].tobytes() and got[2:] == within[1:], (p, s)
            assert SEED not in m.last_kernels() and (SWEEP if s == 1 else DIRECT) in m.last_kernels()
            # n_new == 0: the components of the seeds alone, n_edges 0 -- with cluster_within's labels, those again
            got = m.cluster_extend_within(old, old % 3, blocked_seeds, [], [], p)
            assert got[0].tobytes() == blocked_seeds.tobytes() and got[1].shape == (0,) and got[2:] == (n_blocked, 0)
            # ... and cluster's labels as seeds under keys: a seed holds only where its label carries the reference's key
            got = m.cluster_extend_within(old, old % 3, seeds, [], [], p)
            assert got[3] == 0 and (got[0] % 3 == old % 3).all() and (got[0] <= old).all()
    m.set_option("scope_strategy", 0)
    assert _answers(m, [], [], [], [], [], 1000) == ([], [], 0, 0)


# 10 ---- auto's choice

def test_auto_sweeps_a_block_above_the_direct_cap_and_scores_one_at_the_cap_directly():
    cap = 100000                                              # cluster_plan.h: kClusterExtendWithinDirectMax
    n = cap + 1
    hay, off = W.geonames(n, 2000, 41)
    m = _map_of({i + 1: s for i, s in enumerate(W.unpack(hay, off))})
    listed = np.arange(1, n + 1, dtype=np.uint32)
    new = listed[100::333][:300]
    old = listed[~np.isin(listed, new)]
    assert len(new) == 300 and len(old) + len(new) == cap + 1
    keys = lambda refs: np.full(len(refs), 9, dtype=np.uint32)
    m.set_option("scope_strategy", 0)
    seeds, _, old_edges = m.cluster_within(old[1:], keys(old[1:]), 700)
    whole = m.cluster_within(np.concatenate([old[1:], new]), keys(listed[1:]), 700)
    # cap members, old and new together: direct
    at_cap = m.cluster_extend_within(old[1:], keys(old[1:]), seeds, new, keys(new), 700)
    names = m.last_kernels()
    assert DIRECT in names and SWEEP not in names
    assert np.concatenate([at_cap[0], at_cap[1]]).tobytes() == whole[0].tobytes()
    assert at_cap[2] == whole[1] and at_cap[3] == whole[2] - old_edges and at_cap[3] >= 1
    # one listed member more (old[0], its own seed): swept
    more_seeds = np.concatenate([old[:1], seeds])
    above = m.cluster_extend_within(old, keys(old), more_seeds, new, keys(new), 700)
    names = m.last_kernels()
    assert SWEEP in names and DIRECT not in names
    for s in (1, 2):
        m.set_option("scope_strategy", s)
        forced = m.cluster_extend_within(old, keys(old), more_seeds, new, keys(new), 700)
        assert {k for k in m.last_kernels() if k in (SWEEP, DIRECT)} == {SWEEP if s == 1 else DIRECT}
        assert forced[0].tobytes() == above[0].tobytes() and forced[1].tobytes() == above[1].tobytes()
        assert forced[2:] == above[2:]
    m.set_option("scope_strategy", 0)
    m.close()


# 11 ---- around the call

def test_three_calls_give_identical_bytes_and_last_kernels_names_the_whole_sequence():
    c = oracle_case("words", 5000)
    m, listed = c["m"], c["listed"]
    old, new = listed[listed % 7 != 0], listed[listed % 7 == 0]
    for p in (200, 300):
        m.set_option("scope_strategy", 0)
        seeds, _, _ = m.cluster_within(old, old % 3, p)
        for s in STRATEGIES:
            m.set_option("scope_strategy", s)
            one = m.cluster_extend_within(old, old % 3, seeds, new, new % 3, p)
            two, three = (m.cluster_extend_within(old, old % 3, seeds, new, new % 3, p) for _ in range(2))
            assert m.last_kernels() == SEQUENCE[s], s
            for k in range(2):
                assert one[k].tobytes() == two[k].tobytes() == three[k].tobytes()
            assert one[2:] == two[2:] == three[2:]
        moved, now = m.cluster_changes(old, seeds, one[0])
        assert len(moved) >= 1 and np.array_equal(now, one[0][np.isin(old, moved)]) and (now < moved).all()
    m.set_option("scope_strategy", 0)


def test_the_calls_around_an_extend_within_are_unchanged():
    c = oracle_case("words", 5000)
    m, listed = c["m"], c["listed"]
    old, new = listed[listed % 7 != 0], listed[listed % 7 == 0]
    packed, offsets = _pack(c["needles"])
    m.set_option("scope_strategy", 0)
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    find_kernels = m.last_kernels()
    before_within = m.cluster_within(listed, listed % 3, 300)
    within_kernels = m.last_kernels()
    plain_seeds, _, _ = m.cluster(old, 300)
    before_extend = m.cluster_extend(old, plain_seeds, new, 300)
    extend_kernels = m.last_kernels()
    seeds, _, _ = m.cluster_within(old, old % 3, 300)
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        m.cluster_extend_within(old, old % 3, seeds, new, new % 3, 300)
        names = m.last_kernels()
        assert names == SEQUENCE[s], (s, names)
        for other in ("cluster_within_kernel", "cluster_within_sweep_kernel", "cluster_extend_seed_kernel",
                      "cluster_extend_sweep_kernel", "cluster_sweep_kernel", "find_kernel"):
            assert other not in names
    m.set_option("scope_strategy", 0)
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == find_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    after_within = m.cluster_within(listed, listed % 3, 300)
    assert m.last_kernels() == within_kernels
    assert after_within[0].tobytes() == before_within[0].tobytes() and after_within[1:] == before_within[1:]
    after_extend = m.cluster_extend(old, plain_seeds, new, 300)
    assert m.last_kernels() == extend_kernels
    for k in range(2):
        assert after_extend[k].tobytes() == before_extend[k].tobytes()
    assert after_extend[2:] == before_extend[2:]
