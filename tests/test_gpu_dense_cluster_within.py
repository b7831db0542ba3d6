"""cluster_within on tests/dense_case.py's map: cluster_within_sweep_kernel is one more copy of the floor sweep (the
list of at most 64 dense slices, the L = min(t - 1, nd) largest left out and asked about in their bitmaps, 16-bit
counters over two half windows for a needle of more than 255 trigrams, a needle's windows shared among workgroups) with
its needles taken from a list and the block key tested behind the bitmap probes; cluster_within_kernel, the direct
kernel, empties its byte counters every 255 codes.  The other haystacks of tests/test_gpu_cluster_within.py leave no
slice out and hold six wide nodes; here every family head has more than 64 dense slices in window 0, sixteen needles of
T = 122 .. 955 share a tile with members of R up to 955 in front of them, and the keys decide edges that both bitmap
probes and the floor let pass.  Labels, n_clusters and n_edges equal cluster_within_truth.WithinTruth exactly under
"scope_strategy" 1 (the sweep) and 2 (direct), three calls give identical bytes, and last_kernels() names the kernel
that was meant to run and not the other.  tests/test_dense_scoped_case.py proves the inputs' conditions on the host."""
import copy

import numpy as np
import pytest

import dense_case as D
import dense_truths as DT
from blurrily_amd import RawMap
from blurrily_amd.map import _pack
from cluster_within_truth import WithinTruth
from dense_truths import _same_bytes

pytestmark = pytest.mark.gpu
SWEEP, DIRECT = "cluster_within_sweep_kernel", "cluster_within_kernel"
KERNELS = {1: (SWEEP, DIRECT), 2: (DIRECT, SWEEP), 0: (DIRECT, SWEEP)}   # strategy: (runs, does not); auto: every block is small
KEYS = {"pairs": DT.key_pairs, "families": DT.key_families, "parity": DT.key_parity}


def within(m, listed, blocks, p, strategy):
    """Three calls under `strategy`, byte for byte equal, the intended kernel named and the other not: the first."""
    m.set_option("scope_strategy", strategy)
    try:
        one, two, three = (m.cluster_within(listed, blocks, p) for _ in range(3))
        names = m.last_kernels()
    finally:
        m.set_option("scope_strategy", 0)
    ran, idle = KERNELS[strategy]
    assert ran in names and idle not in names and "cluster_sweep_kernel" not in names, (strategy, names)
    _same_bytes(one, two)
    _same_bytes(one, three)
    return one


def equal(got, want, what):
    labels, n_clusters, n_edges = got
    w_labels, w_clusters, w_edges = want[:3]
    print(f"{what}: clusters {n_clusters} (truth {w_clusters}), edges {n_edges} (truth {w_edges})")
    assert n_edges == w_edges and n_clusters == w_clusters, what
    assert labels.dtype == np.uint32 and np.array_equal(labels, w_labels), what


@pytest.fixture(scope="module")
def case():
    import torch
    m, h = D.build()
    c = DT.inputs(h)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # windows_per_workgroup: per = max(1, n_windows * nodes / (8 CUs)), at most n_windows
    assert 2 * len(c.lists["short"]) < 8 * cus, (len(c.lists["short"]), cus)     # per == 1: two workgroups a needle
    assert len(c.lists["long"]) >= 8 * cus, (len(c.lists["long"]), cus)          # per == 2: one
    base = WithinTruth(h.held)
    c.m, c.h, c._truth = m, h, {}

    def truth(name):
        """A WithinTruth per list (a Truth keeps one list's pairs), the tokenisation shared."""
        if name not in c._truth:
            c._truth[name] = copy.copy(base)
            c._truth[name]._pairs = {}
        return c._truth[name]

    c.truth = truth
    yield c
    m.close()


@pytest.mark.parametrize("keys", ["pairs", "families"])
@pytest.mark.parametrize("name", ["short", "long"])
def test_labels_components_and_edges_equal_the_truth_under_the_sweep_and_direct(case, name, keys):
    m, listed = case.m, case.lists[name]
    blocks = KEYS[keys](listed)
    edges = []
    for p in case.floors:
        want = case.truth(name).cluster_within(listed, blocks, p, DT.LEAST)
        swept = within(m, listed, blocks, p, 1)
        equal(swept, want, f"{name}, {keys}, floor {p}, the sweep")
        direct = within(m, listed, blocks, p, 2)
        equal(direct, want, f"{name}, {keys}, floor {p}, direct")
        _same_bytes(within(m, listed, blocks, p, 0), direct)          # auto: the bytes of 2
        edges.append(want[2])
    assert edges[0] > edges[-1] > 0


@pytest.mark.parametrize("strategy", [1, 2])
@pytest.mark.parametrize("name", ["short", "long"])
def test_the_pair_is_one_label_up_to_p_star_under_a_shared_key_and_two_under_different_keys(case, name, strategy):
    """Both members lie in the upper half of window 0 and are wide: under the sweep only the half == 1 pass of the member
    at the higher position can find the edge.  Listed without the rest of their family (which joins them at every floor
    used, through the head), the two are one label up to p* and two at p* + 1; in the whole list the edge count falls by
    exactly this edge.  Under ref % 2 both bitmap probes and the floor pass, and only the key test says no."""
    m, listed = case.m, case.lists[name]
    low, high = case.pair
    alone = np.concatenate([listed[:-len(case.family)], np.array([low, high], dtype=np.uint32)])
    at = {int(r): i for i, r in enumerate(listed.tolist())}
    n_edges = {}
    for p in case.floors:
        want = case.truth(name + ", the pair alone").cluster_within(alone, DT.key_pairs(alone), p, DT.LEAST)
        got = within(m, alone, DT.key_pairs(alone), p, strategy)
        equal(got, want, f"{name}, the pair alone, floor {p}, strategy {strategy}")
        assert (got[0][-2] == got[0][-1]) == (p <= case.p_star), p
        n_edges[p] = within(m, listed, DT.key_pairs(listed), p, strategy)[2]
        want = case.truth(name).cluster_within(listed, DT.key_parity(listed), p, DT.LEAST)
        got = within(m, listed, DT.key_parity(listed), p, strategy)
        equal(got, want, f"{name}, ref % 2, floor {p}, strategy {strategy}")
        assert got[0][at[low]] != got[0][at[high]], p
    assert n_edges[case.p_star] == n_edges[case.p_star + 1] + 1


def test_a_within_block_edge_from_window_1_into_window_0_is_found_by_the_workgroup_of_window_0(case):
    m, h, listed = case.m, case.h, case.lists["short"]
    blocks = DT.key_pairs(listed)
    family = set(case.family.tolist())
    at = {int(r): i for i, r in enumerate(listed.tolist())}
    for p in (350, case.p_star):
        across = [e for e in DT.within_edges(case.truth("short"), listed, blocks, p)
                  if e[0] in family and {h.loc[e[0]][0], h.loc[e[1]][0]} == {0, 1}]
        assert across
        labels, _, _ = within(m, listed, blocks, p, 1)
        for a, b in across:
            assert labels[at[a]] == labels[at[b]], (p, a, b)


@pytest.mark.parametrize("strategy", [1, 2])
def test_the_list_reversed_and_the_families_listed_twice_give_the_same_label_per_reference(case, strategy):
    m, listed = case.m, case.lists["short"]
    for p in (200, 350, case.p_star + 1):
        want = case.truth("short").cluster_within(listed, DT.key_pairs(listed), p, DT.LEAST)
        base = within(m, listed, DT.key_pairs(listed), p, strategy)
        equal(base, want, f"floor {p}")
        label_of = dict(zip(listed.tolist(), base[0].tolist()))
        for other in (listed[::-1].copy(), np.concatenate([case.family, listed]), np.concatenate([listed[::-1], case.family])):
            labels, n_clusters, n_edges = within(m, other, DT.key_pairs(other), p, strategy)
            assert (n_clusters, n_edges) == base[1:], p
            assert labels.tolist() == [label_of[r] for r in other.tolist()], p


@pytest.mark.parametrize("name", ["short", "long"])
def test_all_keys_equal_is_the_plain_cluster_call_byte_for_byte(case, name):
    m, listed = case.m, case.lists[name]
    blocks = np.full(len(listed), 7, dtype=np.uint32)
    for p in case.floors:
        want = m.cluster(listed, p)                                # (proven on this map by tests/test_gpu_dense_floor_sweeps.py)
        assert "cluster_sweep_kernel" in m.last_kernels()
        for strategy in (1, 2):
            _same_bytes(within(m, listed, blocks, p, strategy), want)


def test_matches_exactly_the_bar_and_all_in_the_densest_slices_within_a_block_and_across_two():
    """The hand-made case: L = t - 1 and not one more, now with the key test behind the probes.  All under one key: the
    glued string has its 70 edges at floor 500 and none at 501; under a key of its own it has none at either floor and is
    one more cluster."""
    c = DT.handmade()
    pairs = 70 * 69 // 2
    truth = WithinTruth(c.held)
    strings = [c.held[int(r)] for r in c.refs]
    m = RawMap()
    m.set_option("dense_min", D.DENSE_MIN)
    m.put_many_packed(*_pack(strings), c.refs, c.weights)
    try:
        m.sync_device()
        assert m.device_info()["n_bitmaps"] == 6
        one_key = np.zeros(len(c.refs), dtype=np.uint32)
        own_key = (c.refs == 1).astype(np.uint32)
        for strategy in (1, 2):
            for p, blocks, edges, clusters in ((500, one_key, pairs + 70, 3), (501, one_key, pairs, 4),
                                               (500, own_key, pairs, 4), (501, own_key, pairs, 4)):
                want = truth.cluster_within(c.refs, blocks, p)
                assert (want[1], want[2]) == (clusters, edges)
                equal(within(m, c.refs, blocks, p, strategy), want, f"hand-made, floor {p}, strategy {strategy}")
    finally:
        m.close()


def test_the_default_dense_min_with_families_in_the_upper_half_and_across_it():
    m, h = D.build_default()
    try:
        family = np.array([r for head in h.heads for r in h.family(head)], dtype=np.uint32)
        listed = np.unique(np.concatenate([h.refs[::5], family]))
        blocks = DT.key_pairs(listed)
        truth = WithinTruth(h.held)
        floors = (350, 600)
        for p in floors:
            # every dense slice of a family's is left out: 1 <= nd <= t - 1
            assert all(1 <= h.dense_padded(x, 0) <= min(DT.floor_bar(h.T(x), p) - 1, D.MAX_DENSE) for x in h.heads)
            want = truth.cluster_within(listed, blocks, p, floors[0])
            plain = truth.cluster(listed, p, floors[0])
            assert 0 < want[2] < plain[2]
            for strategy in (1, 2):
                equal(within(m, listed, blocks, p, strategy), want, f"defaults, floor {p}, strategy {strategy}")
            # a family's members under one key stay joined in the upper half and across the halves
            for head in h.heads:
                for k in (0, 1):
                    members = [r for r in h.family(head) if (r // 2) % 2 == k]
                    assert len(members) >= 2 and len({want[3][r] for r in members}) == 1, (p, head, k)
    finally:
        m.close()
