"""cluster_cores_within, cluster_core_tree_within and cluster_extend_within on tests/dense_delta_case.py's map: a base
image with tombstones behind its bitmaps and a delta image with dense slices of its own.  Each of the three entries has a
sweep kernel of its own (cluster_cores_within_sweep_kernel and its <unite> ending, cluster_core_tree_within_sweep_kernel
<height> and <tree>, cluster_extend_within_sweep_kernel), a further copy of the floor sweep that ClusterCall::sweep launches
once per image, and a direct kernel; on the delta image the sweeps' lists of 64 dense slices, the ranking of the L
largest, the left-out slices' bitmaps read from the delta's entries, the rank bound against the delta's n_refs and the
positions from win0 run here for the first time, and the base image is swept where its bitmaps still pass tombstoned
ranks.  The keys are dense_truths.key_pairs (two blocks of both images) and dense_delta_case.key_families (a moved row
stays with its base family: blocks with an edge across the images).  Everything is compared exactly with the host's
truths over what is held now by the checkers of tests/test_gpu_cluster_cores_within.py,
tests/test_gpu_cluster_core_tree_within.py and tests/test_gpu_cluster_extend_within.py under "scope_strategy" 0, 1 and
2; three calls under the sweep give identical bytes, last_kernels() names the sweep, and after the log is folded into a
rebuilt base image every answer is the same bytes again.  tests/test_dense_delta_case.py proves the map's conditions on
the host.

Not covered: a delta image of more than one window or with ranks of 32 768 and more (a base of millions of references);
DeviceInfo.n_bitmaps counts the base image's bitmaps only."""
import numpy as np
import pytest

import dense_delta_case as C
import dense_truths as DT
from cluster_core_tree_truth import NO_CORE
from cluster_core_tree_within_truth import blocked_over
from cluster_cores_truth import BORDER, CORE, NONE
from cluster_truth import NO_CLUSTER
from cluster_within_truth import WithinTruth
from test_gpu_cluster_core_tree_within import (DIRECT as TREE_DIRECT, SWEEP as TREE_SWEEP, call as core_tree_within,
                                               check as check_core_tree, passes_for, same_bytes)
from test_gpu_cluster_cores_within import DIRECT as CORES_DIRECT, SWEEP as CORES_SWEEP, check as check_cores, edges_of
from test_gpu_cluster_extend_within import (DIRECT as EXTEND_DIRECT, SWEEP as EXTEND_SWEEP, check as check_extend,
                                            check_contract)

pytestmark = pytest.mark.gpu
LISTS = ["short", "long"]
KEYS = ["pairs", "families"]
FLOORS = range(5)                                              # indices into case.floors: 200, 350, 600, p*, p* + 1
MIN_DEGREES = (0, 2, 3, 5)
STALE_FLOORS = (200, 600)
MERGE = "cluster_tree_merge_kernel"


@pytest.fixture(scope="module")
def case():
    h = C.host()
    stale = {}

    def before(m):
        """On the synced base image, in front of the first mutation: a job's labels of the base families."""
        for p in STALE_FLOORS:
            stale[p] = m.cluster_within(h.base_family, C.key_families(h.base_family), p)[0]

    c = C.gpu_case(before=before)
    c.stale = stale
    c.core_cases = ((200, 2), (350, 3), (600, 2), (c.p_star, 5))   # tests/test_gpu_dense_delta_trees.py's
    w = WithinTruth.__new__(WithinTruth)
    w.__dict__ = dict(h.truth.__dict__, _pairs={})               # (the tokenisation shared, the pairs its own)
    c.within_truth = w
    assert len(c.floors) == len(FLOORS)
    yield c
    c.m.close()


def _images(m):
    """One sweep per image: two before the fold, one after."""
    return 2 if m.device_info()["n_pending"] else 1


def _swept(m, entry, ran, idle, *args):
    """An entry under "scope_strategy" 1: its sweep kernels named, its direct ones not."""
    m.set_option("scope_strategy", 1)
    try:
        out = getattr(m, entry)(*args)
        names = m.last_kernels()
    finally:
        m.set_option("scope_strategy", 0)
    assert all(k in names for k in ran) and not any(k in names for k in idle), names
    return out, names


def _cores(m, listed, blocks, p, min_degree):
    return _swept(m, "cluster_cores_within", CORES_SWEEP, CORES_DIRECT, listed, blocks, p, min_degree)[0]


def _core_tree(m, listed, blocks, p, min_degree):
    out, names = _swept(m, "cluster_core_tree_within", TREE_SWEEP[1:], TREE_DIRECT, listed, blocks, p, min_degree)
    # every launch is named: per image one sweep per height pass and one per round
    assert names.count(TREE_SWEEP[0]) == _images(m) * (passes_for(p) if min_degree else 0), names
    assert names.count(TREE_SWEEP[1]) == _images(m) * names.count(MERGE) >= _images(m), names
    return out


def _extend(m, old, okeys, seeds, new, nkeys, p):
    return _swept(m, "cluster_extend_within", [EXTEND_SWEEP], [EXTEND_DIRECT], old, okeys, seeds, new, nkeys, p)[0]


def test_the_log_is_as_the_host_books_it(case):
    C.assert_log(case.m, case.h)


# ---- cluster_cores_within -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("name", LISTS)
def test_cluster_cores_within_equals_the_truth_at_every_floor_and_min_degree(case, name, keys):
    m, h, listed, truth = case.m, case.h, case.lists[name], case.truth(name)
    blocks = C.keys_of(keys)(listed)
    twin = np.isin(listed, h.twins)
    borders = 0
    for p in case.floors:
        e = edges_of(truth, listed, blocks, p, least=DT.LEAST)
        for min_degree in MIN_DEGREES:
            want = check_cores(m, e, min_degree)
            one = C.thrice(case, f"cores within {name} {keys} {p, min_degree}",
                           lambda p=p, k=min_degree: _cores(m, listed, blocks, p, k))
            labels, degrees, kinds, n_clusters, n_edges, n_core_edges = one
            assert labels.tobytes() == want.labels.tobytes() and degrees.tobytes() == want.degrees.tobytes()
            assert kinds.tobytes() == want.kinds.tobytes(), (p, min_degree)
            assert (n_clusters, n_edges, n_core_edges) == (want.n_clusters, want.n_edges, want.n_core_edges)
            borders += int((kinds == BORDER).sum())
            # a deleted twin, listed, is no node
            assert twin.sum() == len(h.twins) and (labels[twin] == NO_CLUSTER).all() and not degrees[twin].any()
            assert (kinds[twin] == NONE).all()
            if min_degree == 0:                                   # cluster_within's labels and counts, byte for byte
                w_labels, w_clusters, w_edges = m.cluster_within(listed, blocks, p)
                assert labels.tobytes() == w_labels.tobytes() and (n_clusters, n_edges) == (w_clusters, w_edges), p
                assert n_core_edges == n_edges and ((kinds == CORE) | (labels == NO_CLUSTER)).all()
    print(f"{name}, {keys}: {borders} borders over every floor and min_degree")
    assert borders >= 1


@pytest.mark.parametrize("name", LISTS)
def test_cores_within_one_key_is_cluster_cores_byte_for_byte(case, name):
    m, listed = case.m, case.lists[name]
    blocks = np.full(len(listed), 7, dtype=np.uint32)
    for p in case.floors:
        for min_degree in (2, 5):
            same_bytes(_cores(m, listed, blocks, p, min_degree), m.cluster_cores(listed, p, min_degree), (p, min_degree))


# ---- cluster_core_tree_within ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("name", LISTS)
def test_cluster_core_tree_within_equals_the_blocked_truth_at_every_case(case, name, keys):
    m, h, listed, truth = case.m, case.h, case.lists[name], C.blocked_truth(case, name, keys)
    blocks = C.keys_of(keys)(listed)
    across = 0
    for p, min_degree in case.core_cases:
        want, (labels, core, merges) = check_core_tree(m, truth, listed, blocks, p, min_degree, least=DT.LEAST, cuts=1)
        one = C.thrice(case, f"core tree within {name} {keys} {p, min_degree}",
                       lambda p=p, k=min_degree: _core_tree(m, listed, blocks, p, k))
        same_bytes(one, (labels, core, merges, want.n_clusters, want.n_edges, want.n_core_edges), (p, min_degree))
        across += int((C.delta_ends(h, merges) == 1).sum())
        assert (core[np.isin(listed, h.twins)] == NO_CORE).all() and not np.isin(merges[:, :2], h.twins).any()
    print(f"{name}, {keys}: {across} records with an end in each image")
    assert across >= 1 or keys != "families"                      # a moved row's block holds nodes of both images
    # min_degree 0: cluster_tree_within's records and labels byte for byte, no height pass
    for p in (200, case.p_star):
        t_labels, t_merges, t_clusters, t_edges = m.cluster_tree_within(listed, blocks, p)
        labels, core, merges, n_clusters, n_edges, n_core_edges = _core_tree(m, listed, blocks, p, 0)
        assert merges.tobytes() == t_merges.tobytes() and labels.tobytes() == t_labels.tobytes(), p
        assert (n_clusters, n_edges, n_core_edges) == (t_clusters, t_edges, t_edges), p


@pytest.mark.parametrize("name", LISTS)
def test_the_core_tree_within_one_key_is_the_core_tree_byte_for_byte(case, name):
    m, listed = case.m, case.lists[name]
    blocks = np.full(len(listed), 7, dtype=np.uint32)
    for p, min_degree in case.core_cases:
        same_bytes(_core_tree(m, listed, blocks, p, min_degree), m.cluster_core_tree(listed, p, min_degree), (p, min_degree))


# ---- cluster_extend_within ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", FLOORS)
@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("name", LISTS)
def test_extend_within_with_the_base_old_and_the_pending_new_and_the_other_way_round(case, name, keys, k):
    m, h, truth, p = case.m, case.h, case.truth(name), case.floors[k]
    key = C.keys_of(keys)
    in_base, in_delta = C.by_image(h, case.lists[name])            # (the deleted, listed among the base's, are no nodes)
    for old, new, what in ((in_base, in_delta, "pending new"), (in_delta, in_base, "base new")):
        want, seeds, got = check_contract(m, truth, old, key(old), new, key(new), p, least=DT.LEAST)
        one = C.thrice(case, f"extend within {name} {keys} {what} {p}",
                       lambda old=old, new=new, seeds=seeds: _extend(m, old, key(old), seeds, new, key(new), p))
        DT._same_bytes(one, got)
        assert want.old_new_edges >= 1 and want.new_new_edges >= 1, (p, what)


@pytest.mark.parametrize("name", LISTS)
def test_extend_within_one_key_is_cluster_extend_byte_for_byte(case, name):
    m, h = case.m, case.h
    in_base, in_delta = C.by_image(h, case.lists[name])
    for p in case.floors:
        for old, new in ((in_base, in_delta), (in_delta, in_base)):
            seeds = m.cluster(old, p)[0]
            one = _extend(m, old, np.full(len(old), 7, dtype=np.uint32), seeds, new, np.full(len(new), 7, dtype=np.uint32), p)
            DT._same_bytes(one, m.cluster_extend(old, seeds, new, p))


@pytest.mark.parametrize("p", STALE_FLOORS)
def test_seeds_from_before_the_mutations_with_the_groups_that_lost_a_member_clustered_again(case, p):
    """A job's labels of the base families, made before the first mutation (the `before` hook), serve an extend by the
    delta families after it.  The documented recipe: a group that lost a member -- its twin to a tombstone behind a
    bitmap, or its moved row -- is clustered again first, over its remaining members; the deleted twins stay in the old
    list and get NO_CLUSTER."""
    m, h = case.m, case.h
    stays = ~np.isin(h.base_family, h.moved)
    old, new = h.base_family[stays], h.delta_family
    okeys, nkeys = C.key_families(old), C.key_families(new)
    seeds = case.stale[p][stays].copy()
    assert (case.stale[p] != NO_CLUSTER).all()                    # (then, every one of them was held)
    gone = np.isin(old, h.twins)
    lost = np.unique(np.concatenate([seeds[gone], case.stale[p][~stays]]))
    twin_groups = {int(seeds[old == x][0]) for x in h.twin_heads}
    assert twin_groups <= set(lost.tolist()) and len(twin_groups) == len(h.twins)
    for label in lost.tolist():
        at = (seeds == label) & ~gone
        again = m.cluster_within(old[at], okeys[at], p)[0]
        assert again.tobytes() == case.within_truth.cluster_within(old[at], okeys[at], p, DT.LEAST)[0].tobytes()
        seeds[at] = again
    want = check_extend(m, case.truth("the families"), old, okeys, seeds, new, nkeys, p, least=DT.LEAST)
    one = C.thrice(case, f"extend within, stale seeds {p}", lambda: _extend(m, old, okeys, seeds, new, nkeys, p))
    assert one[0].tobytes() == want.labels_old.tobytes() and one[1].tobytes() == want.labels_new.tobytes()
    assert (one[0][gone] == NO_CLUSTER).all() and (one[0][~gone] != NO_CLUSTER).all() and want.n_seeds >= len(old) // 2
    assert want.new_new_edges >= 1


# ---- the exact bar, in the delta ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [500, 501])
def test_the_copies_whose_matches_are_exactly_the_bar_under_one_key_and_the_glued_string_under_its_own(case, p):
    m, h, g = case.m, case.h, case.h.handmade
    listed, truth = case.lists["handmade"], case.truth("handmade")
    copies = len(g.held_copies)
    among = copies * (copies - 1) // 2
    one_key = np.zeros(len(listed), dtype=np.uint32)
    own = (listed == g.glued).astype(np.uint32)                   # under a key of its own the glued string joins nothing
    glued = np.array([g.glued], dtype=np.uint32)
    gone = listed == h.copy_deleted
    for blocks, edges in ((one_key, among + (copies if p == 500 else 0)), (own, among)):
        key_of = dict(zip(listed.tolist(), blocks.tolist()))
        e = edges_of(truth, listed, blocks, p)
        for min_degree in (0, copies, copies + 1):
            want = check_cores(m, e, min_degree)
            assert want.n_edges == edges and want.labels[gone] == NO_CLUSTER, (p, min_degree)
            # a copy has 68 edges at 1000 and, at floor 500 under one key, the glued string's; the glued string 69 or none
            is_core = min_degree <= copies - 1 + (edges > among)
            assert (want.kind_of[int(g.held_copies[0])] == CORE) == is_core, (p, min_degree)
            assert want.degree_of[g.glued] == edges - among, (p, min_degree)
        b_truth = blocked_over(truth, listed, blocks)
        for min_degree in (copies, copies + 1):
            want, (labels, core, merges) = check_core_tree(m, b_truth, listed, blocks, p, min_degree, cuts=1)
            assert want.n_edges == edges and core[gone] == NO_CORE, (p, min_degree)
        for old, new in ((g.held_copies, glued), (glued, g.held_copies)):
            okeys, nkeys = (np.array([key_of[int(r)] for r in x], dtype=np.uint32) for x in (old, new))
            want, _, _ = check_contract(m, truth, old, okeys, new, nkeys, p)
            assert want.old_new_edges == edges - among, (p, len(old))


# ---- fold invariance (the last test: it changes the map) -----------------------------------------------------------------

def test_after_the_fold_one_image_answers_every_call_with_the_same_bytes(case):
    C.fold_and_compare(case, at_least=138)
