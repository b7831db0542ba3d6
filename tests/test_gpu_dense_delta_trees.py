"""cluster_tree, cluster_core_tree, cluster_tree_within under the sweep and cluster_tree_extend on
tests/dense_delta_case.py's map: a base image with tombstones behind its bitmaps and a delta image with dense slices of
its own.  cluster_tree_sweep_kernel, the two endings of the core sweep (cluster_core_height_sweep_kernel,
cluster_core_tree_sweep_kernel), cluster_tree_within_sweep_kernel and cluster_tree_extend_sweep_kernel are further copies
of the floor sweep, launched once per image and round by ClusterCall::sweep; on the delta image their lists of 64 dense
slices, their left-out slices' bitmaps and their positions from win0 run here for the first time, and a needle of the
delta image finds its base neighbours through the base's bitmaps, where a deleted twin and a moved row's old rank pass
the bar and are no nodes.  Their endings write the height floor(1000 m / (T + R - m)) into the records: an m that is off
by one moves a record where the components stay the same.  Everything is compared exactly with the host's truths over
what is held now by the checkers of tests/test_gpu_cluster_tree.py, tests/test_gpu_cluster_core_tree.py,
tests/test_gpu_cluster_tree_within.py and tests/test_gpu_cluster_tree_extend.py; three calls give identical bytes,
last_kernels() names the sweep, and after the log is folded into a rebuilt base image every answer is the same bytes
again.  tests/test_dense_delta_case.py proves the map's conditions on the host.

Not covered: a delta image of more than one window or with ranks of 32 768 and more (a base of millions of references);
DeviceInfo.n_bitmaps counts the base image's bitmaps only."""
import numpy as np
import pytest

import dense_delta_case as C
import dense_tree_case as DTC
import dense_truths as DT
from cluster_core_tree_truth import NO_CORE
from cluster_truth import NO_CLUSTER
from test_gpu_cluster_core_tree import check_core_tree
from test_gpu_cluster_tree import check_tree
from test_gpu_cluster_tree_extend import check_contract
from test_gpu_cluster_tree_within import DIRECT, SWEEP, check_tree as check_within

pytestmark = pytest.mark.gpu
CUTS = 1
KEYS = {"pairs": DT.key_pairs, "families": C.key_families}
LISTS = ["short", "long"]
TREE, MERGE = "cluster_tree_sweep_kernel", "cluster_tree_merge_kernel"


@pytest.fixture(scope="module")
def case():
    c = C.gpu_case()
    c._blocked = {}

    def blocked(name, keys):
        if (name, keys) not in c._blocked:
            c.truth(name).pairs(c.lists[name], DT.LEAST)            # (the list's pairs once: the blocked truths filter them)
            c._blocked[name, keys] = DTC.blocked_on(c.truth(name), c.lists[name], KEYS[keys](c.lists[name]))
        return c._blocked[name, keys]

    c.blocked = blocked
    c.core_cases = ((200, 2), (350, 3), (600, 2), (c.p_star, 5))
    yield c
    c.m.close()


def _per_image(m, sweep):
    """One sweep per image and round: twice the merges."""
    names = m.last_kernels()
    assert names.count(sweep) == 2 * names.count(MERGE) >= 4, (sweep, names)


def test_the_log_is_as_the_host_books_it(case):
    C.assert_log(case.m, case.h)


@pytest.mark.parametrize("name", LISTS)
def test_cluster_tree_equals_kruskal_and_the_cluster_call_at_every_floor(case, name):
    m, h, truth, listed = case.m, case.h, case.truth(name), case.lists[name]
    pending = set(h.pending)
    for p in case.floors:
        labels, merges = check_tree(m, truth, listed, p, least=DT.LEAST, cuts=CUTS)
        one = C.thrice(case, f"tree {name} {p}", lambda p=p: m.cluster_tree(listed, p))
        _per_image(m, TREE)
        assert one[0].tobytes() == labels.tobytes() and one[1].tobytes() == merges.tobytes()
        ends = [(a in pending) + (b in pending) for a, b, _ in merges.tolist()]
        print(f"{name}, floor {p}: {len(merges)} records, {ends.count(2)} within the delta, {ends.count(1)} base-delta")
        assert ends.count(2) >= 40 and ends.count(1) >= len(h.moved) and ends.count(0) >= 40, p
        at = dict(zip(listed.tolist(), labels.tolist()))
        assert all(at[r] == NO_CLUSTER for r in h.twins) and not np.isin(merges[:, :2], h.twins).any()


@pytest.mark.parametrize("name", LISTS)
def test_the_delta_pairs_record_disappears_from_p_star_to_p_star_plus_1_without_its_family(case, name):
    m, h, listed = case.m, case.h, case.lists[name]
    low, high = case.pair
    alone = np.concatenate([listed[~np.isin(listed, h.delta_family)], np.array([low, high], dtype=np.uint32)])
    truth = case.truth(name + ", the pair alone")
    rows = {}
    for p in (case.p_star, case.p_star + 1):
        labels, merges = check_tree(m, truth, alone, p, least=DT.LEAST, cuts=1)
        assert (labels[-2] == labels[-1]) == (p == case.p_star), p
        rows[p] = set(map(tuple, merges.tolist()))
    assert (min(low, high), max(low, high), case.p_star) in rows[case.p_star]
    assert rows[case.p_star + 1] == {r for r in rows[case.p_star] if r[2] > case.p_star}


@pytest.mark.parametrize("name", LISTS)
def test_cluster_core_tree_equals_the_truth_at_every_case(case, name):
    m, truth, listed = case.m, case.truth(name), case.lists[name]
    for p, k in case.core_cases:
        labels, core, merges = check_core_tree(m, truth, listed, p, k, least=DT.LEAST, cuts=CUTS)
        one = C.thrice(case, f"core tree {name} {p, k}", lambda p=p, k=k: m.cluster_core_tree(listed, p, k))
        names = m.last_kernels()
        assert names.count("cluster_core_tree_sweep_kernel") >= 2 and names.count("cluster_core_height_sweep_kernel") >= 2
        assert TREE not in names, names
        assert one[1].tobytes() == core.tobytes() and one[2].tobytes() == merges.tobytes()
        delta = np.isin(listed, case.h.delta_family)
        assert ((core[delta] != NO_CORE).any() or k >= 5) and len(merges) >= 3, (p, k)
    # min_degree 0: the cluster tree's records byte for byte, no height sweep
    for p in (200, case.p_star):
        t_labels, t_merges, t_clusters, t_edges = m.cluster_tree(listed, p)
        labels, core, merges, n_clusters, n_edges, n_core_edges = m.cluster_core_tree(listed, p, 0)
        assert "cluster_core_height_sweep_kernel" not in m.last_kernels()
        assert merges.tobytes() == t_merges.tobytes() and labels.tobytes() == t_labels.tobytes(), p
        assert (n_clusters, n_edges, n_core_edges) == (t_clusters, t_edges, t_edges), p


# ---- cluster_tree_within under the sweep ------------------------------------------------------------------------------------

def _within(m, listed, blocks, p):
    m.set_option("scope_strategy", 1)
    try:
        out = m.cluster_tree_within(listed, blocks, p)
        names = m.last_kernels()
    finally:
        m.set_option("scope_strategy", 0)
    images = 2 if m.device_info()["n_pending"] else 1             # (one sweep per image and round; after the fold one image)
    assert names.count(SWEEP) == images * names.count(MERGE) >= 2 * images, names
    assert DIRECT not in names and TREE not in names, names
    return out


@pytest.mark.parametrize("keys", ["pairs", "families"])
@pytest.mark.parametrize("name", LISTS)
def test_cluster_tree_within_under_the_sweep_equals_the_blocked_truth(case, name, keys):
    m, h, listed, truth = case.m, case.h, case.lists[name], case.blocked(name, keys)
    blocks = KEYS[keys](listed)
    key_of = dict(zip(listed.tolist(), blocks.tolist()))
    pending = set(h.pending)
    for p in case.floors:
        labels, merges = check_within(m, truth, listed, blocks, p, least=DT.LEAST, cuts=CUTS, strategies=(1,))
        one = C.thrice(case, f"tree within {name} {keys} {p}", lambda p=p: _within(m, listed, blocks, p))
        assert one[0].tobytes() == labels.tobytes() and one[1].tobytes() == merges.tobytes()
        # a record of a block that holds nodes of both images, one end in each
        across = [r for r in merges.tolist() if (r[0] in pending) != (r[1] in pending)]
        assert len(across) >= (len(h.moved) if keys == "families" else 1), p
        assert all(key_of[a] == key_of[b] for a, b, _ in across)


@pytest.mark.parametrize("name", LISTS)
def test_all_keys_equal_is_the_cluster_tree_byte_for_byte(case, name):
    m, listed = case.m, case.lists[name]
    blocks = np.full(len(listed), 7, dtype=np.uint32)
    for p in case.floors:
        DT._same_bytes(_within(m, listed, blocks, p), m.cluster_tree(listed, p))


# ---- cluster_tree_extend: the tree after a batch of fresh puts, and the other way round ----------------------------------

@pytest.mark.parametrize("name", LISTS)
def test_cluster_tree_extend_with_the_base_old_and_the_pending_new_and_the_other_way_round(case, name):
    m, h, listed = case.m, case.h, case.lists[name]
    pending = np.isin(listed, np.array(sorted(h.pending), dtype=np.uint32))
    in_base, in_delta = listed[~pending], listed[pending]          # (the deleted, listed among the base's, are no nodes)
    truth = case.truth(name)
    for p in case.floors:
        for old, new, what in ((in_base, in_delta, "pending new"), (in_delta, in_base, "base new")):
            want, held, got = check_contract(m, truth, old, new, p, least=DT.LEAST)
            C.thrice(case, f"tree extend {name} {what} {p}",
                     lambda old=old, held=held, new=new, p=p: m.cluster_tree_extend(old, held, new, p))
            _per_image(m, "cluster_tree_extend_sweep_kernel")
            assert want.old_new_edges >= 1 and want.new_new_edges >= 1, (p, what)
    # records made at 200 serve a call at 600
    check_contract(m, truth, in_base, in_delta, 600, f_old=200, least=DT.LEAST)


# ---- the exact bar, in the delta ------------------------------------------------------------------------------------------

def test_the_glued_strings_record_at_500_is_there_at_floor_500_and_not_at_501(case):
    m, h, g = case.m, case.h, case.h.handmade
    listed, truth = case.lists["handmade"], case.truth("handmade")
    copies = len(g.held_copies)
    first = int(g.held_copies[0])
    among = [[first, int(r), 1000] for r in g.held_copies[1:]]
    want = {500: among + [[g.glued, first, 500]], 501: among}
    one_key = np.zeros(len(listed), dtype=np.uint32)
    for p in (500, 501):
        labels, merges = check_tree(m, truth, listed, p)
        assert merges.tolist() == want[p] and len(merges) == copies - (p == 501), p
        assert labels[listed == h.copy_deleted] == NO_CLUSTER
        labels, core, merges = check_core_tree(m, truth, listed, p, copies)
        of = dict(zip(listed.tolist(), core.tolist()))
        # a copy's edges: 68 at 1000 and, at floor 500, one at 500; the glued string's: 69 at 500, none at 501
        assert of[g.glued] == (500 if p == 500 else NO_CORE) and of[first] == (500 if p == 500 else NO_CORE), p
        assert _within(m, listed, one_key, p)[1].tolist() == want[p], p
        own = (listed == g.glued).astype(np.uint32)               # under a key of its own the glued string joins nothing
        assert _within(m, listed, own, p)[1].tolist() == among, p
        check_contract(m, truth, g.held_copies, np.array([g.glued], dtype=np.uint32), p)


# ---- fold invariance (the last test: it changes the map) -----------------------------------------------------------------

def test_after_the_fold_one_image_answers_every_call_with_the_same_bytes(case):
    C.fold_and_compare(case, at_least=50)
