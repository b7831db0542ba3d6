"""cluster, cluster_levels, cluster_centres, cluster_cores, cluster_within under the sweep and cluster_extend on
tests/dense_delta_case.py's map: a base image with tombstones behind its bitmaps and a delta image with dense slices of
its own.  ClusterCall::sweep launches each of these sweeps once per image, the delta's with win0 = the base's windows and
the delta's own slice table, entries, rank tables and n_refs.  On the other maps of the suite the delta image has no
bitmap, so the lines of each copy of the sweep that are live only with dense slices -- the fill of the list of 64, the
ranking, the left-out slices' bitmaps read from the image's entries, the rank bound against n_refs, the position from
win0 -- have never run on a second image; here every delta head has more than 64 dense slices in the delta's window, under
both counter widths.  A needle of the delta image also sweeps the base image (an edge is its higher end's to find, and the
delta lies behind the base), so every base-delta edge is found through the base's bitmaps, where a deleted twin and a
moved row's old rank pass the bar and are no nodes.  Every answer is compared exactly with the host's truths over what is
held now, three calls give identical bytes, last_kernels() names the sweep, and after the log is folded into a rebuilt
base image every answer is the same bytes again.  tests/test_dense_delta_case.py proves the map's conditions on the host.

Not covered: a delta image of more than one window or with ranks of 32 768 and more (a base of millions of references);
DeviceInfo.n_bitmaps counts the base image's bitmaps only."""
import numpy as np
import pytest

import dense_delta_case as C
import dense_truths as DT
from cluster_centres_truth import CentresTruth
from cluster_cores_truth import BORDER, CORE, CoresEdges
from cluster_truth import NO_CLUSTER
from cluster_within_truth import WithinTruth
from test_gpu_cluster_extend import check_contract

pytestmark = pytest.mark.gpu
MIN_DEGREES = (0, 2, 3, 5)
W_SWEEP, W_DIRECT = "cluster_within_sweep_kernel", "cluster_within_kernel"
KEYS = {"pairs": DT.key_pairs, "families": C.key_families}
LISTS = ["short", "long"]


@pytest.fixture(scope="module")
def case():
    c = C.gpu_case()
    h = c.h
    c._truths, c._within = {}, {}

    def truths(name):
        """{floor: (Truth.cluster's answer, CentresTruth, CoresEdges)} of a list."""
        if name not in c._truths:
            listed, truth = c.lists[name], c.truth(name)
            c._truths[name] = {p: (truth.cluster(listed, p, DT.LEAST), CentresTruth(truth, listed, p, DT.LEAST),
                                   CoresEdges(truth, listed, p, DT.LEAST)) for p in c.floors}
        return c._truths[name]

    def within_truth(name):
        if name not in c._within:
            w = WithinTruth.__new__(WithinTruth)
            w.__dict__ = dict(c.truth(name).__dict__)                # (the tokenisation shared, the list's pairs its own)
            w._pairs = {}
            c._within[name] = w
        return c._within[name]

    c.truths, c.within_truth = truths, within_truth
    # a listed reference that is not held -- a deleted twin, a deleted word, the deleted copy -- is no node
    for name in LISTS:
        listed = set(c.lists[name].tolist())
        assert set(h.twins) <= listed and listed & set(h.words_deleted.tolist()) and set(h.moved) <= listed
    yield c
    c.m.close()


def _named(m, kernel):
    """(last_kernels() keeps distinct names: one entry for the sweeps of both images)"""
    assert kernel in m.last_kernels(), (kernel, m.last_kernels())


def test_the_log_is_as_the_host_books_it(case):
    C.assert_log(case.m, case.h)


@pytest.mark.parametrize("name", LISTS)
def test_cluster_equals_the_truth_at_every_floor(case, name):
    m, h, listed = case.m, case.h, case.lists[name]
    for p in case.floors:
        (w_labels, w_clusters, w_edges, of_ref), _, _ = case.truths(name)[p]
        labels, n_clusters, n_edges = C.thrice(case, f"cluster {name} {p}", lambda p=p: m.cluster(listed, p))
        _named(m, "cluster_sweep_kernel")
        print(f"{name}, floor {p}: clusters {n_clusters} (truth {w_clusters}), edges {n_edges} (truth {w_edges})")
        assert n_edges == w_edges and n_clusters == w_clusters, p
        assert labels.dtype == np.uint32 and np.array_equal(labels, w_labels), p
        at = dict(zip(listed.tolist(), labels.tolist()))
        assert all(at[r] == NO_CLUSTER for r in h.twins) and at[int(h.words_deleted[0])] == NO_CLUSTER
        # a moved row is a node of the delta image in its base family's cluster
        assert all(at[r] == at[x] != NO_CLUSTER for r, x in zip(h.moved, h.moved_heads)), p
    assert case.truths(name)[200][0][2] > case.truths(name)[600][0][2] > 0


@pytest.mark.parametrize("name", LISTS)
def test_the_delta_pair_is_an_edge_up_to_p_star_and_none_one_permille_above(case, name):
    """Both wide, both in the delta image: listed without the rest of their family, the edge is found by the member at the
    higher delta position, in the delta's own sweep, or not at all."""
    m, h, listed = case.m, case.h, case.lists[name]
    low, high = case.pair
    alone = np.concatenate([listed[~np.isin(listed, h.delta_family)], np.array([low, high], dtype=np.uint32)])
    truth = case.truth(name + ", the pair alone")
    for p in (case.p_star, case.p_star + 1):
        w_labels, w_clusters, w_edges, _ = truth.cluster(alone, p, DT.LEAST)
        labels, n_clusters, n_edges = m.cluster(alone, p)
        assert (n_clusters, n_edges) == (w_clusters, w_edges) and np.array_equal(labels, w_labels), p
        assert (labels[-2] == labels[-1]) == (p == case.p_star), p


@pytest.mark.parametrize("name", LISTS)
def test_cluster_levels_equals_the_truth_and_the_single_floor_calls(case, name):
    m, listed, floors = case.m, case.lists[name], case.floors
    labels, n_clusters, n_edges = C.thrice(case, f"levels {name}", lambda: m.cluster_levels(listed, floors))
    _named(m, "cluster_levels_sweep_kernel")
    assert labels.dtype == np.uint32 and labels.shape == (len(floors), len(listed))
    for k, p in enumerate(floors):
        (w_labels, w_clusters, w_edges, _), _, _ = case.truths(name)[p]
        assert n_edges[k] == w_edges and n_clusters[k] == w_clusters, p
        assert np.array_equal(labels[k], w_labels), p


@pytest.mark.parametrize("name", LISTS)
def test_cluster_centres_equals_the_truth_at_every_floor(case, name):
    m, listed = case.m, case.lists[name]
    for p in case.floors:
        want = case.truths(name)[p][1]
        one = C.thrice(case, f"centres {name} {p}", lambda p=p: m.cluster_centres(listed, p, attached=True))
        assert {"cluster_centres_sweep_kernel", "cluster_centres_sweep_kernel<mark>"} <= set(m.last_kernels())
        labels, degrees, centres, attached, n_clusters, n_edges = one
        print(f"{name}, floor {p}: clusters {n_clusters} (truth {want.n_clusters}), edges {n_edges} (truth "
              f"{want.n_edges}), unattached {int((attached == 0).sum())} (truth {int((want.attached == 0).sum())})")
        assert n_edges == want.n_edges and n_clusters == want.n_clusters, p
        assert labels.dtype == np.uint32 and np.array_equal(labels, want.labels), p
        assert degrees.dtype == np.uint32 and np.array_equal(degrees, want.degrees), p
        assert centres.dtype == np.uint32 and np.array_equal(centres, want.centres), p
        assert attached.dtype == np.uint8 and np.array_equal(attached, want.attached), p
        assert int(degrees.sum(dtype=np.uint64)) == 2 * n_edges, p   # (no reference is listed twice)


@pytest.mark.parametrize("name", LISTS)
def test_cluster_cores_equals_the_truth_at_every_floor_and_min_degree(case, name):
    m, listed = case.m, case.lists[name]
    borders = 0
    for p in case.floors:
        e = case.truths(name)[p][2]
        for min_degree in MIN_DEGREES:
            want = e.cores(min_degree)
            one = C.thrice(case, f"cores {name} {p, min_degree}",
                           lambda p=p, k=min_degree: m.cluster_cores(listed, p, k))
            assert {"cluster_cores_sweep_kernel", "cluster_cores_sweep_kernel<unite>"} <= set(m.last_kernels())
            _named(m, "cluster_cores_sweep_kernel")
            labels, degrees, kinds, n_clusters, n_edges, n_core_edges = one
            print(f"{name}, floor {p}, min_degree {min_degree}: clusters {n_clusters} (truth {want.n_clusters}), edges "
                  f"{n_edges} (truth {want.n_edges}), core edges {n_core_edges} (truth {want.n_core_edges}), borders "
                  f"{int((kinds == BORDER).sum())} (truth {want.n_borders})")
            assert n_edges == want.n_edges and n_core_edges == want.n_core_edges, (p, min_degree)
            assert n_clusters == want.n_clusters, (p, min_degree)
            assert degrees.dtype == np.uint32 and np.array_equal(degrees, want.degrees), (p, min_degree)
            assert kinds.dtype == np.uint8 and np.array_equal(kinds, want.kinds), (p, min_degree)
            assert labels.dtype == np.uint32 and np.array_equal(labels, want.labels), (p, min_degree)
            borders += want.n_borders
            if min_degree == 0:
                s_labels, s_clusters, s_edges = m.cluster(listed, p)
                assert labels.tobytes() == s_labels.tobytes() and (n_clusters, n_edges) == (s_clusters, s_edges)
                assert n_core_edges == n_edges and ((kinds == CORE) | (labels == NO_CLUSTER)).all()
    assert borders > 0


# ---- cluster_within under the sweep ---------------------------------------------------------------------------------------

def _within(m, listed, blocks, p):
    m.set_option("scope_strategy", 1)
    try:
        out = m.cluster_within(listed, blocks, p)
        names = m.last_kernels()
    finally:
        m.set_option("scope_strategy", 0)
    assert W_SWEEP in names and W_DIRECT not in names and "cluster_sweep_kernel" not in names, names
    return out


@pytest.mark.parametrize("keys", ["pairs", "families"])
@pytest.mark.parametrize("name", LISTS)
def test_cluster_within_under_the_sweep_equals_the_blocked_truth(case, name, keys):
    m, h, listed = case.m, case.h, case.lists[name]
    blocks = KEYS[keys](listed)
    # a block with nodes of both images: under `families` a moved row stays with its base family
    held = np.array([int(r) in h.held for r in listed])
    image = np.array([h.image(r) if ok else -1 for r, ok in zip(listed.tolist(), held.tolist())])
    both = [k for k in np.unique(blocks).tolist() if {0, 1} <= set(image[blocks == k].tolist())]
    assert both and (keys != "families" or set(C.key_families(np.array(h.moved_heads, dtype=np.uint32)).tolist()) <= set(both))
    edges = []
    for p in case.floors:
        w_labels, w_clusters, w_edges, _ = case.within_truth(name).cluster_within(listed, blocks, p, DT.LEAST)
        labels, n_clusters, n_edges = C.thrice(case, f"within {name} {keys} {p}", lambda p=p: _within(m, listed, blocks, p))
        print(f"{name}, {keys}, floor {p}: clusters {n_clusters} (truth {w_clusters}), edges {n_edges} (truth {w_edges})")
        assert n_edges == w_edges and n_clusters == w_clusters, p
        assert labels.dtype == np.uint32 and np.array_equal(labels, w_labels), p
        edges.append(w_edges)
    assert edges[0] > edges[-1] > 0
    plain = [case.truths(name)[p][0][2] for p in case.floors]
    assert edges[0] < plain[0] or keys == "families"             # (the keys cut edges)


@pytest.mark.parametrize("name", LISTS)
def test_all_keys_equal_is_the_plain_cluster_call_byte_for_byte(case, name):
    m, listed = case.m, case.lists[name]
    blocks = np.full(len(listed), 7, dtype=np.uint32)
    for p in case.floors:
        DT._same_bytes(_within(m, listed, blocks, p), m.cluster(listed, p))


# ---- cluster_extend: fresh puts labelled against what is there, and the other way round ----------------------------------

@pytest.mark.parametrize("name", LISTS)
def test_cluster_extend_with_the_base_old_and_the_pending_new_and_the_other_way_round(case, name):
    m, h, listed = case.m, case.h, case.lists[name]
    pending = np.isin(listed, np.array(sorted(h.pending), dtype=np.uint32))
    in_base, in_delta = listed[~pending], listed[pending]          # (the deleted, listed among the base's, are no nodes)
    assert len(in_delta) >= 60 and len(in_base) >= 700
    truth = case.truth(name)
    for p in case.floors:
        for old, new, what in ((in_base, in_delta, "pending new"), (in_delta, in_base, "base new")):
            want, seeds, got = check_contract(m, truth, old, new, p, least=DT.LEAST)
            C.thrice(case, f"extend {name} {what} {p}", lambda old=old, seeds=seeds, new=new, p=p: m.cluster_extend(old, seeds, new, p))
            _named(m, "cluster_extend_sweep_kernel")
            assert want.old_new_edges >= 1 and want.new_new_edges >= 1, (p, what)


# ---- the exact bar, in the delta ------------------------------------------------------------------------------------------

def test_the_copies_whose_matches_are_exactly_the_bar_join_the_glued_string_at_500_and_not_at_501(case):
    m, h, g = case.m, case.h, case.h.handmade
    listed = case.lists["handmade"]
    truth = case.truth("handmade")
    copies = len(g.held_copies)
    for p, edges, clusters in ((500, copies * (copies - 1) // 2 + copies, 1), (501, copies * (copies - 1) // 2, 2)):
        w_labels, w_clusters, w_edges, _ = truth.cluster(listed, p)
        assert (w_clusters, w_edges) == (clusters, edges)
        labels, n_clusters, n_edges = m.cluster(listed, p)
        assert (n_clusters, n_edges) == (w_clusters, w_edges) and np.array_equal(labels, w_labels), p
        assert labels[listed == h.copy_deleted] == NO_CLUSTER
        l_labels, l_clusters, l_edges = m.cluster_levels(listed, [p])
        assert (l_clusters[0], l_edges[0]) == (w_clusters, w_edges) and np.array_equal(l_labels[0], w_labels), p
        want = CentresTruth(truth, listed, p)
        labels, degrees, centres, attached, n_clusters, n_edges = m.cluster_centres(listed, p)
        assert (n_clusters, n_edges) == (w_clusters, w_edges) and np.array_equal(labels, w_labels), p
        assert np.array_equal(degrees, want.degrees) and np.array_equal(centres, want.centres), p
        assert np.array_equal(attached, want.attached), p
        for min_degree in (0, copies, copies + 1):
            want = CoresEdges(truth, listed, p).cores(min_degree)
            labels, degrees, kinds, n_clusters, n_edges, n_core_edges = m.cluster_cores(listed, p, min_degree)
            assert (n_clusters, n_edges, n_core_edges) == (want.n_clusters, want.n_edges, want.n_core_edges), (p, min_degree)
            assert np.array_equal(labels, want.labels) and np.array_equal(degrees, want.degrees), (p, min_degree)
            assert np.array_equal(kinds, want.kinds), (p, min_degree)
        own = (listed == g.glued).astype(np.uint32)               # the glued string under a key of its own joins nothing
        for blocks, w in ((np.zeros(len(listed), dtype=np.uint32), (w_labels, w_clusters, w_edges)),
                          (own, (truth.cluster(listed, 501)[0], 2, copies * (copies - 1) // 2))):
            labels, n_clusters, n_edges = _within(m, listed, blocks, p)
            assert (n_clusters, n_edges) == w[1:] and np.array_equal(labels, w[0]), p
        old, new = g.held_copies, np.array([g.glued], dtype=np.uint32)
        check_contract(m, truth, old, new, p)


# ---- fold invariance (the last test: it changes the map) -----------------------------------------------------------------

def test_after_the_fold_one_image_answers_every_call_with_the_same_bytes(case):
    C.fold_and_compare(case, at_least=100)
