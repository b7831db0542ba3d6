"""The floor sweeps where dense slices are left out of the count: above_sweep_kernel, the similarity sweep,
cluster_sweep_kernel, cluster_levels_sweep_kernel, cluster_centres_sweep_kernel (count and mark) and
cluster_cores_sweep_kernel (degree and unite) each carry their own copy of the same sweep over a window's postings --
the list of at most 64 dense slices, the L largest left out and asked about in their bitmaps, 16-bit counters over two
half windows for a needle of more than 255 trigrams, and a needle's windows shared among workgroups.  On the other
haystacks of the suite hardly a slice is dense; here, on dense_case.py's map ("dense_min" 64, two windows, families of
glued words with T = 122 .. 955 and 85 .. 673 dense trigrams in window 0), every copy runs with more than 64 dense
slices, with L below, at and capped under the list's length, with neighbours in the upper half window of a wide needle,
with held strings that are no nodes behind a bitmap hit, and with one and with two workgroups a needle.  Every answer
is compared exactly with the host's truths (cluster_truth.py, cluster_centres_truth.py, cluster_cores_truth.py,
above_truth.py, similar_truth.py: numpy over the strings' tokenisations, nothing of the library), and three calls in a
row give identical bytes, whatever order the list of 64 was filled in.  One more map has every option at its default."""
from types import SimpleNamespace

import numpy as np
import pytest

import above_truth
import dense_case as D
import similar_truth
from blurrily_amd.map import _pack
from cluster_centres_truth import CentresTruth
from cluster_cores_truth import BORDER, CORE, CoresEdges
from dense_truths import ArrayAbove, FlooredSimilar, _same_bytes, floor_bar
from helpers import Oracle

pytestmark = pytest.mark.gpu
FIXED_FLOORS = (200, 350, 600)
LEAST = 200                                                    # every floor is at least this: the truths keep no pair below it
MIN_DEGREES = (0, 2, 3, 5)
# the family pair whose permille p* gives the last two floors, p* and p* + 1: of the thirteenth family (110 words),
# the string without its first fifth and the one with its words reversed
PAIR_FAMILY, PAIR_MEMBERS = 12, (4, 5)


@pytest.fixture(scope="module")
def case():
    """dense_case.py's map, the two lists, the floors, and the truths of each list, computed once and left unchanged."""
    import torch
    m, h = D.build()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    family = np.array([r for head in h.heads for r in h.family(head)], dtype=np.uint32)
    words = h.refs[:D.N_WORDS]
    lists = {"short": np.concatenate([words[::97], family]), "long": np.concatenate([words[::9], family])}
    # windows_per_workgroup: per = max(1, n_windows * nodes / (8 CUs)), at most n_windows
    assert 2 * len(lists["short"]) < 8 * cus, (len(lists["short"]), cus)     # per == 1: two workgroups a needle
    assert len(lists["long"]) >= 8 * cus, (len(lists["long"]), cus)          # per == 2: one
    head = h.heads[PAIR_FAMILY]
    low, high = (head + k for k in PAIR_MEMBERS)
    if h.loc[low][1] > h.loc[high][1]:
        low, high = high, low
    # both in window 0 at ranks of the upper half, the family wide: `high` finds `low` in its half == 1 pass
    assert h.T(head) > 255 and h.T(low) > 255 and h.T(high) > 255
    assert h.loc[low][0] == h.loc[high][0] == 0 and D.HALF <= h.loc[low][1] < h.loc[high][1]
    p_star = h.permille(low, high)
    assert 350 <= p_star < 999 and not {p_star, p_star + 1} & set(FIXED_FLOORS), p_star
    floors = tuple(sorted(FIXED_FLOORS + (p_star, p_star + 1)))
    c = SimpleNamespace(m=m, h=h, lists=lists, floors=floors, pair=(low, high), p_star=p_star, family=family, cus=cus,
                        _truths={})

    def truths(name):
        """{floor: (Truth.cluster's answer, CentresTruth, CoresEdges)} of a list (Truth keeps one list's pairs)."""
        if name not in c._truths:
            listed = lists[name]
            c._truths[name] = {p: (h.truth.cluster(listed, p, LEAST), CentresTruth(h.truth, listed, p, LEAST),
                                   CoresEdges(h.truth, listed, p, LEAST)) for p in floors}
        return c._truths[name]

    c.truths = truths
    yield c
    m.close()


def test_the_bars_put_L_on_all_three_sides_of_the_list_of_64(case):
    h, heads = case.h, case.h.heads
    # every head has more dense slices in window 0 than the list holds: nd recorded = 64 < s_nd
    assert all(h.dense(x, 0) > D.MAX_DENSE for x in heads)
    sides = {"below": 0, "cap": 0, "all": 0}
    for x in heads:
        for p in case.floors:
            t = floor_bar(h.T(x), p)
            sides["below"] += 1 < t and t - 1 < D.MAX_DENSE          # t - 1 < nd: only the largest are left out
            sides["cap"] += D.MAX_DENSE < t - 1                       # L is capped at the 64 recorded
            sides["all"] += 1 <= h.dense_padded(x, 1) <= min(t - 1, D.MAX_DENSE)   # window 1: nd <= t - 1, all are left out
    print(sides)
    assert min(sides.values()) >= 3, sides
    narrow = [x for x in heads if h.T(x) <= 255]
    wide = [x for x in heads if h.T(x) > 255]
    assert len(narrow) >= 3 and len(wide) >= 3                     # both counter widths leave slices out


def _edge_set(h, e):
    """A CoresEdges' edges as a set of sorted pairs of references."""
    refs = h.truth.refs
    return {(min(a, b), max(a, b)) for a, b in zip(refs[e.a].tolist(), refs[e.b].tolist())}


def test_the_upper_half_pair_and_a_pair_across_the_windows_are_edges(case):
    h = case.h
    pair = (min(case.pair), max(case.pair))
    family = set(case.family.tolist())
    for name in ("short", "long"):
        of = case.truths(name)
        # found by the half == 1 pass of the member at the higher position and nowhere else: an edge is its higher
        # end's to find.  An edge up to p*, none at p* + 1.
        assert pair in _edge_set(h, of[350][2]) and pair in _edge_set(h, of[case.p_star][2]), name
        assert pair not in _edge_set(h, of[case.p_star + 1][2]), name
        # a family member of window 1 with an edge into window 0
        assert any(a in family and {h.loc[a][0], h.loc[b][0]} == {0, 1} for a, b in _edge_set(h, of[350][2])), name


@pytest.mark.parametrize("name", ["short", "long"])
def test_cluster_equals_the_truth_at_every_floor(case, name):
    m, listed = case.m, case.lists[name]
    for p in case.floors:
        (w_labels, w_clusters, w_edges, _), _, _ = case.truths(name)[p]
        one, two, three = (m.cluster(listed, p) for _ in range(3))
        labels, n_clusters, n_edges = one
        print(f"{name}, floor {p}: clusters {n_clusters} (truth {w_clusters}), edges {n_edges} (truth {w_edges})")
        assert "cluster_sweep_kernel" in m.last_kernels()
        assert n_edges == w_edges and n_clusters == w_clusters, p
        assert labels.dtype == np.uint32 and np.array_equal(labels, w_labels), p
        _same_bytes(one, two)
        _same_bytes(one, three)
    assert case.truths(name)[200][0][2] > case.truths(name)[600][0][2] > 0


@pytest.mark.parametrize("name", ["short", "long"])
def test_cluster_levels_equals_the_truth_and_the_single_floor_calls(case, name):
    m, listed, floors = case.m, case.lists[name], case.floors
    one, two, three = (m.cluster_levels(listed, floors) for _ in range(3))
    assert "cluster_levels_sweep_kernel" in m.last_kernels()
    labels, n_clusters, n_edges = one
    assert labels.dtype == np.uint32 and labels.shape == (len(floors), len(listed))
    for k, p in enumerate(floors):
        (w_labels, w_clusters, w_edges, _), _, _ = case.truths(name)[p]
        print(f"{name}, floor {p}: clusters {n_clusters[k]} (truth {w_clusters}), edges {n_edges[k]} (truth {w_edges})")
        assert n_edges[k] == w_edges and n_clusters[k] == w_clusters, p
        assert np.array_equal(labels[k], w_labels), p
        s_labels, s_clusters, s_edges = m.cluster(listed, p)
        assert labels[k].tobytes() == s_labels.tobytes() and (s_clusters, s_edges) == (n_clusters[k], n_edges[k]), p
    _same_bytes(one, two)
    _same_bytes(one, three)


@pytest.mark.parametrize("name", ["short", "long"])
def test_cluster_centres_equals_the_truth_at_every_floor(case, name):
    m, listed = case.m, case.lists[name]
    for p in case.floors:
        want = case.truths(name)[p][1]
        one, two, three = (m.cluster_centres(listed, p, attached=True) for _ in range(3))
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
        _same_bytes(one, two)
        _same_bytes(one, three)


def _anchors_across(h, e, want, members):
    """The borders among `members` whose anchor -- the core neighbour of the highest degree, the smallest reference
    among equals -- lies in the other window: (border, anchor), from the truth's edges."""
    refs, out = h.truth.refs, []
    for r in members:
        if want.kind_of[r] != BORDER:
            continue
        i = int(np.searchsorted(refs, r))
        near = refs[np.concatenate([e.b[e.a == i], e.a[e.b == i]])].tolist()
        best = max((x for x in near if want.kind_of[x] == CORE), key=lambda x: (want.degree_of[x], -x))
        assert want.label_of[r] == want.label_of[best]
        if h.loc[best][0] != h.loc[r][0]:
            out.append((r, best))
    return out


@pytest.mark.parametrize("name", ["short", "long"])
def test_cluster_cores_equals_the_truth_at_every_floor_and_min_degree(case, name):
    m, h, listed = case.m, case.h, case.lists[name]
    across = []
    for p in case.floors:
        e = case.truths(name)[p][2]
        for min_degree in MIN_DEGREES:
            want = e.cores(min_degree)
            one, two, three = (m.cluster_cores(listed, p, min_degree) for _ in range(3))
            assert {"cluster_cores_sweep_kernel", "cluster_cores_sweep_kernel<unite>"} <= set(m.last_kernels())
            labels, degrees, kinds, n_clusters, n_edges, n_core_edges = one
            print(f"{name}, floor {p}, min_degree {min_degree}: clusters {n_clusters} (truth {want.n_clusters}), edges "
                  f"{n_edges} (truth {want.n_edges}), core edges {n_core_edges} (truth {want.n_core_edges}), borders "
                  f"{int((kinds == BORDER).sum())} (truth {want.n_borders})")
            assert n_edges == want.n_edges and n_core_edges == want.n_core_edges, (p, min_degree)
            assert n_clusters == want.n_clusters, (p, min_degree)
            assert degrees.dtype == np.uint32 and np.array_equal(degrees, want.degrees), (p, min_degree)
            assert kinds.dtype == np.uint8 and np.array_equal(kinds, want.kinds), (p, min_degree)
            assert labels.dtype == np.uint32 and np.array_equal(labels, want.labels), (p, min_degree)
            assert int(degrees.sum(dtype=np.uint64)) == 2 * n_edges, (p, min_degree)
            _same_bytes(one, two)
            _same_bytes(one, three)
            if min_degree == 0:
                s_labels, s_clusters, s_edges = m.cluster(listed, p)
                assert labels.tobytes() == s_labels.tobytes() and (n_clusters, n_edges) == (s_clusters, s_edges)
                assert n_core_edges == n_edges and (kinds == CORE).all()
            else:
                across += _anchors_across(h, e, want, case.family.tolist())
    # a needle of window 1 whose anchor lies in window 0: with two workgroups a needle (the short list) the one that
    # sweeps window 0 raises anchor[q] from its own reduction, and the one that sweeps window 1 has nothing to raise
    print(f"{name}: family borders anchored in the other window {sorted(set(across))}")
    if name == "short":
        assert any(h.loc[r][0] == 1 and h.loc[best][0] == 0 for r, best in across)


# ---- the threshold find and the similarity find ----------------------------------------------------------------------

ABOVE_BARS = ((1, 0), (3, 0), (0, 200), (0, 600), (0, 1000))
SIMILAR_LIMITS = (10, 1000)


def _needles(h, words):
    heads = [h.held[x] for x in h.heads]
    wide = heads[-1]
    other = [wide + b" qq", heads[9][len(heads[9]) // 3:2 * len(heads[9]) // 3]]
    assert not set(other) & set(h.held.values())                  # two strings that are not held
    plain = words[::len(words) // 40][:40]
    return heads + other + [b"", b"a"] + plain


@pytest.fixture(scope="module")
def finds(case):
    """The needles, the two restatements over the whole map, and each anchored on the oracle for four needles over a
    one-window prefix of the map (the first 15 000 words under default weights, which is what the oracle's bulk put
    takes)."""
    h = case.h
    words = h.strings[:D.N_WORDS]
    needles = _needles(h, words)
    assert len(needles) == 15 + 2 + 2 + 40
    prefix = words[:15000]
    o = Oracle()
    hay, off = _pack(prefix)
    o.put_many(np.frombuffer(hay, dtype=np.uint8), off)
    refs, zeros = np.arange(1, 15001), np.zeros(15000, dtype=np.int64)
    a_small, r_small = above_truth.Truth(prefix, refs, zeros), ArrayAbove(prefix, refs, zeros)
    s_small = similar_truth.Truth(prefix, refs, zeros)
    f_small = FlooredSimilar(prefix, refs, zeros, LEAST)
    for s in (needles[0], needles[14], needles[-1], b"a"):
        full = o.find(s, 65535)
        assert len(full) < 65535
        assert a_small.rows(s, 1, 0) == full, s[:40]
        for mm, mp in ABOVE_BARS:
            assert r_small.rows(s, mm, mp).tolist() == a_small.rows(s, mm, mp), (s[:40], mm, mp)
        T = len(Oracle.tokenise(s))
        ranked = similar_truth.ranked([(r, mm, w, int(s_small.R[r - 1])) for r, mm, w in full], T)
        assert s_small.rows(s, 65535, 0) == similar_truth.cut(ranked, T, 65535, 0), s[:40]
        for p in FIXED_FLOORS:
            assert f_small.rows(s, 1000, p) == similar_truth.cut(ranked, T, 1000, p), (s[:40], p)
    return SimpleNamespace(needles=needles, above=ArrayAbove(h.strings, h.refs, h.weights),
                           similar=FlooredSimilar(h.strings, h.refs, h.weights, LEAST))


def _above_equal(rows, row_off, needles, truth, mm, mp):
    assert rows.dtype == np.uint32 and len(row_off) == len(needles) + 1
    for i, s in enumerate(needles):
        assert np.array_equal(rows[int(row_off[i]):int(row_off[i + 1])], truth.rows(s, mm, mp)), (s[:40], mm, mp)


def test_find_above_equals_the_numpy_restatement(case, finds):
    m, h, needles = case.m, case.h, finds.needles
    packed, offsets = _pack(needles)
    T = [len(Oracle.tokenise(s)) for s in needles]
    # bars on either side of the list's 64, for both counter widths
    assert any(t <= 255 and above_truth.bar(t, 0, 200) - 1 < D.MAX_DENSE for t in T[:15])
    assert any(t > 255 and above_truth.bar(t, 0, 600) - 1 > D.MAX_DENSE for t in T[:15])
    for mm, mp in ABOVE_BARS:
        one = m.find_batch_above_packed(packed, offsets, mm, mp)
        assert "above_sweep_kernel" in m.last_kernels()
        _above_equal(*one, needles, finds.above, mm, mp)
        _same_bytes(one, m.find_batch_above_packed(packed, offsets, mm, mp))
        print(f"above {mm, mp}: {len(one[0])} rows")
    # a family's rows at the floors: its members, on both sides of rank 32768 and in both windows
    rows, row_off = m.find_batch_above_packed(packed, offsets, 0, 600)
    for i, head in enumerate(h.heads):
        got = set(rows[int(row_off[i]):int(row_off[i + 1]), 0].tolist())
        assert got >= {head, head + 1, head + 2, head + 3}, head


def test_find_above_by_reference_equals_the_numpy_restatement(case, finds):
    m, h = case.m, case.h
    refs = np.concatenate([case.family, np.array([123456789], dtype=np.uint32)])
    strings = [h.held[int(r)] for r in case.family]
    for mm, mp in ((0, 200), (0, 600), (0, 1000)):
        rows, row_off, ntri = m.find_batch_by_reference_above(refs, mm, mp)
        assert "above_sweep_kernel" in m.last_kernels()
        assert ntri.tolist() == [h.T(int(r)) for r in case.family] + [0]
        assert row_off[-1] == row_off[-2]                          # (the absent reference: no rows)
        _above_equal(rows, row_off[:-1], strings, finds.above, mm, mp)


def _similar_equal(out, needles, truth, limit, p):
    rows, counts, ntri = out[:3]
    for i, s in enumerate(needles):
        got = [r + [t] for r, t in zip(rows[i, :counts[i]].tolist(), ntri[i, :counts[i]].tolist())]
        assert got == truth.rows(s, limit, p), (s[:40], limit, p)


def test_find_similar_equals_the_numpy_restatement(case, finds):
    m, needles = case.m, finds.needles
    packed, offsets = _pack(needles)
    for limit in SIMILAR_LIMITS:
        for p in FIXED_FLOORS:
            one = m.find_batch_similar_packed(packed, offsets, limit, p)
            assert "similar_sweep_kernel" in m.last_kernels()
            _similar_equal(one, needles, finds.similar, limit, p)
            _same_bytes(one, m.find_batch_similar_packed(packed, offsets, limit, p))
    # the rows of a head at the lowest floor hold the members of its family in the upper half and in window 1
    low, high = case.pair
    head = case.h.heads[PAIR_FAMILY]
    assert {low, high} <= {r[0] for r in finds.similar.rows(case.h.held[head], 1000, 200)}


def test_find_similar_by_reference_equals_the_numpy_restatement(case, finds):
    m, h = case.m, case.h
    refs = np.concatenate([case.family, np.array([123456789], dtype=np.uint32)])
    strings = [h.held[int(r)] for r in case.family]
    for limit, p in ((10, 350), (1000, 200), (1000, 600)):
        rows, counts, ntri, nb = m.find_batch_by_reference_similar(refs, limit, p)
        assert "similar_sweep_kernel" in m.last_kernels()
        assert nb.tolist() == [h.T(int(r)) for r in case.family] + [0] and counts[-1] == 0
        _similar_equal((rows[:-1], counts[:-1], ntri[:-1]), strings, finds.similar, limit, p)


# ---- exactly t matches, every one of them in the needle's largest dense slices ---------------------------------------

def test_a_neighbour_whose_matches_are_exactly_the_bar_and_all_in_the_densest_slices_is_found():
    """L = t - 1 and not one more: seventy copies of a word and, at the highest position, the word glued to another.
    The word's six trigrams are the glued string's only dense slices, the bar at floor 500 is t = 6 of its 12, and a copy
    shares exactly those six -- with five slices left out, the sixth is the one counted match that gets it asked about."""
    from blurrily_amd import RawMap
    word, other = b"klmno", b"pqrst"
    glued = word + b" " + other
    held = {1: glued, 100: other, 101: b"uvwxy"}
    held.update({r: word for r in range(2, 72)})
    refs = np.array(sorted(held), dtype=np.uint32)
    weights = np.where(refs == 1, 100, 1).astype(np.uint32)        # (the glued string last: the edges are its to find)
    strings = [held[int(r)] for r in refs]
    h = D.Host(held, weights, [], D.DENSE_MIN)
    assert set(h.codes(2).tolist()) < set(h.codes(1).tolist()) and (h.T(2), h.T(1)) == (6, 12)
    assert h.loc[1] == (0, len(held) - 1) and floor_bar(12, 500) == 6 and h.permille(1, 2) == 500
    assert h.dense_padded(1, 0) == h.dense(1, 0) == 6 and sorted(h.postings[0][h.codes(2)].tolist()) == [71] * 6
    m = RawMap()
    m.set_option("dense_min", D.DENSE_MIN)
    m.put_many_packed(*_pack(strings), refs, weights)
    try:
        m.sync_device()
        assert m.device_info()["n_bitmaps"] == 6
        listed = refs
        for p, edges in ((500, 70 * 69 // 2 + 70), (501, 70 * 69 // 2)):
            w_labels, w_clusters, w_edges, _ = h.truth.cluster(listed, p)
            assert w_edges == edges and w_clusters == (3 if p == 500 else 4)
            labels, n_clusters, n_edges = m.cluster(listed, p)
            assert (n_clusters, n_edges) == (w_clusters, w_edges) and np.array_equal(labels, w_labels), p
            l_labels, l_clusters, l_edges = m.cluster_levels(listed, [p])
            assert (l_clusters[0], l_edges[0]) == (w_clusters, w_edges) and np.array_equal(l_labels[0], w_labels), p
            want = CentresTruth(h.truth, listed, p)
            labels, degrees, centres, attached, n_clusters, n_edges = m.cluster_centres(listed, p)
            assert (n_clusters, n_edges) == (w_clusters, w_edges) and np.array_equal(labels, w_labels), p
            assert np.array_equal(degrees, want.degrees) and np.array_equal(centres, want.centres), p
            assert np.array_equal(attached, want.attached), p
            if p == 500:                                            # the glued string is the centre: a copy's edge with it attaches it
                assert want.centre_of[2] == 1 and want.attached_of[2] == 1 and want.degree_of[1] == 70
            for min_degree in (0, 70, 71):
                want = CoresEdges(h.truth, listed, p).cores(min_degree)
                labels, degrees, kinds, n_clusters, n_edges, n_core_edges = m.cluster_cores(listed, p, min_degree)
                assert (n_clusters, n_edges, n_core_edges) == (want.n_clusters, want.n_edges, want.n_core_edges)
                assert np.array_equal(labels, want.labels) and np.array_equal(degrees, want.degrees), (p, min_degree)
                assert np.array_equal(kinds, want.kinds), (p, min_degree)
            above = ArrayAbove(strings, refs, weights)
            similar = similar_truth.Truth(strings, refs, weights)
            needles = [glued, word, other]
            assert len(above.rows(glued, 0, p)) == (71 if p == 500 else 1)
            _above_equal(*m.find_batch_above_packed(*_pack(needles), 0, p), needles, above, 0, p)
            _similar_equal(m.find_batch_similar_packed(*_pack(needles), 1000, p), needles, similar, 1000, p)
            rows, row_off, _ = m.find_batch_by_reference_above(np.array([1], dtype=np.uint32), 0, p)
            assert np.array_equal(rows, above.rows(glued, 0, p))
    finally:
        m.close()


# ---- every option at its default ---------------------------------------------------------------------------------------

def test_the_default_dense_min_with_families_in_the_upper_half_and_across_it():
    m, h = D.build_default()
    try:
        family = np.array([r for head in h.heads for r in h.family(head)], dtype=np.uint32)
        listed = np.unique(np.concatenate([h.refs[::5], family]))
        floors = (350, 600)
        above = ArrayAbove(h.strings, h.refs, h.weights)
        similar = FlooredSimilar(h.strings, h.refs, h.weights, floors[0])
        needles = [h.held[int(r)] for r in family] + h.strings[7::1000] + [b"", b"a"]
        packed, offsets = _pack(needles)
        for p in floors:
            # every dense slice of a family's is left out: 1 <= nd <= t - 1
            assert all(1 <= h.dense_padded(x, 0) <= min(floor_bar(h.T(x), p) - 1, D.MAX_DENSE) for x in h.heads)
            w_labels, w_clusters, w_edges, _ = h.truth.cluster(listed, p, floors[0])
            labels, n_clusters, n_edges = m.cluster(listed, p)
            print(f"floor {p}: clusters {n_clusters} (truth {w_clusters}), edges {n_edges} (truth {w_edges})")
            assert (n_clusters, n_edges) == (w_clusters, w_edges) and np.array_equal(labels, w_labels), p
            want = CoresEdges(h.truth, listed, p, floors[0]).cores(2)
            labels, degrees, kinds, n_clusters, n_edges, n_core_edges = m.cluster_cores(listed, p, 2)
            assert (n_clusters, n_edges, n_core_edges) == (want.n_clusters, want.n_edges, want.n_core_edges), p
            assert np.array_equal(labels, want.labels) and np.array_equal(degrees, want.degrees), p
            assert np.array_equal(kinds, want.kinds) and int(degrees.sum(dtype=np.uint64)) == 2 * n_edges, p
            # the families are joined within the upper half and across the halves
            for head in h.heads:
                assert len({want.label_of[r] for r in h.family(head)}) == 1 and want.degree_of[head] >= 5, (p, head)
            _above_equal(*m.find_batch_above_packed(packed, offsets, 0, p), needles, above, 0, p)
            for limit in SIMILAR_LIMITS:
                _similar_equal(m.find_batch_similar_packed(packed, offsets, limit, p), needles, similar, limit, p)
    finally:
        m.close()
