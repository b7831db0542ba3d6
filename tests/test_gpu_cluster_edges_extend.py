"""Cluster edges extend and between on the GPU (cluster_edges_extend.hip, cluster_edges_extend_kernels.hip): the records
are compared byte for byte with the host's (cluster_edges_extend_truth.py over cluster_edges_truth.py: nothing of the
library) and with what the other entries say of the same graph -- blurrily_storage_cluster_edges over the old list, the
new list and both (the two contracts and the identity between the two entries), blurrily_storage_cluster_extend's
n_edges, the count-only calls -- and ``between`` both ways round, so that both needle sides run.  Over the oracle
haystacks split mod 7 at floors where the split is telling (asserted), test_gpu_cluster_levels.py's built case (the
chain, twins of every counter width, the exact floors, empty strings), record counts at the sort's tile and the first
merge pass, option "cluster_edges_max" against the append cursor, a haystack of two windows, both images either way
round with pending puts, a deleted end, a reference put again and the fold, dense_case.py's map where slices are left
out, repeated calls, and beside the find, ``cluster`` and ``cluster_edges``, which it leaves as they were."""
import ctypes
import errno

import numpy as np
import pytest

import dense_case as D
import workloads as W
from blurrily_amd import RawMap, _native
from blurrily_amd.map import _pack
import cluster_edges_truth as CE
from cluster_edges_extend_truth import Split
from cluster_truth import Truth
from helpers import ORACLE_CASES, oracle_case_inputs
# (ORACLE_FLOORS: per oracle haystack the floors, and per floor the old-old, old-new and new-new edges of the split mod 7,
# from a CPU run of the truth, which tests/test_cluster_edges_extend_abi.py asserts without a GPU)
from test_cluster_edges_extend_abi import ORACLE_FLOORS
from test_gpu_cluster_levels import A, B, C, SHORT, _j, _map_of, built_case

pytestmark = pytest.mark.gpu
TILE = 4096                                                   # the sort's tile (cluster.h: kClusterEdgesTile)
SWEEP, OLD_SWEEP = "cluster_edges_extend_sweep_kernel", "cluster_edges_sweep_kernel"
TILES, MERGE, ROWS = "cluster_edges_tiles_kernel", "cluster_edges_merge_kernel", "cluster_edges_rows_kernel"
EMPTY = np.zeros((0, 3), dtype=np.uint32)
EXTEND, BETWEEN = "blurrily_storage_cluster_edges_extend", "blurrily_storage_cluster_edges_between"


def ours(m):
    """The clustering kernels the last call launched (a table built at an image's first call is not the call's)."""
    return [k for k in m.last_kernels() if k.startswith("cluster_")]


def check(m, truth, first, second, p, least=None, around=True):
    """Both entries on two lists at one floor against the truth, byte for byte (truth None: left out); with ``around``
    against the other entries too: the two contracts, the identity, the counts.  Returns (the truth's split, extend's
    records, between's)."""
    first, second = np.asarray(first, dtype=np.uint32), np.asarray(second, dtype=np.uint32)
    s = Split(truth, first, second, p, least).check_itself() if truth is not None else None
    ext = m.cluster_edges_extend(first, second, p)
    names = ours(m)
    btw = m.cluster_edges_between(first, second, p)
    print(f"floor {p}: {len(first)} + {len(second)} listed; old-old, old-new, new-new edges "
          f"{s.figures() if s else '(no truth)'}; extend {len(ext)} records, between {len(btw)}")
    assert ext.dtype == np.uint32 and btw.dtype == np.uint32 and ext.shape[1:] == btw.shape[1:] == (3,)
    if s:
        assert ext.shape == s.extend.shape and ext.tobytes() == s.extend.tobytes(), p
        assert btw.shape == s.between.shape and btw.tobytes() == s.between.tobytes(), p
    if len(second):
        assert names[0] == "cluster_nodes_kernel" and SWEEP in names and OLD_SWEEP not in names, names
        assert (TILES in names) == (ROWS in names and len(ext) >= 2) and (MERGE in names) == (len(ext) > TILE), names
    if not around:
        return s, ext, btw
    # the contracts: the old list's records and the extend's are the whole; between and the new list's are the extend's
    before, among = m.cluster_edges(first[~np.isin(first, second)], p), m.cluster_edges(second, p)
    whole = m.cluster_edges(np.concatenate([first, second]), p)
    assert RawMap.merge_edges(before, ext).tobytes() == whole.tobytes() and (s is None or whole.tobytes() == s.whole.tobytes()), p
    assert RawMap.merge_edges(btw, among).tobytes() == ext.tobytes(), p
    # the counts: cluster_extend's n_edges (whatever the seeds), and the count-only calls
    seeds = np.asarray(first, dtype=np.uint32)
    assert m.cluster_extend(first, seeds, second, p)[3] == len(ext), p
    assert m.cluster_edge_count_extend(first, second, p) == len(ext), p
    assert not {TILES, MERGE, ROWS} & set(m.last_kernels()) and (SWEEP in m.last_kernels()) == bool(len(second))
    assert m.cluster_edge_count_between(first, second, p) == len(btw), p
    # between the other way round: for disjoint lists identical bytes (the side that sweeps does not show)
    if not np.isin(first, second).any():
        assert m.cluster_edges_between(second, first, p).tobytes() == btw.tobytes(), p
        assert m.cluster_edge_count_between(second, first, p) == len(btw), p
    return s, ext, btw


@pytest.mark.parametrize("kind,n,_limit", ORACLE_CASES)
def test_the_oracle_haystacks_split_mod_seven_both_contracts_the_identity_and_the_counts(kind, n, _limit):
    hay, off, _ = oracle_case_inputs(kind, n)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    m, truth = _map_of(held), Truth(held)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    old, new = listed[listed % 7 != 0], listed[listed % 7 == 0]     # 6 / 7 against 1 / 7: between sweeps either side
    floors, figures = ORACLE_FLOORS[kind]
    for p, figure in zip(floors, figures):
        s, ext, btw = check(m, truth, old, new, p, least=floors[0])
        print(f"{kind} at {p}: old-old, old-new, new-new edges: {s.figures()}")
        assert min(s.figures()) >= 1 and s.figures() == figure, (p, s.figures())
    m.close()


@pytest.fixture(scope="module")
def built():
    """test_gpu_cluster_levels.py's built case with the pair one trigram short of the chain's, in a map of its own.
    Left unchanged."""
    held = built_case()
    held.update({5004: SHORT, 5005: A[:-1]})                  # 7 / 15 against each other: 466 per mille
    assert _j(A, B) == (8, 16) and _j(B, C) == (6, 17) and _j(A, C)[0] == 0 and _j(A[:-1], SHORT) == (7, 15)
    m = _map_of(held)
    yield dict(m=m, held=held, truth=Truth(held), everything=np.array(sorted(held), dtype=np.uint32))
    m.close()


TWINS = (6000, 6004, 6008, 6012, 6016)                         # s of 15, 16, 255, 256 and 700 trigrams; s again behind it


def test_the_chain_the_twins_at_every_counter_width_the_exact_floors_and_the_empty_strings(built):
    m, truth, everything = built["m"], built["truth"], built["everything"]
    ext, btw = m.cluster_edges_extend, m.cluster_edges_between
    # B new, between old A and C: both its edges, at their whole per mille; at 353 the lower one is gone
    assert ext([5001, 5003], [5002], 300).tolist() == [[5001, 5002, 500], [5002, 5003, 352]]
    assert btw([5001, 5003], [5002], 300).tolist() == [[5001, 5002, 500], [5002, 5003, 352]]
    assert btw([5002], [5001, 5003], 352).tolist() == [[5001, 5002, 500], [5002, 5003, 352]]
    assert ext([5001, 5003], [5002], 353).tolist() == [[5001, 5002, 500]] == btw([5002], [5003, 5001], 353).tolist()
    # A and C new with B old; B held but not listed: no edge, whichever of them is new
    assert ext([5002], [5001, 5003], 300).tolist() == [[5001, 5002, 500], [5002, 5003, 352]]
    assert ext([5001], [5003], 0).shape == (0, 3) and btw([5003], [5001], 0).shape == (0, 3)
    assert ext([], [5001, 5003], 0).shape == (0, 3)
    # exactly at the floor and one per mille above, either way round
    for a, b, at in ((5001, 5002, 500), (5004, 5005, 466), (5002, 5003, 352)):
        for old, new in ((a, b), (b, a)):
            assert ext([old], [new], at).tolist() == [[a, b, at]] == btw([old], [new], at).tolist(), (old, new)
            assert ext([old], [new], at + 1).shape == (0, 3) and btw([old], [new], at + 1).shape == (0, 3)
        assert ext([], [a, b], at).tolist() == [[a, b, at]] and btw([], [a, b], at).shape == (0, 3)
    for t in TWINS:
        # a twin on each side, either way round: found wherever the other lies
        for old, new in ((t, t + 1), (t + 1, t)):
            assert ext([old], [new], 1000).tolist() == [[t, t + 1, 1000]] == btw([old], [new], 1000).tolist(), t
        # both twins new: the pair once, no needle counts itself; between has nothing across
        assert ext([], [t, t + 1], 1000).tolist() == [[t, t + 1, 1000]] and btw([], [t, t + 1], 1000).shape == (0, 3)
        assert ext([t + 2], [t + 1, t], 1000).tolist() == [[t, t + 1, 1000]] and btw([t + 2], [t + 1, t], 1000).shape == (0, 3)
        assert ext([], [t], 0).shape == (0, 3) and ext([t], [t], 0).shape == (0, 3)
    assert ext([7001], [7002], 1000).tolist() == [[7001, 7002, 1000]] == btw([7002], [7001], 1000).tolist()   # T == 1
    # a reference in both lists is new, on the right only: t old against t + 1 new; both named again, nothing lies across
    t = TWINS[2]
    assert ext([t, t + 1], [t + 1], 1000).tolist() == [[t, t + 1, 1000]] == btw([t, t + 1], [t + 1], 1000).tolist()
    assert ext([t, t + 1], [t, t + 1], 1000).tolist() == [[t, t + 1, 1000]] and btw([t, t + 1], [t + 1, t], 1000).shape == (0, 3)
    # an unheld reference on either side: never an end
    assert ext([5001, 4000], [5002, 9999, 0xFFFFFFFF], 500).tolist() == [[5001, 5002, 500]]
    assert btw([0, 5001], [9999, 5002], 500).tolist() == [[5001, 5002, 500]]
    assert ext([4000], [9999, 0], 0).shape == (0, 3) and m.cluster_edge_count_between([4000], [9999, 0], 0) == 0
    # the whole case split mod 7, the counter-width nodes among old and new, at the exact floors
    old, new = everything[everything % 7 != 0], everything[everything % 7 == 0]
    assert any((t % 7 == 0) != ((t + 1) % 7 == 0) for t in TWINS)   # (a twin on either side of the split)
    # (a CPU run of the truth: 320 136 old-old, 103 363 old-new and 8 363 new-new edges at 0, 768, 261 and 27 at 200;
    # from 352 on no two multiples of 7 share an edge -- the twins below, both new, stand for those floors)
    for p in (0, 200, 352, 353, 500, 1000):
        s, _, _ = check(m, truth, old, new, p)
        assert min(s.figures()[:2]) >= 1 and (s.figures()[2] >= 1) == (p <= 200), (p, s.figures())
    # ... with both twins of every width new, and with B alone new
    twins = np.array([t + k for t in TWINS for k in (0, 1)], dtype=np.uint32)
    for new in (twins, np.array([5002], dtype=np.uint32)):
        s, got, _ = check(m, truth, everything[~np.isin(everything, new)], new, 352)
        rows = set(map(tuple, got.tolist()))
        assert ({(t, t + 1, 1000) for t in TWINS} <= rows) == (len(new) > 1) and ((5002, 5003, 352) in rows) == (len(new) == 1)


def test_both_lists_shuffled_with_repeats_overlaps_and_either_list_empty(built):
    m, truth, everything = built["m"], built["truth"], built["everything"]
    p = 200
    old, new = everything[everything % 7 != 0], everything[everything % 7 == 0]
    _, base_ext, base_btw = check(m, truth, old, new, p)
    rng = np.random.default_rng(5)
    absent = np.array([4000, 4001, 9999, 0xFFFFFFFF, 0], dtype=np.uint32)
    old_mixed = np.concatenate([old, old[::7], absent[:3]])
    new_mixed = np.concatenate([new, new[::3], absent[2:], absent[3:]])
    rng.shuffle(old_mixed)
    rng.shuffle(new_mixed)
    assert m.cluster_edges_extend(old_mixed, new_mixed, p).tobytes() == base_ext.tobytes() and len(base_ext) > 0
    assert m.cluster_edges_between(old_mixed, new_mixed, p).tobytes() == base_btw.tobytes() and len(base_btw) > 0
    assert m.cluster_edges_between(new_mixed, old_mixed, p).tobytes() == base_btw.tobytes()
    check(m, truth, old_mixed, new_mixed, p, around=False)
    # old references named again by the new list are new: the same as leaving them out of the old list
    again = np.concatenate([old, new[::2]])
    rng.shuffle(again)
    assert m.cluster_edges_extend(again, new, p).tobytes() == base_ext.tobytes()
    assert m.cluster_edges_between(again, new, p).tobytes() == base_btw.tobytes()
    s, _, _ = check(m, truth, everything, new, p)              # (every new reference is named by the old list too)
    assert len(s.first_only) == len(old)
    # n_old == 0: cluster_edges(new_refs); n_new == 0: no edge, no sweep; between with a side empty: no edge
    for listed in (everything, new_mixed):
        assert m.cluster_edges_extend([], listed, p).tobytes() == m.cluster_edges(listed, p).tobytes()
        assert m.cluster_edges_between([], listed, p).shape == (0, 3) and m.cluster_edges_between(listed, [], p).shape == (0, 3)
    assert m.cluster_edges_extend(everything, [], p).shape == (0, 3) and m.cluster_edge_count_extend(everything, [], 0) == 0
    assert m.cluster_edges_extend([], [], p).shape == (0, 3) and m.cluster_edge_count_between([], [], p) == 0
    check(m, truth, [], everything, p)
    # the records as they are: adjacency's first neighbour of a left row is its best link; cut_tree takes them
    listed = np.concatenate([old, new])
    row_off, neighbour, permille = RawMap.adjacency(base_btw, listed)
    want = CE.adjacency(base_btw, listed)
    assert row_off.tolist() == want[0].tolist() and neighbour.tolist() == want[1].tolist()
    linked = np.nonzero(np.diff(row_off.astype(np.int64))[:len(old)])[0]
    assert len(linked) > 0
    for i in linked.tolist()[:200]:
        mine = base_btw[(base_btw[:, :2] == old[i]).any(axis=1)]
        assert permille[row_off[i]] == mine[:, 2].max() and neighbour[row_off[i]] in new
    labels = m.cluster(listed, p)[0]
    whole = RawMap.merge_edges(m.cluster_edges(old, p), base_ext)
    assert RawMap.cut_tree(listed, labels, whole, p, min_permille=p).tobytes() == labels.tobytes()
    assert sum(r["merges"] == len(base_ext) for r in RawMap.merge_profile(base_ext)) == 1


def _raw(m, symbol, first, second, floor, edges, capacity):
    """A C entry as it is: (result, errno, n_edges)."""
    fn = getattr(_native.lib(), symbol)
    first, second = (np.ascontiguousarray(x, dtype=np.uint32) for x in (first, second))
    n_edges = ctypes.c_uint64(0xABCDEF)
    ctypes.set_errno(0)
    r = fn(m.handle, first.ctypes.data if len(first) else None, len(first), second.ctypes.data if len(second) else None,
           len(second), floor, edges.ctypes.data if edges is not None else None, capacity, ctypes.byref(n_edges))
    return r, ctypes.get_errno(), n_edges.value


def test_the_capacity_protocol_and_the_option_against_the_append_cursor():
    same = b"five of a kind"
    m = _map_of({r: same for r in (1, 2, 3, 4, 5)})
    # six edges each: 1 old and 2, 3, 4 new (three across, three among the new); 1, 2 left and 3, 4, 5 right
    cases = ((EXTEND, [1], [2, 3, 4], [[1, 2, 1000], [1, 3, 1000], [1, 4, 1000], [2, 3, 1000], [2, 4, 1000], [3, 4, 1000]]),
             (BETWEEN, [1, 2], [3, 4, 5], [[1, 3, 1000], [1, 4, 1000], [1, 5, 1000], [2, 3, 1000], [2, 4, 1000], [2, 5, 1000]]),
             (BETWEEN, [3, 4, 5], [1, 2], [[1, 3, 1000], [1, 4, 1000], [1, 5, 1000], [2, 3, 1000], [2, 4, 1000], [2, 5, 1000]]))
    was = m.get_option("cluster_edges_max")
    try:
        for symbol, first, second, want in cases:
            buf = np.full((8, 3), 0xEE, dtype=np.uint32)
            # count only; exactly enough room; one record less is ERANGE with the count and the buffer untouched
            assert _raw(m, symbol, first, second, 1000, None, 12345) == (0, 0, 6)
            assert not {TILES, MERGE, ROWS} & set(m.last_kernels()) and SWEEP in m.last_kernels()
            assert _raw(m, symbol, first, second, 1000, buf, 6) == (0, 0, 6)
            assert buf[:6].tolist() == want and (buf[6:] == 0xEE).all()
            buf[:] = 0xEE
            assert _raw(m, symbol, first, second, 1000, buf, 5) == (-1, errno.ERANGE, 6) and (buf == 0xEE).all()
            assert not {TILES, MERGE, ROWS} & set(m.last_kernels())
            assert _raw(m, symbol, first, second, 1000, buf, 0) == (-1, errno.ERANGE, 6) and (buf == 0xEE).all()
            # the option bounds the stored keys, never the count: 5 against 6 edges is EOVERFLOW, 6 fits
            m.set_option("cluster_edges_max", 5)
            assert _raw(m, symbol, first, second, 1000, buf, 8) == (-1, errno.EOVERFLOW, 6) and (buf == 0xEE).all()
            assert _raw(m, symbol, first, second, 1000, None, 0) == (0, 0, 6)           # (counting is not bounded)
            assert _raw(m, symbol, first, second, 1000, buf, 5) == (-1, errno.ERANGE, 6) and (buf == 0xEE).all()
            method = m.cluster_edges_extend if symbol == EXTEND else m.cluster_edges_between
            with pytest.raises(OSError) as err:
                method(first, second, 1000)
            assert err.value.errno == errno.EOVERFLOW
            m.set_option("cluster_edges_max", 6)
            assert _raw(m, symbol, first, second, 1000, buf, 8) == (0, 0, 6) and buf[:6].tolist() == want
            buf[:] = 0xEE
            assert _raw(m, symbol, first, second, 1000, buf, 1 << 40) == (0, 0, 6) and buf[:6].tolist() == want
            assert (buf[6:] == 0xEE).all()
            m.set_option("cluster_edges_max", was)
            # the Python method grows once from too small a room
            assert method(first, second, 1000, capacity=1).tolist() == want
            # nothing to find: no edge at capacity 0, a side with nothing on it, nothing listed
            assert _raw(m, symbol, [1], [99], 1000, buf, 0) == (0, 0, 0)
            assert _raw(m, symbol, first, [], 1000, buf, 2) == (0, 0, 0) and _raw(m, symbol, [], [], 0, None, 0) == (0, 0, 0)
            assert (buf[6:] == 0xEE).all()
    finally:
        m.set_option("cluster_edges_max", was)
    assert m.get_option("cluster_edges_max") == 1 << 28
    m.close()


def _pair_string(i):
    abc = "abcdefghijklmnopqrstuvwxyz"
    return b"pair " + bytes(abc[(i // 676) % 26] + abc[(i // 26) % 26] + abc[i % 26], "ascii") + b" twin"


@pytest.mark.parametrize("total", [TILE, TILE + 1, 2 * TILE + 1])
def test_the_sort_at_its_tile_one_above_it_and_one_above_twice_it(total):
    # between: a clique of 128 identical strings, 64 on each side (4 096 edges across), and disjoint identical pairs
    # with an end on each side on top
    held = {r: b"identical strings" for r in range(1, 129)}
    a, b = np.meshgrid(np.arange(1, 65), np.arange(65, 129), indexing="ij")
    want = [np.stack([a.reshape(-1), b.reshape(-1), np.full(TILE, 1000)], axis=1)]
    left, right = list(range(1, 65)), list(range(65, 129))
    for i in range(total - TILE):
        held[1000 + 2 * i] = held[1001 + 2 * i] = _pair_string(i)
        want.append(np.array([[1000 + 2 * i, 1001 + 2 * i, 1000]]))
        (left if i % 2 else right).append(1000 + 2 * i)
        (right if i % 2 else left).append(1001 + 2 * i)
    want = np.concatenate(want).astype(np.uint32)
    assert len(want) == total
    m = _map_of(held)
    for one, two in ((left, right), (right, left)):
        got = m.cluster_edges_between(one, two, 1000)
        assert got.tobytes() == want.tobytes()
        assert (MERGE in m.last_kernels()) == (total > TILE) and TILES in m.last_kernels() and SWEEP in m.last_kernels()
    assert m.cluster_edge_count_between(left, right, 1000) == total
    m.close()
    # extend: a clique of 91, all new (4 095 edges among the new), and pairs with the lower end old on top
    held = {r: b"identical strings" for r in range(1, 92)}
    old, new = [], list(range(1, 92))
    for i in range(total - TILE + 1):
        held[1000 + 2 * i] = held[1001 + 2 * i] = _pair_string(i)
        old.append(1000 + 2 * i)
        new.append(1001 + 2 * i)
    m = _map_of(held)
    got = m.cluster_edges_extend(old, new, 1000)
    assert len(got) == total and (MERGE in m.last_kernels()) == (total > TILE)
    assert got.tobytes() == m.cluster_edges(np.array(sorted(held), dtype=np.uint32), 1000).tobytes()   # (no old-old edge)
    assert got[:TILE - 1].tolist() == [[x, y, 1000] for x in range(1, 92) for y in range(x + 1, 92)]
    assert got[TILE - 1:].tolist() == [[1000 + 2 * i, 1001 + 2 * i, 1000] for i in range(total - TILE + 1)]
    m.close()


def test_a_haystack_of_two_windows_a_new_needle_in_each():
    n, p = 70000, 300
    hay, off = W.words(n, seed=17)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    weights = np.random.default_rng(23).integers(1, 1 << 20, size=n).astype(np.uint32)   # ranks unrelated to length
    m, truth = _map_of(held, weights), Truth(held)
    listed = np.arange(1, n + 1, dtype=np.uint32)
    loc = D.locate(listed, weights)
    old, new = listed[listed % 7 != 0], listed[listed % 7 == 0]
    # (all the pairs sharing a trigram do not fit the host: the truth keeps the pairs at or above the floor)
    s, ext, btw = check(m, truth, old, new, p, least=p)
    assert m.device_info()["n_windows"] >= 2 and min(s.figures()) >= 1
    is_new = set(new.tolist())
    # new needles with an edge in each window, edges across the windows, and new-new edges across them (a CPU run of
    # the truth: 21 277 old-old, 7 841 old-new and 699 new-new edges, 970 with a new end across the windows, 76 new-new)
    windows = {loc[x][0] for a, b, _ in ext.tolist() for x in (a, b) if x in is_new}
    across = sum(loc[a][0] != loc[b][0] for a, b, _ in ext.tolist())
    new_across = sum(loc[a][0] != loc[b][0] for a, b, _ in s.new_new.tolist())
    print(f"windows with a new end of an edge: {sorted(windows)}; edges across the windows: {across}, new-new: {new_across}")
    assert windows >= {0, 1} and across >= 1 and new_across >= 1
    # fifty new references that have an edge: tasks = n_windows, each needle gets many workgroups.  (Against the other
    # entries only: the contracts tie the records to cluster_edges', which the truth has just confirmed on this map.)
    ends = np.unique(s.whole[:, :2])
    few = np.concatenate([ends[:25], ends[-25:]]).astype(np.uint32)
    _, ext, _ = check(m, None, listed[~np.isin(listed, few)], few, p)
    assert len(ext) >= 25 and {loc[int(r)][0] for r in few} >= {0, 1}
    m.close()


def test_both_images_either_way_round_pending_puts_a_deleted_end_a_reference_put_again_and_the_fold():
    p = 200
    hay, off = W.words(5000, seed=7)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({9001: A, 9002: B, 9003: C})
    m = _map_of(held)
    m.sync_device()
    builds = m.device_info()["base_builds"]
    base = np.array(sorted(held), dtype=np.uint32)
    # a deleted end takes its edges with it, on either side
    m.delete(9002)
    del held[9002]
    truth = Truth(held)
    for first, second in ((base[base != 9002], [9002, 9001]), ([9002, 9003], base[base != 9002])):
        s, ext, _ = check(m, truth, first, second, p)
        assert 9002 not in ext[:, :2]
    base = base[base != 9002]
    # old in the base image, new as pending puts: edges into the base image and inside the delta image
    m.put(B, 9500, 0)
    m.put(B + b"x", 9501, 0)
    m.put(b"zzkkqqvv", 9502, 0)
    held.update({9500: B, 9501: B + b"x", 9502: b"zzkkqqvv"})
    truth = Truth(held)
    pending = np.array([9500, 9501, 9502], dtype=np.uint32)
    info = m.device_info()
    assert info["n_pending"] >= 3 and info["base_builds"] == builds
    s, ext, btw = check(m, truth, base, pending, p)
    rows = set(map(tuple, ext.tolist()))
    assert (9001, 9500, 500) in rows and (9003, 9500, 352) in rows and any(r[:2] == (9500, 9501) for r in rows)
    assert s.figures()[2] >= 1 and not any(r[:2] == (9500, 9501) for r in map(tuple, btw.tolist()))
    m.cluster_edges_extend(base, pending, p)
    assert m.last_kernels().count(SWEEP) == 2                 # (two images: the base and the pending puts)
    # the reverse: old pending, new in the base image; and either list across both images
    s, ext, _ = check(m, truth, pending, base, p)
    assert (9001, 9500, 500) in set(map(tuple, ext.tolist()))
    mixed_old = np.concatenate([base[base % 7 == 0], pending[:2]])
    mixed_new = np.concatenate([base[base % 7 != 0], pending[2:]])
    check(m, truth, mixed_old, mixed_new, p)
    # a reference deleted and put again with another text: a node of the delta image, its base rank no node
    m.delete(16)
    m.put(C + b"x", 16, 0)
    held[16] = C + b"x"
    truth = Truth(held)
    for first, second in ((base, pending), (base[base != 16], np.concatenate([pending, [16]])), (pending, base)):
        s, ext, _ = check(m, truth, first, second, p)
    assert any(r[:2] == (16, 9003) for r in map(tuple, ext.tolist()))
    before = m.cluster_edges_extend(base, pending, p)
    # the same after the log folds into a rebuilt base image
    big, bo = W.words(9000, seed=34)
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    folded = m.cluster_edges_extend(base, pending, p)          # (the same lists: the bulk is held but not listed)
    info = m.device_info()
    assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    assert folded.tobytes() == before.tobytes() and m.last_kernels().count(SWEEP) == 1
    check(m, Truth(held), np.concatenate([base, pending]), bulk[::3], p)
    m.close()


def test_dense_slices_left_out_and_sixteen_bit_halves_on_the_dense_map():
    m, h = D.build()
    family = np.array([r for head in h.heads for r in h.family(head)], dtype=np.uint32)
    listed = np.concatenate([h.refs[:D.N_WORDS][::97], family])
    old, new = listed[listed % 5 != 1], listed[listed % 5 == 1]
    # among the needles of either side: both counter widths with more dense slices than the list of 64 holds
    for side in (new, old):
        fam = [int(r) for r in side if r >= D.FAMILY_REF0]
        assert any(h.T(r) > 255 and h.dense(r, 0) > D.MAX_DENSE for r in fam)
        assert any(h.T(r) <= 255 and h.dense(r, 0) > D.MAX_DENSE for r in fam)
    found = [0, 0, 0]
    for p in (200, 350, 600):                                 # (tests/test_gpu_dense_floor_sweeps.py's fixed floors)
        s, _, _ = check(m, h.truth, old, new, p, least=200)
        found = [x + y for x, y in zip(found, s.figures())]
    assert min(found) >= 1, found
    m.close()


@pytest.fixture(scope="module")
def words_case():
    """The words oracle haystack in a map of its own, shared by the tests below and closed behind them."""
    hay, off, needles = oracle_case_inputs("words", 5000)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    m = _map_of(held)
    listed = np.arange(1, 5001, dtype=np.uint32)
    yield dict(m=m, needles=needles, old=listed[listed % 7 != 0], new=listed[listed % 7 == 0])
    m.close()


def test_three_calls_give_identical_bytes(words_case):
    m, old, new = words_case["m"], words_case["old"], words_case["new"]
    for p in (100, 200):
        for call in (lambda: m.cluster_edges_extend(old, new, p), lambda: m.cluster_edges_between(old, new, p),
                     lambda: m.cluster_edges_between(new, old, p)):
            one, two, three = (call() for _ in range(3))
            assert one.tobytes() == two.tobytes() == three.tobytes() and len(one) > 0


def test_the_calls_around_a_call_are_unchanged_and_the_kernels_are_named(words_case):
    c = words_case
    m, old, new = c["m"], c["old"], c["new"]
    listed = np.concatenate([old, new])
    packed, offsets = _pack(c["needles"])
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    find_kernels = m.last_kernels()
    around = [(lambda: m.cluster(listed, 200)), (lambda: m.cluster_edges(listed, 200))]
    before = []
    for call in around:
        result = call()
        before.append((result, m.last_kernels()))
    ext = m.cluster_edges_extend(old, new, 200)
    assert ours(m) == ["cluster_nodes_kernel", SWEEP, TILES, ROWS] and 2 <= len(ext) <= TILE
    for call in (lambda: m.cluster_edges_between(old, new, 200), lambda: m.cluster_edges_between(new, old, 200)):
        call()
        names = ours(m)
        assert names == ["cluster_nodes_kernel", SWEEP, TILES, ROWS], names
        for name in (OLD_SWEEP, "cluster_sweep_kernel", "cluster_extend_sweep_kernel", "cluster_extend_seed_kernel",
                     "cluster_edges_within_kernel", "cluster_label_kernel", "find_kernel"):
            assert name not in names, name
    m.cluster_edges_extend(old, new, 50)
    assert ours(m) == ["cluster_nodes_kernel", SWEEP, TILES, MERGE, ROWS]
    m.cluster_edge_count_extend(old, new, 200)
    assert ours(m) == ["cluster_nodes_kernel", SWEEP]
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == find_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    for call, (was, was_kernels) in zip(around, before):
        now = call()
        assert m.last_kernels() == was_kernels and SWEEP not in was_kernels
        for x, y in (zip(was, now) if isinstance(was, tuple) else ((was, now),)):
            assert x.tobytes() == y.tobytes() if isinstance(x, np.ndarray) else x == y
