"""Cluster edges on the GPU (cluster_edges.hip, cluster_edges_kernels.hip): the records are compared byte for byte with
the host's list of every pair at or above the floor (cluster_edges_truth.py: nothing of the library) and with what the
other entries say of the same graph -- blurrily_storage_cluster's edge count and labels, blurrily_storage_cluster_tree's
merges (Kruskal on the host over the GPU's records), blurrily_storage_cluster_centres' degrees -- and, blocked, with
blurrily_storage_cluster_within and blurrily_storage_cluster_tree_within, under "scope_strategy" 0, 1 and 2.  Over the
oracle haystacks at four floors, the capacity protocol and option "cluster_edges_max", cliques of identical strings
around the wave, the direct kernel's tile and the sort's tile, test_gpu_cluster_levels.py's built case, blocks of every
size, the direct cap, a haystack of more than one window, dense_case.py's map where slices are left out, mutations,
repeated calls, and beside the other entries, which it leaves as they were."""
import ctypes
import errno

import numpy as np
import pytest

import workloads as W
from blurrily_amd import RawMap, _native
from blurrily_amd.map import _pack
import cluster_edges_truth as CE
from cluster_tree_within_truth import BlockedTruth, blocked
from cluster_truth import Truth
from helpers import oracle_case_inputs
from test_gpu_cluster_levels import A, B, C, SHORT, _j, _map_of, built_case

pytestmark = pytest.mark.gpu
FLOORS = (200, 300, 500, 700)
STRATEGIES = (0, 1, 2)                                        # "scope_strategy": auto, the sweep, the direct kernel
G = 16                                                        # the direct kernel's tile (cluster.h: kClusterWithinTile)
TILE = 4096                                                   # the sort's tile (cluster.h: kClusterEdgesTile)
SWEEP, DIRECT = "cluster_edges_sweep_kernel", "cluster_edges_within_kernel"
TILES, MERGE, ROWS = "cluster_edges_tiles_kernel", "cluster_edges_merge_kernel", "cluster_edges_rows_kernel"
EMPTY = np.zeros((0, 3), dtype=np.uint32)


def forest_of(rows):
    """Kruskal over records that come in the total order: the accepted ones, in order (cluster_tree_truth.kruskal's
    growing runs: the edges whose ends were together when a run began are dropped without a loop)."""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, 3)
    nodes = np.unique(rows[:, :2])
    lo, hi = np.searchsorted(nodes, rows[:, 0]), np.searchsorted(nodes, rows[:, 1])
    parent = list(range(len(nodes)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    out, at, step = [], 0, 4096
    while at < len(rows):
        root = np.array([find(x) for x in range(len(parent))], dtype=np.int64)
        apart = np.nonzero(root[lo[at:at + step]] != root[hi[at:at + step]])[0] + at
        for i in apart.tolist():
            rl, rh = find(int(lo[i])), find(int(hi[i]))
            if rl != rh:
                parent[max(rl, rh)] = min(rl, rh)
                out.append(i)
        at, step = at + step, step * 2
    return rows[np.array(out, dtype=np.int64)] if out else EMPTY


def ours(m):
    """The clustering kernels the last call launched (a table built at an image's first call is not the call's)."""
    return [k for k in m.last_kernels() if k.startswith("cluster_")]


def united(rows, listed, labels):
    """The labels after uniting every record's ends, by RawMap.cut_tree at no floor (labels tell what is held)."""
    return RawMap.cut_tree(listed, labels, rows, 0)


def check_plain(m, listed, floor, want):
    """One unblocked call against the truth's records and the other entries on the same list and floor."""
    listed = np.asarray(listed, dtype=np.uint32)
    edges = m.cluster_edges(listed, floor)
    names = ours(m)
    labels, n_clusters, n_edges = m.cluster(listed, floor)
    print(f"floor {floor}: {len(edges)} records (truth {len(want)}, cluster's n_edges {n_edges})")
    assert edges.dtype == np.uint32 and edges.shape == want.shape and edges.tobytes() == want.tobytes(), floor
    assert len(edges) == n_edges == m.cluster_edge_count(listed, floor), floor
    assert names[0] == "cluster_nodes_kernel" and SWEEP in names and DIRECT not in names
    assert (TILES in names) == (ROWS in names and len(edges) >= 2) and (MERGE in names) == (len(edges) > TILE), names
    assert united(edges, listed, labels).tobytes() == labels.tobytes(), floor
    tree = m.cluster_tree(listed, floor)
    assert forest_of(edges).tobytes() == tree[1].tobytes() and tree[3] == n_edges, floor
    degrees = m.cluster_centres(listed, floor, attached=False)[1]
    nodes = np.unique(listed)
    count = np.bincount(np.searchsorted(nodes, edges[:, :2].reshape(-1)), minlength=len(nodes))
    assert np.array_equal(count[np.searchsorted(nodes, listed)], degrees), floor
    return edges


def check_blocked(m, listed, blocks, floor, want, strategies=STRATEGIES):
    """One blocked call under every strategy against the blocked truth's records, cluster_within's counts and labels
    and cluster_tree_within's merges."""
    listed, blocks = np.asarray(listed, dtype=np.uint32), np.asarray(blocks, dtype=np.uint32)
    m.set_option("scope_strategy", 0)
    labels, n_clusters, n_edges = m.cluster_within(listed, blocks, floor)
    tree = m.cluster_tree_within(listed, blocks, floor)
    edges = None
    for s in strategies:
        m.set_option("scope_strategy", s)
        edges = m.cluster_edges(listed, floor, blocks=blocks)
        names = m.last_kernels()
        print(f"floor {floor} strategy {s}: {len(edges)} records (truth {len(want)}, cluster_within's n_edges {n_edges})")
        assert edges.dtype == np.uint32 and edges.shape == want.shape and edges.tobytes() == want.tobytes(), (floor, s)
        assert len(edges) == n_edges == m.cluster_edge_count(listed, floor, blocks), (floor, s)
        assert "cluster_sweep_kernel" not in names and "cluster_within_kernel" not in names
        if s:
            assert (DIRECT if s == 1 else SWEEP) not in names, (s, names)
    m.set_option("scope_strategy", 0)
    assert united(edges, listed, labels).tobytes() == labels.tobytes(), floor
    assert forest_of(edges).tobytes() == tree[1].tobytes(), floor
    key_of = dict(zip(listed.tolist(), blocks.tolist()))
    assert all(key_of[a] == key_of[b] for a, b in edges[:, :2].tolist()[:100000])
    return edges


_ORACLE = {}


def oracle_case(kind, n):
    """The map, the truth and the blocked truth (keys: reference % 3) of one oracle haystack, made once."""
    if (kind, n) not in _ORACLE:
        hay, off, needles = oracle_case_inputs(kind, n)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        listed = np.arange(1, n + 1, dtype=np.uint32)
        _ORACLE[kind, n] = dict(m=_map_of(held), held=held, truth=Truth(held), needles=needles, listed=listed,
                                blocks=(listed % 3).astype(np.uint32), blocked=blocked(held, listed, listed % 3))
    return _ORACLE[kind, n]


@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("kind,n", [("words", 5000), ("geonames", 8000), ("skewed", 6000)])
def test_the_records_equal_the_truth_and_agree_with_cluster_the_tree_and_the_degrees(kind, n, floor):
    c = oracle_case(kind, n)
    want = CE.records(c["truth"], c["listed"], floor, FLOORS[0])
    check_plain(c["m"], c["listed"], floor, want)
    if (kind, floor) in (("geonames", 200), ("skewed", 200)):
        assert len(want) > 4 * TILE                           # (several merge passes)


@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("kind,n", [("words", 5000), ("geonames", 8000), ("skewed", 6000)])
def test_the_blocked_records_equal_the_blocked_truth_cluster_within_and_the_blocked_tree(kind, n, floor):
    c = oracle_case(kind, n)
    want = CE.records(c["blocked"], c["listed"], floor, FLOORS[0])
    edges = check_blocked(c["m"], c["listed"], c["blocks"], floor, want)
    plain = CE.records(c["truth"], c["listed"], floor, FLOORS[0])
    if len(plain):
        assert len(edges) < len(plain)                        # (the keys cut edges)


def _raw(m, listed, floor, edges, capacity, blocks=None):
    """The C entry as it is: (result, errno, n_edges)."""
    lib = _native.lib()
    listed = np.ascontiguousarray(listed, dtype=np.uint32)
    n_edges = ctypes.c_uint64(0xABCDEF)
    ptr = edges.ctypes.data if edges is not None else None
    ctypes.set_errno(0)
    if blocks is None:
        r = lib.blurrily_storage_cluster_edges(m.handle, listed.ctypes.data if len(listed) else None, len(listed), floor,
                                               ptr, capacity, ctypes.byref(n_edges))
    else:
        blocks = np.ascontiguousarray(blocks, dtype=np.uint32)
        r = lib.blurrily_storage_cluster_edges_within(m.handle, listed.ctypes.data if len(listed) else None,
                                                      blocks.ctypes.data if len(listed) else None, len(listed), floor,
                                                      ptr, capacity, ctypes.byref(n_edges))
    return r, ctypes.get_errno(), n_edges.value


def test_the_capacity_protocol():
    c = oracle_case("words", 5000)
    m, listed = c["m"], c["listed"]
    want = CE.records(c["truth"], listed, 500, FLOORS[0])
    count = len(want)
    assert count >= 2
    for blocks, expect in ((None, want), (np.zeros(len(listed), dtype=np.uint32), want)):
        # count only: the count, and no sort or rows kernel
        assert _raw(m, listed, 500, None, 12345, blocks) == (0, 0, count)
        names = m.last_kernels()
        assert not {TILES, MERGE, ROWS} & set(names) and (SWEEP in names or DIRECT in names), names
        # exactly enough room fills; one record less is ERANGE with the count and the buffer untouched
        buf = np.full((count + 1, 3), 0xEE, dtype=np.uint32)
        assert _raw(m, listed, 500, buf, count, blocks) == (0, 0, count)
        assert buf[:count].tobytes() == expect.tobytes() and (buf[count] == 0xEE).all()
        assert ROWS in m.last_kernels() and TILES in m.last_kernels()
        buf[:] = 0xEE
        assert _raw(m, listed, 500, buf, count - 1, blocks) == (-1, errno.ERANGE, count)
        assert (buf == 0xEE).all() and not {TILES, MERGE, ROWS} & set(m.last_kernels())
        assert _raw(m, listed, 500, buf, 0, blocks) == (-1, errno.ERANGE, count) and (buf == 0xEE).all()
    # a list with no edges at capacity 0; nothing listed
    buf = np.full((2, 3), 0xEE, dtype=np.uint32)
    assert _raw(m, listed[:50], 1000, buf, 0) == (0, 0, 0) and (buf == 0xEE).all()
    assert _raw(m, listed[:50], 1000, buf, 0, listed[:50] % 2) == (0, 0, 0)
    assert _raw(m, [], 500, buf, 2) == (0, 0, 0) and _raw(m, [], 500, None, 0) == (0, 0, 0)
    assert _raw(m, [], 500, buf, 2, []) == (0, 0, 0) and (buf == 0xEE).all()
    assert m.cluster_edges([], 500).shape == (0, 3) and m.cluster_edge_count([], 500, blocks=[]) == 0
    # the Python method grows once from too small a room
    assert m.cluster_edges(listed, 500, capacity=1).tobytes() == want.tobytes()


def test_the_option_bounds_the_emission():
    same = b"four of a kind"
    m = _map_of({r: same for r in (1, 2, 3, 4)})
    listed = np.array([1, 2, 3, 4], dtype=np.uint32)
    want = [[1, 2, 1000], [1, 3, 1000], [1, 4, 1000], [2, 3, 1000], [2, 4, 1000], [3, 4, 1000]]
    was = m.get_option("cluster_edges_max")
    try:
        for blocks in (None, [7, 7, 7, 7]):
            for s in STRATEGIES:
                m.set_option("scope_strategy", s)
                buf = np.full((8, 3), 0xEE, dtype=np.uint32)
                m.set_option("cluster_edges_max", 5)
                assert _raw(m, listed, 1000, buf, 8, blocks) == (-1, errno.EOVERFLOW, 6) and (buf == 0xEE).all()
                assert _raw(m, listed, 1000, None, 0, blocks) == (0, 0, 6)                  # (counting is not bounded)
                assert _raw(m, listed, 1000, buf, 5, blocks) == (-1, errno.ERANGE, 6) and (buf == 0xEE).all()
                with pytest.raises(OSError) as err:
                    m.cluster_edges(listed, 1000, blocks=blocks)
                assert err.value.errno == errno.EOVERFLOW
                m.set_option("cluster_edges_max", 6)
                assert _raw(m, listed, 1000, buf, 8, blocks) == (0, 0, 6) and buf[:6].tolist() == want
                # a capacity far above the option with a count below it
                buf[:] = 0xEE
                assert _raw(m, listed, 1000, buf, 1 << 40, blocks) == (0, 0, 6) and buf[:6].tolist() == want
                assert (buf[6:] == 0xEE).all()
    finally:
        m.set_option("cluster_edges_max", was)
        m.set_option("scope_strategy", 0)
    assert m.get_option("cluster_edges_max") == 1 << 28
    m.close()


def _clique_records(k, first=1):
    a, b = np.triu_indices(k, 1)
    return np.stack([a + first, b + first, np.full(len(a), 1000)], axis=1).astype(np.uint32)


@pytest.mark.parametrize("k", [2, 3, 16, 17, 64, 65, 91, 92, 129, 200])
def test_a_clique_of_identical_strings_plain_and_as_one_block(k):
    # every lane of a harvest wave and all 16 needles of a direct tile find edges at once; all at 1000, ordered by ends
    m = _map_of({r: b"identical strings" for r in range(1, k + 1)})
    listed = np.arange(1, k + 1, dtype=np.uint32)
    want = _clique_records(k)
    assert len(want) == k * (k - 1) // 2
    got = m.cluster_edges(listed, 1000)
    assert got.tobytes() == want.tobytes()
    assert (MERGE in m.last_kernels()) == (len(want) > TILE) and (TILES in m.last_kernels()) == (len(want) >= 2)
    assert m.cluster_edges(listed, 0).tobytes() == want.tobytes()
    for s, ran in ((1, SWEEP), (2, DIRECT)):
        m.set_option("scope_strategy", s)
        got = m.cluster_edges(listed, 1000, blocks=np.full(k, 5, dtype=np.uint32))
        assert got.tobytes() == want.tobytes(), s
        assert ran in m.last_kernels() and m.cluster_edge_count(listed, 1000, np.full(k, 5)) == len(want)
    m.close()


@pytest.mark.parametrize("pairs,total", [(1, TILE), (2, TILE + 1), (TILE + 2, 2 * TILE + 1)])
def test_the_sort_at_its_tile_one_above_it_and_one_above_twice_it(pairs, total):
    # the clique of 91 (4 095 edges) and disjoint identical pairs on top
    held = {r: b"identical strings" for r in range(1, 92)}
    want = [_clique_records(91)]
    for i in range(pairs):
        s = b"pair " + bytes("abcdefghijklmnopqrstuvwxyz"[(i // 676) % 26] + "abcdefghijklmnopqrstuvwxyz"[(i // 26) % 26] +
                             "abcdefghijklmnopqrstuvwxyz"[i % 26], "ascii") + b" twin"
        held[1000 + 2 * i] = held[1001 + 2 * i] = s
        want.append(np.array([[1000 + 2 * i, 1001 + 2 * i, 1000]], dtype=np.uint32))
    want = np.concatenate(want)
    assert len(want) == total and TILE == 91 * 90 // 2 + 1
    m = _map_of(held)
    listed = np.array(sorted(held), dtype=np.uint32)
    got = m.cluster_edges(listed, 1000)
    assert got.tobytes() == want.tobytes()
    assert (MERGE in m.last_kernels()) == (total > TILE)
    for s in (1, 2):
        m.set_option("scope_strategy", s)
        assert m.cluster_edges(listed, 1000, blocks=np.zeros(len(listed), dtype=np.uint32)).tobytes() == want.tobytes(), s
    m.close()


def test_built_cases_the_chain_an_unlisted_bridge_the_exact_floor_and_the_counter_widths():
    held = built_case()
    held.update({5004: SHORT, 5005: A[:-1]})                  # 7 / 15 against each other: 466 permille
    assert _j(A, B) == (8, 16) and _j(B, C) == (6, 17) and _j(A, C)[0] == 0 and _j(A[:-1], SHORT) == (7, 15)
    m = _map_of(held)
    chain = [5001, 5002, 5003]
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        for blocks in (None, [4, 4, 4]):
            # the chain: two edges at their whole per mille; with B, the bridge, held but not listed: none
            assert m.cluster_edges(chain, 300, blocks=blocks).tolist() == [[5001, 5002, 500], [5002, 5003, 352]]
            assert m.cluster_edges(chain, 353, blocks=blocks).tolist() == [[5001, 5002, 500]]
            assert m.cluster_edges([5001, 5003], 0, blocks=blocks and blocks[:2]).shape == (0, 3)
            # exactly at the floor and one per mille above
            for pair, at in (([5001, 5002], 500), ([5004, 5005], 466)):
                assert m.cluster_edges(pair, at, blocks=blocks and blocks[:2]).tolist() == [pair + [at]]
                assert m.cluster_edges(pair, at + 1, blocks=blocks and blocks[:2]).shape == (0, 3)
        assert m.cluster_edges(chain, 300, blocks=[1, 2, 1]).shape == (0, 3)   # (the bridge under another key)
    m.set_option("scope_strategy", 0)
    # everything listed: the nodes of T = 1, 15, 16, 255, 256 and 700 with their variants among them
    everything = np.array(sorted(held), dtype=np.uint32)
    truth = Truth(held)
    blocks = np.where(everything > 5000, 7, everything % 3).astype(np.uint32)
    b_truth = blocked(held, everything, blocks)
    for floor in (0, 352, 353, 500, 1000):
        edges = check_plain(m, everything, floor, CE.records(truth, everything, floor))
        rows = set(map(tuple, edges.tolist()))
        assert {(6000, 6001, 1000), (7001, 7002, 1000), (6016, 6017, 1000)} <= rows
        assert ((5002, 5003, 352) in rows) == (floor <= 352) and ((5001, 5002, 500) in rows) == (floor <= 500)
        check_blocked(m, everything, blocks, floor, CE.records(b_truth, everything, floor))
    # without the bridge its edges are not reported, and nothing joins its neighbours
    without = everything[everything != 5002]
    edges = check_plain(m, without, 300, CE.records(truth, without, 300))
    assert 5002 not in edges[:, :2]
    # the list shuffled, with repeats and absent references: the same bytes
    rng = np.random.default_rng(5)
    absent = np.array([4000, 4001, 9999, 0xFFFFFFFF, 0], dtype=np.uint32)
    mixed = np.concatenate([everything, everything[::7], absent, absent[:2]])
    rng.shuffle(mixed)
    for floor in (200, 500):
        base = m.cluster_edges(everything, floor)
        assert len(base) and m.cluster_edges(mixed, floor).tobytes() == base.tobytes()
        key = lambda refs: np.where(refs > 5000, 7, refs % 3).astype(np.uint32)
        for s in STRATEGIES:
            m.set_option("scope_strategy", s)
            assert m.cluster_edges(mixed, floor, blocks=key(mixed)).tobytes() == \
                m.cluster_edges(everything, floor, blocks=key(everything)).tobytes(), (floor, s)
        m.set_option("scope_strategy", 0)
    row_off, neighbour, permille = RawMap.adjacency(base, mixed)
    want = CE.adjacency(base, mixed)
    assert row_off.tolist() == want[0].tolist() and neighbour.tolist() == want[1].tolist()
    assert permille.tolist() == want[2].tolist()
    # nothing listed; nothing held
    assert m.cluster_edges([], 500).shape == (0, 3) and m.cluster_edges(absent, 0).shape == (0, 3)
    assert m.cluster_edges(absent, 0, blocks=[1, 1, 1, 2, 2]).shape == (0, 3) and m.cluster_edge_count(absent, 0) == 0
    m.close()


def _sized_blocks(refs, sizes, rng):
    """Keys for a shuffled prefix of refs: blocks of the given sizes, their members anywhere among the references, the
    key values in no order (as tests/test_gpu_cluster_within.py's)."""
    picked = rng.permutation(refs)[:sum(sizes)]
    keys = rng.permutation(np.arange(1000, 1000 + len(sizes), dtype=np.uint32))
    return picked.astype(np.uint32), np.repeat(keys, sizes).astype(np.uint32)


def test_blocks_of_every_size_around_the_tile_and_the_workgroup_equal_keys_and_distinct_keys():
    c = oracle_case("words", 5000)
    m, everything = c["m"], c["listed"]
    sizes = [1, 2, G - 1, G, G + 1, 2 * G + 1, 255, 256, 257, 600]
    listed, blocks = _sized_blocks(everything, sizes, np.random.default_rng(29))
    want = CE.records(blocked(c["held"], listed, blocks), listed, 100)
    assert len(want) > 0
    edges = check_blocked(m, listed, blocks, 100, want)
    # ... and equal to one cluster_edges call per block, merged under the order
    own = [m.cluster_edges(listed[blocks == k], 100) for k in np.unique(blocks)]
    assert CE.merged(own).tobytes() == edges.tobytes()
    by_block = RawMap.tree_by_block(edges, listed, blocks)
    for k, rows in zip(np.unique(blocks).tolist(), own):
        assert by_block.get(k, EMPTY).tobytes() == rows.tobytes(), k
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        # all keys equal: byte for byte the unblocked call
        for p in (200, 300):
            plain = m.cluster_edges(everything, p)
            got = m.cluster_edges(everything, p, blocks=np.full(len(everything), 0xFFFFFFFF, dtype=np.uint32))
            assert got.tobytes() == plain.tobytes() and len(plain) > 0, (s, p)
        # all keys distinct: no edges
        some = np.concatenate([everything[:700], [888888]]).astype(np.uint32)
        assert m.cluster_edges(some, 0, blocks=some[::-1].copy()).shape == (0, 3)
        assert m.cluster_edge_count(some, 0, blocks=some) == 0
    m.set_option("scope_strategy", 0)


def test_auto_sweeps_a_block_above_the_direct_cap_and_scores_the_others_through_the_same_cursor():
    cap = 100000                                              # cluster_plan.h: kClusterWithinDirectMax
    n = 2 * cap + 301
    hay, off = W.geonames(n, 2000, 41)
    m = _map_of({i + 1: s for i, s in enumerate(W.unpack(hay, off))})
    listed = np.arange(1, n + 1, dtype=np.uint32)
    # interleaving blocks of cap + 1 (swept), cap (the largest scored directly) and 300 members
    blocks = np.where(listed > 2 * cap + 1, 9, listed % 2).astype(np.uint32)
    assert [(blocks == k).sum() for k in (1, 0, 9)] == [cap + 1, cap, 300]
    results = {}
    for s, kernels in ((0, {DIRECT, SWEEP}), (1, {SWEEP}), (2, {DIRECT})):
        m.set_option("scope_strategy", s)
        results[s] = m.cluster_edges(listed, 700, blocks=blocks)
        assert {k for k in m.last_kernels() if k in (DIRECT, SWEEP)} == kernels, s
    m.set_option("scope_strategy", 0)
    edges = results[0]
    assert results[1].tobytes() == edges.tobytes() and results[2].tobytes() == edges.tobytes()
    labels, n_clusters, n_edges = m.cluster_within(listed, blocks, 700)
    assert len(edges) == n_edges > 0 and united(edges, listed, labels).tobytes() == labels.tobytes()
    key = (1000 - edges[:, 2].astype(np.int64)) << 54 | edges[:, 0].astype(np.int64) << 27 | edges[:, 1]
    assert (np.diff(key) > 0).all() and (edges[:, 0] < edges[:, 1]).all() and (edges[:, 2] >= 700).all()
    assert (blocks[edges[:, 0] - 1] == blocks[edges[:, 1] - 1]).all()
    # one member fewer in the swept block: every block is scored directly
    m.cluster_edge_count(listed[2:], 700, blocks[2:])
    assert SWEEP not in m.last_kernels() and DIRECT in m.last_kernels()
    m.close()


def test_a_haystack_of_more_than_one_window_all_every_third_and_blocked():
    n = 70000
    hay, off = W.words(n, seed=17)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    weights = np.random.default_rng(23).integers(1, 1 << 20, size=n).astype(np.uint32)   # ranks unrelated to length
    m = _map_of(held, weights)
    truth = Truth(held)
    everything = np.arange(1, n + 1, dtype=np.uint32)
    p = 700
    for listed in (everything, everything[::3]):
        want = CE.records(truth, listed, p)
        edges = m.cluster_edges(listed, p)
        labels, n_clusters, n_edges = m.cluster(listed, p)
        print(f"{len(listed)} listed: {len(edges)} records (truth {len(want)}, cluster's n_edges {n_edges})")
        assert edges.tobytes() == want.tobytes() and len(edges) == n_edges > 0
        assert united(edges, listed, labels).tobytes() == labels.tobytes()
    assert m.device_info()["n_windows"] >= 2
    blocks = everything % 7
    b_truth = BlockedTruth.__new__(BlockedTruth)              # (the same strings, tokenised once)
    b_truth.__dict__ = dict(truth.__dict__, _pairs={}, key=(truth.refs % 7).astype(np.int64))
    check_blocked(m, everything, blocks, p, CE.records(b_truth, everything, p), strategies=(1, 2))
    m.close()


@pytest.fixture(scope="module")
def dense():
    """dense_case.py's map, the two lists of tests/test_gpu_dense_floor_sweeps.py and the family keys."""
    import dense_case as D
    m, h = D.build()
    family = np.array([r for head in h.heads for r in h.family(head)], dtype=np.uint32)
    words = h.refs[:D.N_WORDS]
    lists = {"short": np.concatenate([words[::97], family]), "long": np.concatenate([words[::9], family])}
    # blocked by family: family k's six members under key k + 1, every word under key 0
    key_of = {int(r): 0 for r in words.tolist()}
    key_of.update({r: k + 1 for k, head in enumerate(h.heads) for r in h.family(head)})
    yield m, h, lists, key_of
    m.close()


@pytest.mark.parametrize("name", ["short", "long"])
def test_the_dense_slice_map_where_slices_are_left_out_plain_and_blocked_by_family(dense, name):
    m, h, lists, key_of = dense
    listed = lists[name]
    blocks = np.array([key_of[int(r)] for r in listed], dtype=np.uint32)
    b_truth = BlockedTruth.__new__(BlockedTruth)
    b_truth.__dict__ = dict(h.truth.__dict__, _pairs={},
                            key=np.array([key_of[int(r)] for r in h.truth.refs], dtype=np.int64))
    found = 0
    for p in (200, 350, 600):                                 # (tests/test_gpu_dense_floor_sweeps.py's fixed floors)
        want = CE.records(h.truth, listed, p, 200)
        edges = m.cluster_edges(listed, p)
        labels, n_clusters, n_edges = m.cluster(listed, p)
        print(f"{name}, floor {p}: {len(edges)} records (truth {len(want)}, cluster's n_edges {n_edges})")
        assert edges.tobytes() == want.tobytes() and len(edges) == n_edges, p
        assert united(edges, listed, labels).tobytes() == labels.tobytes(), p
        check_blocked(m, listed, blocks, p, CE.records(b_truth, listed, p, 200))
        found += len(want)
    assert found > 0


def test_mutations_a_deleted_end_pending_puts_a_reference_put_again_and_the_fold():
    hay, off = W.words(5000, seed=7)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    held.update({9001: A, 9002: B, 9003: C})
    m = _map_of(held)
    m.sync_device()
    builds = m.device_info()["base_builds"]

    def verify():
        listed = np.array(sorted(held) + [123456], dtype=np.uint32)
        truth = Truth(held)
        edges = check_plain(m, listed, 200, CE.records(truth, listed, 200))
        blocks = (listed % 2).astype(np.uint32)
        check_blocked(m, listed, blocks, 200, CE.records(blocked(held, listed, blocks), listed, 200))
        return set(map(tuple, edges.tolist())), listed

    rows, _ = verify()
    assert (9001, 9002, 500) in rows and (9002, 9003, 352) in rows
    m.delete(9002)                                            # a deleted end takes its edges with it
    del held[9002]
    rows, _ = verify()
    assert not any(9002 in r[:2] for r in rows)
    m.put(B, 9500, 0)                                         # a pending put with edges into the base image
    m.put(B + b"x", 9501, 0)                                  # ... and one inside the delta image
    held.update({9500: B, 9501: B + b"x"})
    rows, listed = verify()
    assert (9001, 9500, 500) in rows and (9003, 9500, 352) in rows and any(r[:2] == (9500, 9501) for r in rows)
    assert m.device_info()["n_pending"] >= 2 and m.device_info()["base_builds"] == builds
    m.cluster_edges(listed, 200)
    assert m.last_kernels().count(SWEEP) == 2                 # (two images: the base and the pending puts)
    m.set_option("scope_strategy", 1)
    m.cluster_edge_count(listed, 200, listed % 2)
    assert m.last_kernels().count(SWEEP) == 2 and DIRECT not in m.last_kernels()
    m.set_option("scope_strategy", 0)
    m.delete(16)                                              # deleted and put again with another text: its new R and heights
    m.put(C + b"x", 16, 0)
    held[16] = C + b"x"
    rows, listed = verify()
    assert any(r[:2] == (16, 9003) for r in rows)
    pending = m.cluster_edges(listed, 200)
    big, bo = W.words(9000, seed=34)                          # a log past its budget folds into a rebuilt base image
    bulk = np.arange(2 * 10**6, 2 * 10**6 + 9000, dtype=np.uint32)
    m.put_many_packed(big, bo, bulk, np.zeros(9000, dtype=np.uint32))
    held.update(zip(bulk.tolist(), W.unpack(big, bo)))
    folded = m.cluster_edges(listed, 200)                     # (the same list: the bulk is held but not listed)
    info = m.device_info()
    assert info["base_builds"] > builds and info["n_pending"] == 0 and info["n_tombstones"] == 0
    assert folded.tobytes() == pending.tobytes()
    assert m.last_kernels().count(SWEEP) == 1
    m.close()


def test_three_calls_give_identical_bytes():
    c = oracle_case("words", 5000)
    m, listed, blocks = c["m"], c["listed"], c["blocks"]
    for s in STRATEGIES:
        m.set_option("scope_strategy", s)
        for p in (100, 200):
            one, two, three = (m.cluster_edges(listed, p) for _ in range(3))
            assert one.tobytes() == two.tobytes() == three.tobytes() and len(one) > 0
            one, two, three = (m.cluster_edges(listed, p, blocks=blocks) for _ in range(3))
            assert one.tobytes() == two.tobytes() == three.tobytes() and len(one) > 0
    m.set_option("scope_strategy", 0)


def test_the_calls_around_an_edges_call_are_unchanged_and_the_kernels_are_named():
    c = oracle_case("words", 5000)
    m, listed, blocks = c["m"], c["listed"], c["blocks"]
    packed, offsets = _pack(c["needles"])
    before_rows, before_counts = m.find_batch_packed(packed, offsets, 10)
    before_kernels = m.last_kernels()
    around = [(lambda: m.cluster(listed, 200)), (lambda: m.cluster_within(listed, blocks, 200)),
              (lambda: m.cluster_tree(listed, 200))]
    before = []
    for call in around:
        result = call()
        before.append((result, m.last_kernels()))
    edges = m.cluster_edges(listed, 200)
    assert ours(m) == ["cluster_nodes_kernel", SWEEP, TILES, ROWS] and 2 <= len(edges) <= TILE
    m.cluster_edges(listed, 100)
    assert ours(m) == ["cluster_nodes_kernel", SWEEP, TILES, MERGE, ROWS]
    for s, ran, idle in ((2, DIRECT, SWEEP), (1, SWEEP, DIRECT), (0, DIRECT, SWEEP)):
        m.set_option("scope_strategy", s)
        m.cluster_edges(listed, 200, blocks=blocks)
        names = ours(m)
        assert names == ["cluster_nodes_kernel", ran, TILES, ROWS], (s, names)
        for name in (idle, "cluster_sweep_kernel", "cluster_within_kernel", "cluster_within_sweep_kernel",
                     "cluster_tree_sweep_kernel", "cluster_label_kernel", "find_kernel"):
            assert name not in names, (s, name)
    m.set_option("scope_strategy", 0)
    after_rows, after_counts = m.find_batch_packed(packed, offsets, 10)
    assert m.last_kernels() == before_kernels
    assert np.array_equal(before_rows, after_rows) and np.array_equal(before_counts, after_counts)
    for call, (was, was_kernels) in zip(around, before):
        now = call()
        assert m.last_kernels() == was_kernels
        for x, y in zip(was, now):
            assert x.tobytes() == y.tobytes() if isinstance(x, np.ndarray) else x == y
