"""Cluster edges without a GPU: blurrily_storage_cluster_edges and blurrily_storage_cluster_edges_within are exported
with their seven and eight argtypes set, their prototypes agree with the reference's storage.h in one translation unit
and alone, four drifted prototypes do not compile, every argument error -- n_edges NULL, a reference listed under two
block keys and n = 2^27 + 1 among them -- is EINVAL before a GPU is asked for and leaves the buffer and the count as they
were, valid calls fail loudly (ENODEV) where no GPU is usable, option "cluster_edges_max" has its default and range, the
Python surface checks its arguments, hands the right pointers, grows once on ERANGE, picks the symbol by ``blocks`` and
hands no buffer to count; ``adjacency`` is right on canned records, and ``tree_by_block``, ``cut_tree`` and
``merge_profile`` take edge records as they are.  The truth of tests/cluster_edges_truth.py is checked against itself on
the inputs the GPU tests use, with the edge counts those tests stand on."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, RawMap, _native
import cluster_edges_truth as CE
import cluster_tree_truth as TT
from cluster_truth import Truth
from helpers import ORACLE_CASES, compile_c, einval, oracle_case_inputs, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster_edges.c")
NO = _native.NO_CLUSTER
TILE = 4096                                                   # the sort's tile (cluster.h: kClusterEdgesTile)
CLIQUES = (2, 3, 16, 17, 64, 65, 91, 92, 129, 200)


def test_the_cluster_edges_symbols_are_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name, n_args in (("blurrily_storage_cluster_edges", 7), ("blurrily_storage_cluster_edges_within", 8)):
        assert f" T {name}\n" in out
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args
        assert name in _native.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "blurrily_storage.h")).read()
    assert ("int blurrily_storage_cluster_edges(trigram_map haystack, const uint32_t* references, size_t n,\n"
            "                                   uint32_t min_permille, blurrily_cluster_merge_t* edges,\n"
            "                                   uint64_t capacity, uint64_t* n_edges);") in header
    assert ("int blurrily_storage_cluster_edges_within(trigram_map haystack, const uint32_t* references,\n"
            "                                          const uint32_t* blocks, size_t n, uint32_t min_permille,\n"
            "                                          blurrily_cluster_merge_t* edges, uint64_t capacity,\n"
            "                                          uint64_t* n_edges);") in header


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_cluster_edges_prototypes_compile_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_edges_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("was,now", [
    ("(trigram_map, const uint32_t*, const uint32_t*, size_t,", "(trigram_map, const uint32_t*, size_t,"),
    ("(trigram_map, const uint32_t*, size_t, uint32_t,", "(trigram_map, const uint32_t*, uint32_t, uint32_t,"),
    ("blurrily_cluster_merge_t*, uint64_t,\n                 uint64_t*)", "uint32_t*, uint64_t,\n                 uint64_t*)"),
    ("blurrily_cluster_merge_t*, uint64_t,\n                  uint64_t*)",
     "blurrily_cluster_merge_t*, uint32_t,\n                  uint64_t*)")],
    ids=["no_blocks", "n_as_a_word", "edges_as_words", "capacity_as_a_word"])
def test_a_drifted_cluster_edges_prototype_does_not_compile(tmp_path, was, now):
    write_recorded_storage_h(tmp_path)
    text = open(SRC).read()
    assert text.count(was) == 1
    src = tmp_path / "drifted.c"
    src.write_text(text.replace(was, now))
    assert compile_c(tmp_path, src).returncode != 0
    r = compile_c(tmp_path, SRC)                              # (the drift alone is what does not compile)
    assert r.returncode == 0, r.stderr


# a shuffled list that names 11 and 14 twice: under one key each (fine), or 14 under two keys (EINVAL)
SHUFFLED = [14, 10, 17, 11, 15, 14, 99, 11]
KEYS_SAME = [2, 1, 3, 1, 2, 2, 5, 1]
KEYS_TWO = [2, 1, 3, 1, 2, 7, 5, 1]


def test_argument_errors_are_einval_before_any_gpu_and_write_nothing():
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs, keys = np.array([1, 2, 3], dtype=np.uint32), np.array([5, 5, 6], dtype=np.uint32)
    edges = np.full((8, 3), 7, dtype=np.uint32)
    n_edges = ctypes.c_uint64(7)
    plain, within = lib.blurrily_storage_cluster_edges, lib.blurrily_storage_cluster_edges_within
    r, k, e, count = refs.ctypes.data, keys.ctypes.data, edges.ctypes.data, ctypes.byref(n_edges)
    einval(lambda: plain(None, r, 3, 500, e, 8, count))                             # no map
    einval(lambda: plain(m.handle, r, 3, 1001, e, 8, count))                        # min_permille > 1000
    einval(lambda: plain(m.handle, None, 0, 1001, None, 0, count))                  # ... with nothing listed too
    einval(lambda: plain(m.handle, None, 3, 500, e, 8, count))                      # references NULL, n > 0
    einval(lambda: plain(m.handle, r, 3, 500, e, 8, None))                          # n_edges is required
    einval(lambda: plain(m.handle, r, 3, 500, None, 0, None))                       # ... to count only, too
    einval(lambda: plain(m.handle, None, 0, 500, None, 0, None))                    # ... and with nothing listed
    einval(lambda: plain(m.handle, r, (1 << 27) + 1, 500, e, 8, count))             # more than the key's 27 bits number
    einval(lambda: plain(m.handle, r, 0xFFFFFFF1, 500, e, 8, count))
    einval(lambda: plain(m.handle, r, 2**64 - 1, 500, None, 0, count))
    einval(lambda: within(None, r, k, 3, 500, e, 8, count))
    einval(lambda: within(m.handle, r, k, 3, 1001, e, 8, count))
    einval(lambda: within(m.handle, None, k, 3, 500, e, 8, count))
    einval(lambda: within(m.handle, r, None, 3, 500, e, 8, count))                  # blocks NULL, n > 0
    einval(lambda: within(m.handle, r, k, 3, 500, e, 8, None))
    einval(lambda: within(m.handle, None, None, 0, 500, None, 0, None))
    einval(lambda: within(m.handle, r, k, (1 << 27) + 1, 500, e, 8, count))
    # a reference listed twice under different keys: in a shuffled list, and side by side
    sh, two = np.array(SHUFFLED, dtype=np.uint32), np.array(KEYS_TWO, dtype=np.uint32)
    einval(lambda: within(m.handle, sh.ctypes.data, two.ctypes.data, len(sh), 500, e, 8, count))
    pair, pk = np.array([4, 4], dtype=np.uint32), np.array([0, 1], dtype=np.uint32)
    einval(lambda: within(m.handle, pair.ctypes.data, pk.ctypes.data, 2, 0, None, 0, count))
    assert n_edges.value == 7 and (edges == 7).all()                                # nothing written
    for one in (lambda: m.cluster_edges(SHUFFLED, 500, blocks=KEYS_TWO), lambda: m.cluster_edge_count(SHUFFLED, 500, KEYS_TWO)):
        with pytest.raises(OSError) as err:
            one()
        assert err.value.errno == errno.EINVAL
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster_edges.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs, keys = np.array([1, 2, 3], dtype=np.uint32), np.array([5, 5, 6], dtype=np.uint32)
    edges = np.zeros((8, 3), dtype=np.uint32)
    n_edges = ctypes.c_uint64(0)
    plain, within = lib.blurrily_storage_cluster_edges, lib.blurrily_storage_cluster_edges_within
    r, k, e, count = refs.ctypes.data, keys.ctypes.data, edges.ctypes.data, ctypes.byref(n_edges)
    sh, same = np.array(SHUFFLED, dtype=np.uint32), np.array(KEYS_SAME, dtype=np.uint32)
    for one in (lambda: plain(m.handle, r, 3, 500, e, 8, count),
                lambda: plain(m.handle, r, 3, 0, None, 0, count),                   # count only
                lambda: plain(m.handle, r, 3, 1000, e, 0, count),
                lambda: plain(m.handle, None, 0, 500, None, 0, count),              # nothing listed
                lambda: plain(m.handle, sh.ctypes.data, len(sh), 500, e, 8, count),
                lambda: within(m.handle, r, k, 3, 500, e, 8, count),
                lambda: within(m.handle, r, k, 3, 500, None, 0, count),
                lambda: within(m.handle, None, None, 0, 500, None, 0, count),
                lambda: within(m.handle, sh.ctypes.data, same.ctypes.data, len(sh), 500, e, 8, count)):
        ctypes.set_errno(0)
        assert one() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for one in (lambda: m.cluster_edges([1, 2], 700), lambda: m.cluster_edges([], 0), lambda: m.cluster_edge_count([1, 2], 700),
                lambda: m.cluster_edges(SHUFFLED, 1000, blocks=KEYS_SAME), lambda: m.cluster_edge_count([], 0, blocks=[])):
        with pytest.raises(OSError) as err:
            one()
        assert err.value.errno == errno.ENODEV
    m.close()


def test_the_option_has_its_default_and_its_range():
    m = RawMap()
    assert m.get_option("cluster_edges_max") == 1 << 28
    for v in (1 << 31, 1):
        m.set_option("cluster_edges_max", v)
        assert m.get_option("cluster_edges_max") == v
    for v in (0, (1 << 31) + 1, -1):
        with pytest.raises(OSError) as err:
            m.set_option("cluster_edges_max", v)
        assert err.value.errno == errno.EINVAL and m.get_option("cluster_edges_max") == 1
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    for call in (m.cluster_edges, m.cluster_edge_count):
        with pytest.raises(ValueError):
            call([1], 1001)
        with pytest.raises(OverflowError):
            call([1], -1)
        with pytest.raises(OverflowError):
            call([-1], 500)
        with pytest.raises(OverflowError):
            call([1 << 32], 500, blocks=[0])
        with pytest.raises(OverflowError):
            call([1], 500, blocks=[1 << 32])
        with pytest.raises(OverflowError):
            call([1], 500, blocks=[-3])
        with pytest.raises(ValueError):
            call([[1, 2]], 500)
        with pytest.raises(ValueError):
            call([1, 2], 500, blocks=[0])                         # a key per reference
    with pytest.raises(OverflowError):
        m.cluster_edges([1], 500, capacity=-1)
    with pytest.raises(OverflowError):
        m.cluster_edges([1], 500, capacity=1 << 64)
    m.close()
    with pytest.raises(RawMap.ClosedError):
        m.cluster_edges([1], 500)
    with pytest.raises(RawMap.ClosedError):
        m.cluster_edge_count([1], 500, blocks=[0])


class _StubLib:
    """Stands where the library stands in a RawMap: records what the two entries are handed and answers from canned
    records as the library would (the count always, ERANGE where the room is too small, the records where it is not)."""

    def __init__(self, records):
        self.records, self.calls = np.array(records, dtype=np.uint32).reshape(-1, 3), []

    def _answer(self, symbol, refs, keys, n, mp, edges, capacity, n_edges):
        u32 = ctypes.POINTER(ctypes.c_uint32)
        seen = lambda p: np.ctypeslib.as_array(ctypes.cast(p, u32), shape=(n,)).tolist() if n and p else []
        self.calls.append(dict(symbol=symbol, refs=refs, keys=keys, n=n, mp=mp, edges=edges, capacity=capacity,
                               listed=seen(refs), listed_keys=seen(keys)))
        n_edges._obj.value = len(self.records)
        if not edges:
            return 0
        if capacity < len(self.records):
            ctypes.set_errno(errno.ERANGE)
            return -1
        if len(self.records):
            ctypes.memmove(edges, self.records.ctypes.data, self.records.nbytes)
        return 0

    def blurrily_storage_cluster_edges(self, handle, refs, n, mp, edges, capacity, n_edges):
        return self._answer("plain", refs, None, n, mp, edges, capacity, n_edges)

    def blurrily_storage_cluster_edges_within(self, handle, refs, keys, n, mp, edges, capacity, n_edges):
        return self._answer("within", refs, keys, n, mp, edges, capacity, n_edges)


RECORDS = [(14, 15, 900), (10, 11, 800), (11, 17, 800), (10, 17, 705)]


def _stubbed(records=RECORDS):
    m = RawMap()
    m._real, m._lib = m._lib, _StubLib(records)
    return m


def _unstub(m):
    m._lib = m._real
    m.close()


def test_cluster_edges_hands_every_pointer_shapes_the_records_and_picks_the_symbol_by_blocks():
    m = _stubbed()
    edges = m.cluster_edges(SHUFFLED, 700)
    call = m._lib.calls[-1]
    assert len(m._lib.calls) == 1 and call["symbol"] == "plain" and call["refs"] and call["edges"] and not call["keys"]
    assert (call["n"], call["mp"], call["capacity"], call["listed"]) == (8, 700, 1024, SHUFFLED)
    assert edges.dtype == np.uint32 and edges.shape == (4, 3) and edges.tolist() == [list(e) for e in RECORDS]
    edges = m.cluster_edges(np.array(SHUFFLED, dtype=np.uint32), 0, blocks=np.array(KEYS_SAME, dtype=np.uint32))
    call = m._lib.calls[-1]
    assert call["symbol"] == "within" and call["keys"] and (call["listed"], call["listed_keys"]) == (SHUFFLED, KEYS_SAME)
    assert (call["mp"], call["capacity"]) == (0, 1024) and edges.tolist() == [list(e) for e in RECORDS]
    # the first room: the caller's, or max(1024, 8 n)
    m.cluster_edges(list(range(1, 301)), 500)
    assert m._lib.calls[-1]["capacity"] == 2400
    m.cluster_edges(SHUFFLED, 500, capacity=4)
    assert m._lib.calls[-1]["capacity"] == 4
    # nothing listed hands no list, and still a buffer: the call is no count
    m._lib.records = np.zeros((0, 3), dtype=np.uint32)
    out = m.cluster_edges([], 1000)
    last = m._lib.calls[-1]
    assert last["n"] == 0 and not last["refs"] and last["symbol"] == "plain"
    assert out.shape == (0, 3) and out.dtype == np.uint32
    out = m.cluster_edges([], 1000, blocks=[])
    assert m._lib.calls[-1]["symbol"] == "within" and not m._lib.calls[-1]["keys"] and out.shape == (0, 3)
    _unstub(m)


def test_cluster_edges_grows_once_to_the_reported_count():
    m = _stubbed()
    for blocks, symbol in ((None, "plain"), (KEYS_SAME, "within")):
        m._lib.calls.clear()
        edges = m.cluster_edges(SHUFFLED, 700, blocks=blocks, capacity=3)
        assert [(c["symbol"], c["capacity"]) for c in m._lib.calls] == [(symbol, 3), (symbol, 4)]
        assert edges.tolist() == [list(e) for e in RECORDS]
        m._lib.calls.clear()
        assert m.cluster_edges(SHUFFLED, 700, blocks=blocks, capacity=0).shape == (4, 3)
        assert [c["capacity"] for c in m._lib.calls] == [0, 4]
    _unstub(m)


def test_cluster_edge_count_hands_no_buffer():
    m = _stubbed()
    assert m.cluster_edge_count(SHUFFLED, 700) == 4
    call = m._lib.calls[-1]
    assert call["symbol"] == "plain" and not call["edges"] and call["capacity"] == 0 and call["listed"] == SHUFFLED
    count = m.cluster_edge_count(SHUFFLED, 700, KEYS_SAME)
    call = m._lib.calls[-1]
    assert count == 4 and isinstance(count, int) and call["symbol"] == "within" and not call["edges"] and call["keys"]
    assert len(m._lib.calls) == 2
    _unstub(m)


def test_adjacency_on_canned_records():
    listed = [10, 11, 14, 15, 17, 99]
    row_off, neighbour, permille = RawMap.adjacency(RECORDS, listed)
    assert (row_off.dtype, neighbour.dtype, permille.dtype) == (np.uint64, np.uint32, np.uint32)
    assert row_off.tolist() == [0, 2, 4, 5, 6, 8, 8]
    assert neighbour.tolist() == [11, 17, 10, 17, 15, 14, 11, 10]             # (in the records' order, row by row)
    assert permille.tolist() == [800, 705, 800, 800, 900, 900, 800, 705]
    # one row per element: a shuffled list with repeats
    for refs in (SHUFFLED, np.array(SHUFFLED, dtype=np.uint32), listed, listed[::-1]):
        got, want = RawMap.adjacency(RECORDS, refs), CE.adjacency(RECORDS, refs)
        for x, y in zip(got, want):
            assert x.dtype == y.dtype and x.tolist() == y.tolist()
    row_off, neighbour, permille = RawMap.adjacency(RECORDS, SHUFFLED)
    assert row_off.tolist() == [0, 1, 3, 5, 7, 8, 9, 9, 11] and len(neighbour) == 11
    # no records; nothing listed
    row_off, neighbour, permille = RawMap.adjacency([], listed)
    assert row_off.tolist() == [0] * 7 and neighbour.shape == permille.shape == (0,)
    assert RawMap.adjacency([], [])[0].tolist() == [0]
    with pytest.raises(ValueError):
        RawMap.adjacency(RECORDS, [10, 11, 14, 15])               # a record names a reference that is not listed
    with pytest.raises(ValueError):
        RawMap.adjacency(RECORDS, [])
    with pytest.raises(ValueError):
        RawMap.adjacency([(10, 11)], listed)                      # rows of three
    with pytest.raises(ValueError):
        RawMap.adjacency(RECORDS, [[10, 11]])


def test_tree_by_block_cut_tree_and_merge_profile_accept_edge_records():
    # 10, 11 and 17 form a triangle: no forest, and still the tools take the records as they are
    listed, keys = [10, 11, 14, 15, 17, 99], [1, 1, 2, 2, 1, 5]
    by_block = RawMap.tree_by_block(RECORDS, listed, keys)
    assert sorted(by_block) == [1, 2]
    assert by_block[1].tolist() == [[10, 11, 800], [11, 17, 800], [10, 17, 705]] and by_block[2].tolist() == [[14, 15, 900]]
    labels = np.array([10, 10, 14, 14, 10, NO], dtype=np.uint32)   # (what cluster gives at 700)
    assert RawMap.cut_tree(listed, labels, RECORDS, 700, min_permille=700).tolist() == [10, 10, 14, 14, 10, NO]
    assert RawMap.cut_tree(listed, labels, RECORDS, 801, min_permille=700).tolist() == [10, 11, 14, 14, 17, NO]
    assert RawMap.cut_tree(listed, labels, RECORDS, 706, min_permille=700).tolist() == [10, 10, 14, 14, 10, NO]
    assert RawMap.cut_tree(listed, labels, np.array(RECORDS, dtype=np.uint32), 901, min_permille=700).tolist() == \
        [10, 11, 14, 15, 17, NO]
    assert [(r["permille"], r["merges"]) for r in RawMap.merge_profile(RECORDS)] == [(900, 1), (800, 3), (705, 4)]


def _words():
    kind, n, _ = ORACLE_CASES[0]
    assert (kind, n) == ("words", 5000)
    hay, off, _ = oracle_case_inputs(kind, n)
    return {i + 1: s for i, s in enumerate(W.unpack(hay, off))}, np.arange(1, n + 1, dtype=np.uint32)


def _sound(truth, listed, floor, least=None):
    """The truth's records at a floor: sorted, distinct, a < b, heights at or above the floor; uniting them gives
    Truth.cluster's labels and edge count; Kruskal's records are a subsequence."""
    rows = CE.records(truth, listed, floor, least)
    keys = [(-p, a, b) for a, b, p in rows.tolist()]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert (rows[:, 0] < rows[:, 1]).all() and (rows[:, 2] >= floor).all() and (rows[:, 2] <= 1000).all()
    labels, _, n_edges, of_ref = truth.cluster(listed, floor, floor if least is None else least)
    assert len(rows) == n_edges
    assert np.array_equal(CE.labels(rows, listed, of_ref), labels)
    assert np.array_equal(RawMap.cut_tree(listed, labels, rows, floor, min_permille=floor), labels)
    forest = TT.kruskal(truth, listed, floor, least)
    at = iter(map(tuple, rows.tolist()))
    assert all(any(e == r for r in at) for e in map(tuple, forest.tolist()))   # (in order: a subsequence)
    return rows


def test_the_truth_is_sound_on_the_words_haystack_and_the_oracle_haystacks_fill_more_than_four_sort_tiles_at_200():
    """The words haystack has 2 618 edges at 200 per mille, less than one sort tile (so it is the oracle case of a single
    tile and no merge pass); more than four tiles of edges at 200, which the GPU file's merge passes stand on, come
    from its two other oracle haystacks: geonames 8 000 has 1 848 535 and skewed 6 000 has 1 949 550."""
    held, listed = _words()
    truth = Truth(held)
    counts = {}
    for floor in (200, 300, 500, 700):
        counts[floor] = len(_sound(truth, listed, floor, least=200))
    print("words 5000, edges by floor:", counts)
    assert 2 <= counts[200] <= TILE and counts[200] > counts[300] > counts[500] >= counts[700]
    for kind, n in (("geonames", 8000), ("skewed", 6000)):
        hay, off, _ = oracle_case_inputs(kind, n)
        other = Truth({i + 1: s for i, s in enumerate(W.unpack(hay, off))})
        many = len(CE.records(other, np.arange(1, n + 1, dtype=np.uint32), 200))
        print(kind, n, "edges at 200:", many)
        assert many > 4 * TILE                                # (what the GPU file's merge passes stand on)
    # the adjacency of the truth's records: every record twice, the rows in the records' order
    rows = CE.records(truth, listed, 300, 200)
    row_off, neighbour, permille = RawMap.adjacency(rows, listed)
    want = CE.adjacency(rows, listed)
    assert row_off.tolist() == want[0].tolist() and neighbour.tolist() == want[1].tolist()
    assert permille.tolist() == want[2].tolist() and len(neighbour) == 2 * len(rows)


def test_the_blocked_truth_is_the_per_block_truths_merged():
    held, listed = _words()
    blocks = listed % 3
    for floor in (200, 500):
        rows, truth = CE.blocked_records(held, listed, blocks, floor)
        _sound(truth, listed, floor)
        plain = Truth(held)
        own = [CE.records(plain, listed[blocks == k], floor) for k in np.unique(blocks)]
        assert np.array_equal(CE.merged(own), rows)
        assert len(rows) < len(CE.records(plain, listed, floor))
        by_block = RawMap.tree_by_block(rows, listed, blocks)
        for k, one in zip(np.unique(blocks).tolist(), own):
            assert np.array_equal(by_block.get(k, np.zeros((0, 3), dtype=np.uint32)), one)


def test_cliques_of_identical_strings_have_the_edge_counts_the_gpu_tests_stand_on():
    for k in CLIQUES:
        held = {r: b"identical strings" for r in range(1, k + 1)}
        rows = _sound(Truth(held), np.arange(1, k + 1), 1000)
        assert len(rows) == k * (k - 1) // 2 and (rows[:, 2] == 1000).all()
        assert rows[0].tolist() == [1, 2, 1000] and rows[-1].tolist() == [k - 1, k, 1000]
    # where they land against the sort's tile: one tile up to 91 (4 095 edges), merge passes from 92 (4 186) on, and
    # 200 (19 900) cuts into five runs, an odd number, of which the last is short
    edges = {k: k * (k - 1) // 2 for k in CLIQUES}
    assert edges[91] == TILE - 1 and edges[92] > TILE and edges[129] == 2 * TILE + 64
    assert -(-edges[200] // TILE) == 5 and edges[200] % TILE != 0
    # disjoint identical pairs on top of the clique of 91 land exactly on the tile, one above, and one above twice it
    for pairs, total in ((1, TILE), (2, TILE + 1), (TILE + 2, 2 * TILE + 1)):
        assert edges[91] + pairs == total
