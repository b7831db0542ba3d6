"""The cluster tree, without a GPU: blurrily_storage_cluster_tree is exported with its argtypes set, its prototype agrees
with the reference's storage.h in one translation unit and alone, a drifted prototype does not compile, every argument
error is EINVAL before a GPU is asked for and leaves all five outputs as they were, valid calls fail loudly (ENODEV)
where no GPU is usable, the Python surface checks its arguments, hands the right pointers and shapes canned arrays
rightly, and cut_tree and merge_profile -- numpy over a tree's records, no map, no GPU -- cut the chain of
tests/test_gpu_cluster_levels.py on both sides of both of its edges.  The truth's two spanning forests (Kruskal's and
Boruvka's, tests/cluster_tree_truth.py) agree on inputs the GPU tests use."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, RawMap, _native
from cluster_truth import Truth
import cluster_tree_truth as TT
from helpers import ORACLE_CASES, compile_c, einval, oracle_case_inputs, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster_tree.c")
NO = _native.NO_CLUSTER


def test_the_cluster_tree_symbol_is_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert " T blurrily_storage_cluster_tree\n" in out
    fn = lib.blurrily_storage_cluster_tree
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert "blurrily_storage_cluster_tree" in _native.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "blurrily_storage.h")).read()
    assert ("int blurrily_storage_cluster_tree(trigram_map haystack, const uint32_t* references, size_t n, "
            "uint32_t min_permille,") in header
    assert "typedef struct { uint32_t a, b, permille; } blurrily_cluster_merge_t;" in header
    assert "#define BLURRILY_CLUSTER_TREE_MAX 0x8000000u" in header and _native.CLUSTER_TREE_MAX == 0x8000000 == 1 << 27


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_cluster_tree_prototype_compiles_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_tree_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("was,now", [("uint32_t*, blurrily_cluster_merge_t*, uint32_t*,", "uint32_t*, uint32_t*,"),
                                     ("uint32_t*, uint64_t*) =", "uint32_t*, uint32_t*) ="),
                                     ("const uint32_t*, size_t, uint32_t,", "const uint32_t*, uint32_t, uint32_t,"),
                                     ("uint32_t*, blurrily_cluster_merge_t*,", "uint32_t*, uint32_t*,"),
                                     ("sizeof(blurrily_cluster_merge_t) == 12", "sizeof(blurrily_cluster_merge_t) == 16")],
                         ids=["no_merges", "edges_as_a_word", "n_as_a_word", "merges_as_words", "records_of_four_words"])
def test_a_drifted_cluster_tree_prototype_does_not_compile(tmp_path, was, now):
    write_recorded_storage_h(tmp_path)
    text = open(SRC).read()
    drifted = text.replace(was, now)
    assert drifted != text
    src = tmp_path / "drifted.c"
    src.write_text(drifted)
    assert compile_c(tmp_path, src).returncode != 0


def test_argument_errors_are_einval_before_any_gpu_and_write_nothing():
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs = np.array([1, 2, 3], dtype=np.uint32)
    labels = np.full(8, 7, dtype=np.uint32)
    merges = np.full((8, 3), 7, dtype=np.uint32)
    n_merges, n_clusters, n_edges = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint64(7)
    counts = (ctypes.byref(n_merges), ctypes.byref(n_clusters), ctypes.byref(n_edges))
    call = lib.blurrily_storage_cluster_tree
    r, lab, mer = refs.ctypes.data, labels.ctypes.data, merges.ctypes.data
    einval(lambda: call(None, r, 3, 500, lab, mer, *counts))                        # no map
    einval(lambda: call(m.handle, r, 3, 1001, lab, mer, *counts))                   # min_permille > 1000
    einval(lambda: call(m.handle, None, 0, 1001, None, None, *counts))              # ... with nothing listed too
    einval(lambda: call(m.handle, None, 3, 500, lab, mer, *counts))                 # references NULL, n > 0
    einval(lambda: call(m.handle, r, 3, 500, None, mer, *counts))                   # labels NULL, n > 0
    einval(lambda: call(m.handle, r, 3, 500, lab, None, *counts))                   # merges NULL, n > 0
    einval(lambda: call(m.handle, r, (1 << 27) + 1, 500, lab, mer, *counts))        # more than the key's 27 bits number
    einval(lambda: call(m.handle, r, 0xFFFFFFF1, 500, lab, mer, *counts))
    einval(lambda: call(m.handle, r, 2**64 - 1, 500, lab, mer, *counts))
    einval(lambda: call(m.handle, r, 3, 1001, lab, mer, None, None, None))          # the counts are optional
    assert (n_merges.value, n_clusters.value, n_edges.value) == (7, 7, 7)           # nothing written
    assert (labels == 7).all() and (merges == 7).all()
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster_tree.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs = np.array([1, 2, 3], dtype=np.uint32)
    labels, merges = np.zeros(8, dtype=np.uint32), np.zeros((8, 3), dtype=np.uint32)
    n_merges, n_clusters, n_edges = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
    call = lib.blurrily_storage_cluster_tree
    r, lab, mer = refs.ctypes.data, labels.ctypes.data, merges.ctypes.data
    sh = np.array([14, 10, 17, 11, 15, 14, 99, 11], dtype=np.uint32)               # shuffled, with repeats
    for one in (lambda: call(m.handle, r, 3, 500, lab, mer, ctypes.byref(n_merges), ctypes.byref(n_clusters),
                             ctypes.byref(n_edges)),
                lambda: call(m.handle, r, 3, 0, lab, mer, None, None, None),
                lambda: call(m.handle, r, 3, 1000, lab, mer, None, None, None),
                lambda: call(m.handle, sh.ctypes.data, len(sh), 500, lab, mer, None, None, None),
                lambda: call(m.handle, None, 0, 500, None, None, None, None, None)):
        ctypes.set_errno(0)
        assert one() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for one in (lambda: m.cluster_tree([1, 2], 700), lambda: m.cluster_tree([], 0), lambda: m.cluster_tree(sh, 1000)):
        with pytest.raises(OSError) as e:
            one()
        assert e.value.errno == errno.ENODEV
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    with pytest.raises(ValueError):
        m.cluster_tree([1], 1001)
    with pytest.raises(OverflowError):
        m.cluster_tree([1], -1)
    with pytest.raises(OverflowError):
        m.cluster_tree([-1], 500)
    with pytest.raises(OverflowError):
        m.cluster_tree([1 << 32], 500)
    with pytest.raises(ValueError):
        m.cluster_tree([[1, 2]], 500)
    m.close()
    with pytest.raises(RawMap.ClosedError):
        m.cluster_tree([1], 500)


class _StubLib:
    """Stands where the library stands in a RawMap: records what blurrily_storage_cluster_tree is handed and fills the
    outputs from canned arrays (no GPU is asked for)."""

    def __init__(self, canned):
        self.canned, self.calls = canned, []

    def blurrily_storage_cluster_tree(self, handle, refs, n, mp, labels, merges, n_merges, n_clusters, n_edges):
        u32 = ctypes.POINTER(ctypes.c_uint32)
        listed = np.ctypeslib.as_array(ctypes.cast(refs, u32), shape=(n,)).tolist() if n else []
        self.calls.append(dict(refs=refs, n=n, mp=mp, labels=labels, merges=merges, listed=listed))
        c = self.canned
        if labels:
            out = np.array([c["label_of"].get(r, NO) for r in listed], dtype=np.uint32)
            ctypes.memmove(labels, out.ctypes.data, 4 * n)
        rows = np.array(c["merges"], dtype=np.uint32).reshape(-1, 3)
        if merges and len(rows):
            assert len(rows) <= n                                                   # (room for n records was handed)
            ctypes.memmove(merges, rows.ctypes.data, rows.nbytes)
        n_merges._obj.value, n_clusters._obj.value, n_edges._obj.value = len(rows), c["n_clusters"], c["n_edges"]
        return 0


# the chain of tests/test_gpu_cluster_levels.py: A = qxzqvwkj, B = qxzqvwkjxqzzvk, C = jxqzzvk; J(A, B) = 8 / 16,
# J(B, C) = 6 / 17 (352.9 per mille), J(A, C) = 0; 17 stands alone, 99 is absent
A, B, C_ = 5001, 5002, 5003
CHAIN = [(A, B, 500), (B, C_, 352)]
CANNED = dict(label_of={A: A, B: A, C_: A, 17: 17}, merges=CHAIN, n_clusters=2, n_edges=2)
SHUFFLED = [C_, 17, A, 99, B, C_]


def _stubbed():
    m = RawMap()
    m._real, m._lib = m._lib, _StubLib(CANNED)
    return m


def _unstub(m):
    m._lib = m._real
    m.close()


def test_cluster_tree_hands_every_pointer_and_shapes_the_outputs():
    m = _stubbed()
    labels, merges, n_clusters, n_edges = m.cluster_tree(SHUFFLED, 300)
    call = m._lib.calls[-1]
    assert all(call[k] for k in ("refs", "labels", "merges"))
    assert (call["n"], call["mp"], call["listed"]) == (6, 300, SHUFFLED)
    assert labels.dtype == np.uint32 and labels.tolist() == [A, 17, A, NO, A, A]
    assert merges.dtype == np.uint32 and merges.shape == (2, 3) and merges.tolist() == [list(e) for e in CHAIN]
    assert (n_clusters, n_edges) == (2, 2) and isinstance(n_clusters, int) and isinstance(n_edges, int)
    # arrays of the right type go as they are; nothing listed hands no pointer
    labels, merges, _, _ = m.cluster_tree(np.array(SHUFFLED, dtype=np.uint32), 0)
    assert labels.tolist() == [A, 17, A, NO, A, A] and m._lib.calls[-1]["mp"] == 0
    m._lib.canned = dict(label_of={}, merges=[], n_clusters=0, n_edges=0)
    out = m.cluster_tree([], 1000)
    last = m._lib.calls[-1]
    assert last["n"] == 0 and not any(last[k] for k in ("refs", "labels", "merges"))
    assert out[0].shape == (0,) and out[0].dtype == np.uint32 and out[1].shape == (0, 3) and out[1].dtype == np.uint32
    assert out[2:] == (0, 0)
    _unstub(m)


@pytest.mark.parametrize("floor,want", [(352, [A, A, A]), (353, [A, A, C_]), (500, [A, A, C_]), (501, [A, B, C_])])
def test_cut_tree_cuts_the_chain_on_both_sides_of_both_edges(floor, want):
    refs, labels = [A, B, C_], [A, A, A]
    got = RawMap.cut_tree(refs, labels, CHAIN, floor)
    assert got.dtype == np.uint32 and got.tolist() == want
    # the list shuffled, with a repeat, a singleton and an absent reference; the records in any order
    of = dict(zip(refs, want))
    of[17] = 17
    tree_labels = [CANNED["label_of"].get(r, NO) for r in SHUFFLED]
    got = RawMap.cut_tree(SHUFFLED, tree_labels, CHAIN[::-1], floor, min_permille=300)
    assert got.tolist() == [of.get(r, NO) for r in SHUFFLED]
    assert np.array_equal(got, TT.cut(CHAIN, tree_labels, SHUFFLED, floor))


def test_cut_tree_checks_its_arguments_and_takes_empty_trees():
    refs, labels = [A, B, C_], [A, A, A]
    with pytest.raises(ValueError):
        RawMap.cut_tree(refs, labels, CHAIN, 1001)
    with pytest.raises(ValueError):
        RawMap.cut_tree(refs, labels, CHAIN, 351, min_permille=352)                 # below the tree's floor
    assert RawMap.cut_tree(refs, labels, CHAIN, 352, min_permille=352).tolist() == [A, A, A]
    with pytest.raises(OverflowError):
        RawMap.cut_tree(refs, labels, CHAIN, -1)
    with pytest.raises(ValueError):
        RawMap.cut_tree(refs, labels[:2], CHAIN, 400)
    with pytest.raises(ValueError):
        RawMap.cut_tree([A, B], [A, A], CHAIN, 300)                                 # a record names a reference not listed
    with pytest.raises(ValueError):
        RawMap.cut_tree([A, B, C_], [A, A, NO], CHAIN, 300)                         # ... or one the labels do not hold
    assert RawMap.cut_tree([], [], np.zeros((0, 3), dtype=np.uint32), 0).shape == (0,)
    assert RawMap.cut_tree([7, 9, 8], [7, NO, 8], [], 1000).tolist() == [7, NO, 8]
    # a longer path whose records come in an order that a single pass of label propagation does not settle
    path = [(i, i + 1, 900 - i) for i in range(1, 40)]
    everyone = list(range(1, 41))
    assert RawMap.cut_tree(everyone, [1] * 40, path[::-1], 0).tolist() == [1] * 40
    assert RawMap.cut_tree(everyone, [1] * 40, path, 881).tolist() == [1] * 20 + list(range(21, 41))


def test_merge_profile_counts_the_clusters_left_after_every_height():
    assert RawMap.merge_profile(CHAIN) == [{"permille": 500, "merges": 1, "n_clusters": 2},
                                           {"permille": 352, "merges": 2, "n_clusters": 1}]
    assert RawMap.merge_profile(CHAIN, nodes=4) == [{"permille": 500, "merges": 1, "n_clusters": 3},
                                                    {"permille": 352, "merges": 2, "n_clusters": 2}]
    ties = [(1, 2, 1000), (1, 3, 1000), (1, 4, 1000), (5, 6, 1000), (1, 5, 400)]
    assert RawMap.merge_profile(np.array(ties, dtype=np.uint32)) == [{"permille": 1000, "merges": 4, "n_clusters": 2},
                                                                      {"permille": 400, "merges": 5, "n_clusters": 1}]
    assert RawMap.merge_profile([]) == []


def _agree(held, listed, floor):
    truth = Truth(held)
    records = TT.kruskal(truth, listed, floor)
    forest, rounds = TT.boruvka(truth, listed, floor)
    assert set(map(tuple, records.tolist())) == forest and len(forest) == len(records)
    # the records are sorted by the total order and name each pair once
    keys = [(-p, a, b) for a, b, p in records.tolist()]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and all(a < b for a, b, _ in records.tolist())
    # cutting them at their own floor gives the truth's components
    labels, n_clusters, _, of_ref = truth.cluster(listed, floor)
    assert len(records) == len(of_ref) - n_clusters
    assert np.array_equal(TT.cut(records, labels, listed, floor), labels)
    assert np.array_equal(RawMap.cut_tree(listed, labels, records, floor, min_permille=floor), labels)
    return records, rounds


def test_kruskal_and_boruvka_give_one_forest_on_the_words_haystack_and_need_three_rounds():
    kind, n, _ = ORACLE_CASES[0]
    hay, off, _ = oracle_case_inputs(kind, n)
    held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
    listed = np.arange(1, n + 1, dtype=np.uint32)
    rounds = {floor: _agree(held, listed, floor)[1] for floor in (200, 300, 500, 1000)}
    assert rounds[200] >= 3                                   # (what tests/test_gpu_cluster_tree.py's rounds test stands on)


def test_kruskal_and_boruvka_give_one_forest_on_ties():
    same = b"tied strings"
    held = {1: same, 2: same, 3: same, 4: same}
    records, rounds = _agree(held, [1, 2, 3, 4], 1000)
    assert records.tolist() == [[1, 2, 1000], [1, 3, 1000], [1, 4, 1000]] and rounds == 1
    other = b"another group"
    held.update({11: other, 12: other, 13: other, 14: other, 5: same + b" another"})
    records, _ = _agree(held, sorted(held), 0)
    assert records.tolist()[:6] == [[1, 2, 1000], [1, 3, 1000], [1, 4, 1000], [11, 12, 1000], [11, 13, 1000],
                                    [11, 14, 1000]]
    assert len(records) == 8
