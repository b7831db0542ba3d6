"""The cluster core tree, without a GPU: blurrily_storage_cluster_core_tree is exported with its twelve argtypes set,
its prototype agrees with the reference's storage.h in one translation unit and alone, a drifted prototype does not
compile, every argument error is EINVAL before a GPU is asked for and leaves all outputs as they were, valid calls fail
loudly (ENODEV) where no GPU is usable, the Python surface checks its arguments, hands the right pointers and shapes
canned arrays rightly, and cut_core_tree -- numpy over a tree's records, no map, no GPU -- does what it says on
hand-made records.  Last, the definition itself: the truth (tests/cluster_core_tree_truth.py), cut at each of its
heights and one per mille above, gives the core set, the cores' labels and the clusters of the cores' own truth
(tests/cluster_cores_truth.py) at that floor -- the equivalence the GPU tests lean on."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, RawMap, _native
from cluster_cores_truth import CORE, CoresEdges
from cluster_core_tree_truth import CoreTreeTruth
from cluster_truth import Truth
from helpers import ORACLE_CASES, compile_c, einval, oracle_case_inputs, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster_core_tree.c")
NO, NO_CORE = _native.NO_CLUSTER, _native.NO_CORE


def test_the_cluster_core_tree_symbol_is_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert " T blurrily_storage_cluster_core_tree\n" in out
    fn = lib.blurrily_storage_cluster_core_tree
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 12
    assert "blurrily_storage_cluster_core_tree" in _native.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "blurrily_storage.h")).read()
    assert "int blurrily_storage_cluster_core_tree(trigram_map haystack, const uint32_t* references, size_t n," in header
    assert "#define BLURRILY_NO_CORE 0xFFFFFFFFu" in header and NO_CORE == 0xFFFFFFFF


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_cluster_core_tree_prototype_compiles_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_core_tree_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("was,now", [("uint32_t, uint32_t, uint32_t*, uint32_t*,", "uint32_t, uint32_t, uint32_t*,"),
                                     ("size_t, uint32_t, uint32_t, uint32_t*,", "size_t, uint32_t, uint32_t*,"),
                                     ("uint64_t*, uint64_t*) =", "uint64_t*, uint32_t*) ="),
                                     ("const uint32_t*, size_t, uint32_t,", "const uint32_t*, uint32_t, uint32_t,"),
                                     ("blurrily_cluster_merge_t*, uint32_t*, uint32_t*, uint64_t*,",
                                      "uint32_t*, uint32_t*, uint32_t*, uint64_t*,")],
                         ids=["no_core_permille", "no_min_degree", "core_edges_as_a_word", "n_as_a_word", "merges_as_words"])
def test_a_drifted_cluster_core_tree_prototype_does_not_compile(tmp_path, was, now):
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
    labels, heights = np.full(8, 7, dtype=np.uint32), np.full(8, 7, dtype=np.uint32)
    merges = np.full((8, 3), 7, dtype=np.uint32)
    n_merges, n_clusters, n_edges, n_core = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    counts = (ctypes.byref(n_merges), ctypes.byref(n_clusters), ctypes.byref(n_edges), ctypes.byref(n_core))
    call = lib.blurrily_storage_cluster_core_tree
    r, lab, cor, mer = refs.ctypes.data, labels.ctypes.data, heights.ctypes.data, merges.ctypes.data
    einval(lambda: call(None, r, 3, 500, 2, lab, cor, mer, *counts))                    # no map
    einval(lambda: call(m.handle, r, 3, 1001, 2, lab, cor, mer, *counts))               # min_permille > 1000
    einval(lambda: call(m.handle, None, 0, 1001, 2, None, None, None, *counts))         # ... with nothing listed too
    einval(lambda: call(m.handle, None, 3, 500, 2, lab, cor, mer, *counts))             # references NULL, n > 0
    einval(lambda: call(m.handle, r, 3, 500, 2, None, cor, mer, *counts))               # labels NULL, n > 0
    einval(lambda: call(m.handle, r, 3, 500, 2, lab, None, mer, *counts))               # core_permille NULL, n > 0
    einval(lambda: call(m.handle, r, 3, 500, 2, lab, cor, None, *counts))               # merges NULL, n > 0
    einval(lambda: call(m.handle, r, (1 << 27) + 1, 500, 2, lab, cor, mer, *counts))    # more than the key's 27 bits number
    einval(lambda: call(m.handle, r, 0xFFFFFFF1, 500, 0, lab, cor, mer, *counts))
    einval(lambda: call(m.handle, r, 2**64 - 1, 500, 0xFFFFFFFF, lab, cor, mer, *counts))
    einval(lambda: call(m.handle, r, 3, 1001, 2, lab, cor, mer, None, None, None, None))   # the counts are optional
    assert (n_merges.value, n_clusters.value, n_edges.value, n_core.value) == (7, 7, 7, 7)   # nothing written
    assert (labels == 7).all() and (heights == 7).all() and (merges == 7).all()
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster_core_tree.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs = np.array([1, 2, 3], dtype=np.uint32)
    labels, heights, merges = np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32), np.zeros((8, 3), dtype=np.uint32)
    n_merges, n_clusters, n_edges, n_core = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    call = lib.blurrily_storage_cluster_core_tree
    r, lab, cor, mer = refs.ctypes.data, labels.ctypes.data, heights.ctypes.data, merges.ctypes.data
    sh = np.array([14, 10, 17, 11, 15, 14, 99, 11], dtype=np.uint32)                   # shuffled, with repeats
    for one in (lambda: call(m.handle, r, 3, 500, 2, lab, cor, mer, ctypes.byref(n_merges), ctypes.byref(n_clusters),
                             ctypes.byref(n_edges), ctypes.byref(n_core)),
                lambda: call(m.handle, r, 3, 0, 0, lab, cor, mer, None, None, None, None),
                lambda: call(m.handle, r, 3, 1000, 0xFFFFFFFF, lab, cor, mer, None, None, None, None),   # any min_degree
                lambda: call(m.handle, sh.ctypes.data, len(sh), 500, 3, lab, cor, mer, None, None, None, None),
                lambda: call(m.handle, None, 0, 500, 2, None, None, None, None, None, None, None)):
        ctypes.set_errno(0)
        assert one() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for one in (lambda: m.cluster_core_tree([1, 2], 700, 2), lambda: m.cluster_core_tree([], 0, 0),
                lambda: m.cluster_core_tree(sh, 1000, 2**32 - 1)):
        with pytest.raises(OSError) as e:
            one()
        assert e.value.errno == errno.ENODEV
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    with pytest.raises(ValueError):
        m.cluster_core_tree([1], 1001, 2)
    with pytest.raises(OverflowError):
        m.cluster_core_tree([1], -1, 2)
    with pytest.raises(OverflowError):
        m.cluster_core_tree([1], 500, -1)
    with pytest.raises(OverflowError):
        m.cluster_core_tree([1], 500, 1 << 32)
    with pytest.raises(OverflowError):
        m.cluster_core_tree([-1], 500, 2)
    with pytest.raises(OverflowError):
        m.cluster_core_tree([1 << 32], 500, 2)
    with pytest.raises(ValueError):
        m.cluster_core_tree([[1, 2]], 500, 2)
    with pytest.raises(ValueError):
        m.dense_tree([1], 1001, 2)
    m.close()
    with pytest.raises(RawMap.ClosedError):
        m.cluster_core_tree([1], 500, 2)


class _StubLib:
    """Stands where the library stands in a RawMap: records what blurrily_storage_cluster_core_tree is handed and fills
    the outputs from canned arrays (no GPU is asked for)."""

    def __init__(self, canned):
        self.canned, self.calls = canned, []

    def blurrily_storage_cluster_core_tree(self, handle, refs, n, mp, md, labels, core, merges, n_merges, n_clusters,
                                           n_edges, n_core_edges):
        u32 = ctypes.POINTER(ctypes.c_uint32)
        listed = np.ctypeslib.as_array(ctypes.cast(refs, u32), shape=(n,)).tolist() if n else []
        self.calls.append(dict(refs=refs, n=n, mp=mp, md=md, labels=labels, core=core, merges=merges, listed=listed))
        c = self.canned
        for to, of, none in ((labels, c["label_of"], NO), (core, c["core_of"], NO_CORE)):
            if to:
                out = np.array([of.get(r, none) for r in listed], dtype=np.uint32)
                ctypes.memmove(to, out.ctypes.data, 4 * n)
        rows = np.array(c["merges"], dtype=np.uint32).reshape(-1, 3)
        if merges and len(rows):
            assert len(rows) <= n                                                   # (room for n records was handed)
            ctypes.memmove(merges, rows.ctypes.data, rows.nbytes)
        n_merges._obj.value, n_clusters._obj.value = len(rows), c["n_clusters"]
        n_edges._obj.value, n_core_edges._obj.value = c["n_edges"], c["n_core_edges"]
        return 0


# a hand-made tree at floor 300, min_degree 2: 1, 2, 3 and 4 have core heights and hang together from 600 down to 400,
# 5 and 6 join each other at 450 and nobody else, 7 is a node with one edge (no core height), 99 is absent
CORE_OF = {1: 800, 2: 600, 3: 700, 4: 400, 5: 450, 6: 500, 7: NO_CORE}
RECORDS = [(1, 3, 700), (1, 2, 600), (5, 6, 450), (3, 4, 400)]
CANNED = dict(label_of={1: 1, 2: 1, 3: 1, 4: 1, 5: 5, 6: 5, 7: 7}, core_of=CORE_OF, merges=RECORDS, n_clusters=2, n_edges=9,
              n_core_edges=6)
SHUFFLED = [6, 7, 1, 99, 3, 2, 6, 4, 5]


def _stubbed():
    m = RawMap()
    m._real, m._lib = m._lib, _StubLib(CANNED)
    return m


def _unstub(m):
    m._lib = m._real
    m.close()


def test_cluster_core_tree_hands_every_pointer_and_shapes_the_outputs():
    m = _stubbed()
    labels, core, merges, n_clusters, n_edges, n_core_edges = m.cluster_core_tree(SHUFFLED, 300, 2)
    call = m._lib.calls[-1]
    assert all(call[k] for k in ("refs", "labels", "core", "merges"))
    assert len({call[k] for k in ("refs", "labels", "core", "merges")}) == 4
    assert (call["n"], call["mp"], call["md"], call["listed"]) == (9, 300, 2, SHUFFLED)
    assert labels.dtype == np.uint32 and labels.tolist() == [5, 7, 1, NO, 1, 1, 5, 1, 5]
    assert core.dtype == np.uint32 and core.tolist() == [500, NO_CORE, 800, NO_CORE, 700, 600, 500, 400, 450]
    assert merges.dtype == np.uint32 and merges.shape == (4, 3) and merges.tolist() == [list(e) for e in RECORDS]
    assert (n_clusters, n_edges, n_core_edges) == (2, 9, 6)
    assert all(isinstance(x, int) for x in (n_clusters, n_edges, n_core_edges))
    # arrays of the right type go as they are; any min_degree goes through; nothing listed hands no pointer
    m.cluster_core_tree(np.array(SHUFFLED, dtype=np.uint32), 0, 2**32 - 1)
    assert (m._lib.calls[-1]["mp"], m._lib.calls[-1]["md"]) == (0, 2**32 - 1)
    m._lib.canned = dict(label_of={}, core_of={}, merges=[], n_clusters=0, n_edges=0, n_core_edges=0)
    out = m.cluster_core_tree([], 1000, 0)
    last = m._lib.calls[-1]
    assert last["n"] == 0 and not any(last[k] for k in ("refs", "labels", "core", "merges"))
    assert [x.shape for x in out[:3]] == [(0,), (0,), (0, 3)] and all(x.dtype == np.uint32 for x in out[:3])
    assert out[3:] == (0, 0, 0)
    _unstub(m)


def test_dense_tree_lists_each_reference_once_and_returns_what_the_cut_takes():
    m = Map()
    m._real, m._lib = m._lib, _StubLib(CANNED)
    refs, labels, core, merges = m.dense_tree(SHUFFLED, 300, 2)
    assert m._lib.calls[-1]["listed"] == [1, 2, 3, 4, 5, 6, 7, 99] == refs.tolist()
    assert labels.tolist() == [1, 1, 1, 1, 5, 5, 7, NO] and core.tolist()[3:] == [400, 450, 500, NO_CORE, NO_CORE]
    at, is_core = RawMap.cut_core_tree(refs, labels, core, merges, 450, min_permille=300)
    assert at.tolist() == [1, 1, 1, 4, 5, 5, 7, NO] and is_core.tolist() == [True] * 3 + [False] + [True] * 2 + [False] * 2
    _unstub(m)


@pytest.mark.parametrize("floor,want,cores", [
    (300, {1: 1, 2: 1, 3: 1, 4: 1, 5: 5, 6: 5, 7: 7}, {1, 2, 3, 4, 5, 6}),
    (400, {1: 1, 2: 1, 3: 1, 4: 1, 5: 5, 6: 5, 7: 7}, {1, 2, 3, 4, 5, 6}),
    (401, {1: 1, 2: 1, 3: 1, 4: 4, 5: 5, 6: 5, 7: 7}, {1, 2, 3, 5, 6}),
    (451, {1: 1, 2: 1, 3: 1, 4: 4, 5: 5, 6: 6, 7: 7}, {1, 2, 3, 6}),
    (601, {1: 1, 2: 2, 3: 1, 4: 4, 5: 5, 6: 6, 7: 7}, {1, 3}),
    (701, {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7}, {1}),
    (801, {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7}, set()),
    (1000, {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7}, set())])
def test_cut_core_tree_cuts_hand_made_records(floor, want, cores):
    refs = sorted(CORE_OF)
    labels, core = [CANNED["label_of"][r] for r in refs], [CORE_OF[r] for r in refs]
    at, is_core = RawMap.cut_core_tree(refs, labels, core, RECORDS, floor, min_permille=300)
    assert at.dtype == np.uint32 and is_core.dtype == bool
    assert dict(zip(refs, at.tolist())) == want and {r for r, c in zip(refs, is_core.tolist()) if c} == cores
    # the list shuffled, with a repeat and an absent reference; the records in any order
    labels = [CANNED["label_of"].get(r, NO) for r in SHUFFLED]
    core = [CORE_OF.get(r, NO_CORE) for r in SHUFFLED]
    at, is_core = RawMap.cut_core_tree(SHUFFLED, labels, core, RECORDS[::-1], floor, min_permille=300)
    assert at.tolist() == [want.get(r, NO) for r in SHUFFLED]
    assert is_core.tolist() == [r in cores for r in SHUFFLED]


def test_cut_core_tree_checks_its_arguments_and_takes_empty_trees():
    refs = sorted(CORE_OF)
    labels, core = [CANNED["label_of"][r] for r in refs], [CORE_OF[r] for r in refs]
    with pytest.raises(ValueError):
        RawMap.cut_core_tree(refs, labels, core, RECORDS, 1001)
    with pytest.raises(ValueError):
        RawMap.cut_core_tree(refs, labels, core, RECORDS, 299, min_permille=300)        # below the tree's floor
    with pytest.raises(OverflowError):
        RawMap.cut_core_tree(refs, labels, core, RECORDS, -1)
    with pytest.raises(ValueError):
        RawMap.cut_core_tree(refs, labels[:2], core, RECORDS, 400)
    with pytest.raises(ValueError):
        RawMap.cut_core_tree(refs, labels, core[:2], RECORDS, 400)
    with pytest.raises(ValueError):
        RawMap.cut_core_tree(refs[:3], labels[:3], core[:3], RECORDS, 300)              # a record names a reference not listed
    with pytest.raises(ValueError):
        RawMap.cut_core_tree(refs, labels, [800, 600, 700, 399, 450, 500, NO_CORE], RECORDS, 400)   # ... or no core at its height
    with pytest.raises(ValueError):
        RawMap.cut_core_tree(refs, labels, core, RECORDS + [(6, 7, 450)], 400)          # ... or one without a core height
    at, is_core = RawMap.cut_core_tree([], [], [], np.zeros((0, 3), dtype=np.uint32), 0)
    assert at.shape == (0,) and is_core.shape == (0,)
    at, is_core = RawMap.cut_core_tree([7, 9, 8], [7, NO, 8], [1000, NO_CORE, NO_CORE], [], 1000)
    assert at.tolist() == [7, NO, 8] and is_core.tolist() == [True, False, False]


_WORDS = {}


def words_truth():
    if not _WORDS:
        kind, n, _ = ORACLE_CASES[0]
        hay, off, _ = oracle_case_inputs(kind, n)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        _WORDS.update(truth=Truth(held), listed=np.arange(1, n + 1, dtype=np.uint32))
    return _WORDS["truth"], _WORDS["listed"]


@pytest.mark.parametrize("min_degree", [2, 4])
@pytest.mark.parametrize("floor", [200, 300, 500])
def test_the_truth_cut_at_every_height_is_the_cores_truth_there(floor, min_degree):
    truth, listed = words_truth()
    tree = CoreTreeTruth(truth, listed, floor, min_degree, least=200)
    # the whole call against the cores' truth at the tree's own floor
    at_floor = CoresEdges(truth, listed, floor, least=200).cores(min_degree)
    assert (tree.n_clusters, tree.n_edges, tree.n_core_edges) == (at_floor.n_clusters, at_floor.n_edges, at_floor.n_core_edges)
    assert np.array_equal(tree.core_permille != NO_CORE, at_floor.kinds == CORE)
    assert np.array_equal(tree.labels[at_floor.kinds == CORE], at_floor.labels[at_floor.kinds == CORE])
    assert np.array_equal(tree.labels[at_floor.kinds != CORE], listed[at_floor.kinds != CORE])
    keys = [(-p, a, b) for a, b, p in tree.merges.tolist()]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and all(a < b for a, b, _ in tree.merges.tolist())
    heights = np.unique(tree.merges[:, 2]).tolist()
    print(f"floor {floor}, min_degree {min_degree}: {len(tree.merges)} merges at {len(heights)} heights, "
          f"{int((tree.c >= 0).sum())} cores, {tree.n_clusters} clusters")
    if (floor, min_degree) == (200, 2):
        assert len(heights) >= 3 and len(tree.merges) >= 3, "this case has no tree to speak of: the test shows nothing"
    refs = truth.refs
    for h in heights:
        for f in (h, h + 1):
            if f > 1000:
                continue
            is_core, label_of, n_clusters = tree.cut(f)
            want = CoresEdges(truth, listed, f, least=200).cores(min_degree)
            want_core = {r for r, k in want.kind_of.items() if k == CORE}
            assert set(refs[is_core].tolist()) == want_core, f
            assert label_of == {r: want.label_of[r] for r in want_core}, f
            assert n_clusters == want.n_clusters, f
            # ... and RawMap.cut_core_tree says the same of the truth's records
            at, core = RawMap.cut_core_tree(listed, tree.labels, tree.core_permille, tree.merges, f, min_permille=floor)
            assert set(listed[core].tolist()) == want_core and dict(zip(listed[core].tolist(), at[core].tolist())) == label_of
            assert np.array_equal(at[~core], listed[~core])
