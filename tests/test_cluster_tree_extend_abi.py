"""Cluster tree extend, without a GPU: blurrily_storage_cluster_tree_extend is exported with its argtypes set, its
prototype agrees with the reference's storage.h in one translation unit and alone, a drifted prototype does not compile,
every argument error is EINVAL before a GPU is asked for and leaves all six outputs as they were, valid calls fail
loudly (ENODEV) where no GPU is usable, the Python surface checks its arguments, hands the right pointers and shapes
canned arrays rightly, and tree_changes -- numpy over two sets of records, no map, no GPU -- names what to delete and
what to insert.  The truth (tests/cluster_tree_extend_truth.py) is held against itself: the forest of (the old tree's
records, the pairs with a new end) is the forest of all pairs, which is the theorem the entry stands on."""
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
from cluster_tree_extend_truth import TreeExtendTruth
from helpers import ORACLE_CASES, compile_c, einval, oracle_case_inputs, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster_tree_extend.c")
NO = _native.NO_CLUSTER


def test_the_cluster_tree_extend_symbol_is_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert " T blurrily_storage_cluster_tree_extend\n" in out
    fn = lib.blurrily_storage_cluster_tree_extend
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    assert "blurrily_storage_cluster_tree_extend" in _native.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "blurrily_storage.h")).read()
    assert ("int blurrily_storage_cluster_tree_extend(trigram_map haystack, const uint32_t* old_refs, size_t n_old,\n"
            "                                         const blurrily_cluster_merge_t* old_merges, size_t n_old_merges,\n"
            "                                         const uint32_t* new_refs, size_t n_new, uint32_t min_permille,\n"
            "                                         uint32_t* labels_old, uint32_t* labels_new,\n"
            "                                         blurrily_cluster_merge_t* merges, uint32_t* n_merges,\n"
            "                                         uint32_t* n_clusters, uint64_t* n_edges);") in header


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_cluster_tree_extend_prototype_compiles_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_tree_extend_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("was,now", [("size_t, const blurrily_cluster_merge_t*, size_t, const uint32_t*, size_t,",
                                      "size_t, const uint32_t*, size_t,"),
                                     ("uint32_t*, uint64_t*) =", "uint32_t*, uint32_t*) ="),
                                     ("(trigram_map, const uint32_t*, size_t,", "(trigram_map, const uint32_t*, uint32_t,"),
                                     ("uint32_t*, uint32_t*, blurrily_cluster_merge_t*,", "uint32_t*, uint32_t*, uint32_t*,"),
                                     ("uint32_t, uint32_t*, uint32_t*, blurrily", "uint32_t, uint32_t*, blurrily"),
                                     ("sizeof(blurrily_cluster_merge_t) == 12", "sizeof(blurrily_cluster_merge_t) == 16")],
                         ids=["no_old_merges", "edges_as_a_word", "n_old_as_a_word", "merges_as_words", "one_label_array",
                              "records_of_four_words"])
def test_a_drifted_cluster_tree_extend_prototype_does_not_compile(tmp_path, was, now):
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
    old = np.array([1, 2, 3], dtype=np.uint32)
    new = np.array([4, 5], dtype=np.uint32)
    held = np.array([[1, 2, 700], [2, 3, 600]], dtype=np.uint32)
    labels_old, labels_new = np.full(8, 7, dtype=np.uint32), np.full(8, 7, dtype=np.uint32)
    merges = np.full((8, 3), 7, dtype=np.uint32)
    n_merges, n_clusters, n_edges = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint64(7)
    counts = (ctypes.byref(n_merges), ctypes.byref(n_clusters), ctypes.byref(n_edges))
    call = lib.blurrily_storage_cluster_tree_extend
    o, w, h = old.ctypes.data, new.ctypes.data, held.ctypes.data
    lo, ln, mer = labels_old.ctypes.data, labels_new.ctypes.data, merges.ctypes.data
    einval(lambda: call(None, o, 3, h, 2, w, 2, 500, lo, ln, mer, *counts))           # no map
    einval(lambda: call(m.handle, o, 3, h, 2, w, 2, 1001, lo, ln, mer, *counts))      # min_permille > 1000
    einval(lambda: call(m.handle, None, 0, None, 0, None, 0, 1001, None, None, None, *counts))   # ... with nothing listed too
    einval(lambda: call(m.handle, None, 3, h, 2, w, 2, 500, lo, ln, mer, *counts))    # old_refs NULL, n_old > 0
    einval(lambda: call(m.handle, o, 3, h, 2, w, 2, 500, None, ln, mer, *counts))     # labels_old NULL, n_old > 0
    einval(lambda: call(m.handle, o, 3, h, 2, None, 2, 500, lo, ln, mer, *counts))    # new_refs NULL, n_new > 0
    einval(lambda: call(m.handle, o, 3, h, 2, w, 2, 500, lo, None, mer, *counts))     # labels_new NULL, n_new > 0
    einval(lambda: call(m.handle, o, 3, None, 2, w, 2, 500, lo, ln, mer, *counts))    # old_merges NULL, n_old_merges > 0
    einval(lambda: call(m.handle, o, 3, h, 2, w, 2, 500, lo, ln, None, *counts))      # merges NULL, n_old + n_new > 0
    einval(lambda: call(m.handle, o, 3, None, 0, None, 0, 500, lo, None, None, *counts))   # ... with old ones alone
    einval(lambda: call(m.handle, None, 0, None, 0, w, 2, 500, None, ln, None, *counts))   # ... with new ones alone
    einval(lambda: call(m.handle, o, (1 << 27) - 1, h, 2, w, 2, 500, lo, ln, mer, *counts))   # more than the key's 27 bits number
    einval(lambda: call(m.handle, o, 3, h, 2, w, 1 << 27, 500, lo, ln, mer, *counts))
    einval(lambda: call(m.handle, o, (1 << 27) + 1, h, 2, None, 0, 500, lo, None, mer, *counts))
    einval(lambda: call(m.handle, o, 2**64 - 1, h, 2, w, 2, 500, lo, ln, mer, *counts))   # (a sum that wraps)
    einval(lambda: call(m.handle, o, 3, h, 2, w, 2**64 - 2, 500, lo, ln, mer, *counts))
    einval(lambda: call(m.handle, o, 1, h, 2, w, 2, 500, lo, ln, mer, *counts))       # more records than old references
    einval(lambda: call(m.handle, None, 0, h, 1, w, 2, 500, None, ln, mer, *counts))
    for bad in ([[2, 2, 700], [2, 3, 600]], [[1, 2, 700], [3, 2, 600]], [[1, 2, 1001], [2, 3, 600]],
                [[1, 2, 700], [2, 3, 0xFFFFFFFF]]):                                   # a >= b, permille > 1000
        rec = np.array(bad, dtype=np.uint32)
        einval(lambda: call(m.handle, o, 3, rec.ctypes.data, 2, w, 2, 500, lo, ln, mer, *counts))
        einval(lambda: call(m.handle, o, 3, rec.ctypes.data, 2, w, 2, 1000, lo, ln, mer, *counts))   # (below the floor or not)
    einval(lambda: call(m.handle, o, 3, h, 2, w, 2, 1001, lo, ln, mer, None, None, None))   # the counts are optional
    assert (n_merges.value, n_clusters.value, n_edges.value) == (7, 7, 7)             # nothing written
    assert (labels_old == 7).all() and (labels_new == 7).all() and (merges == 7).all()
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster_tree_extend.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    old = np.array([1, 2, 3], dtype=np.uint32)
    new = np.array([4, 5], dtype=np.uint32)
    held = np.array([[1, 2, 700], [2, 3, 600]], dtype=np.uint32)
    labels_old, labels_new = np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
    merges = np.zeros((8, 3), dtype=np.uint32)
    n_merges, n_clusters, n_edges = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
    call = lib.blurrily_storage_cluster_tree_extend
    o, w, h = old.ctypes.data, new.ctypes.data, held.ctypes.data
    lo, ln, mer = labels_old.ctypes.data, labels_new.ctypes.data, merges.ctypes.data
    sh = np.array([14, 10, 17, 11, 15, 14, 99, 11], dtype=np.uint32)               # shuffled, with repeats
    for one in (lambda: call(m.handle, o, 3, h, 2, w, 2, 500, lo, ln, mer, ctypes.byref(n_merges),
                             ctypes.byref(n_clusters), ctypes.byref(n_edges)),
                lambda: call(m.handle, o, 3, h, 2, w, 2, 0, lo, ln, mer, None, None, None),
                lambda: call(m.handle, o, 3, h, 2, None, 0, 1000, lo, None, mer, None, None, None),
                lambda: call(m.handle, None, 0, None, 0, sh.ctypes.data, len(sh), 500, None, ln, mer, None, None, None),
                lambda: call(m.handle, o, 3, h, 2, o, 3, 500, lo, ln, mer, None, None, None),   # every reference in both lists
                lambda: call(m.handle, None, 0, None, 0, None, 0, 500, None, None, None, None, None, None)):
        ctypes.set_errno(0)
        assert one() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for one in (lambda: m.cluster_tree_extend([1, 2], [(1, 2, 700)], [3], 700), lambda: m.cluster_tree_extend([], [], [], 0),
                lambda: m.cluster_tree_extend(sh[:4], [], sh[4:], 1000)):
        with pytest.raises(OSError) as e:
            one()
        assert e.value.errno == errno.ENODEV
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    with pytest.raises(ValueError):
        m.cluster_tree_extend([1], [], [2], 1001)
    with pytest.raises(OverflowError):
        m.cluster_tree_extend([1], [], [2], -1)
    with pytest.raises(OverflowError):
        m.cluster_tree_extend([-1], [], [2], 500)
    with pytest.raises(OverflowError):
        m.cluster_tree_extend([1], [], [1 << 32], 500)
    with pytest.raises(ValueError):
        m.cluster_tree_extend([[1, 2]], [], [3], 500)
    with pytest.raises(ValueError):
        m.cluster_tree_extend([1, 2], [(1, 2)], [3], 500)                          # records of two words
    with pytest.raises(ValueError):
        m.cluster_tree_extend([1, 2], [1, 2, 500], [3], 500)                       # one flat record
    with pytest.raises(OverflowError):
        m.cluster_tree_extend([1, 2], [(1, 2, -5)], [3], 500)
    with pytest.raises(OverflowError):
        m.cluster_tree_extend([1, 2], [(1, 1 << 32, 5)], [3], 500)
    with pytest.raises(ValueError):
        m.cluster_tree_extend([1, 2], [(2, 1, 500)], [3], 500)                     # a >= b
    with pytest.raises(ValueError):
        m.cluster_tree_extend([1, 2], [(1, 2, 1001)], [3], 500)                    # permille > 1000
    with pytest.raises(ValueError):
        m.cluster_tree_extend([1], [(1, 2, 500), (1, 3, 400)], [3], 500)           # more records than old references
    m.close()
    with pytest.raises(RawMap.ClosedError):
        m.cluster_tree_extend([1], [], [2], 500)


class _StubLib:
    """Stands where the library stands in a RawMap: records what blurrily_storage_cluster_tree_extend is handed and fills
    the outputs from canned arrays (no GPU is asked for)."""

    def __init__(self, canned):
        self.canned, self.calls = canned, []

    def blurrily_storage_cluster_tree_extend(self, handle, old, n_old, held, n_held, new, n_new, mp, labels_old, labels_new,
                                             merges, n_merges, n_clusters, n_edges):
        u32 = ctypes.POINTER(ctypes.c_uint32)
        words = lambda p, k: np.ctypeslib.as_array(ctypes.cast(p, u32), shape=(k,)).tolist() if k else []
        olds, news = words(old, n_old), words(new, n_new)
        records = np.array(words(held, 3 * n_held), dtype=np.uint32).reshape(-1, 3).tolist()
        self.calls.append(dict(old=old, new=new, held=held, labels_old=labels_old, labels_new=labels_new, merges=merges,
                               n_old=n_old, n_new=n_new, n_held=n_held, mp=mp, olds=olds, news=news, records=records))
        c = self.canned
        for listed, out in ((olds, labels_old), (news, labels_new)):
            if out:
                got = np.array([c["label_of"].get(r, NO) for r in listed], dtype=np.uint32)
                ctypes.memmove(out, got.ctypes.data, 4 * len(listed))
        rows = np.array(c["merges"], dtype=np.uint32).reshape(-1, 3)
        if merges and len(rows):
            assert len(rows) <= n_old + n_new                                       # (room for n_old + n_new records was handed)
            ctypes.memmove(merges, rows.ctypes.data, rows.nbytes)
        n_merges._obj.value, n_clusters._obj.value, n_edges._obj.value = len(rows), c["n_clusters"], c["n_edges"]
        return 0


# the chain of tests/test_gpu_cluster_levels.py: A = qxzqvwkj, B = qxzqvwkjxqzzvk, C = jxqzzvk; J(A, B) = 8 / 16,
# J(B, C) = 6 / 17 (352.9 per mille), J(A, C) = 0; 17 stands alone, 99 is absent.  B arrives: A and C were apart.
A, B, C_ = 5001, 5002, 5003
CHAIN = [(A, B, 500), (B, C_, 352)]
CANNED = dict(label_of={A: A, B: A, C_: A, 17: 17}, merges=CHAIN, n_clusters=2, n_edges=2)


def _stubbed():
    m = RawMap()
    m._real, m._lib = m._lib, _StubLib(CANNED)
    return m


def _unstub(m):
    m._lib = m._real
    m.close()


def test_cluster_tree_extend_hands_every_pointer_and_shapes_the_outputs():
    m = _stubbed()
    old, new = [C_, 17, A, 99, C_], [B, 99]
    held = [(17, A, 250)]
    labels_old, labels_new, merges, n_clusters, n_edges = m.cluster_tree_extend(old, held, new, 300)
    call = m._lib.calls[-1]
    assert all(call[k] for k in ("old", "new", "held", "labels_old", "labels_new", "merges"))
    assert (call["n_old"], call["n_new"], call["n_held"], call["mp"]) == (5, 2, 1, 300)
    assert (call["olds"], call["news"], call["records"]) == (old, new, [list(held[0])])
    assert labels_old.dtype == np.uint32 and labels_old.tolist() == [A, 17, A, NO, A]
    assert labels_new.dtype == np.uint32 and labels_new.tolist() == [A, NO]
    assert merges.dtype == np.uint32 and merges.shape == (2, 3) and merges.tolist() == [list(e) for e in CHAIN]
    assert (n_clusters, n_edges) == (2, 2) and isinstance(n_clusters, int) and isinstance(n_edges, int)
    # arrays of the right type go as they are; an empty list hands no pointer
    got = m.cluster_tree_extend(np.array(old, dtype=np.uint32), np.array(held, dtype=np.uint32), np.array(new, dtype=np.uint32), 0)
    assert got[0].tolist() == [A, 17, A, NO, A] and m._lib.calls[-1]["records"] == [list(held[0])]
    got = m.cluster_tree_extend(old, [], new, 0)
    last = m._lib.calls[-1]
    assert not last["held"] and last["n_held"] == 0 and last["old"] and last["new"] and last["merges"]
    got = m.cluster_tree_extend([], np.zeros((0, 3), dtype=np.uint32), [A, B, C_], 0)
    last = m._lib.calls[-1]
    assert not last["old"] and not last["labels_old"] and not last["held"] and last["new"] and last["merges"]
    assert got[0].shape == (0,) and got[1].tolist() == [A, A, A] and got[2].shape == (2, 3)
    m._lib.canned = dict(label_of={}, merges=[], n_clusters=0, n_edges=0)
    out = m.cluster_tree_extend([], [], [], 1000)
    last = m._lib.calls[-1]
    assert (last["n_old"], last["n_new"], last["n_held"]) == (0, 0, 0)
    assert not any(last[k] for k in ("old", "new", "held", "labels_old", "labels_new", "merges"))
    assert out[0].shape == (0,) and out[1].shape == (0,) and out[0].dtype == out[1].dtype == np.uint32
    assert out[2].shape == (0, 3) and out[2].dtype == np.uint32 and out[3:] == (0, 0)
    _unstub(m)


def test_tree_changes_on_hand_made_records():
    none = np.zeros((0, 3), dtype=np.uint32)
    # nothing changed (the records in any order, a list or an array)
    removed, added = RawMap.tree_changes(CHAIN, CHAIN[::-1])
    assert removed.dtype == added.dtype == np.uint32 and removed.shape == added.shape == (0, 3)
    removed, added = RawMap.tree_changes(np.array(CHAIN, dtype=np.uint32), np.array(CHAIN, dtype=np.uint32))
    assert removed.shape == added.shape == (0, 3)
    # one displaced: N = 6000 arrives closer to both ends of (A, B)
    now = [(B, 6000, 800), (A, 6000, 700), (B, C_, 352)]
    removed, added = RawMap.tree_changes(CHAIN, now)
    assert removed.tolist() == [[A, B, 500]] and added.tolist() == [[B, 6000, 800], [A, 6000, 700]]
    # the rows are compared whole: a height that moved is one record out and one in
    removed, added = RawMap.tree_changes(CHAIN, [(A, B, 501), (B, C_, 352)])
    assert removed.tolist() == [[A, B, 500]] and added.tolist() == [[A, B, 501]]
    # everything new, everything gone, nothing at all
    removed, added = RawMap.tree_changes([], now)
    assert removed.shape == (0, 3) and added.tolist() == [[B, 6000, 800], [A, 6000, 700], [B, C_, 352]]   # (the tree's order)
    removed, added = RawMap.tree_changes(now, none)
    assert added.shape == (0, 3) and removed.tolist() == [[B, 6000, 800], [A, 6000, 700], [B, C_, 352]]
    removed, added = RawMap.tree_changes([], [])
    assert removed.shape == added.shape == (0, 3) and removed.dtype == np.uint32
    # the order among equal heights: a, then b
    removed, added = RawMap.tree_changes([], [(2, 9, 400), (1, 7, 400), (1, 3, 400), (5, 6, 1000)])
    assert added.tolist() == [[5, 6, 1000], [1, 3, 400], [1, 7, 400], [2, 9, 400]]
    with pytest.raises(ValueError):
        RawMap.tree_changes([(1, 2)], [])
    with pytest.raises(OverflowError):
        RawMap.tree_changes([(1, 2, -1)], [])


_WORDS = {}


def words_case():
    if not _WORDS:
        kind, n, _ = ORACLE_CASES[0]
        hay, off, _ = oracle_case_inputs(kind, n)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        listed = np.arange(1, n + 1, dtype=np.uint32)
        _WORDS.update(truth=Truth(held), listed=listed, old=listed[listed % 7 != 0], new=listed[listed % 7 == 0])
    return _WORDS


def test_the_forest_of_the_old_tree_and_the_edges_with_a_new_end_is_the_forest_of_all_edges():
    c = words_case()
    truth, listed, old, new = c["truth"], c["listed"], c["old"], c["new"]
    displaced = 0
    for floor in (200, 300, 500, 1000):
        held = TT.kruskal(truth, old, floor, 200)
        want = TT.kruskal(truth, listed, floor, 200)
        got = TreeExtendTruth(truth, old, held, new, floor, 200)
        assert got.records.dtype == np.uint32 and got.records.tobytes() == want.tobytes(), floor
        labels, n_clusters, n_edges, _ = truth.cluster(np.concatenate([old, new]), floor, 200)
        assert np.concatenate([got.labels_old, got.labels_new]).tobytes() == labels.astype(np.uint32).tobytes()
        assert got.n_clusters == n_clusters and got.n_edges == n_edges - truth.cluster(old, floor, 200)[2]
        assert got.n_old_candidates == len(held)
        displaced += len(got.dropped)
        print(f"floor {floor}: {len(held)} old records, {len(got.dropped)} displaced, {len(want)} records in all, "
              f"{got.n_edges} edges with a new end")
    assert displaced >= 1, "no split displaces an old record: the test shows nothing"


def test_old_records_made_at_a_lower_floor_serve_a_call_at_a_higher_one():
    c = words_case()
    truth, listed, old, new = c["truth"], c["listed"], c["old"], c["new"]
    held = TT.kruskal(truth, old, 200, 200)
    got = TreeExtendTruth(truth, old, held, new, 500, 200)
    assert 0 < got.n_old_candidates < len(held)                                    # (records below the floor are passed over)
    assert got.records.tobytes() == TT.kruskal(truth, listed, 500, 200).tobytes()
    assert got.records.tobytes() == TreeExtendTruth(truth, old, TT.kruskal(truth, old, 500, 200), new, 500, 200).records.tobytes()
