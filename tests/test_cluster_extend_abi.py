"""Cluster extend, without a GPU: blurrily_storage_cluster_extend is exported with its argtypes set, its prototype agrees
with the reference's storage.h in one translation unit and alone, a drifted prototype does not compile, every argument
error is EINVAL before a GPU is asked for and leaves all four outputs as they were, valid calls fail loudly (ENODEV)
where no GPU is usable, and the Python surface checks its arguments, hands the right pointers and shapes canned
arrays rightly (cluster_changes is numpy alone)."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

from blurrily_amd import Map, RawMap, _native
from helpers import compile_c, einval, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster_extend.c")
NO = _native.NO_CLUSTER


def test_the_cluster_extend_symbol_is_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert " T blurrily_storage_cluster_extend\n" in out
    fn = lib.blurrily_storage_cluster_extend
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 11
    assert "blurrily_storage_cluster_extend" in _native.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "blurrily_storage.h")).read()
    assert "int blurrily_storage_cluster_extend(trigram_map haystack, const uint32_t* old_refs," in header


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_cluster_extend_prototype_compiles_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_extend_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("was,now", [("const uint32_t*, const uint32_t*, size_t, const uint32_t*, size_t, uint32_t,",
                                      "const uint32_t*, size_t, const uint32_t*, size_t, uint32_t,"),
                                     ("uint32_t*, uint32_t*, uint32_t*, uint64_t*) =",
                                      "uint32_t*, uint32_t*, uint32_t*, uint32_t*) ="),
                                     ("uint32_t*, uint32_t*, uint32_t*, uint64_t*) =",
                                      "uint32_t*, uint32_t*, uint64_t*) ="),
                                     ("const uint32_t*, size_t, uint32_t,", "const uint32_t*, uint32_t, uint32_t,")],
                         ids=["no_old_labels", "edges_as_a_word", "one_label_array", "n_new_as_a_word"])
def test_a_drifted_cluster_extend_prototype_does_not_compile(tmp_path, was, now):
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
    old, seeds, new = (np.array(x, dtype=np.uint32) for x in ([1, 2], [1, 1], [3]))
    labels_old, labels_new = np.full(2, 7, dtype=np.uint32), np.full(1, 7, dtype=np.uint32)
    n_clusters, n_edges = ctypes.c_uint32(7), ctypes.c_uint64(7)
    counts = (ctypes.byref(n_clusters), ctypes.byref(n_edges))
    call = lib.blurrily_storage_cluster_extend
    o, s, w, lo, ln = (a.ctypes.data for a in (old, seeds, new, labels_old, labels_new))
    einval(lambda: call(None, o, s, 2, w, 1, 500, lo, ln, *counts))                  # no map
    einval(lambda: call(m.handle, o, s, 2, w, 1, 1001, lo, ln, *counts))             # min_permille > 1000
    einval(lambda: call(m.handle, None, None, 0, None, 0, 1001, None, None, *counts))   # ... with nothing listed too
    einval(lambda: call(m.handle, None, s, 2, w, 1, 500, lo, ln, *counts))           # old_refs NULL, n_old > 0
    einval(lambda: call(m.handle, o, None, 2, w, 1, 500, lo, ln, *counts))           # old_labels NULL, n_old > 0
    einval(lambda: call(m.handle, o, s, 2, w, 1, 500, None, ln, *counts))            # labels_old NULL, n_old > 0
    einval(lambda: call(m.handle, o, s, 2, None, 1, 500, lo, ln, *counts))           # new_refs NULL, n_new > 0
    einval(lambda: call(m.handle, o, s, 2, w, 1, 500, lo, None, *counts))            # labels_new NULL, n_new > 0
    einval(lambda: call(m.handle, o, s, 0xFFFFFFF0, w, 1, 500, lo, ln, *counts))     # the two together: more than a call takes
    einval(lambda: call(m.handle, o, s, 2, w, 0xFFFFFFEF, 500, lo, ln, *counts))
    einval(lambda: call(m.handle, o, s, 0xFFFFFFF1, None, 0, 500, lo, None, *counts))
    einval(lambda: call(m.handle, None, None, 0, w, 0xFFFFFFF1, 500, None, ln, *counts))
    einval(lambda: call(m.handle, o, s, 2**64 - 1, w, 2, 500, lo, ln, *counts))      # (a sum that wraps round)
    einval(lambda: call(m.handle, o, s, 2, w, 1, 1001, lo, ln, None, None))          # the counts are optional
    assert n_clusters.value == 7 and n_edges.value == 7                              # nothing written
    assert (labels_old == 7).all() and (labels_new == 7).all()
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster_extend.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    old, seeds, new = (np.array(x, dtype=np.uint32) for x in ([1, 2], [1, 1], [3]))
    labels_old, labels_new = np.zeros(2, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    n_clusters, n_edges = ctypes.c_uint32(0), ctypes.c_uint64(0)
    call = lib.blurrily_storage_cluster_extend
    o, s, w, lo, ln = (a.ctypes.data for a in (old, seeds, new, labels_old, labels_new))
    for one in (lambda: call(m.handle, o, s, 2, w, 1, 500, lo, ln, ctypes.byref(n_clusters), ctypes.byref(n_edges)),
                lambda: call(m.handle, o, s, 2, w, 1, 0, lo, ln, None, None),
                lambda: call(m.handle, o, s, 2, None, 0, 1000, lo, None, None, None),
                lambda: call(m.handle, None, None, 0, w, 1, 500, None, ln, None, None),
                lambda: call(m.handle, None, None, 0, None, 0, 500, None, None, None, None)):
        ctypes.set_errno(0)
        assert one() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for one in (lambda: m.cluster_extend([1, 2], [1, 1], [3], 700), lambda: m.cluster_extend([], [], [], 0)):
        with pytest.raises(OSError) as e:
            one()
        assert e.value.errno == errno.ENODEV
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    with pytest.raises(ValueError):
        m.cluster_extend([1], [1], [2], 1001)
    with pytest.raises(OverflowError):
        m.cluster_extend([1], [1], [2], -1)
    with pytest.raises(OverflowError):
        m.cluster_extend([-1], [1], [2], 500)
    with pytest.raises(OverflowError):
        m.cluster_extend([1], [1 << 32], [2], 500)
    with pytest.raises(OverflowError):
        m.cluster_extend([1], [1], [-2], 500)
    with pytest.raises(ValueError):
        m.cluster_extend([[1, 2]], [1], [2], 500)
    with pytest.raises(ValueError):
        m.cluster_extend([1, 2], [1], [3], 500)                   # a label per old reference
    with pytest.raises(ValueError):
        m.cluster_changes([1, 2], [1], [1, 1])
    m.close()
    with pytest.raises(RawMap.ClosedError):
        m.cluster_extend([1], [1], [2], 500)


class _StubLib:
    """Stands where the library stands in a RawMap: records what blurrily_storage_cluster_extend is handed and fills
    the outputs from canned arrays (no GPU is asked for)."""

    def __init__(self, canned):
        self.canned, self.calls = canned, []

    def blurrily_storage_cluster_extend(self, handle, old, seeds, n_old, new, n_new, mp, labels_old, labels_new,
                                        n_clusters, n_edges):
        u32 = ctypes.POINTER(ctypes.c_uint32)
        seen = lambda p, n: np.ctypeslib.as_array(ctypes.cast(p, u32), shape=(n,)).tolist() if n else []
        self.calls.append(dict(old=old, seeds=seeds, n_old=n_old, new=new, n_new=n_new, mp=mp, labels_old=labels_old,
                               labels_new=labels_new, listed_old=seen(old, n_old), listed_seeds=seen(seeds, n_old),
                               listed_new=seen(new, n_new)))
        c = self.canned
        for ptr, refs in ((labels_old, self.calls[-1]["listed_old"]), (labels_new, self.calls[-1]["listed_new"])):
            if ptr:
                out = np.array([c["label_of"].get(r, NO) for r in refs], dtype=np.uint32)
                ctypes.memmove(ptr, out.ctypes.data, 4 * len(refs))
        n_clusters._obj.value, n_edges._obj.value = c["n_clusters"], c["n_edges"]
        return 0


# old groups {10, 11}, {14, 15} and 17 alone; the new 12 joins the two groups, the new 20 stands alone, 99 is absent
CANNED = dict(label_of={10: 10, 11: 10, 14: 10, 15: 10, 17: 17, 12: 10, 20: 20}, n_clusters=3, n_edges=2)
OLD, SEEDS, NEW = [10, 11, 14, 15, 17, 99], [10, 10, 14, 14, 17, NO], [12, 20]


def _stubbed():
    m = RawMap()
    m._real, m._lib = m._lib, _StubLib(CANNED)
    return m


def _unstub(m):
    m._lib = m._real
    m.close()


def test_cluster_extend_hands_every_pointer_and_shapes_the_outputs():
    m = _stubbed()
    labels_old, labels_new, n_clusters, n_edges = m.cluster_extend(OLD, SEEDS, NEW, 700)
    call = m._lib.calls[-1]
    assert all(call[k] for k in ("old", "seeds", "new", "labels_old", "labels_new"))
    assert (call["n_old"], call["n_new"], call["mp"]) == (6, 2, 700)
    assert (call["listed_old"], call["listed_seeds"], call["listed_new"]) == (OLD, SEEDS, NEW)
    assert labels_old.dtype == labels_new.dtype == np.uint32
    assert labels_old.tolist() == [10, 10, 10, 10, 17, NO] and labels_new.tolist() == [10, 20]
    assert (n_clusters, n_edges) == (3, 2)
    # an empty side hands no pointer for it
    out = m.cluster_extend([], [], NEW, 0)
    last = m._lib.calls[-1]
    assert last["n_old"] == 0 and not any(last[k] for k in ("old", "seeds", "labels_old")) and last["new"]
    assert out[0].shape == (0,) and out[1].tolist() == [10, 20]
    out = m.cluster_extend(np.array(OLD, dtype=np.uint32), np.array(SEEDS, dtype=np.uint32), [], 1000)
    last = m._lib.calls[-1]
    assert last["n_new"] == 0 and not any(last[k] for k in ("new", "labels_new")) and last["old"]
    assert out[1].shape == (0,) and out[0].tolist() == [10, 10, 10, 10, 17, NO]
    _unstub(m)


def test_cluster_changes_gives_the_old_references_whose_label_moved():
    m = _stubbed()
    labels_old, _, _, _ = m.cluster_extend(OLD, SEEDS, NEW, 700)
    moved, now = m.cluster_changes(OLD, SEEDS, labels_old)
    assert moved.dtype == now.dtype == np.uint32
    assert (moved.tolist(), now.tolist()) == ([14, 15], [10, 10])
    moved, now = m.cluster_changes(OLD, labels_old, labels_old)
    assert (moved.tolist(), now.tolist()) == ([], [])
    moved, now = m.cluster_changes([], [], [])
    assert (moved.shape, now.shape) == ((0,), (0,))
    _unstub(m)
