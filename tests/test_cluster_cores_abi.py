"""Cluster cores, without a GPU: blurrily_storage_cluster_cores is exported with its argtypes set, its prototype agrees
with the reference's storage.h in one translation unit, every argument error is EINVAL before a GPU is asked for and
leaves all six outputs as they were, valid calls fail loudly (ENODEV) where no GPU is usable, and the Python surface
checks its arguments and shapes canned arrays rightly."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

from blurrily_amd import Map, RawMap, _native
from helpers import compile_c, einval, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster_cores.c")
NO = _native.NO_CLUSTER


def test_the_cluster_cores_symbol_is_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert " T blurrily_storage_cluster_cores\n" in out
    fn = lib.blurrily_storage_cluster_cores
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 11
    assert "blurrily_storage_cluster_cores" in _native.EXPORTED_SYMBOLS
    assert (_native.KIND_NONE, _native.KIND_NOISE, _native.KIND_BORDER, _native.KIND_CORE) == (0, 1, 2, 3)
    header = open(os.path.join(ROOT, "include", "blurrily_storage.h")).read()
    for name, value in (("NONE", 0), ("NOISE", 1), ("BORDER", 2), ("CORE", 3)):
        assert f"#define BLURRILY_KIND_{name:<6} {value}\n" in header


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_cluster_cores_prototype_compiles_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_cores_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("was,now", [("uint32_t*, uint32_t*, uint8_t*,", "uint32_t*, uint32_t*, uint32_t*,"),
                                     ("uint32_t*, uint64_t*, uint64_t*) =", "uint32_t*, uint64_t*, uint32_t*) ="),
                                     ("size_t, uint32_t, uint32_t, uint32_t*,", "size_t, uint32_t, uint32_t*,")],
                         ids=["kinds_as_words", "core_edges_as_a_word", "no_min_degree"])
def test_a_drifted_cluster_cores_prototype_does_not_compile(tmp_path, was, now):
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
    refs = np.array([1, 2], dtype=np.uint32)
    labels, degrees = (np.full(2, 7, dtype=np.uint32) for _ in range(2))
    kinds = np.full(2, 7, dtype=np.uint8)
    n_clusters, n_edges, n_core_edges = ctypes.c_uint32(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    out = (degrees.ctypes.data, kinds.ctypes.data, ctypes.byref(n_clusters), ctypes.byref(n_edges),
           ctypes.byref(n_core_edges))
    cores_call = lib.blurrily_storage_cluster_cores
    einval(lambda: cores_call(None, refs.ctypes.data, 2, 500, 3, labels.ctypes.data, *out))          # no map
    einval(lambda: cores_call(m.handle, refs.ctypes.data, 2, 1001, 3, labels.ctypes.data, *out))     # min_permille > 1000
    einval(lambda: cores_call(m.handle, None, 0, 1001, 0, None, *out))                               # ... with n == 0 too
    einval(lambda: cores_call(m.handle, None, 2, 500, 3, labels.ctypes.data, *out))                  # references NULL, n > 0
    einval(lambda: cores_call(m.handle, refs.ctypes.data, 2, 500, 3, None, *out))                    # labels NULL, n > 0
    einval(lambda: cores_call(m.handle, refs.ctypes.data, 0xFFFFFFF1, 500, 3, labels.ctypes.data, *out))   # more than a call takes
    einval(lambda: cores_call(m.handle, refs.ctypes.data, 2, 1001, 0xFFFFFFFF, labels.ctypes.data, None, None, None, None,
                              None))
    assert n_clusters.value == 7 and n_edges.value == 7 and n_core_edges.value == 7                  # nothing written
    assert (labels == 7).all() and (degrees == 7).all() and (kinds == 7).all()
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster_cores.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs = np.array([1, 2], dtype=np.uint32)
    labels, degrees = (np.zeros(2, dtype=np.uint32) for _ in range(2))
    kinds = np.zeros(2, dtype=np.uint8)
    n_clusters, n_edges, n_core_edges = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    call = lib.blurrily_storage_cluster_cores
    for one in (lambda: call(m.handle, refs.ctypes.data, 2, 500, 3, labels.ctypes.data, degrees.ctypes.data,
                             kinds.ctypes.data, ctypes.byref(n_clusters), ctypes.byref(n_edges),
                             ctypes.byref(n_core_edges)),
                lambda: call(m.handle, refs.ctypes.data, 2, 0, 0, labels.ctypes.data, None, None, None, None, None),
                lambda: call(m.handle, refs.ctypes.data, 1, 1000, 0xFFFFFFFF, labels.ctypes.data, None,
                             kinds.ctypes.data, None, None, None),
                lambda: call(m.handle, None, 0, 500, 3, None, None, None, None, None, None)):
        ctypes.set_errno(0)
        assert one() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for one in (lambda: m.cluster_cores([1, 2], 700, 3), lambda: m.cluster_cores([], 0, 0),
                lambda: m.dense_duplicates(refs, 500, 2)):
        with pytest.raises(OSError) as e:
            one()
        assert e.value.errno == errno.ENODEV
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    for method in (m.cluster_cores, m.dense_duplicates):
        with pytest.raises(ValueError):
            method([1], 1001, 3)
        with pytest.raises(OverflowError):
            method([1], -1, 3)
        with pytest.raises(OverflowError):
            method([1], 500, -1)
        with pytest.raises(OverflowError):
            method([1], 500, 1 << 32)
        with pytest.raises(OverflowError):
            method([-1], 500, 3)
        with pytest.raises(OverflowError):
            method([1 << 32], 500, 3)
        with pytest.raises(ValueError):
            method([[1, 2]], 500, 3)
    m.close()
    with pytest.raises(RawMap.ClosedError):
        m.cluster_cores([1], 500, 3)


class _StubLib:
    """Stands where the library stands in a RawMap: records what blurrily_storage_cluster_cores is handed and fills the
    outputs from canned arrays (no GPU is asked for)."""

    def __init__(self, canned):
        self.canned, self.calls = canned, []

    def blurrily_storage_cluster_cores(self, handle, refs, n, mp, md, labels, degrees, kinds, n_clusters, n_edges,
                                       n_core_edges):
        self.calls.append(dict(refs=refs, n=n, mp=mp, md=md, labels=labels, degrees=degrees, kinds=kinds))
        seen = np.ctypeslib.as_array(ctypes.cast(refs, ctypes.POINTER(ctypes.c_uint32)), shape=(n,)) if n else np.zeros(0)
        self.calls[-1]["listed"] = seen.tolist()
        of = {r: k for k, r in enumerate(LISTED)}                 # (the canned answers belong to LISTED's references)
        at = [of[int(r)] for r in seen.tolist()]
        c = self.canned
        for ptr, key, ctype in ((labels, "labels", ctypes.c_uint32), (degrees, "degrees", ctypes.c_uint32),
                                (kinds, "kinds", ctypes.c_uint8)):
            if ptr:
                ctypes.memmove(ptr, np.ascontiguousarray(np.array(c[key])[at], dtype=ctype).ctypes.data,
                               n * ctypes.sizeof(ctype))
        n_clusters._obj.value, n_edges._obj.value, n_core_edges._obj.value = c["n_clusters"], c["n_edges"], c["n_core_edges"]
        return 0


# references 10 .. 18 and an absent 99 at min_degree 2: two triangles {10, 11, 12} and {14, 15, 16}, a pendant 13 on 12
# (degree 1: a border), a pair 17 - 18 below min_degree (noise)
CANNED = dict(labels=[10, 10, 10, 10, 14, 14, 14, 17, 18, NO], degrees=[2, 2, 3, 1, 2, 2, 2, 1, 1, 0],
              kinds=[3, 3, 3, 2, 3, 3, 3, 1, 1, 0], n_clusters=2, n_edges=8, n_core_edges=6)
LISTED = [10, 11, 12, 13, 14, 15, 16, 17, 18, 99]


def _stubbed():
    m = RawMap()
    m._real, m._lib = m._lib, _StubLib(CANNED)
    return m


def _unstub(m):
    m._lib = m._real
    m.close()


def test_cluster_cores_hands_every_pointer_and_shapes_the_outputs():
    m = _stubbed()
    labels, degrees, kinds, n_clusters, n_edges, n_core_edges = m.cluster_cores(LISTED, 700, 2)
    call = m._lib.calls[-1]
    assert all(call[k] for k in ("refs", "labels", "degrees", "kinds"))
    assert (call["n"], call["mp"], call["md"], call["listed"]) == (10, 700, 2, LISTED)
    assert [a.dtype for a in (labels, degrees, kinds)] == [np.uint32, np.uint32, np.uint8]
    assert (labels.tolist(), degrees.tolist(), kinds.tolist()) == (CANNED["labels"], CANNED["degrees"], CANNED["kinds"])
    assert (n_clusters, n_edges, n_core_edges) == (2, 8, 6)
    empty = m.cluster_cores([], 0, 0)                             # nothing listed: no pointer is handed
    last = m._lib.calls[-1]
    assert last["n"] == 0 and not any(last[k] for k in ("refs", "labels", "degrees", "kinds"))
    assert [len(a) for a in empty[:3]] == [0, 0, 0]
    m.cluster_cores([10], 0, 0xFFFFFFFF)                          # min_degree is a whole unsigned word
    assert m._lib.calls[-1]["md"] == 0xFFFFFFFF
    _unstub(m)


def test_dense_duplicates_over_canned_arrays():
    m = _stubbed()
    want = [[10, 11, 12, 13], [14, 15, 16]]                       # cores and the border, ascending; noise and absent left out
    assert m.dense_duplicates(LISTED, 700, 2) == want
    assert (m._lib.calls[-1]["mp"], m._lib.calls[-1]["md"]) == (700, 2)
    # a list with repeats and out of order gives the same lists
    assert m.dense_duplicates(LISTED[::-1] + [12, 10, 13], 700, 2) == want
    assert m.dense_duplicates([17, 18, 99], 700, 2) == []         # noise only
    assert m.dense_duplicates([], 700, 2) == []
    _unstub(m)
