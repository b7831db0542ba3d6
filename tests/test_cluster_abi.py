"""Clusters, without a GPU: blurrily_storage_cluster is exported with its argtypes set, its prototype agrees with the
reference's storage.h in one translation unit, every argument error is EINVAL before a GPU is asked for, valid calls
fail loudly (ENODEV) where no GPU is usable, and the Python surface checks its arguments."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

from blurrily_amd import Map, RawMap, _native
from helpers import compile_c, einval, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster.c")


def test_the_cluster_symbol_is_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert " T blurrily_storage_cluster\n" in out
    fn = lib.blurrily_storage_cluster
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 7
    assert "blurrily_storage_cluster" in _native.EXPORTED_SYMBOLS
    assert _native.NO_CLUSTER == 0xFFFFFFFF
    assert "#define BLURRILY_NO_CLUSTER 0xFFFFFFFFu" in open(os.path.join(ROOT, "include", "blurrily_storage.h")).read()


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_cluster_prototype_compiles_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


def test_a_drifted_cluster_prototype_does_not_compile(tmp_path):
    write_recorded_storage_h(tmp_path)
    text = open(SRC).read()
    drifted = text.replace("size_t, uint32_t, uint32_t*, uint32_t*, uint64_t*) =",
                           "size_t, uint32_t, uint32_t*, uint32_t*, uint32_t*) =")
    assert drifted != text
    src = tmp_path / "drifted.c"
    src.write_text(drifted)
    assert compile_c(tmp_path, src).returncode != 0


def test_argument_errors_are_einval_before_any_gpu():
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs = np.array([1, 2], dtype=np.uint32)
    labels = np.zeros(2, dtype=np.uint32)
    n_clusters, n_edges = ctypes.c_uint32(7), ctypes.c_uint64(7)
    cluster = lib.blurrily_storage_cluster
    out = (ctypes.byref(n_clusters), ctypes.byref(n_edges))
    einval(lambda: cluster(None, refs.ctypes.data, 2, 500, labels.ctypes.data, *out))       # no map
    einval(lambda: cluster(m.handle, refs.ctypes.data, 2, 1001, labels.ctypes.data, *out))  # min_permille > 1000
    einval(lambda: cluster(m.handle, None, 0, 1001, None, *out))                            # ... with n == 0 too
    einval(lambda: cluster(m.handle, None, 2, 500, labels.ctypes.data, *out))               # references NULL, n > 0
    einval(lambda: cluster(m.handle, refs.ctypes.data, 2, 500, None, *out))                 # labels NULL, n > 0
    einval(lambda: cluster(m.handle, refs.ctypes.data, 0xFFFFFFF1, 500, labels.ctypes.data, *out))   # more than a call takes
    einval(lambda: cluster(m.handle, refs.ctypes.data, 2, 1001, labels.ctypes.data, None, None))
    assert n_clusters.value == 7 and n_edges.value == 7 and not labels.any()                # nothing written
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    for method in (m.cluster, m.duplicates):
        with pytest.raises(ValueError):
            method([1], 1001)
        with pytest.raises(OverflowError):
            method([1], -1)
        with pytest.raises(OverflowError):
            method([-1], 500)
        with pytest.raises(OverflowError):
            method([1 << 32], 500)
        with pytest.raises(ValueError):
            method([[1, 2]], 500)
    m.close()
    with pytest.raises(RawMap.ClosedError):
        m.cluster([1], 500)


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs = np.array([1, 2], dtype=np.uint32)
    labels = np.zeros(2, dtype=np.uint32)
    n_clusters, n_edges = ctypes.c_uint32(0), ctypes.c_uint64(0)
    for call in (lambda: lib.blurrily_storage_cluster(m.handle, refs.ctypes.data, 2, 500, labels.ctypes.data,
                                                      ctypes.byref(n_clusters), ctypes.byref(n_edges)),
                 lambda: lib.blurrily_storage_cluster(m.handle, refs.ctypes.data, 2, 0, labels.ctypes.data, None, None),
                 lambda: lib.blurrily_storage_cluster(m.handle, refs.ctypes.data, 1, 1000, labels.ctypes.data, None, None),
                 lambda: lib.blurrily_storage_cluster(m.handle, None, 0, 500, None, None, None)):
        ctypes.set_errno(0)
        assert call() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for call in (lambda: m.cluster([1, 2], 700), lambda: m.cluster([], 0), lambda: m.duplicates(refs, 500)):
        with pytest.raises(OSError) as e:
            call()
        assert e.value.errno == errno.ENODEV
    m.close()
