"""Cluster levels, without a GPU: blurrily_storage_cluster_levels is exported with its argtypes set, its prototype
agrees with the reference's storage.h in one translation unit, every argument error is EINVAL before a GPU is asked for
and leaves all three outputs as they were, valid calls fail loudly (ENODEV) where no GPU is usable, and the Python
surface checks its floors before any C call."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

from blurrily_amd import Map, RawMap, _native
from helpers import compile_c, einval, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster_levels.c")
CAP = 8


def test_the_cluster_levels_symbol_is_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert " T blurrily_storage_cluster_levels\n" in out
    fn = lib.blurrily_storage_cluster_levels
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 8
    assert "blurrily_storage_cluster_levels" in _native.EXPORTED_SYMBOLS
    assert _native.CLUSTER_MAX_LEVELS == CAP
    assert f"#define BLURRILY_CLUSTER_MAX_LEVELS {CAP}\n" in open(os.path.join(ROOT, "include", "blurrily_storage.h")).read()


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_cluster_levels_prototype_compiles_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_levels_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


def test_a_drifted_cluster_levels_prototype_does_not_compile(tmp_path):
    write_recorded_storage_h(tmp_path)
    text = open(SRC).read()
    drifted = text.replace("const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint64_t*) =",
                           "const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*) =")
    assert drifted != text
    src = tmp_path / "drifted.c"
    src.write_text(drifted)
    assert compile_c(tmp_path, src).returncode != 0


def test_argument_errors_are_einval_before_any_gpu_and_write_nothing():
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs = np.array([1, 2], dtype=np.uint32)
    labels = np.full(CAP * 2, 7, dtype=np.uint32)
    n_clusters, n_edges = np.full(CAP, 7, dtype=np.uint32), np.full(CAP, 7, dtype=np.uint64)
    out = (n_clusters.ctypes.data, n_edges.ctypes.data)
    levels = lib.blurrily_storage_cluster_levels

    def fl(*values):
        a = np.array(values, dtype=np.uint32)
        return a, a.ctypes.data

    good, p_good = fl(500, 700)
    nine, p_nine = fl(100, 200, 300, 400, 500, 600, 700, 800, 900)
    high, p_high = fl(500, 1001)
    same, p_same = fl(500, 500)
    down, p_down = fl(700, 500)
    einval(lambda: levels(None, refs.ctypes.data, 2, p_good, 2, labels.ctypes.data, *out))            # no map
    einval(lambda: levels(m.handle, refs.ctypes.data, 2, None, 2, labels.ctypes.data, *out))          # no floors
    einval(lambda: levels(m.handle, refs.ctypes.data, 2, p_good, 0, labels.ctypes.data, *out))        # n_floors 0
    einval(lambda: levels(m.handle, refs.ctypes.data, 2, p_nine, CAP + 1, labels.ctypes.data, *out))  # ... above the cap
    einval(lambda: levels(m.handle, refs.ctypes.data, 2, p_high, 2, labels.ctypes.data, *out))        # a floor above 1000
    einval(lambda: levels(m.handle, None, 0, p_high, 2, None, *out))                                  # ... with n == 0 too
    einval(lambda: levels(m.handle, refs.ctypes.data, 2, p_same, 2, labels.ctypes.data, *out))        # not strictly ascending
    einval(lambda: levels(m.handle, refs.ctypes.data, 2, p_down, 2, labels.ctypes.data, *out))        # descending
    einval(lambda: levels(m.handle, None, 2, p_good, 2, labels.ctypes.data, *out))                    # references NULL, n > 0
    einval(lambda: levels(m.handle, refs.ctypes.data, 2, p_good, 2, None, *out))                      # labels NULL, n > 0
    einval(lambda: levels(m.handle, refs.ctypes.data, 0xFFFFFFF1, p_good, 2, labels.ctypes.data, *out))   # more than a call takes
    einval(lambda: levels(m.handle, refs.ctypes.data, 2, p_down, 2, labels.ctypes.data, None, None))
    assert (n_clusters == 7).all() and (n_edges == 7).all() and (labels == 7).all()                   # nothing written
    del good, nine, high, same, down
    m.close()


def test_the_python_surface_checks_its_floors_before_any_c_call():
    m = Map()
    m.put("san jose", 1)
    for method in (m.cluster_levels, m.cluster_profile):
        for floors in ([], [500, 500], [700, 500], [500, 1001], list(range(100, 1000, 100))):
            with pytest.raises(ValueError):
                method([1], floors)
        with pytest.raises(OverflowError):
            method([1], [-1, 500])
        with pytest.raises(OverflowError):
            method([-1], [500])
        with pytest.raises(OverflowError):
            method([1 << 32], [500])
        with pytest.raises(ValueError):
            method([[1, 2]], [500])
    m.close()
    with pytest.raises(RawMap.ClosedError):
        m.cluster_levels([1], [500])


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster_levels.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs = np.array([1, 2], dtype=np.uint32)
    labels = np.zeros(CAP * 2, dtype=np.uint32)
    n_clusters, n_edges = np.zeros(CAP, dtype=np.uint32), np.zeros(CAP, dtype=np.uint64)
    eight = np.array([0, 1, 200, 300, 500, 700, 999, 1000], dtype=np.uint32)
    one = np.array([1000], dtype=np.uint32)
    levels = lib.blurrily_storage_cluster_levels
    for call in (lambda: levels(m.handle, refs.ctypes.data, 2, eight.ctypes.data, CAP, labels.ctypes.data,
                                n_clusters.ctypes.data, n_edges.ctypes.data),
                 lambda: levels(m.handle, refs.ctypes.data, 2, one.ctypes.data, 1, labels.ctypes.data, None, None),
                 lambda: levels(m.handle, None, 0, eight.ctypes.data, 3, None, None, None)):
        ctypes.set_errno(0)
        assert call() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for call in (lambda: m.cluster_levels([1, 2], [500, 700]), lambda: m.cluster_levels([], [0]),
                 lambda: m.cluster_profile(refs, (500, 700, 900))):
        with pytest.raises(OSError) as e:
            call()
        assert e.value.errno == errno.ENODEV
    m.close()
