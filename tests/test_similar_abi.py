"""Similarity find, without a GPU: blurrily_storage_find_batch_similar, _find_similar and _find_references_similar
are exported with their argtypes set, their prototypes agree with the reference's storage.h in one translation unit,
every argument error is EINVAL before a GPU is asked for, valid calls fail loudly (ENODEV) where no GPU is usable, and
the Python surface checks its arguments."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

from blurrily_amd import Map, RawMap, _native
from helpers import compile_c, einval, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"blurrily_storage_find_batch_similar": 9, "blurrily_storage_find_similar": 6,
       "blurrily_storage_find_references_similar": 9}
SRC = os.path.join(ROOT, "tests", "c", "header_compat_similar.c")


def test_the_similar_symbols_are_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for sym, n_args in NEW.items():
        assert f" T {sym}\n" in out, sym
        fn = getattr(lib, sym)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args, sym
        assert sym in _native.EXPORTED_SYMBOLS


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_similar_prototypes_compile_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "similar_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


def test_a_drifted_similar_prototype_does_not_compile(tmp_path):
    write_recorded_storage_h(tmp_path)
    text = open(SRC).read()
    drifted = text.replace("uint16_t, uint32_t, trigram_match, uint32_t*) =\n      blurrily_storage_find_similar",
                           "uint32_t, uint32_t, trigram_match, uint32_t*) =\n      blurrily_storage_find_similar")
    assert drifted != text
    src = tmp_path / "drifted.c"
    src.write_text(drifted)
    assert compile_c(tmp_path, src).returncode != 0


def test_argument_errors_are_einval_before_any_gpu():
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    packed = b"san jose"
    offs = np.array([0, len(packed)], dtype=np.uint64)
    rows = np.zeros((16, 3), dtype=np.uint32)
    counts = np.zeros(1, dtype=np.uint32)
    ntri = np.zeros(16, dtype=np.uint32)
    refs = np.array([1], dtype=np.uint32)
    batch = lib.blurrily_storage_find_batch_similar
    by_ref = lib.blurrily_storage_find_references_similar
    # min_permille > 1000
    einval(lambda: batch(m.handle, packed, offs.ctypes.data, 1, 10, 1001, rows.ctypes.data, counts.ctypes.data, None))
    einval(lambda: lib.blurrily_storage_find_similar(m.handle, b"san jose", 10, 1001, rows.ctypes.data, None))
    einval(lambda: by_ref(m.handle, refs.ctypes.data, 1, 10, 1001, rows.ctypes.data, counts.ctypes.data, None, None))
    # counts NULL (with n == 0 too)
    einval(lambda: batch(m.handle, packed, offs.ctypes.data, 1, 10, 500, rows.ctypes.data, None, None))
    einval(lambda: batch(m.handle, None, None, 0, 10, 500, None, None, None))
    einval(lambda: by_ref(m.handle, refs.ctypes.data, 1, 10, 500, rows.ctypes.data, None, None, None))
    # results NULL with limit > 0 and n > 0
    einval(lambda: batch(m.handle, packed, offs.ctypes.data, 1, 10, 500, None, counts.ctypes.data, None))
    einval(lambda: lib.blurrily_storage_find_similar(m.handle, b"san jose", 10, 500, None, None))
    einval(lambda: by_ref(m.handle, refs.ctypes.data, 1, 10, 500, None, counts.ctypes.data, None, None))
    # packed or offsets NULL with n > 0; references NULL with n > 0; no needle; no map
    einval(lambda: batch(m.handle, None, offs.ctypes.data, 1, 10, 500, rows.ctypes.data, counts.ctypes.data, None))
    einval(lambda: batch(m.handle, packed, None, 1, 10, 500, rows.ctypes.data, counts.ctypes.data, None))
    einval(lambda: by_ref(m.handle, None, 1, 10, 500, rows.ctypes.data, counts.ctypes.data, None, None))
    einval(lambda: lib.blurrily_storage_find_similar(m.handle, None, 10, 500, rows.ctypes.data, None))
    einval(lambda: batch(None, packed, offs.ctypes.data, 1, 10, 500, rows.ctypes.data, counts.ctypes.data, None))
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    with pytest.raises(ValueError):
        m.find_similar("san jose", 10, 1001)
    with pytest.raises(ValueError):
        m.find_batch_similar(["san jose"], 10, 1001)
    with pytest.raises(ValueError):
        m.find_batch_by_reference_similar([1], 10, 1001)
    with pytest.raises(ValueError):
        m.find_batch_similar_packed(b"san jose", np.array([0, 8], dtype=np.uint64), 10, 5000)
    with pytest.raises(OverflowError):
        m.find_similar("san jose", 10, -1)
    with pytest.raises(OverflowError):
        m.find_similar("san jose", 1 << 40, 0)
    with pytest.raises(OverflowError):
        m.find_batch_by_reference_similar([-1], 10, 0)
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_similar.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    packed = b"san jose"
    offs = np.array([0, len(packed)], dtype=np.uint64)
    rows = np.zeros((16, 3), dtype=np.uint32)
    counts = np.zeros(1, dtype=np.uint32)
    refs = np.array([1], dtype=np.uint32)
    for call in (lambda: lib.blurrily_storage_find_batch_similar(m.handle, packed, offs.ctypes.data, 1, 10, 500,
                                                                 rows.ctypes.data, counts.ctypes.data, None),
                 lambda: lib.blurrily_storage_find_batch_similar(m.handle, packed, offs.ctypes.data, 1, 0, 500,
                                                                 None, counts.ctypes.data, None),
                 lambda: lib.blurrily_storage_find_batch_similar(m.handle, None, None, 0, 10, 500, None,
                                                                 counts.ctypes.data, None),
                 lambda: lib.blurrily_storage_find_references_similar(m.handle, refs.ctypes.data, 1, 10, 500,
                                                                      rows.ctypes.data, counts.ctypes.data, None, None),
                 lambda: lib.blurrily_storage_find_similar(m.handle, b"san jose", 10, 500, rows.ctypes.data, None)):
        ctypes.set_errno(0)
        assert call() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for call in (lambda: m.find_similar(b"san jose", 10, 700), lambda: m.find_batch_by_reference_similar([1], 10, 700),
                 lambda: m.find_batch_similar_packed(packed, offs, 10, 0)):
        with pytest.raises(OSError) as e:
            call()
        assert e.value.errno == errno.ENODEV
    m.close()
