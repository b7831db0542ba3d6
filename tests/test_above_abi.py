"""Threshold find, without a GPU: blurrily_storage_find_batch_above, _find_above and _find_references_above are
exported with their argtypes set, their prototypes agree with the reference's storage.h in one translation unit, every
argument error is EINVAL before a GPU is asked for, valid calls fail loudly (ENODEV) where no GPU is usable, and the
Python surface raises accordingly."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

from blurrily_amd import Map, RawMap, _native
from helpers import compile_c, einval, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"blurrily_storage_find_batch_above": 9, "blurrily_storage_find_above": 7,
       "blurrily_storage_find_references_above": 9}
SRC = os.path.join(ROOT, "tests", "c", "header_compat_above.c")


def test_the_above_symbols_are_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for sym, n_args in NEW.items():
        assert f" T {sym}\n" in out, sym
        fn = getattr(lib, sym)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args, sym
        assert sym in _native.EXPORTED_SYMBOLS


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_above_prototypes_compile_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "above_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


def test_a_drifted_above_prototype_does_not_compile(tmp_path):
    write_recorded_storage_h(tmp_path)
    text = open(SRC).read()
    drifted = text.replace("uint32_t, trigram_match, uint64_t, uint64_t*) =\n      blurrily_storage_find_above",
                           "uint32_t, trigram_match, uint64_t, uint32_t*) =\n      blurrily_storage_find_above")
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
    row_off = np.zeros(2, dtype=np.uint64)
    refs = np.array([1], dtype=np.uint32)
    total = ctypes.c_uint64(0)
    einval(lambda: lib.blurrily_storage_find_batch_above(m.handle, packed, offs.ctypes.data, 1, 0, 1001,
                                                          rows.ctypes.data, 16, row_off.ctypes.data))
    einval(lambda: lib.blurrily_storage_find_batch_above(m.handle, packed, offs.ctypes.data, 1, 0, 500,
                                                          rows.ctypes.data, 16, None))
    einval(lambda: lib.blurrily_storage_find_batch_above(m.handle, None, offs.ctypes.data, 1, 0, 500,
                                                          rows.ctypes.data, 16, row_off.ctypes.data))
    einval(lambda: lib.blurrily_storage_find_batch_above(m.handle, packed, None, 1, 0, 500,
                                                          rows.ctypes.data, 16, row_off.ctypes.data))
    einval(lambda: lib.blurrily_storage_find_batch_above(None, packed, offs.ctypes.data, 1, 0, 500,
                                                          rows.ctypes.data, 16, row_off.ctypes.data))
    einval(lambda: lib.blurrily_storage_find_above(m.handle, b"san jose", 0, 1001, rows.ctypes.data, 16,
                                                    ctypes.byref(total)))
    einval(lambda: lib.blurrily_storage_find_above(m.handle, None, 0, 500, rows.ctypes.data, 16, ctypes.byref(total)))
    einval(lambda: lib.blurrily_storage_find_references_above(m.handle, refs.ctypes.data, 1, 0, 1001,
                                                               rows.ctypes.data, 16, row_off.ctypes.data, None))
    einval(lambda: lib.blurrily_storage_find_references_above(m.handle, refs.ctypes.data, 1, 0, 500,
                                                               rows.ctypes.data, 16, None, None))
    einval(lambda: lib.blurrily_storage_find_references_above(m.handle, None, 1, 0, 500,
                                                               rows.ctypes.data, 16, row_off.ctypes.data, None))
    m.close()


def test_the_python_surface_checks_the_bar():
    m = Map()
    m.put("san jose", 1)
    with pytest.raises(ValueError):
        m.find_above("san jose", 0, 1001)
    with pytest.raises(ValueError):
        m.find_batch_above(["san jose"], 0, 1001)
    with pytest.raises(ValueError):
        m.find_batch_by_reference_above([1], 0, 1001)
    with pytest.raises(OverflowError):
        m.find_above("san jose", -1, 0)
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_above.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    packed = b"san jose"
    offs = np.array([0, len(packed)], dtype=np.uint64)
    row_off = np.zeros(2, dtype=np.uint64)
    refs = np.array([1], dtype=np.uint32)
    for call in (lambda: lib.blurrily_storage_find_batch_above(m.handle, packed, offs.ctypes.data, 1, 0, 500, None, 0,
                                                               row_off.ctypes.data),
                 lambda: lib.blurrily_storage_find_references_above(m.handle, refs.ctypes.data, 1, 0, 500, None, 0,
                                                                    row_off.ctypes.data, None),
                 lambda: lib.blurrily_storage_find_above(m.handle, b"san jose", 0, 500, None, 0, None)):
        ctypes.set_errno(0)
        assert call() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for call in (lambda: m.find_above(b"san jose", 0, 700), lambda: m.find_batch_by_reference_above([1], 0, 700),
                 lambda: m.find_batch_above_packed(packed, offs, 2, 0), lambda: m.join_above([1], 0, 800)):
        with pytest.raises(OSError) as e:
            call()
        assert e.value.errno == errno.ENODEV
    m.close()
