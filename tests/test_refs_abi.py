"""By reference, without a GPU: blurrily_storage_get / _get_batch / _find_references / _find_references_device are
exported with their argtypes set, their prototypes agree with the reference's storage.h in one translation unit, they
fail loudly (ENODEV) where no GPU is usable, the Python surface checks its arguments, and the Ruby glue that binds them
passes the compiler's front end."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

from blurrily_amd import Map, RawMap, _native
from blurrily_amd.map import ClosedError
from helpers import FLAGS, compile_c, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blurrily_storage_get", "blurrily_storage_get_batch", "blurrily_storage_find_references",
       "blurrily_storage_find_references_device")


def test_the_new_symbols_are_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for sym in NEW:
        assert f" T {sym}\n" in out, sym
        assert getattr(lib, sym).argtypes is not None and getattr(lib, sym).restype is ctypes.c_int, sym
        assert sym in _native.EXPORTED_SYMBOLS
    assert len(lib.blurrily_storage_get.argtypes) == 5
    assert len(lib.blurrily_storage_get_batch.argtypes) == 7
    assert len(lib.blurrily_storage_find_references.argtypes) == 7
    assert len(lib.blurrily_storage_find_references_device.argtypes) == 8


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_new_prototypes_compile_beside_the_reference_header(tmp_path, order):
    src = os.path.join(ROOT, "tests", "c", "header_compat_refs.c")
    if order == "ours_alone":
        text = open(src).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = str(tmp_path / "refs_alone.c")
        open(src, "w").write(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


def test_a_drifted_new_prototype_does_not_compile(tmp_path):
    write_recorded_storage_h(tmp_path)
    text = open(os.path.join(ROOT, "tests", "c", "header_compat_refs.c")).read()
    drifted = text.replace("int (*f_get)(trigram_map, uint32_t, uint32_t*, int, uint16_t*)",
                           "int (*f_get)(trigram_map, uint32_t, uint32_t*, int, uint32_t*)")
    assert drifted != text
    src = tmp_path / "drifted.c"
    src.write_text(drifted)
    assert compile_c(tmp_path, src).returncode != 0


def test_by_reference_fails_loudly_without_a_gpu(has_gpu, capfd):
    if has_gpu:
        pytest.skip("a GPU is present: the HIP path runs instead (tests/test_gpu_refs.py)")
    m = Map()
    m.put("london", 123)
    for call in (lambda: m.get(123), lambda: m.find_by_reference(123), lambda: m.find_batch_by_reference([123, 7]),
                 lambda: m.get_batch([123])):
        with pytest.raises(OSError) as e:
            call()
        assert e.value.errno == errno.ENODEV
    assert "no usable HIP device" in capfd.readouterr().err
    lib = _native.lib()
    w = ctypes.c_uint32(0)
    codes = (ctypes.c_uint16 * 16)()
    assert lib.blurrily_storage_get(m.handle, 123, ctypes.byref(w), 16, codes) == -1
    assert ctypes.get_errno() == errno.ENODEV
    rows = (_native.TrigramMatch * 10)()
    refs = (ctypes.c_uint32 * 1)(123)
    counts = (ctypes.c_uint32 * 1)()
    assert lib.blurrily_storage_find_references(m.handle, refs, 1, 10, rows, counts, None) == -1
    assert ctypes.get_errno() == errno.ENODEV


def test_the_map_methods_check_their_arguments():
    m = Map()
    for bad in (-1, 1 << 32):
        with pytest.raises(OverflowError):
            m.get(bad)
        with pytest.raises(OverflowError):
            m.find_by_reference(bad)
        with pytest.raises(OverflowError):
            m.find_batch_by_reference([1, bad])
        with pytest.raises(OverflowError):
            m.get_batch([bad])
    with pytest.raises(ValueError):
        m.get_batch(np.zeros((2, 2), dtype=np.uint32))
    m.close()
    for call in (lambda: m.get(1), lambda: m.find_by_reference(1), lambda: m.find_batch_by_reference([1]),
                 lambda: m.get_batch([1])):
        with pytest.raises(ClosedError):
            call()
    r = RawMap()
    r.close()
    with pytest.raises(RawMap.ClosedError):
        r.find_by_reference(1, 10)


def test_the_ruby_glue_binds_them_and_passes_the_front_end(tmp_path):
    glue = os.path.join(ROOT, "ruby", "ext", "blurrily", "map_ext_batch.c")
    text = open(glue).read()
    for sym in ("blurrily_storage_find_references", "blurrily_storage_get"):
        assert sym + "(" in text, sym
    assert '"find_by_reference"' in text and '"get",' in text
    write_recorded_storage_h(tmp_path)
    cmd = ["gcc", "-fsyntax-only", *FLAGS, "-I", os.path.join(ROOT, "tests", "c", "mock_ruby"), "-I", str(tmp_path),
           "-I", os.path.join(ROOT, "include"), glue]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
