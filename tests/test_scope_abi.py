"""Scoped find, without a GPU: blurrily_scope_* and blurrily_storage_find_in / _find_batch_in[_device] are exported with
their argtypes set, their prototypes agree with the reference's storage.h in one translation unit, a scope is made,
counted and closed on the host alone, the entry points check their arguments (EINVAL) and a scoped find fails loudly
(ENODEV) where no GPU is usable."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

from blurrily_amd import Map, RawMap, Scope, _native
from helpers import FLAGS, compile_c, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"blurrily_scope_new": 4, "blurrily_scope_close": 1, "blurrily_scope_members": 2, "blurrily_storage_find_in": 5,
       "blurrily_storage_find_batch_in": 8, "blurrily_storage_find_batch_in_device": 10}


def test_the_scope_symbols_are_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for sym, n_args in NEW.items():
        assert f" T {sym}\n" in out, sym
        fn = getattr(lib, sym)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args, sym
        assert sym in _native.EXPORTED_SYMBOLS


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_scope_prototypes_compile_beside_the_reference_header(tmp_path, order):
    src = os.path.join(ROOT, "tests", "c", "header_compat_scope.c")
    if order == "ours_alone":
        text = open(src).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "scope_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


def test_a_drifted_scope_prototype_does_not_compile(tmp_path):
    write_recorded_storage_h(tmp_path)
    text = open(os.path.join(ROOT, "tests", "c", "header_compat_scope.c")).read()
    drifted = text.replace("int (*f_members)(blurrily_scope, uint32_t*)", "int (*f_members)(blurrily_scope, uint64_t*)")
    assert drifted != text
    src = tmp_path / "drifted.c"
    src.write_text(drifted)
    assert compile_c(tmp_path, src).returncode != 0


def _new_scope(m, refs):
    lib = _native.lib()
    arr = (ctypes.c_uint32 * max(len(refs), 1))(*refs)
    h = ctypes.c_void_p()
    assert lib.blurrily_scope_new(m.handle, arr, len(refs), ctypes.byref(h)) == 0
    return h


def _members(h):
    held = ctypes.c_uint32(99)
    assert _native.lib().blurrily_scope_members(h, ctypes.byref(held)) == 0
    return held.value


def test_a_scope_is_made_counted_and_closed_without_a_gpu():
    lib = _native.lib()
    m = RawMap()
    for ref, s in ((1, "london"), (2, "paris"), (3, "berlin"), (4, "madrid")):
        m.put(s, ref, 0)
    h = _new_scope(m, [3, 1, 3, 3, 77, 1, 1 << 31])       # duplicates once, absent references ignored
    assert _members(h) == 2
    m.delete(3)
    assert _members(h) == 1                               # read against the map as it is now
    m.put("dublin", 77, 0)
    assert _members(h) == 2
    m.put("berlin mitte", 3, 0)                           # deleted and put again
    assert _members(h) == 3
    assert lib.blurrily_scope_close(ctypes.byref(h)) == 0
    assert h.value is None                                # NULLed
    assert lib.blurrily_scope_close(ctypes.byref(h)) == 0    # (a NULL scope: no-op)
    empty = _new_scope(m, [])
    assert _members(empty) == 0
    assert lib.blurrily_scope_close(ctypes.byref(empty)) == 0
    m.close()


def test_the_python_scope_counts_its_members():
    m = Map()
    m.put("london", 1)
    m.put("paris", 2)
    with m.scope([1, 2, 2, 5]) as sc:
        assert isinstance(sc, Scope) and sc.members() == 2
        m.delete(2)
        assert sc.members() == 1
    with pytest.raises(Scope.ClosedError):
        sc.members()
    with m.scope(r for r in (1, 2)) as sc2:             # any iterable of references
        assert sc2.members() == 1
    other = Map()
    with other.scope([1]) as foreign:
        with pytest.raises(ValueError):
            m.find_in(foreign, "london")
    with pytest.raises(OverflowError):
        m.scope([1, -1])
    m.close()
    other.close()


def test_einval_for_nulls_and_for_a_foreign_map():
    lib = _native.lib()
    m, other = RawMap(), RawMap()
    m.put("london", 1, 0)
    refs = (ctypes.c_uint32 * 1)(1)
    h = ctypes.c_void_p()
    assert lib.blurrily_scope_new(None, refs, 1, ctypes.byref(h)) == -1 and ctypes.get_errno() == errno.EINVAL
    assert lib.blurrily_scope_new(m.handle, None, 1, ctypes.byref(h)) == -1 and ctypes.get_errno() == errno.EINVAL
    assert lib.blurrily_scope_new(m.handle, refs, 1, None) == -1 and ctypes.get_errno() == errno.EINVAL
    assert lib.blurrily_scope_close(None) == -1 and ctypes.get_errno() == errno.EINVAL
    held = ctypes.c_uint32()
    assert lib.blurrily_scope_members(None, ctypes.byref(held)) == -1 and ctypes.get_errno() == errno.EINVAL
    h = _new_scope(m, [1])
    assert lib.blurrily_scope_members(h, None) == -1 and ctypes.get_errno() == errno.EINVAL
    rows = (_native.TrigramMatch * 10)()
    counts = (ctypes.c_uint32 * 1)()
    off = (ctypes.c_uint64 * 2)(0, 6)
    # a scope used with a map other than its own, a NULL scope, a NULL map: EINVAL before any GPU is asked
    assert lib.blurrily_storage_find_in(other.handle, h, b"london", 10, rows) == -1
    assert ctypes.get_errno() == errno.EINVAL
    assert lib.blurrily_storage_find_in(m.handle, None, b"london", 10, rows) == -1
    assert ctypes.get_errno() == errno.EINVAL
    assert lib.blurrily_storage_find_in(m.handle, h, None, 10, rows) == -1
    assert ctypes.get_errno() == errno.EINVAL
    assert lib.blurrily_storage_find_batch_in(other.handle, h, b"london", off, 1, 10, rows, counts) == -1
    assert ctypes.get_errno() == errno.EINVAL
    assert lib.blurrily_storage_find_batch_in(m.handle, h, None, off, 1, 10, rows, counts) == -1
    assert ctypes.get_errno() == errno.EINVAL
    assert lib.blurrily_storage_find_batch_in_device(None, h, None, 0, None, 1, 10, None, None, None) == -1
    assert ctypes.get_errno() == errno.EINVAL
    assert lib.blurrily_storage_find_batch_in_device(other.handle, h, None, 0, None, 1, 10, None, None, None) == -1
    assert ctypes.get_errno() == errno.EINVAL
    assert lib.blurrily_scope_close(ctypes.byref(h)) == 0
    m.close()
    other.close()


def test_scope_options_are_in_the_table():
    m = RawMap()
    assert m.get_option("scope_strategy") == 0
    for v in (1, 2, 0):
        m.set_option("scope_strategy", v)
        assert m.get_option("scope_strategy") == v
    with pytest.raises(OSError):
        m.set_option("scope_strategy", 3)
    m.set_option("scope_direct_max", 123456)
    assert m.get_option("scope_direct_max") == 123456
    m.close()


def test_a_scoped_find_fails_loudly_without_a_gpu(has_gpu, capfd):
    if has_gpu:
        pytest.skip("a GPU is present: the HIP path runs instead (tests/test_gpu_scope.py)")
    lib = _native.lib()
    m = Map()
    m.put("london", 123)
    h = _new_scope(m, [123])
    rows = (_native.TrigramMatch * 10)()
    assert lib.blurrily_storage_find_in(m.handle, h, b"london", 10, rows) == -1
    assert ctypes.get_errno() == errno.ENODEV
    counts = (ctypes.c_uint32 * 1)()
    off = (ctypes.c_uint64 * 2)(0, 6)
    assert lib.blurrily_storage_find_batch_in(m.handle, h, b"london", off, 1, 10, rows, counts) == -1
    assert ctypes.get_errno() == errno.ENODEV
    assert lib.blurrily_scope_close(ctypes.byref(h)) == 0
    for call in (lambda: m.find_in([123], "london"), lambda: m.find_batch_in([123], ["london", "paris"])):
        with pytest.raises(OSError) as e:
            call()
        assert e.value.errno == errno.ENODEV
    assert "no usable HIP device" in capfd.readouterr().err
    m.close()


def test_a_scoped_batch_of_nothing_but_empty_needles_is_a_valid_call(has_gpu):
    """Such a batch has no bytes to point to; the binding passes a dummy byte (NULL with n > 0 is EINVAL), so the call
    answers what any valid call does: its rows where a GPU is usable, ENODEV where none is."""
    m = Map()
    m.put("london", 123)
    calls = (lambda: m.find_batch_in([123], [""]), lambda: m.find_batch_in([123], ["", "  ", ""]),
             lambda: RawMap.find_batch_in(m, [123], b"", np.zeros(2, dtype=np.uint64), 10))
    with m.scope([123]) as held:
        calls += (lambda: m.find_batch_in(held, [""]),)
        for call in calls:
            if has_gpu:
                call()
                continue
            with pytest.raises(OSError) as e:
                call()
            assert e.value.errno == errno.ENODEV
    if has_gpu:
        assert m.find_batch_in([123], [""]) == [m.find_in([123], "")] == [[]]
    m.close()


def test_the_ruby_glue_binds_find_among_and_passes_the_front_end(tmp_path):
    glue = os.path.join(ROOT, "ruby", "ext", "blurrily", "map_ext_batch.c")
    text = open(glue).read()
    for sym in ("blurrily_scope_new", "blurrily_storage_find_batch_in", "blurrily_scope_close"):
        assert sym + "(" in text, sym
    assert '"find_among"' in text
    write_recorded_storage_h(tmp_path)
    cmd = ["gcc", "-fsyntax-only", *FLAGS, "-I", os.path.join(ROOT, "tests", "c", "mock_ruby"), "-I", str(tmp_path),
           "-I", os.path.join(ROOT, "include"), glue]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
