"""A scope per needle, without a GPU: blurrily_storage_find_batch_each_in[_device] and _find_references_each_in are
exported with their argtypes set, their prototypes agree with the reference's storage.h in one translation unit, every
argument error is EINVAL before a GPU is asked for, valid calls fail loudly (ENODEV) where no GPU is usable, and the
Python surface checks `which` and the scopes' map."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

from blurrily_amd import Map, RawMap, _native
from helpers import compile_c, einval, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"blurrily_storage_find_batch_each_in": 10, "blurrily_storage_find_batch_each_in_device": 12,
       "blurrily_storage_find_references_each_in": 10}
SRC = os.path.join(ROOT, "tests", "c", "header_compat_scope_each.c")


def test_the_each_in_symbols_are_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for sym, n_args in NEW.items():
        assert f" T {sym}\n" in out, sym
        fn = getattr(lib, sym)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args, sym
        assert sym in _native.EXPORTED_SYMBOLS
    assert _native.NO_SCOPE == 0xFFFFFFFF


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_each_in_prototypes_compile_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "scope_each_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("drift", [
    ("const uint32_t*, const char*, size_t, const uint64_t*", "uint32_t*, const char*, size_t, const uint64_t*"),
    ("trigram_match, uint32_t*, uint32_t*) = blurrily_storage_find_references_each_in",
     "trigram_match, uint32_t*, uint64_t*) = blurrily_storage_find_references_each_in"),
])
def test_a_drifted_each_in_prototype_does_not_compile(tmp_path, drift):
    write_recorded_storage_h(tmp_path)
    text = open(SRC).read()
    drifted = text.replace(*drift)
    assert drifted != text
    src = tmp_path / "drifted.c"
    src.write_text(drifted)
    assert compile_c(tmp_path, src).returncode != 0


def _scope(m, refs):
    arr = (ctypes.c_uint32 * max(len(refs), 1))(*refs)
    h = ctypes.c_void_p()
    assert _native.lib().blurrily_scope_new(m.handle, arr, len(refs), ctypes.byref(h)) == 0
    return h


def test_every_argument_error_is_einval_before_a_gpu_is_asked_for(capfd):
    lib = _native.lib()
    m, other = RawMap(), RawMap()
    m.put("london", 1, 0)
    m.put("paris", 2, 0)
    a, b, foreign = _scope(m, [1]), _scope(m, [2]), _scope(other, [1])
    rows = (_native.TrigramMatch * 20)()
    counts = (ctypes.c_uint32 * 2)()
    nb = (ctypes.c_uint32 * 2)()
    off = (ctypes.c_uint64 * 3)(0, 6, 11)
    refs = (ctypes.c_uint32 * 2)(1, 2)
    two = (ctypes.c_void_p * 2)(a.value, b.value)

    def batch(scopes, n_scopes, which, mp=m):
        w = (ctypes.c_uint32 * 2)(*which)
        return lambda: lib.blurrily_storage_find_batch_each_in(mp.handle, scopes, n_scopes, w, b"londonparis", off, 2,
                                                               10, rows, counts)

    def by_ref(scopes, n_scopes, which):
        w = (ctypes.c_uint32 * 2)(*which)
        return lambda: lib.blurrily_storage_find_references_each_in(m.handle, scopes, n_scopes, w, refs, 2, 10, rows,
                                                                    counts, nb)

    def device(scopes, n_scopes):
        return lambda: lib.blurrily_storage_find_batch_each_in_device(m.handle, scopes, n_scopes, None, None, 0, None,
                                                                      2, 10, None, None, None)

    for make in (batch, by_ref):
        einval(make(two, 2, [0, 2]))                                  # which[i] >= n_scopes
        einval(make(two, 1, [0, 1]))
        einval(make(None, 0, [0, _native.NO_SCOPE]))                  # ... with no scopes at all
        einval(make(None, 2, [0, 1]))                                 # n_scopes > 0, scopes NULL
        einval(make((ctypes.c_void_p * 2)(a.value, None), 2, [0, 1]))            # a NULL handle
        einval(make((ctypes.c_void_p * 2)(a.value, foreign.value), 2, [0, 0]))   # a scope of another map
    einval(batch(two, 2, [0, 1], mp=other))                           # every scope is another map's
    einval(device(None, 2))
    einval(device((ctypes.c_void_p * 2)(a.value, foreign.value), 2))
    einval(lambda: lib.blurrily_storage_find_batch_each_in(None, two, 2, None, None, None, 0, 10, None, None))
    assert "no usable HIP device" not in capfd.readouterr().err      # (no GPU was asked for)
    for h in (a, b, foreign):
        assert lib.blurrily_scope_close(ctypes.byref(h)) == 0
    m.close()
    other.close()


def test_valid_calls_fail_loudly_without_a_gpu(has_gpu, capfd):
    if has_gpu:
        pytest.skip("a GPU is present: the HIP path runs instead (tests/test_gpu_scope_each.py)")
    lib = _native.lib()
    m = Map()
    m.put("london", 1)
    m.put("paris", 2)
    a = _scope(m, [1])
    two = (ctypes.c_void_p * 2)(a.value, a.value)                      # (a handle twice is allowed)
    rows = (_native.TrigramMatch * 20)()
    counts = (ctypes.c_uint32 * 2)()
    off = (ctypes.c_uint64 * 3)(0, 6, 11)
    which = (ctypes.c_uint32 * 2)(1, _native.NO_SCOPE)
    refs = (ctypes.c_uint32 * 2)(1, 2)
    calls = [
        lambda: lib.blurrily_storage_find_batch_each_in(m.handle, two, 2, which, b"londonparis", off, 2, 10, rows, counts),
        lambda: lib.blurrily_storage_find_references_each_in(m.handle, two, 2, which, refs, 2, 10, rows, counts, None),
        lambda: lib.blurrily_storage_find_batch_each_in_device(m.handle, two, 2, None, None, 0, None, 0, 10, None, None,
                                                               None),
    ]
    for call in calls:
        ctypes.set_errno(0)
        assert call() == -1 and ctypes.get_errno() == errno.ENODEV
    assert lib.blurrily_scope_close(ctypes.byref(a)) == 0
    for call in (lambda: m.find_batch_each_in([[1], [2]], [0, None], ["london", "paris"]),
                 lambda: m.join_within([[1], [2]])):
        with pytest.raises(OSError) as e:
            call()
        assert e.value.errno == errno.ENODEV
    assert "no usable HIP device" in capfd.readouterr().err
    m.close()


def test_an_each_in_batch_of_nothing_but_empty_needles_is_a_valid_call(has_gpu):
    """Such a batch has no bytes to point to; the binding passes a dummy byte (NULL with n > 0 is EINVAL), so the call
    answers what any valid call does: its rows where a GPU is usable, ENODEV where none is."""
    m = Map()
    m.put("london", 1)
    with m.scope([1]) as held:
        for call in (lambda: m.find_batch_each_in([[1]], [0], [""]),
                     lambda: m.find_batch_each_in([held, [1]], [0, None, 1], ["", "  ", ""]),
                     lambda: RawMap.find_batch_each_in(m, [held], [0], b"", np.zeros(2, dtype=np.uint64), 10)):
            if has_gpu:
                call()
                continue
            with pytest.raises(OSError) as e:
                call()
            assert e.value.errno == errno.ENODEV
    if has_gpu:
        assert m.find_batch_each_in([[1]], [0], [""]) == [m.find_in([1], "")] == [[]]
    m.close()


def test_python_rejects_a_which_of_the_wrong_length_and_foreign_scopes():
    m, other = Map(), Map()
    m.put("london", 1)
    with other.scope([1]) as foreign, m.scope([1]) as mine:
        with pytest.raises(ValueError):
            m.find_batch_each_in([mine], [0], ["london", "paris"])
        with pytest.raises(ValueError):
            m.find_batch_each_in([mine], [0, 0, None], ["london", "paris"])
        with pytest.raises(ValueError):
            m.find_batch_each_in([mine, foreign], [0, 1], ["london", "paris"])
        with pytest.raises(ValueError):
            RawMap.find_batch_by_reference_each_in(m, [foreign], [0], [1], 10)
        with pytest.raises(ValueError):
            m.join_within([mine, foreign])
        with pytest.raises(OverflowError):
            m.find_batch_each_in([mine], [-1], ["london"])
    m.close()
    other.close()


def test_the_ruby_glue_binds_find_batch_among_and_passes_the_front_end():
    glue = os.path.join(ROOT, "ruby", "ext", "blurrily", "map_ext_batch.c")
    text = open(glue).read()
    for sym in ("blurrily_scope_new", "blurrily_storage_find_batch_each_in", "blurrily_scope_close"):
        assert sym + "(" in text, sym
    assert '"find_batch_among"' in text and "BLURRILY_NO_SCOPE" in text
