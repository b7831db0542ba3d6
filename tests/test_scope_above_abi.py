"""Scoped threshold find, without a GPU: blurrily_storage_find_batch_above_in, _find_above_in,
_find_batch_above_each_in and _find_references_above_each_in are exported with their argtypes set, their prototypes
compile beside the reference's storage.h and alone, every argument error is EINVAL before a GPU is asked for and
leaves the outputs as they were, valid calls fail loudly (ENODEV) where no GPU is usable, and the Python surface exists
and checks its arguments."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

from blurrily_amd import Map, RawMap, _native
from helpers import compile_c, einval, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"blurrily_storage_find_batch_above_in": 10, "blurrily_storage_find_above_in": 8,
       "blurrily_storage_find_batch_above_each_in": 12, "blurrily_storage_find_references_above_each_in": 12}
SRC = os.path.join(ROOT, "tests", "c", "header_compat_scope_above.c")
SENTINEL = 0xA5A5A5A5
SENTINEL64 = 0xA5A5A5A5A5A5A5A5


def test_the_four_symbols_are_exported_and_listed():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for sym, n_args in NEW.items():
        assert f" T {sym}\n" in out, sym
        fn = getattr(lib, sym)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args, sym
        assert sym in _native._ENTRIES and sym in _native.EXPORTED_SYMBOLS


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_prototypes_compile_beside_the_reference_header_and_alone(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "scope_above_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


def test_a_drifted_prototype_does_not_compile(tmp_path):
    write_recorded_storage_h(tmp_path)
    text = open(SRC).read()
    drifted = text.replace("uint32_t, uint32_t, trigram_match, uint64_t, uint64_t*) =\n      blurrily_storage_find_above_in",
                           "uint32_t, uint32_t, trigram_match, uint64_t, uint32_t*) =\n      blurrily_storage_find_above_in")
    assert drifted != text
    src = tmp_path / "drifted.c"
    src.write_text(drifted)
    assert compile_c(tmp_path, src).returncode != 0


def _scope(m, refs):
    arr = (ctypes.c_uint32 * max(len(refs), 1))(*refs)
    h = ctypes.c_void_p()
    assert _native.lib().blurrily_scope_new(m.handle, arr, len(refs), ctypes.byref(h)) == 0
    return h


def test_every_argument_error_is_einval_before_a_gpu_and_writes_nothing(capfd):
    lib = _native.lib()
    m, other = RawMap(), RawMap()
    m.put("london", 1, 0)
    m.put("paris", 2, 0)
    a, b, foreign = _scope(m, [1]), _scope(m, [2]), _scope(other, [1])
    rows = np.full((16, 3), SENTINEL, dtype=np.uint32)
    row_off = np.full(3, SENTINEL64, dtype=np.uint64)
    nb = np.full(2, SENTINEL, dtype=np.uint32)
    total = ctypes.c_uint64(SENTINEL64)
    R, Ro, Nb = rows.ctypes.data, row_off.ctypes.data, nb.ctypes.data
    packed = b"londonparis"
    off = (ctypes.c_uint64 * 3)(0, 6, 11)
    refs = (ctypes.c_uint32 * 2)(1, 2)
    two = (ctypes.c_void_p * 2)(a.value, b.value)
    too_many = 0xFFFFFFF1                                             # above the batch's cap of needles

    single = lib.blurrily_storage_find_batch_above_in
    one = lib.blurrily_storage_find_above_in
    each = lib.blurrily_storage_find_batch_above_each_in
    by_ref = lib.blurrily_storage_find_references_above_each_in

    # the single-scope entries
    einval(lambda: single(None, a, packed, off, 2, 0, 500, R, 16, Ro))             # no map
    einval(lambda: single(m.handle, None, packed, off, 2, 0, 500, R, 16, Ro))      # no scope
    einval(lambda: single(m.handle, foreign, packed, off, 2, 0, 500, R, 16, Ro))   # a scope of another map
    einval(lambda: single(m.handle, a, packed, off, 2, 0, 1001, R, 16, Ro))        # min_permille > 1000
    einval(lambda: single(m.handle, a, packed, off, 2, 0, 500, R, 16, None))       # row_off NULL
    einval(lambda: single(m.handle, a, None, None, 0, 0, 500, None, 0, None))      # ... with n == 0 too
    einval(lambda: single(m.handle, a, None, off, 2, 0, 500, R, 16, Ro))           # needles NULL with n > 0
    einval(lambda: single(m.handle, a, packed, None, 2, 0, 500, R, 16, Ro))
    einval(lambda: single(m.handle, a, packed, off, too_many, 0, 500, R, 16, Ro))
    einval(lambda: one(m.handle, a, None, 0, 500, R, 16, ctypes.byref(total)))
    einval(lambda: one(m.handle, a, b"london", 0, 1001, R, 16, ctypes.byref(total)))
    einval(lambda: one(m.handle, None, b"london", 0, 500, R, 16, ctypes.byref(total)))
    einval(lambda: one(m.handle, foreign, b"london", 0, 500, R, 16, ctypes.byref(total)))
    einval(lambda: one(None, a, b"london", 0, 500, R, 16, ctypes.byref(total)))

    # the each-in entries
    def batch(scopes, n_scopes, which, mp=m, n=2, mpm=500, ro=Ro, pk=packed, of=off):
        w = (ctypes.c_uint32 * 2)(*which) if which is not None else None
        return lambda: each(mp.handle if mp else None, scopes, n_scopes, w, pk, of, n, 0, mpm, R, 16, ro)

    def refs_call(scopes, n_scopes, which, mp=m, n=2, mpm=500, ro=Ro, pk=refs, of=None):
        w = (ctypes.c_uint32 * 2)(*which) if which is not None else None
        return lambda: by_ref(mp.handle if mp else None, scopes, n_scopes, w, pk, n, 0, mpm, R, 16, ro, Nb)

    for make in (batch, refs_call):
        einval(make(two, 2, [0, 2]))                                  # which[i] >= n_scopes
        einval(make(two, 1, [0, 1]))
        einval(make(None, 0, [0, _native.NO_SCOPE]))                  # ... with no scopes at all
        einval(make(None, 2, [0, 1]))                                 # n_scopes > 0, scopes NULL
        einval(make((ctypes.c_void_p * 2)(a.value, None), 2, [0, 1]))            # a NULL handle
        einval(make((ctypes.c_void_p * 2)(a.value, foreign.value), 2, [0, 0]))   # a scope of another map
        einval(make(two, 2, [0, 1], mp=other))                        # every scope is another map's
        einval(make(two, 2, [0, 1], mp=None))                         # no map
        einval(make(two, 2, [0, 1], mpm=1001))                        # min_permille > 1000
        einval(make(two, 2, [0, 1], ro=None))                         # row_off NULL
        einval(make(two, 2, [0, 1], ro=None, n=0))
        einval(make(two, 2, [0, 1], pk=None))                         # needles (references) NULL with n > 0
        einval(make(two, 2, None))                                    # which NULL with n > 0
        einval(make(two, 2, [0, 1], n=too_many))
    einval(batch(two, 2, [0, 1], of=None))

    assert "no usable HIP device" not in capfd.readouterr().err      # (no GPU was asked for)
    assert (rows == SENTINEL).all() and (nb == SENTINEL).all()        # nothing was written
    assert (row_off == SENTINEL64).all() and total.value == SENTINEL64
    for h in (a, b, foreign):
        assert lib.blurrily_scope_close(ctypes.byref(h)) == 0
    m.close()
    other.close()


def test_valid_calls_fail_loudly_without_a_gpu(has_gpu):
    """ENODEV where no GPU is usable; with one, the same calls succeed (tests/test_gpu_scope_above.py checks what they
    return)."""
    lib = _native.lib()
    m = Map()
    m.put("london", 1)
    m.put("paris", 2)
    a = _scope(m, [1])
    two = (ctypes.c_void_p * 2)(a.value, a.value)                      # (a handle twice is allowed)
    rows = (_native.TrigramMatch * 20)()
    row_off = (ctypes.c_uint64 * 3)()
    total = ctypes.c_uint64(0)
    off = (ctypes.c_uint64 * 3)(0, 6, 11)
    which = (ctypes.c_uint32 * 2)(1, _native.NO_SCOPE)
    refs = (ctypes.c_uint32 * 2)(1, 2)
    calls = [
        lambda: lib.blurrily_storage_find_batch_above_in(m.handle, a, b"londonparis", off, 2, 0, 500, rows, 20, row_off),
        lambda: lib.blurrily_storage_find_batch_above_in(m.handle, a, None, None, 0, 0, 500, None, 0, row_off),
        lambda: lib.blurrily_storage_find_batch_above_in(m.handle, a, b"londonparis", off, 2, 2, 0, None, 0, row_off),
        lambda: lib.blurrily_storage_find_above_in(m.handle, a, b"london", 0, 500, rows, 20, ctypes.byref(total)),
        lambda: lib.blurrily_storage_find_above_in(m.handle, a, b"london", 0, 500, None, 0, None),
        lambda: lib.blurrily_storage_find_batch_above_each_in(m.handle, two, 2, which, b"londonparis", off, 2, 0, 0,
                                                              rows, 20, row_off),
        lambda: lib.blurrily_storage_find_references_above_each_in(m.handle, two, 2, which, refs, 2, 0, 1000, rows, 20,
                                                                   row_off, None),
    ]
    for call in calls:
        ctypes.set_errno(0)
        if has_gpu:
            assert call() >= 0
        else:
            assert call() == -1 and ctypes.get_errno() == errno.ENODEV
    assert lib.blurrily_scope_close(ctypes.byref(a)) == 0
    for call in (lambda: m.find_above_in([1], "london", 0, 700),
                 lambda: m.find_batch_above_in([1], ["london", "paris"], 2, 0),
                 lambda: m.find_batch_above_each_in([[1], [2]], [0, None], ["london", "paris"]),
                 lambda: m.join_above_within([[1], [2]], 0, 700),
                 lambda: m.find_batch_by_reference_above_each_in([[1], [2]], [0, None], [1, 2], 0, 700),
                 lambda: RawMap.find_batch_above_in_packed(m, [1], b"london", np.array([0, 6], dtype=np.uint64), 0, 500)):
        if has_gpu:
            call()
        else:
            with pytest.raises(OSError) as e:
                call()
            assert e.value.errno == errno.ENODEV
    m.close()


def test_the_python_surface_exists_and_checks_min_permille():
    for name in ("find_above_in", "find_batch_above_in_packed", "find_batch_above_each_in",
                 "find_batch_by_reference_above_each_in", "join_above_within"):
        assert callable(getattr(RawMap, name)), name
    for name in ("find_above_in", "find_batch_above_in", "find_batch_above_each_in", "join_above_within"):
        assert callable(getattr(Map, name)), name
    for name in ("find_above_in", "find_batch_above_each_in"):
        assert getattr(Map, name) is not getattr(RawMap, name), name   # (Map's take strings and normalise them)
    m = Map()
    m.put("san jose", 1)
    offs = np.array([0, 8], dtype=np.uint64)
    for call in (lambda: m.find_above_in([1], "san jose", 0, 1001),
                 lambda: m.find_batch_above_in([1], ["san jose"], 0, 1001),
                 lambda: m.find_batch_above_each_in([[1]], [0], ["san jose"], 0, 1001),
                 lambda: m.join_above_within([[1]], 0, 1001),
                 lambda: RawMap.find_batch_above_in_packed(m, [1], b"san jose", offs, 0, 5000),
                 lambda: m.find_batch_by_reference_above_each_in([[1]], [0], [1], 0, 1001)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(OverflowError):
        m.find_above_in([1], "san jose", -1, 0)
    other = Map()
    with m.scope([1]) as mine:
        with pytest.raises(ValueError):
            other.find_above_in(mine, "san jose", 0, 500)
        with pytest.raises(ValueError):
            m.find_batch_above_each_in([mine], [0, 0], ["san jose"], 0, 500)   # which and needles differ in length
    other.close()
    m.close()
