"""Scoped similarity find, without a GPU: blurrily_storage_find_batch_similar_in, _find_similar_in,
_find_batch_similar_each_in and _find_references_similar_each_in are exported with their argtypes set, their prototypes
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
NEW = {"blurrily_storage_find_batch_similar_in": 10, "blurrily_storage_find_similar_in": 7,
       "blurrily_storage_find_batch_similar_each_in": 12, "blurrily_storage_find_references_similar_each_in": 12}
SRC = os.path.join(ROOT, "tests", "c", "header_compat_scope_similar.c")
SENTINEL = 0xA5A5A5A5


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
        src = tmp_path / "scope_similar_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


def test_a_drifted_prototype_does_not_compile(tmp_path):
    write_recorded_storage_h(tmp_path)
    text = open(SRC).read()
    drifted = text.replace("uint16_t, uint32_t, trigram_match, uint32_t*) =\n      blurrily_storage_find_similar_in",
                           "uint32_t, uint32_t, trigram_match, uint32_t*) =\n      blurrily_storage_find_similar_in")
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
    rows = np.full((2, 10, 3), SENTINEL, dtype=np.uint32)
    counts = np.full(2, SENTINEL, dtype=np.uint32)
    ntri = np.full((2, 10), SENTINEL, dtype=np.uint32)
    nb = np.full(2, SENTINEL, dtype=np.uint32)
    R, Cn, Nt, Nb = rows.ctypes.data, counts.ctypes.data, ntri.ctypes.data, nb.ctypes.data
    packed = b"londonparis"
    off = (ctypes.c_uint64 * 3)(0, 6, 11)
    refs = (ctypes.c_uint32 * 2)(1, 2)
    two = (ctypes.c_void_p * 2)(a.value, b.value)
    too_many = 0xFFFFFFF1                                             # above the batch's cap of needles

    single = lib.blurrily_storage_find_batch_similar_in
    one = lib.blurrily_storage_find_similar_in
    each = lib.blurrily_storage_find_batch_similar_each_in
    by_ref = lib.blurrily_storage_find_references_similar_each_in

    # the single-scope entries
    einval(lambda: single(None, a, packed, off, 2, 10, 500, R, Cn, Nt))            # no map
    einval(lambda: single(m.handle, None, packed, off, 2, 10, 500, R, Cn, Nt))     # no scope
    einval(lambda: single(m.handle, foreign, packed, off, 2, 10, 500, R, Cn, Nt))  # a scope of another map
    einval(lambda: single(m.handle, a, packed, off, 2, 10, 1001, R, Cn, Nt))       # min_permille > 1000
    einval(lambda: single(m.handle, a, packed, off, 2, 10, 500, R, None, Nt))      # counts NULL
    einval(lambda: single(m.handle, a, None, None, 0, 10, 500, None, None, None))  # ... with n == 0 too
    einval(lambda: single(m.handle, a, packed, off, 2, 10, 500, None, Cn, Nt))     # results NULL, n and limit non-zero
    einval(lambda: single(m.handle, a, None, off, 2, 10, 500, R, Cn, Nt))          # needles NULL with n > 0
    einval(lambda: single(m.handle, a, packed, None, 2, 10, 500, R, Cn, Nt))
    einval(lambda: single(m.handle, a, packed, off, too_many, 10, 500, R, Cn, Nt))
    einval(lambda: one(m.handle, a, None, 10, 500, R, Nt))
    einval(lambda: one(m.handle, a, b"london", 10, 1001, R, Nt))
    einval(lambda: one(m.handle, None, b"london", 10, 500, R, Nt))
    einval(lambda: one(m.handle, foreign, b"london", 10, 500, R, Nt))
    einval(lambda: one(m.handle, a, b"london", 10, 500, None, Nt))

    # the each-in entries
    def batch(scopes, n_scopes, which, mp=m, n=2, mpm=500, res=R, cnt=Cn, pk=packed, of=off):
        w = (ctypes.c_uint32 * 2)(*which) if which is not None else None
        return lambda: each(mp.handle if mp else None, scopes, n_scopes, w, pk, of, n, 10, mpm, res, cnt, Nt)

    def refs_call(scopes, n_scopes, which, mp=m, n=2, mpm=500, res=R, cnt=Cn, pk=refs, of=None):
        w = (ctypes.c_uint32 * 2)(*which) if which is not None else None
        return lambda: by_ref(mp.handle if mp else None, scopes, n_scopes, w, pk, n, 10, mpm, res, cnt, Nt, Nb)

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
        einval(make(two, 2, [0, 1], cnt=None))                        # counts NULL
        einval(make(two, 2, [0, 1], cnt=None, n=0))
        einval(make(two, 2, [0, 1], res=None))                        # results NULL, n and limit non-zero
        einval(make(two, 2, [0, 1], pk=None))                         # needles NULL with n > 0
        einval(make(two, 2, None))                                    # which NULL with n > 0
        einval(make(two, 2, [0, 1], n=too_many))
    einval(batch(two, 2, [0, 1], of=None))

    assert "no usable HIP device" not in capfd.readouterr().err      # (no GPU was asked for)
    for out in (rows, counts, ntri, nb):
        assert (out == SENTINEL).all()                                # nothing was written
    for h in (a, b, foreign):
        assert lib.blurrily_scope_close(ctypes.byref(h)) == 0
    m.close()
    other.close()


def test_valid_calls_fail_loudly_without_a_gpu(has_gpu):
    """ENODEV where no GPU is usable; with one, the same calls succeed (tests/test_gpu_scope_similar.py checks what
    they return)."""
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
        lambda: lib.blurrily_storage_find_batch_similar_in(m.handle, a, b"londonparis", off, 2, 10, 500, rows, counts,
                                                           None),
        lambda: lib.blurrily_storage_find_batch_similar_in(m.handle, a, None, None, 0, 10, 500, None, counts, None),
        lambda: lib.blurrily_storage_find_batch_similar_in(m.handle, a, b"londonparis", off, 2, 0, 500, None, counts,
                                                           None),
        lambda: lib.blurrily_storage_find_similar_in(m.handle, a, b"london", 10, 500, rows, None),
        lambda: lib.blurrily_storage_find_batch_similar_each_in(m.handle, two, 2, which, b"londonparis", off, 2, 10, 0,
                                                                rows, counts, None),
        lambda: lib.blurrily_storage_find_references_similar_each_in(m.handle, two, 2, which, refs, 2, 10, 1000, rows,
                                                                     counts, None, None),
    ]
    for call in calls:
        ctypes.set_errno(0)
        if has_gpu:
            assert call() >= 0
        else:
            assert call() == -1 and ctypes.get_errno() == errno.ENODEV
    assert lib.blurrily_scope_close(ctypes.byref(a)) == 0
    for call in (lambda: m.find_similar_in([1], "london", 10, 700),
                 lambda: m.find_batch_similar_each_in([[1], [2]], [0, None], ["london", "paris"]),
                 lambda: m.join_similar_within([[1], [2]], 10, 700),
                 lambda: RawMap.find_batch_similar_in_packed(m, [1], b"london", np.array([0, 6], dtype=np.uint64), 10)):
        if has_gpu:
            call()
        else:
            with pytest.raises(OSError) as e:
                call()
            assert e.value.errno == errno.ENODEV
    m.close()


def test_the_python_surface_exists_and_checks_min_permille():
    for name in ("find_similar_in", "find_batch_similar_in_packed", "find_batch_similar_each_in",
                 "find_batch_by_reference_similar_each_in", "join_similar_within"):
        assert callable(getattr(RawMap, name)), name
    for name in ("find_similar_in", "find_batch_similar_each_in", "join_similar_within"):
        assert getattr(Map, name) is not getattr(RawMap, name), name   # (Map's take normalised strings)
    m = Map()
    m.put("san jose", 1)
    offs = np.array([0, 8], dtype=np.uint64)
    for call in (lambda: m.find_similar_in([1], "san jose", 10, 1001),
                 lambda: m.find_batch_similar_each_in([[1]], [0], ["san jose"], 10, 1001),
                 lambda: m.join_similar_within([[1]], 10, 1001),
                 lambda: RawMap.find_batch_similar_in_packed(m, [1], b"san jose", offs, 10, 5000),
                 lambda: m.find_batch_by_reference_similar_each_in([[1]], [0], [1], 10, 1001)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(OverflowError):
        m.find_similar_in([1], "san jose", 10, -1)
    other = Map()
    with m.scope([1]) as mine:
        with pytest.raises(ValueError):
            other.find_similar_in(mine, "san jose", 10, 500)
        with pytest.raises(ValueError):
            m.find_batch_similar_each_in([mine], [0, 0], ["san jose"], 10, 500)   # which and needles differ in length
    other.close()
    m.close()
