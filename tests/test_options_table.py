"""Every tunable of blurrily_storage_set_option / blurrily_storage_get_option, one by one (no GPU needed: a map that
was never searched has no device side).  The figures below are written out here -- key, range, default -- and never
read from the library's own table: a row that moves, a range that changes or a default that drifts shows up as a
difference against this list."""
import ctypes
import errno

import pytest

from blurrily_amd import RawMap, _native

U32 = 0xFFFFFFFF
# key, lo, hi, default
MAP_OPTIONS = [
    ("wsweep", 0, 1, 1),
    ("ws_cmin", 1, 64, 3),
    ("ws_min_windows", 0, 1 << 20, 8),
    ("ws_min_needles", 0, 1 << 32, 16384),
    ("ws_min_slice", 0, 1 << 31, 1550),
    ("dense_min", 64, 65536, 1024),
    ("host_chunk", 0, 1 << 30, 131072),
    ("ws_autotune", 0, 1, 1),
    ("ws_static_slice", 0, 1 << 31, 2200),
    ("ws_choice", 0, 0, 0),
    ("nm_cmin", 0, 64, 3),
    ("nm_dense", 64, 65536, 3072),
    ("last_sweep", 0, 0, 0),
    ("devices", 1, 64, 1),
    ("nm_min_windows", 0, 1 << 20, 256),
    ("tuned_class", 0, 0, -1),
    ("tuned_nm_us", 0, 0, 0),
    ("tuned_ws_us", 0, 0, 0),
    ("tuned_leave_us", 0, 0, 0),
    ("small_sweep", 0, 1, 1),
    ("small_min_needles", 0, 1 << 32, 4096),
    ("one_launch", 0, 1, 1),
    ("one_taken", 0, 0, 0),
    ("one_windows_per_wg", 0, 1 << 20, 0),
    ("retunes", 0, 0, 0),
    ("tune_inject", 0, 3, 0),
    ("mid_workgroups", 64, 1 << 16, 1024),
    ("few_max", 1, 128, 24),
    ("mid_max", 0, 128, 128),
    ("latency_tasks", 0, 16, 0),
    ("scope_strategy", 0, 2, 0),
    ("scope_direct_max", 0, 1 << 40, 150000),
]
CLAMPED = {"ws_min_needles", "small_min_needles"}              # 2^32 is accepted and stored as 2^32 - 1


def _refused(call, *args):
    with pytest.raises(OSError) as e:
        call(*args)
    assert e.value.errno == errno.EINVAL, args


def test_the_list_is_the_whole_table():
    assert len(MAP_OPTIONS) == 32 and len({k for k, *_ in MAP_OPTIONS}) == 32


@pytest.mark.parametrize("key,lo,hi,default", MAP_OPTIONS, ids=[k for k, *_ in MAP_OPTIONS])
def test_a_map_option_has_its_default_and_its_range(key, lo, hi, default):
    m = RawMap()
    try:
        assert m.get_option(key) == default
        if lo == hi == 0:                                       # read-only (or reset-only): 0 is taken and changes nothing
            m.set_option(key, 0)
            assert m.get_option(key) == default
            for v in (1, -1):
                _refused(m.set_option, key, v)
            assert m.get_option(key) == default
            return
        for v in (hi, lo):
            m.set_option(key, v)
            assert m.get_option(key) == (min(v, U32) if key in CLAMPED else v), (key, v)
        for v in (lo - 1, hi + 1):
            _refused(m.set_option, key, v)
            assert m.get_option(key) == lo, (key, v)
        if key == "devices":
            m.set_option(key, 1)
    finally:
        m.close()


def test_options_are_per_map_and_unknown_keys_are_refused():
    lib = _native.lib()
    m, other = RawMap(), RawMap()
    m.set_option("nm_dense", 64)
    assert other.get_option("nm_dense") == 3072
    out = ctypes.c_longlong(-7)
    _refused(m.set_option, "no_such_option", 0)
    _refused(m.get_option, "no_such_option")
    for key in ("", "ws_cmin ", "WS_CMIN"):
        _refused(m.set_option, key, 3)
        _refused(m.get_option, key)
    ctypes.set_errno(0)
    assert lib.blurrily_storage_set_option(m.handle, None, 0) == -1 and ctypes.get_errno() == errno.EINVAL
    ctypes.set_errno(0)
    assert lib.blurrily_storage_get_option(m.handle, None, ctypes.byref(out)) == -1 and ctypes.get_errno() == errno.EINVAL
    ctypes.set_errno(0)
    assert lib.blurrily_storage_get_option(m.handle, b"ws_cmin", None) == -1 and ctypes.get_errno() == errno.EINVAL
    assert out.value == -7
    # a process key on a map
    for key in ("host_threads", "build_trace"):
        _refused(m.set_option, key, 0)
        _refused(m.get_option, key)
    m.close(); other.close()


def test_process_options_and_map_keys_on_the_null_map():
    lib = _native.lib()
    out = ctypes.c_longlong(-7)

    def get(key):
        ctypes.set_errno(0)
        if lib.blurrily_storage_get_option(None, key, ctypes.byref(out)) != 0:
            raise OSError(ctypes.get_errno(), "get_option")
        return out.value

    def put(key, value):
        ctypes.set_errno(0)
        if lib.blurrily_storage_set_option(None, key, ctypes.c_longlong(value)) != 0:
            raise OSError(ctypes.get_errno(), "set_option")

    try:
        hardware = get(b"host_threads")                         # 0: the hardware's threads, 64 at the most
        assert 1 <= hardware <= 64 and get(b"build_trace") == 0
        for v in (256, 1):
            put(b"host_threads", v)
            assert get(b"host_threads") == v
        for v in (-1, 257):
            _refused(put, b"host_threads", v)
            assert get(b"host_threads") == 1
        put(b"host_threads", 0)
        assert get(b"host_threads") == hardware
        for v in (1, 0):
            put(b"build_trace", v)
            assert get(b"build_trace") == v
        for v in (-1, 2):
            _refused(put, b"build_trace", v)
            assert get(b"build_trace") == 0
        # a per-map key on the NULL map, an unknown one, no key, nowhere to put the value
        for key, *_ in MAP_OPTIONS:
            _refused(put, key.encode(), 0)
            _refused(get, key.encode())
        _refused(put, b"no_such_option", 0)
        _refused(get, b"no_such_option")
        _refused(put, None, 0)
        _refused(get, None)
        ctypes.set_errno(0)
        assert lib.blurrily_storage_get_option(None, b"host_threads", None) == -1 and ctypes.get_errno() == errno.EINVAL
    finally:
        lib.blurrily_storage_set_option(None, b"host_threads", ctypes.c_longlong(0))
        lib.blurrily_storage_set_option(None, b"build_trace", ctypes.c_longlong(0))
