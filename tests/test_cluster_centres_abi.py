"""Cluster centres, without a GPU: blurrily_storage_cluster_centres is exported with its argtypes set, its prototype
agrees with the reference's storage.h in one translation unit, every argument error is EINVAL before a GPU is asked for
and leaves all six outputs as they were, valid calls fail loudly (ENODEV) where no GPU is usable, and the Python
surface checks its arguments, hands NULL for `attached` when it is not wanted and shapes canned arrays rightly."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

from blurrily_amd import Map, RawMap, _native
from helpers import compile_c, einval, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster_centres.c")
NO = _native.NO_CLUSTER


def test_the_cluster_centres_symbol_is_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert " T blurrily_storage_cluster_centres\n" in out
    fn = lib.blurrily_storage_cluster_centres
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10
    assert "blurrily_storage_cluster_centres" in _native.EXPORTED_SYMBOLS


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_cluster_centres_prototype_compiles_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_centres_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("was,now", [("uint32_t*, uint32_t*, uint32_t*, uint8_t*,", "uint32_t*, uint32_t*, uint32_t*, uint32_t*,"),
                                     ("uint32_t*, uint64_t*) =", "uint32_t*, uint32_t*) =")],
                         ids=["attached_as_words", "edges_as_a_word"])
def test_a_drifted_cluster_centres_prototype_does_not_compile(tmp_path, was, now):
    write_recorded_storage_h(tmp_path)
    text = open(SRC).read()
    drifted = text.replace(was, now)
    assert drifted != text
    src = tmp_path / "drifted.c"
    src.write_text(drifted)
    assert compile_c(tmp_path, src).returncode != 0


def test_argument_errors_are_einval_before_any_gpu_and_write_nothing():
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs = np.array([1, 2], dtype=np.uint32)
    labels, degrees, centres = (np.full(2, 7, dtype=np.uint32) for _ in range(3))
    attached = np.full(2, 7, dtype=np.uint8)
    n_clusters, n_edges = ctypes.c_uint32(7), ctypes.c_uint64(7)
    per = (degrees.ctypes.data, centres.ctypes.data, attached.ctypes.data)
    out = per + (ctypes.byref(n_clusters), ctypes.byref(n_edges))
    centres_call = lib.blurrily_storage_cluster_centres
    einval(lambda: centres_call(None, refs.ctypes.data, 2, 500, labels.ctypes.data, *out))        # no map
    einval(lambda: centres_call(m.handle, refs.ctypes.data, 2, 1001, labels.ctypes.data, *out))   # min_permille > 1000
    einval(lambda: centres_call(m.handle, None, 0, 1001, None, *out))                             # ... with n == 0 too
    einval(lambda: centres_call(m.handle, None, 2, 500, labels.ctypes.data, *out))                # references NULL, n > 0
    einval(lambda: centres_call(m.handle, refs.ctypes.data, 2, 500, None, *out))                  # labels NULL, n > 0
    einval(lambda: centres_call(m.handle, refs.ctypes.data, 0xFFFFFFF1, 500, labels.ctypes.data, *out))   # more than a call takes
    einval(lambda: centres_call(m.handle, refs.ctypes.data, 2, 1001, labels.ctypes.data, None, None, None, None, None))
    assert n_clusters.value == 7 and n_edges.value == 7                                           # nothing written
    assert (labels == 7).all() and (degrees == 7).all() and (centres == 7).all() and (attached == 7).all()
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster_centres.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs = np.array([1, 2], dtype=np.uint32)
    labels, degrees, centres = (np.zeros(2, dtype=np.uint32) for _ in range(3))
    attached = np.zeros(2, dtype=np.uint8)
    n_clusters, n_edges = ctypes.c_uint32(0), ctypes.c_uint64(0)
    call = lib.blurrily_storage_cluster_centres
    for one in (lambda: call(m.handle, refs.ctypes.data, 2, 500, labels.ctypes.data, degrees.ctypes.data,
                             centres.ctypes.data, attached.ctypes.data, ctypes.byref(n_clusters), ctypes.byref(n_edges)),
                lambda: call(m.handle, refs.ctypes.data, 2, 0, labels.ctypes.data, None, None, None, None, None),
                lambda: call(m.handle, refs.ctypes.data, 1, 1000, labels.ctypes.data, None, centres.ctypes.data, None,
                             None, None),
                lambda: call(m.handle, None, 0, 500, None, None, None, None, None, None)):
        ctypes.set_errno(0)
        assert one() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for one in (lambda: m.cluster_centres([1, 2], 700), lambda: m.cluster_centres([], 0, attached=False),
                lambda: m.cluster_shapes(refs, 500)):
        with pytest.raises(OSError) as e:
            one()
        assert e.value.errno == errno.ENODEV
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    for method in (m.cluster_centres, m.cluster_shapes):
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
        m.cluster_centres([1], 500)


class _StubLib:
    """Stands where the library stands in a RawMap: records what blurrily_storage_cluster_centres is handed and fills
    the outputs from canned arrays (no GPU is asked for)."""

    def __init__(self, canned):
        self.canned, self.calls = canned, []

    def blurrily_storage_cluster_centres(self, handle, refs, n, mp, labels, degrees, centres, attached, n_clusters, n_edges):
        self.calls.append(dict(refs=refs, n=n, mp=mp, labels=labels, degrees=degrees, centres=centres, attached=attached))
        c = self.canned
        seen = np.ctypeslib.as_array(ctypes.cast(refs, ctypes.POINTER(ctypes.c_uint32)), shape=(n,)) if n else np.zeros(0)
        self.calls[-1]["listed"] = seen.tolist()
        for ptr, key, ctype in ((labels, "labels", ctypes.c_uint32), (degrees, "degrees", ctypes.c_uint32),
                                (centres, "centres", ctypes.c_uint32), (attached, "attached", ctypes.c_uint8)):
            if ptr:
                ctypes.memmove(ptr, np.ascontiguousarray(c[key], dtype=ctype).ctypes.data, n * ctypes.sizeof(ctype))
        n_clusters._obj.value, n_edges._obj.value = c["n_clusters"], c["n_edges"]
        return 0


# references 10 .. 17 and an absent 99: a star {10, 11, 12} around 11, a chain 13 - 14 - 15 - 16 whose centre is 14 and
# whose far end 16 is unattached, a singleton 17
CANNED = dict(labels=[10, 10, 10, 13, 13, 13, 13, 17, NO], degrees=[1, 2, 1, 1, 2, 2, 1, 0, 0],
              centres=[11, 11, 11, 14, 14, 14, 14, 17, NO], attached=[1, 1, 1, 1, 1, 1, 0, 1, 0], n_clusters=3, n_edges=5)
LISTED = [10, 11, 12, 13, 14, 15, 16, 17, 99]


def _stubbed():
    m = RawMap()
    m._real, m._lib = m._lib, _StubLib(CANNED)
    return m


def _unstub(m):
    m._lib = m._real
    m.close()


def test_attached_false_hands_null_and_the_other_pointers_stay():
    m = _stubbed()
    labels, degrees, centres, attached, n_clusters, n_edges = m.cluster_centres(LISTED, 700)
    with_it = m._lib.calls[-1]
    assert with_it["attached"] and with_it["n"] == 9 and with_it["mp"] == 700 and with_it["listed"] == LISTED
    assert attached.dtype == np.uint8 and attached.tolist() == CANNED["attached"]
    assert [a.dtype for a in (labels, degrees, centres)] == [np.uint32] * 3
    assert (labels.tolist(), degrees.tolist(), centres.tolist()) == (CANNED["labels"], CANNED["degrees"], CANNED["centres"])
    assert (n_clusters, n_edges) == (3, 5)
    out = m.cluster_centres(LISTED, 700, attached=False)
    without = m._lib.calls[-1]
    assert without["attached"] is None and out[3] is None
    assert all(without[k] for k in ("refs", "labels", "degrees", "centres")) and without["n"] == 9
    assert (out[0].tolist(), out[1].tolist(), out[2].tolist(), out[4], out[5]) == \
        (CANNED["labels"], CANNED["degrees"], CANNED["centres"], 3, 5)
    empty = m.cluster_centres([], 0)                              # nothing listed: no pointer is handed
    last = m._lib.calls[-1]
    assert last["n"] == 0 and not any(last[k] for k in ("refs", "labels", "degrees", "centres", "attached"))
    assert [len(a) for a in empty[:4]] == [0, 0, 0, 0]
    _unstub(m)


def test_cluster_shapes_over_canned_arrays():
    m = _stubbed()
    want = [dict(label=10, size=3, edges=2, centre=11, attached=3, star=True),
            dict(label=13, size=4, edges=3, centre=14, attached=3, star=False)]
    assert m.cluster_shapes(LISTED, 700) == want
    assert m._lib.calls[-1]["listed"] == LISTED and m._lib.calls[-1]["attached"]
    _unstub(m)
    # a list with repeats and out of order is one node per reference: the stub sees it sorted and without repeats
    m = _stubbed()
    assert m.cluster_shapes(LISTED[::-1] + [12, 10], 700) == want
    assert m._lib.calls[-1]["listed"] == LISTED
    _unstub(m)
