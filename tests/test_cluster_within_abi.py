"""Clusters within blocks, without a GPU: blurrily_storage_cluster_within is exported with its argtypes set, its
prototype agrees with the reference's storage.h in one translation unit and alone, a drifted prototype does not
compile, every argument error -- a reference listed under two block keys among them -- is EINVAL before a GPU is asked
for and leaves the outputs as they were, the same list under consistent keys is not, valid calls fail loudly (ENODEV)
where no GPU is usable, and the Python surface checks its arguments, hands the right pointers and shapes canned arrays
rightly (duplicates_within is numpy over the labels)."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

from blurrily_amd import Map, RawMap, _native
from helpers import compile_c, einval, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster_within.c")
NO = _native.NO_CLUSTER


def test_the_cluster_within_symbol_is_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert " T blurrily_storage_cluster_within\n" in out
    fn = lib.blurrily_storage_cluster_within
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 8
    assert "blurrily_storage_cluster_within" in _native.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "blurrily_storage.h")).read()
    assert ("int blurrily_storage_cluster_within(trigram_map haystack, const uint32_t* references, "
            "const uint32_t* blocks, size_t n,") in header


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_cluster_within_prototype_compiles_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_within_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("was,now", [("const uint32_t*, const uint32_t*, size_t, uint32_t,",
                                      "const uint32_t*, size_t, uint32_t,"),
                                     ("uint32_t*, uint32_t*, uint64_t*) =", "uint32_t*, uint32_t*, uint32_t*) ="),
                                     ("const uint32_t*, size_t, uint32_t,", "const uint32_t*, uint32_t, uint32_t,"),
                                     ("const uint32_t*, const uint32_t*, size_t,",
                                      "const uint32_t*, const uint64_t*, size_t,")],
                         ids=["no_blocks", "edges_as_a_word", "n_as_a_word", "keys_of_64_bits"])
def test_a_drifted_cluster_within_prototype_does_not_compile(tmp_path, was, now):
    write_recorded_storage_h(tmp_path)
    text = open(SRC).read()
    drifted = text.replace(was, now)
    assert drifted != text
    src = tmp_path / "drifted.c"
    src.write_text(drifted)
    assert compile_c(tmp_path, src).returncode != 0


# a shuffled list that names 11 and 14 twice: under one key each (fine), or 14 under two keys (EINVAL)
SHUFFLED = [14, 10, 17, 11, 15, 14, 99, 11]
KEYS_SAME = [2, 1, 3, 1, 2, 2, 5, 1]
KEYS_TWO = [2, 1, 3, 1, 2, 7, 5, 1]


def test_argument_errors_are_einval_before_any_gpu_and_write_nothing():
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs, keys = np.array([1, 2, 3], dtype=np.uint32), np.array([5, 5, 6], dtype=np.uint32)
    labels = np.full(8, 7, dtype=np.uint32)
    n_clusters, n_edges = ctypes.c_uint32(7), ctypes.c_uint64(7)
    counts = (ctypes.byref(n_clusters), ctypes.byref(n_edges))
    call = lib.blurrily_storage_cluster_within
    r, k, lab = refs.ctypes.data, keys.ctypes.data, labels.ctypes.data
    einval(lambda: call(None, r, k, 3, 500, lab, *counts))                          # no map
    einval(lambda: call(m.handle, r, k, 3, 1001, lab, *counts))                     # min_permille > 1000
    einval(lambda: call(m.handle, None, None, 0, 1001, None, *counts))              # ... with nothing listed too
    einval(lambda: call(m.handle, None, k, 3, 500, lab, *counts))                   # references NULL, n > 0
    einval(lambda: call(m.handle, r, None, 3, 500, lab, *counts))                   # blocks NULL, n > 0
    einval(lambda: call(m.handle, r, k, 3, 500, None, *counts))                     # labels NULL, n > 0
    einval(lambda: call(m.handle, r, k, 0xFFFFFFF1, 500, lab, *counts))             # more than a call takes
    einval(lambda: call(m.handle, r, k, 2**64 - 1, 500, lab, *counts))
    einval(lambda: call(m.handle, r, k, 3, 1001, lab, None, None))                  # the counts are optional
    # a reference listed twice under different keys: in a shuffled list, and side by side
    sh, two = np.array(SHUFFLED, dtype=np.uint32), np.array(KEYS_TWO, dtype=np.uint32)
    einval(lambda: call(m.handle, sh.ctypes.data, two.ctypes.data, len(sh), 500, lab, *counts))
    pair, pk = np.array([4, 4], dtype=np.uint32), np.array([0, 1], dtype=np.uint32)
    einval(lambda: call(m.handle, pair.ctypes.data, pk.ctypes.data, 2, 500, lab, None, None))
    einval(lambda: call(m.handle, pair.ctypes.data, pk.ctypes.data, 2, 0, lab, *counts))
    assert n_clusters.value == 7 and n_edges.value == 7                             # nothing written
    assert (labels == 7).all()
    with pytest.raises(OSError) as e:
        m.cluster_within(SHUFFLED, KEYS_TWO, 500)
    assert e.value.errno == errno.EINVAL
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster_within.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs, keys = np.array([1, 2, 3], dtype=np.uint32), np.array([5, 5, 6], dtype=np.uint32)
    labels = np.zeros(8, dtype=np.uint32)
    n_clusters, n_edges = ctypes.c_uint32(0), ctypes.c_uint64(0)
    call = lib.blurrily_storage_cluster_within
    r, k, lab = refs.ctypes.data, keys.ctypes.data, labels.ctypes.data
    # the shuffled list with its repeats under consistent keys is a valid call: ENODEV here, not EINVAL
    sh, same = np.array(SHUFFLED, dtype=np.uint32), np.array(KEYS_SAME, dtype=np.uint32)
    for one in (lambda: call(m.handle, r, k, 3, 500, lab, ctypes.byref(n_clusters), ctypes.byref(n_edges)),
                lambda: call(m.handle, r, k, 3, 0, lab, None, None),
                lambda: call(m.handle, r, k, 3, 1000, lab, None, None),
                lambda: call(m.handle, sh.ctypes.data, same.ctypes.data, len(sh), 500, lab, None, None),
                lambda: call(m.handle, None, None, 0, 500, None, None, None)):
        ctypes.set_errno(0)
        assert one() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for one in (lambda: m.cluster_within([1, 2], [0, 0], 700), lambda: m.cluster_within([], [], 0),
                lambda: m.cluster_within(SHUFFLED, KEYS_SAME, 500), lambda: m.duplicates_within([1, 2], [0, 0], 700)):
        with pytest.raises(OSError) as e:
            one()
        assert e.value.errno == errno.ENODEV
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    with pytest.raises(ValueError):
        m.cluster_within([1], [0], 1001)
    with pytest.raises(OverflowError):
        m.cluster_within([1], [0], -1)
    with pytest.raises(OverflowError):
        m.cluster_within([-1], [0], 500)
    with pytest.raises(OverflowError):
        m.cluster_within([1], [1 << 32], 500)
    with pytest.raises(OverflowError):
        m.cluster_within([1], [-3], 500)
    with pytest.raises(ValueError):
        m.cluster_within([[1, 2]], [0], 500)
    with pytest.raises(ValueError):
        m.cluster_within([1, 2], [0], 500)                        # a key per reference
    with pytest.raises(ValueError):
        m.duplicates_within([1, 2], [0, 0, 0], 500)
    m.close()
    with pytest.raises(RawMap.ClosedError):
        m.cluster_within([1], [0], 500)


class _StubLib:
    """Stands where the library stands in a RawMap: records what blurrily_storage_cluster_within is handed and fills
    the outputs from canned arrays (no GPU is asked for)."""

    def __init__(self, canned):
        self.canned, self.calls = canned, []

    def blurrily_storage_cluster_within(self, handle, refs, keys, n, mp, labels, n_clusters, n_edges):
        u32 = ctypes.POINTER(ctypes.c_uint32)
        seen = lambda p: np.ctypeslib.as_array(ctypes.cast(p, u32), shape=(n,)).tolist() if n else []
        self.calls.append(dict(refs=refs, keys=keys, n=n, mp=mp, labels=labels, listed=seen(refs), listed_keys=seen(keys)))
        c = self.canned
        if labels:
            out = np.array([c["label_of"].get(r, NO) for r in self.calls[-1]["listed"]], dtype=np.uint32)
            ctypes.memmove(labels, out.ctypes.data, 4 * n)
        n_clusters._obj.value, n_edges._obj.value = c["n_clusters"], c["n_edges"]
        return 0


# block 1: {10, 11} together; block 2: {14, 15} together; 17 alone in block 3; 99 is absent
CANNED = dict(label_of={10: 10, 11: 10, 14: 14, 15: 14, 17: 17}, n_clusters=3, n_edges=2)


def _stubbed():
    m = RawMap()
    m._real, m._lib = m._lib, _StubLib(CANNED)
    return m


def _unstub(m):
    m._lib = m._real
    m.close()


def test_cluster_within_hands_every_pointer_and_shapes_the_outputs():
    m = _stubbed()
    labels, n_clusters, n_edges = m.cluster_within(SHUFFLED, KEYS_SAME, 700)
    call = m._lib.calls[-1]
    assert all(call[k] for k in ("refs", "keys", "labels"))
    assert (call["n"], call["mp"]) == (8, 700)
    assert (call["listed"], call["listed_keys"]) == (SHUFFLED, KEYS_SAME)
    assert labels.dtype == np.uint32 and labels.shape == (8,)
    assert labels.tolist() == [14, 10, 17, 10, 14, 14, NO, 10]
    assert (n_clusters, n_edges) == (3, 2) and isinstance(n_clusters, int) and isinstance(n_edges, int)
    # arrays of the right type go as they are; nothing listed hands no pointer
    labels, _, _ = m.cluster_within(np.array(SHUFFLED, dtype=np.uint32), np.array(KEYS_SAME, dtype=np.uint32), 0)
    assert labels.tolist() == [14, 10, 17, 10, 14, 14, NO, 10] and m._lib.calls[-1]["mp"] == 0
    out = m.cluster_within([], [], 1000)
    last = m._lib.calls[-1]
    assert last["n"] == 0 and not any(last[k] for k in ("refs", "keys", "labels"))
    assert out[0].shape == (0,) and out[0].dtype == np.uint32
    _unstub(m)


def test_duplicates_within_groups_the_canned_labels():
    m = _stubbed()
    assert m.duplicates_within(SHUFFLED, KEYS_SAME, 700) == [[10, 11], [14, 15]]
    assert m._lib.calls[-1]["listed"] == SHUFFLED and m._lib.calls[-1]["listed_keys"] == KEYS_SAME
    assert m.duplicates_within([17, 99], [3, 5], 700) == []
    assert m.duplicates_within([], [], 700) == []
    _unstub(m)
