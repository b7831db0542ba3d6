"""Cluster cores within blocks, without a GPU: blurrily_storage_cluster_cores_within is exported with its twelve
argtypes set, its prototype agrees with the reference's storage.h in one translation unit and alone, a drifted prototype
does not compile, every argument error -- a reference listed under two block keys and a count above what a call takes
among them -- is EINVAL before a GPU is asked for and leaves all six outputs as they were, valid calls fail loudly
(ENODEV) where no GPU is usable while a call with nothing listed succeeds, and the Python surface checks its arguments,
hands the right pointers and shapes canned arrays rightly (dense_duplicates_within is numpy over the labels and kinds).
The truth the GPU tests compare with (cluster_cores_within_truth.py) is checked against itself here: all keys equal
against CoresTruth, min_degree 0 against WithinTruth, the per-block truths put back against the whole, and the oracle
haystacks under interleaving keys against the figures the issue gives."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, RawMap, _native
from cluster_cores_truth import BORDER, CORE, NOISE, CoresEdges
from cluster_cores_within_truth import CoresWithinEdges, dense_lists, per_block, telling
from cluster_within_truth import WithinTruth
from helpers import compile_c, einval, oracle_case_inputs, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster_cores_within.c")
NO = _native.NO_CLUSTER


def test_the_cluster_cores_within_symbol_is_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert " T blurrily_storage_cluster_cores_within\n" in out
    fn = lib.blurrily_storage_cluster_cores_within
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 12
    vp, u32, u64 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    assert list(fn.argtypes[1:]) == [vp, vp, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, u32, u64, u64]
    assert "blurrily_storage_cluster_cores_within" in _native.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "blurrily_storage.h")).read()
    assert ("int blurrily_storage_cluster_cores_within(trigram_map haystack, const uint32_t* references, "
            "const uint32_t* blocks,") in header


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_cluster_cores_within_prototype_compiles_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_cores_within_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("was,now", [("const uint32_t*, const uint32_t*, size_t, uint32_t, uint32_t,",
                                      "const uint32_t*, size_t, uint32_t, uint32_t,"),
                                     ("size_t, uint32_t, uint32_t, uint32_t*,", "size_t, uint32_t, uint32_t*,"),
                                     ("uint8_t*, uint32_t*,", "uint32_t*, uint32_t*,"),
                                     ("uint32_t*, uint64_t*, uint64_t*) =", "uint32_t*, uint64_t*, uint32_t*) ="),
                                     ("const uint32_t*, const uint32_t*, size_t,", "const uint32_t*, const uint64_t*, size_t,"),
                                     ("const uint32_t*, size_t, uint32_t, uint32_t,", "const uint32_t*, uint32_t, uint32_t, uint32_t,")],
                         ids=["no_blocks", "no_min_degree", "kinds_as_words", "core_edges_as_a_word", "keys_of_64_bits",
                              "n_as_a_word"])
def test_a_drifted_cluster_cores_within_prototype_does_not_compile(tmp_path, was, now):
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
    labels, degrees = (np.full(8, 7, dtype=np.uint32) for _ in range(2))
    kinds = np.full(8, 7, dtype=np.uint8)
    n_clusters, n_edges, n_core_edges = ctypes.c_uint32(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    out = (degrees.ctypes.data, kinds.ctypes.data, ctypes.byref(n_clusters), ctypes.byref(n_edges),
           ctypes.byref(n_core_edges))
    nothing = (None,) * 5
    call = lib.blurrily_storage_cluster_cores_within
    r, k, lab = refs.ctypes.data, keys.ctypes.data, labels.ctypes.data
    einval(lambda: call(None, r, k, 3, 500, 3, lab, *out))                          # no map
    einval(lambda: call(m.handle, r, k, 3, 1001, 3, lab, *out))                     # min_permille > 1000
    einval(lambda: call(m.handle, None, None, 0, 1001, 0, None, *out))              # ... with nothing listed too
    einval(lambda: call(m.handle, None, k, 3, 500, 3, lab, *out))                   # references NULL, n > 0
    einval(lambda: call(m.handle, r, None, 3, 500, 3, lab, *out))                   # blocks NULL, n > 0
    einval(lambda: call(m.handle, r, k, 3, 500, 3, None, *out))                     # labels NULL, n > 0
    einval(lambda: call(m.handle, r, k, 0xFFFFFFF1, 500, 3, lab, *out))             # more than a call takes
    einval(lambda: call(m.handle, r, k, 2**64 - 1, 500, 3, lab, *out))
    einval(lambda: call(m.handle, r, k, 3, 1001, 0xFFFFFFFF, lab, *nothing))        # the other outputs are optional
    # a reference listed twice under different keys: in a shuffled list, and side by side
    sh, two = np.array(SHUFFLED, dtype=np.uint32), np.array(KEYS_TWO, dtype=np.uint32)
    einval(lambda: call(m.handle, sh.ctypes.data, two.ctypes.data, len(sh), 500, 2, lab, *out))
    pair, pk = np.array([4, 4], dtype=np.uint32), np.array([0, 1], dtype=np.uint32)
    einval(lambda: call(m.handle, pair.ctypes.data, pk.ctypes.data, 2, 500, 0, lab, *nothing))
    einval(lambda: call(m.handle, pair.ctypes.data, pk.ctypes.data, 2, 0, 0xFFFFFFFF, lab, *out))
    assert n_clusters.value == 7 and n_edges.value == 7 and n_core_edges.value == 7   # nothing written
    assert (labels == 7).all() and (degrees == 7).all() and (kinds == 7).all()
    with pytest.raises(OSError) as e:
        m.cluster_cores_within(SHUFFLED, KEYS_TWO, 500, 2)
    assert e.value.errno == errno.EINVAL
    m.close()


def test_nothing_listed_is_success_with_the_counts_given_and_nothing_else_written():
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    call = lib.blurrily_storage_cluster_cores_within
    labels, degrees = (np.full(2, 7, dtype=np.uint32) for _ in range(2))
    kinds = np.full(2, 7, dtype=np.uint8)
    n_clusters, n_edges, n_core_edges = ctypes.c_uint32(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    for min_degree in (0, 3, 0xFFFFFFFF):                     # (any min_degree is valid)
        assert call(m.handle, None, None, 0, 500, min_degree, None, None, None, None, None, None) == 0
    assert call(m.handle, None, None, 0, 1000, 2, labels.ctypes.data, degrees.ctypes.data, kinds.ctypes.data,
                ctypes.byref(n_clusters), None, ctypes.byref(n_core_edges)) == 0
    assert (n_clusters.value, n_edges.value, n_core_edges.value) == (0, 7, 0)       # the counts given, and only those
    assert (labels == 7).all() and (degrees == 7).all() and (kinds == 7).all()
    out = m.cluster_cores_within([], [], 0, 0)
    assert [a.shape for a in out[:3]] == [(0,)] * 3 and out[3:] == (0, 0, 0)
    assert [a.dtype for a in out[:3]] == [np.uint32, np.uint32, np.uint8]
    assert m.dense_duplicates_within([], [], 700, 2) == []
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster_cores_within.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs, keys = np.array([1, 2, 3], dtype=np.uint32), np.array([5, 5, 6], dtype=np.uint32)
    labels, degrees = (np.zeros(8, dtype=np.uint32) for _ in range(2))
    kinds = np.zeros(8, dtype=np.uint8)
    n_clusters, n_edges, n_core_edges = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    call = lib.blurrily_storage_cluster_cores_within
    r, k, lab = refs.ctypes.data, keys.ctypes.data, labels.ctypes.data
    # the shuffled list with its repeats under consistent keys is a valid call: ENODEV here, not EINVAL
    sh, same = np.array(SHUFFLED, dtype=np.uint32), np.array(KEYS_SAME, dtype=np.uint32)
    for one in (lambda: call(m.handle, r, k, 3, 500, 3, lab, degrees.ctypes.data, kinds.ctypes.data,
                             ctypes.byref(n_clusters), ctypes.byref(n_edges), ctypes.byref(n_core_edges)),
                lambda: call(m.handle, r, k, 3, 0, 0, lab, None, None, None, None, None),
                lambda: call(m.handle, r, k, 1, 1000, 0xFFFFFFFF, lab, None, kinds.ctypes.data, None, None, None),
                lambda: call(m.handle, sh.ctypes.data, same.ctypes.data, len(sh), 500, 2, lab, None, None, None, None, None)):
        ctypes.set_errno(0)
        assert one() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for one in (lambda: m.cluster_cores_within([1, 2], [0, 0], 700, 3),
                lambda: m.cluster_cores_within(SHUFFLED, KEYS_SAME, 500, 2),
                lambda: m.dense_duplicates_within([1, 2], [0, 0], 700, 2)):
        with pytest.raises(OSError) as e:
            one()
        assert e.value.errno == errno.ENODEV
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    for method in (m.cluster_cores_within, m.dense_duplicates_within):
        with pytest.raises(ValueError):
            method([1], [0], 1001, 3)
        with pytest.raises(OverflowError):
            method([1], [0], -1, 3)
        with pytest.raises(OverflowError):
            method([1], [0], 500, -1)
        with pytest.raises(OverflowError):
            method([1], [0], 500, 1 << 32)
        with pytest.raises(OverflowError):
            method([-1], [0], 500, 3)
        with pytest.raises(OverflowError):
            method([1], [1 << 32], 500, 3)
        with pytest.raises(OverflowError):
            method([1], [-3], 500, 3)
        with pytest.raises(ValueError):
            method([[1, 2]], [0], 500, 3)
        with pytest.raises(ValueError):
            method([1, 2], [0], 500, 3)                            # a key per reference
        with pytest.raises(ValueError):
            method([1, 2], [0, 0, 0], 500, 3)
    m.close()
    with pytest.raises(RawMap.ClosedError):
        m.cluster_cores_within([1], [0], 500, 3)


class _StubLib:
    """Stands where the library stands in a RawMap: records what blurrily_storage_cluster_cores_within is handed and
    fills the outputs from canned answers by reference (no GPU is asked for)."""

    def __init__(self, canned):
        self.canned, self.calls = canned, []

    def blurrily_storage_cluster_cores_within(self, handle, refs, keys, n, mp, md, labels, degrees, kinds, n_clusters,
                                              n_edges, n_core_edges):
        u32 = ctypes.POINTER(ctypes.c_uint32)
        seen = lambda p: np.ctypeslib.as_array(ctypes.cast(p, u32), shape=(n,)).tolist() if n else []
        self.calls.append(dict(refs=refs, keys=keys, n=n, mp=mp, md=md, labels=labels, degrees=degrees, kinds=kinds,
                               listed=seen(refs), listed_keys=seen(keys)))
        # (n > 0: the three required pointers are never NULL; the optional ones are all handed by the Python surface)
        assert bool(refs) == bool(keys) == bool(labels) == (n > 0)
        assert bool(degrees) == bool(kinds) == (n > 0)
        assert n_clusters is not None and n_edges is not None and n_core_edges is not None
        c = self.canned
        for ptr, key, nothing, ctype in ((labels, "label_of", NO, ctypes.c_uint32), (degrees, "degree_of", 0, ctypes.c_uint32),
                                         (kinds, "kind_of", 0, ctypes.c_uint8)):
            if ptr:
                out = np.array([c[key].get(r, nothing) for r in self.calls[-1]["listed"]], dtype=ctype)
                ctypes.memmove(ptr, out.ctypes.data, n * ctypes.sizeof(ctype))
        n_clusters._obj.value, n_edges._obj.value, n_core_edges._obj.value = c["n_clusters"], c["n_edges"], c["n_core_edges"]
        return 0


# min_degree 2.  Block 1: a triangle {10, 11, 12} with a pendant 13 on 12 (degree 1: a border); block 2: a triangle
# {14, 15, 16}; block 3: a pair 17 - 18 below min_degree (noise); 99 is absent
CANNED = dict(label_of={10: 10, 11: 10, 12: 10, 13: 10, 14: 14, 15: 14, 16: 14, 17: 17, 18: 18},
              degree_of={10: 2, 11: 2, 12: 3, 13: 1, 14: 2, 15: 2, 16: 2, 17: 1, 18: 1},
              kind_of={10: 3, 11: 3, 12: 3, 13: 2, 14: 3, 15: 3, 16: 3, 17: 1, 18: 1},
              n_clusters=2, n_edges=8, n_core_edges=6)
LISTED = [10, 11, 12, 13, 14, 15, 16, 17, 18, 99]
KEYS = [1, 1, 1, 1, 2, 2, 2, 3, 3, 4]


def _stubbed():
    m = RawMap()
    m._real, m._lib = m._lib, _StubLib(CANNED)
    return m


def _unstub(m):
    m._lib = m._real
    m.close()


def test_cluster_cores_within_hands_every_pointer_and_shapes_the_outputs():
    m = _stubbed()
    labels, degrees, kinds, n_clusters, n_edges, n_core_edges = m.cluster_cores_within(LISTED, KEYS, 700, 2)
    call = m._lib.calls[-1]
    assert all(call[k] for k in ("refs", "keys", "labels", "degrees", "kinds"))
    assert (call["n"], call["mp"], call["md"]) == (10, 700, 2)
    assert (call["listed"], call["listed_keys"]) == (LISTED, KEYS)
    assert [a.dtype for a in (labels, degrees, kinds)] == [np.uint32, np.uint32, np.uint8]
    assert [a.shape for a in (labels, degrees, kinds)] == [(10,)] * 3
    assert labels.tolist() == [10, 10, 10, 10, 14, 14, 14, 17, 18, NO]
    assert degrees.tolist() == [2, 2, 3, 1, 2, 2, 2, 1, 1, 0] and kinds.tolist() == [3, 3, 3, 2, 3, 3, 3, 1, 1, 0]
    assert (n_clusters, n_edges, n_core_edges) == (2, 8, 6)
    assert all(isinstance(x, int) for x in (n_clusters, n_edges, n_core_edges))
    # arrays of the right type go as they are; nothing listed hands no pointer
    out = m.cluster_cores_within(np.array(LISTED, dtype=np.uint32), np.array(KEYS, dtype=np.uint32), 0, 0xFFFFFFFF)
    assert out[0].tolist() == labels.tolist() and (m._lib.calls[-1]["mp"], m._lib.calls[-1]["md"]) == (0, 0xFFFFFFFF)
    empty = m.cluster_cores_within([], [], 1000, 0)
    last = m._lib.calls[-1]
    assert last["n"] == 0 and not any(last[k] for k in ("refs", "keys", "labels", "degrees", "kinds"))
    assert [len(a) for a in empty[:3]] == [0, 0, 0]
    _unstub(m)


def test_dense_duplicates_within_over_canned_arrays():
    m = _stubbed()
    want = [[10, 11, 12, 13], [14, 15, 16]]                       # cores and the border, ascending; noise and absent left out
    assert m.dense_duplicates_within(LISTED, KEYS, 700, 2) == want
    last = m._lib.calls[-1]
    assert (last["mp"], last["md"], last["listed"], last["listed_keys"]) == (700, 2, LISTED, KEYS)
    # a list with repeats (under their one key) and out of order gives the same lists, from one call
    calls = len(m._lib.calls)
    assert m.dense_duplicates_within(LISTED[::-1] + [12, 10, 13], KEYS[::-1] + [1, 1, 1], 700, 2) == want
    assert len(m._lib.calls) == calls + 1
    assert m.dense_duplicates_within([17, 18, 99], [3, 3, 4], 700, 2) == []       # noise only
    _unstub(m)


# ---- the truth, against itself

_CASES = {}


def oracle_truth(kind, n):
    if (kind, n) not in _CASES:
        hay, off, _ = oracle_case_inputs(kind, n)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        _CASES[kind, n] = WithinTruth(held), np.arange(1, n + 1, dtype=np.uint32)
    return _CASES[kind, n]


# (haystack, n, modulus, floor, min_degree, edges, core edges, clusters, (big clusters, borders, noise with an edge), torn
# borders, and at other min_degrees (core edges, clusters)): the figures of the issue
TABLE = [("words", 5000, 3, 200, 3, 873, 102, 55, (17, 241, 795), 6, {2: (311, 134)}),
         ("geonames", 8000, 3, 500, 5, 72710, 70270, 74, (62, 648, 1269), 6, {2: (72060, 246), 3: (71434, 135)}),
         ("geonames", 8000, 64, 300, 3, 13206, 11624, 168, (122, 775, 833), 12, {}),
         ("skewed", 6000, 3, 500, 3, 640, 84, 41, (15, 159, 605), 6, {})]


@pytest.mark.parametrize("kind,n,modulus,p,min_degree,edges,core_edges,clusters,has,torn,others", TABLE,
                         ids=[f"{c[0]}-{c[2]}-{c[3]}" for c in TABLE])
def test_the_truth_on_the_oracle_haystacks_is_telling_and_agrees_with_itself(kind, n, modulus, p, min_degree, edges,
                                                                             core_edges, clusters, has, torn, others):
    truth, listed = oracle_truth(kind, n)
    blocks = listed % modulus
    e = CoresWithinEdges(truth, listed, blocks, p, least=p)
    plain = CoresEdges(truth, listed, p, least=p)
    t = e.cores(min_degree)
    print(f"edges {t.n_edges}, core edges {t.n_core_edges}, clusters {t.n_clusters}, "
          f"{(t.big_clusters, t.n_borders, t.noise_with_an_edge)}, torn {t.torn_borders}")
    assert (t.n_edges, t.n_core_edges, t.n_clusters) == (edges, core_edges, clusters)
    assert (t.big_clusters, t.n_borders, t.noise_with_an_edge) == has and t.torn_borders == torn
    assert telling(t, plain.cores(min_degree))
    for md, (ce, cl) in others.items():
        o = e.cores(md)
        assert (o.n_core_edges, o.n_clusters, o.n_edges) == (ce, cl, edges)
    # a degree counts the edges under the node's key only, and no label crosses a key
    assert int(t.degrees.sum()) == 2 * edges and (t.degrees <= plain.cores(min_degree).degrees).all()
    member = t.kinds >= BORDER
    assert (t.labels[member] % modulus == listed[member] % modulus).all()
    assert np.array_equal(t.labels[t.kinds == NOISE], listed[t.kinds == NOISE])
    # min_degree 0: WithinTruth's labels, clusters and edges; every node a core
    zero = e.cores(0)
    w_labels, w_clusters, w_edges, _ = truth.cluster_within(listed, blocks, p, least=p)
    assert np.array_equal(zero.labels, w_labels) and (zero.n_clusters, zero.n_edges) == (w_clusters, w_edges)
    assert zero.n_core_edges == zero.n_edges and (zero.kinds == CORE).all()
    # one CoresTruth per block, put back, equals the whole
    if modulus <= 3:
        for md in (min_degree, 2):
            whole = e.cores(md)
            labels, degrees, kinds, counts = per_block(truth, listed, blocks, p, md, least=p)
            assert np.array_equal(labels, whole.labels) and np.array_equal(degrees, whole.degrees)
            assert np.array_equal(kinds, whole.kinds) and counts == (whole.n_clusters, whole.n_edges, whole.n_core_edges)
        assert dense_lists(t) and all(len({r % modulus for r in g}) == 1 for g in dense_lists(t))


def test_the_truth_with_all_keys_equal_is_cores_truth_and_with_all_keys_distinct_has_no_edge():
    truth, listed = oracle_truth("words", 5000)
    for p, min_degree in ((200, 3), (300, 2)):
        same = CoresWithinEdges(truth, listed, np.full(len(listed), 9), p, least=p).cores(min_degree)
        plain = CoresEdges(truth, listed, p, least=p).cores(min_degree)
        for k in ("labels", "degrees", "kinds"):
            assert np.array_equal(getattr(same, k), getattr(plain, k))
        assert (same.n_clusters, same.n_edges, same.n_core_edges) == (plain.n_clusters, plain.n_edges, plain.n_core_edges)
        assert plain.n_core_edges > 0
        for md in (0, 1):
            alone = CoresWithinEdges(truth, listed, listed[::-1].copy(), p, least=p).cores(md)
            assert np.array_equal(alone.labels, listed) and not alone.degrees.any()
            assert (alone.kinds == (CORE if md == 0 else NOISE)).all()
            assert (alone.n_clusters, alone.n_edges, alone.n_core_edges) == (len(listed) if md == 0 else 0, 0, 0)
