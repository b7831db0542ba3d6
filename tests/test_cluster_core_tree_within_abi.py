"""The cluster core tree within blocks, without a GPU: blurrily_storage_cluster_core_tree_within is exported with its
thirteen argtypes set, its prototype agrees with the reference's storage.h in one translation unit and alone, a drifted
prototype does not compile, every argument error -- a reference listed under two block keys and n = 2^27 + 1 among them
-- is EINVAL before a GPU is asked for and leaves all seven outputs as they were, valid calls fail loudly (ENODEV) where
no GPU is usable, the Python surface checks its arguments, hands the right pointers and shapes canned arrays rightly,
and dense_tree_within, cut_core_tree, tree_by_block and merge_profile serve a canned result.  Last, the definition
itself: the composed truth (tests/cluster_core_tree_within_truth.py) has the figures of DESIGN.md section 44 on the
oracle haystacks, joins no two keys, cut at its heights is the blocked cores' truth there, equals its per-block trees
put back, differs from the unblocked core tree and from the blocked plain tree, and its forest is the one a Boruvka
over the capped edges finds, in the rounds the GPU tests rely on."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, RawMap, _native
import cluster_core_tree_truth as CT
import cluster_tree_truth as TT
from cluster_cores_truth import CORE
from cluster_cores_within_truth import CoresWithinEdges
from cluster_core_tree_within_truth import blocked, blocked_over, per_block, unblocked
from helpers import compile_c, einval, oracle_case_inputs, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster_core_tree_within.c")
NO, NO_CORE = _native.NO_CLUSTER, _native.NO_CORE
NAME = "blurrily_storage_cluster_core_tree_within"


def test_the_cluster_core_tree_within_symbol_is_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert f" T {NAME}\n" in out
    fn = getattr(lib, NAME)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
    assert NAME in _native.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "blurrily_storage.h")).read()
    assert ("int blurrily_storage_cluster_core_tree_within(trigram_map haystack, const uint32_t* references, "
            "const uint32_t* blocks,\n"
            "                                              size_t n, uint32_t min_permille, uint32_t min_degree,\n"
            "                                              uint32_t* labels, uint32_t* core_permille,\n"
            "                                              blurrily_cluster_merge_t* merges, uint32_t* n_merges,\n"
            "                                              uint32_t* n_clusters, uint64_t* n_edges, "
            "uint64_t* n_core_edges);") in header


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_cluster_core_tree_within_prototype_compiles_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_core_tree_within_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("was,now", [("const uint32_t*, const uint32_t*, size_t, uint32_t,",
                                      "const uint32_t*, size_t, uint32_t,"),
                                     ("size_t, uint32_t, uint32_t, uint32_t*, uint32_t*,",
                                      "size_t, uint32_t, uint32_t*, uint32_t*,"),
                                     ("uint32_t, uint32_t, uint32_t*, uint32_t*,\n", "uint32_t, uint32_t, uint32_t*,\n"),
                                     ("const uint32_t*, size_t, uint32_t,", "const uint32_t*, uint32_t, uint32_t,"),
                                     ("blurrily_cluster_merge_t*, uint32_t*, uint32_t*, uint64_t*,",
                                      "uint32_t*, uint32_t*, uint32_t*, uint64_t*,"),
                                     ("uint64_t*, uint64_t*) =", "uint64_t*, uint32_t*) =")],
                         ids=["no_blocks", "no_min_degree", "no_core_permille", "n_as_a_word", "merges_as_words",
                              "core_edges_as_a_word"])
def test_a_drifted_cluster_core_tree_within_prototype_does_not_compile(tmp_path, was, now):
    write_recorded_storage_h(tmp_path)
    text = open(SRC).read()
    drifted = text.replace(was, now)
    assert drifted != text
    src = tmp_path / "drifted.c"
    src.write_text(drifted)
    assert compile_c(tmp_path, src).returncode != 0
    r = compile_c(tmp_path, SRC)                              # (the drift alone is what does not compile)
    assert r.returncode == 0, r.stderr


# a shuffled list that names 11 and 14 twice: under one key each (fine), or 14 under two keys (EINVAL)
SHUFFLED = [14, 10, 17, 11, 15, 14, 99, 11]
KEYS_SAME = [2, 1, 3, 1, 2, 2, 5, 1]
KEYS_TWO = [2, 1, 3, 1, 2, 7, 5, 1]


def test_argument_errors_are_einval_before_any_gpu_and_write_nothing():
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs, keys = np.array([1, 2, 3], dtype=np.uint32), np.array([5, 5, 6], dtype=np.uint32)
    labels, heights = np.full(8, 7, dtype=np.uint32), np.full(8, 7, dtype=np.uint32)
    merges = np.full((8, 3), 7, dtype=np.uint32)
    n_merges, n_clusters, n_edges, n_core = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    counts = (ctypes.byref(n_merges), ctypes.byref(n_clusters), ctypes.byref(n_edges), ctypes.byref(n_core))
    none = (None, None, None, None)
    call = getattr(lib, NAME)
    r, k, lab, cor, mer = refs.ctypes.data, keys.ctypes.data, labels.ctypes.data, heights.ctypes.data, merges.ctypes.data
    einval(lambda: call(None, r, k, 3, 500, 2, lab, cor, mer, *counts))                  # no map
    einval(lambda: call(m.handle, r, k, 3, 1001, 2, lab, cor, mer, *counts))             # min_permille > 1000
    einval(lambda: call(m.handle, None, None, 0, 1001, 2, None, None, None, *counts))    # ... with nothing listed too
    einval(lambda: call(m.handle, None, k, 3, 500, 2, lab, cor, mer, *counts))           # references NULL, n > 0
    einval(lambda: call(m.handle, r, None, 3, 500, 2, lab, cor, mer, *counts))           # blocks NULL, n > 0
    einval(lambda: call(m.handle, r, k, 3, 500, 2, None, cor, mer, *counts))             # labels NULL, n > 0
    einval(lambda: call(m.handle, r, k, 3, 500, 2, lab, None, mer, *counts))             # core_permille NULL, n > 0
    einval(lambda: call(m.handle, r, k, 3, 500, 2, lab, cor, None, *counts))             # merges NULL, n > 0
    einval(lambda: call(m.handle, r, k, (1 << 27) + 1, 500, 2, lab, cor, mer, *counts))  # more than the key's 27 bits number
    einval(lambda: call(m.handle, r, k, 0xFFFFFFF1, 500, 0, lab, cor, mer, *counts))
    einval(lambda: call(m.handle, r, k, 2**64 - 1, 500, 0xFFFFFFFF, lab, cor, mer, *counts))
    einval(lambda: call(m.handle, r, k, 3, 1001, 2, lab, cor, mer, *none))               # the counts are optional
    # a reference listed twice under different keys: in a shuffled list, and side by side; whatever the min_degree
    sh, two = np.array(SHUFFLED, dtype=np.uint32), np.array(KEYS_TWO, dtype=np.uint32)
    einval(lambda: call(m.handle, sh.ctypes.data, two.ctypes.data, len(sh), 500, 2, lab, cor, mer, *counts))
    pair, pk = np.array([4, 4], dtype=np.uint32), np.array([0, 1], dtype=np.uint32)
    einval(lambda: call(m.handle, pair.ctypes.data, pk.ctypes.data, 2, 500, 0, lab, cor, mer, *none))
    einval(lambda: call(m.handle, pair.ctypes.data, pk.ctypes.data, 2, 0, 0xFFFFFFFF, lab, cor, mer, *counts))
    assert (n_merges.value, n_clusters.value, n_edges.value, n_core.value) == (7, 7, 7, 7)   # nothing written
    assert (labels == 7).all() and (heights == 7).all() and (merges == 7).all()
    with pytest.raises(OSError) as e:
        m.cluster_core_tree_within(SHUFFLED, KEYS_TWO, 500, 2)
    assert e.value.errno == errno.EINVAL
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster_core_tree_within.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs, keys = np.array([1, 2, 3], dtype=np.uint32), np.array([5, 5, 6], dtype=np.uint32)
    labels, heights, merges = np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32), np.zeros((8, 3), dtype=np.uint32)
    n_merges, n_clusters, n_edges, n_core = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    none = (None, None, None, None)
    call = getattr(lib, NAME)
    r, k, lab, cor, mer = refs.ctypes.data, keys.ctypes.data, labels.ctypes.data, heights.ctypes.data, merges.ctypes.data
    # the shuffled list with its repeats under consistent keys is a valid call: ENODEV here, not EINVAL
    sh, same = np.array(SHUFFLED, dtype=np.uint32), np.array(KEYS_SAME, dtype=np.uint32)
    for one in (lambda: call(m.handle, r, k, 3, 500, 2, lab, cor, mer, ctypes.byref(n_merges), ctypes.byref(n_clusters),
                             ctypes.byref(n_edges), ctypes.byref(n_core)),
                lambda: call(m.handle, r, k, 3, 0, 0, lab, cor, mer, *none),
                lambda: call(m.handle, r, k, 3, 1000, 0xFFFFFFFF, lab, cor, mer, *none),    # any min_degree
                lambda: call(m.handle, sh.ctypes.data, same.ctypes.data, len(sh), 500, 3, lab, cor, mer, *none),
                lambda: call(m.handle, None, None, 0, 500, 2, None, None, None, *none)):   # (n == 0 asks for the map too)
        ctypes.set_errno(0)
        assert one() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for one in (lambda: m.cluster_core_tree_within([1, 2], [0, 0], 700, 2),
                lambda: m.cluster_core_tree_within([], [], 0, 0),
                lambda: m.cluster_core_tree_within(SHUFFLED, KEYS_SAME, 1000, 2**32 - 1)):
        with pytest.raises(OSError) as e:
            one()
        assert e.value.errno == errno.ENODEV
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    with pytest.raises(ValueError):
        m.cluster_core_tree_within([1], [0], 1001, 2)
    with pytest.raises(OverflowError):
        m.cluster_core_tree_within([1], [0], -1, 2)
    with pytest.raises(OverflowError):
        m.cluster_core_tree_within([1], [0], 500, -1)
    with pytest.raises(OverflowError):
        m.cluster_core_tree_within([1], [0], 500, 1 << 32)
    with pytest.raises(OverflowError):
        m.cluster_core_tree_within([-1], [0], 500, 2)
    with pytest.raises(OverflowError):
        m.cluster_core_tree_within([1 << 32], [0], 500, 2)
    with pytest.raises(OverflowError):
        m.cluster_core_tree_within([1], [1 << 32], 500, 2)
    with pytest.raises(OverflowError):
        m.cluster_core_tree_within([1], [-3], 500, 2)
    with pytest.raises(ValueError):
        m.cluster_core_tree_within([[1, 2]], [0], 500, 2)
    with pytest.raises(ValueError):
        m.cluster_core_tree_within([1, 2], [0], 500, 2)           # a key per reference
    with pytest.raises(ValueError):
        m.dense_tree_within([1], [0], 1001, 2)
    with pytest.raises(ValueError):
        m.dense_tree_within([1, 2], [0], 500, 2)
    with pytest.raises(ValueError):
        m.dense_tree_within(SHUFFLED, KEYS_TWO, 500, 2)           # a reference under two keys: before the library is asked
    m.close()
    with pytest.raises(RawMap.ClosedError):
        m.cluster_core_tree_within([1], [0], 500, 2)


class _StubLib:
    """Stands where the library stands in a RawMap: records what blurrily_storage_cluster_core_tree_within is handed and
    fills the outputs from canned arrays (no GPU is asked for)."""

    def __init__(self, canned):
        self.canned, self.calls = canned, []

    def blurrily_storage_cluster_core_tree_within(self, handle, refs, keys, n, mp, md, labels, core, merges, n_merges,
                                                  n_clusters, n_edges, n_core_edges):
        u32 = ctypes.POINTER(ctypes.c_uint32)
        seen = lambda p: np.ctypeslib.as_array(ctypes.cast(p, u32), shape=(n,)).tolist() if n else []
        listed = seen(refs)
        self.calls.append(dict(refs=refs, keys=keys, n=n, mp=mp, md=md, labels=labels, core=core, merges=merges,
                               listed=listed, listed_keys=seen(keys)))
        c = self.canned
        for to, of, none in ((labels, c["label_of"], NO), (core, c["core_of"], NO_CORE)):
            if to:
                out = np.array([of.get(r, none) for r in listed], dtype=np.uint32)
                ctypes.memmove(to, out.ctypes.data, 4 * n)
        rows = np.array(c["merges"], dtype=np.uint32).reshape(-1, 3)
        if merges and len(rows):
            assert len(rows) <= n                                                   # (room for n records was handed)
            ctypes.memmove(merges, rows.ctypes.data, rows.nbytes)
        n_merges._obj.value, n_clusters._obj.value = len(rows), c["n_clusters"]
        n_edges._obj.value, n_core_edges._obj.value = c["n_edges"], c["n_core_edges"]
        return 0


# a hand-made result at floor 300, min_degree 2.  Block 1: 10, 11 and 12 have core heights and hang together from 800
# down to 600.  Block 2: 14 and 15 join at 450; 16 is a node of one edge (no core height).  17 is alone in block 3, 99 is
# absent.
CORE_OF = {10: 800, 11: 900, 12: 600, 14: 450, 15: 500, 16: NO_CORE, 17: NO_CORE}
RECORDS = [(10, 11, 800), (11, 12, 600), (14, 15, 450)]
CANNED = dict(label_of={10: 10, 11: 10, 12: 10, 14: 14, 15: 14, 16: 16, 17: 17}, core_of=CORE_OF, merges=RECORDS,
              n_clusters=2, n_edges=5, n_core_edges=4)
LISTED = [14, 10, 17, 11, 15, 14, 99, 11, 12, 16]
KEYS = [2, 1, 3, 1, 2, 2, 5, 1, 1, 2]


def _stubbed(cls=RawMap):
    m = cls()
    m._real, m._lib = m._lib, _StubLib(CANNED)
    return m


def _unstub(m):
    m._lib = m._real
    m.close()


def test_cluster_core_tree_within_hands_every_pointer_and_shapes_the_outputs():
    m = _stubbed()
    labels, core, merges, n_clusters, n_edges, n_core_edges = m.cluster_core_tree_within(LISTED, KEYS, 300, 2)
    call = m._lib.calls[-1]
    pointers = ("refs", "keys", "labels", "core", "merges")
    assert all(call[k] for k in pointers) and len({call[k] for k in pointers}) == 5
    assert (call["n"], call["mp"], call["md"]) == (10, 300, 2)
    assert (call["listed"], call["listed_keys"]) == (LISTED, KEYS)
    assert labels.dtype == np.uint32 and labels.tolist() == [14, 10, 17, 10, 14, 14, NO, 10, 10, 16]
    assert core.dtype == np.uint32 and core.tolist() == [450, 800, NO_CORE, 900, 500, 450, NO_CORE, 900, 600, NO_CORE]
    assert merges.dtype == np.uint32 and merges.shape == (3, 3) and merges.tolist() == [list(e) for e in RECORDS]
    assert (n_clusters, n_edges, n_core_edges) == (2, 5, 4)
    assert all(isinstance(x, int) for x in (n_clusters, n_edges, n_core_edges))
    # arrays of the right type go as they are; any min_degree goes through; nothing listed hands no pointer
    m.cluster_core_tree_within(np.array(LISTED, dtype=np.uint32), np.array(KEYS, dtype=np.uint32), 0, 2**32 - 1)
    assert (m._lib.calls[-1]["mp"], m._lib.calls[-1]["md"]) == (0, 2**32 - 1)
    m._lib.canned = dict(label_of={}, core_of={}, merges=[], n_clusters=0, n_edges=0, n_core_edges=0)
    out = m.cluster_core_tree_within([], [], 1000, 0)
    last = m._lib.calls[-1]
    assert last["n"] == 0 and not any(last[k] for k in pointers)
    assert [x.shape for x in out[:3]] == [(0,), (0,), (0, 3)] and all(x.dtype == np.uint32 for x in out[:3])
    assert out[3:] == (0, 0, 0)
    _unstub(m)


def test_dense_tree_within_lists_each_pair_once_and_the_record_functions_serve_the_result_unchanged():
    m = _stubbed(Map)
    refs, keys, labels, core, merges = m.dense_tree_within(LISTED, KEYS, 300, 2)
    call = m._lib.calls[-1]
    assert call["listed"] == [10, 11, 12, 14, 15, 16, 17, 99] == refs.tolist()
    assert call["listed_keys"] == [1, 1, 1, 2, 2, 2, 3, 5] == keys.tolist()
    assert refs.dtype == keys.dtype == np.uint32
    assert labels.tolist() == [10, 10, 10, 14, 14, 16, 17, NO]
    assert core.tolist() == [800, 900, 600, 450, 500, NO_CORE, NO_CORE, NO_CORE]
    assert merges.tolist() == [list(e) for e in RECORDS]
    # cut_core_tree: the cores and their labels at any floor from the tree's up
    for floor, want, cores in ((300, [10, 10, 10, 14, 14, 16, 17, NO], {10, 11, 12, 14, 15}),
                               (451, [10, 10, 10, 14, 15, 16, 17, NO], {10, 11, 12, 15}),
                               (601, [10, 10, 12, 14, 15, 16, 17, NO], {10, 11}),
                               (801, [10, 11, 12, 14, 15, 16, 17, NO], {11}),
                               (901, [10, 11, 12, 14, 15, 16, 17, NO], set())):
        at, is_core = RawMap.cut_core_tree(refs, labels, core, merges, floor, min_permille=300)
        assert at.tolist() == want and set(refs[is_core].tolist()) == cores, floor
    # ... and over the list as the caller gave it, from the raw call
    raw = RawMap.cluster_core_tree_within(m, LISTED, KEYS, 300, 2)
    at, is_core = RawMap.cut_core_tree(LISTED, raw[0], raw[1], raw[2], 601, min_permille=300)
    assert at.tolist() == [14, 10, 17, 10, 15, 14, NO, 10, 12, 16]
    assert is_core.tolist() == [False, True, False, True, False, False, False, True, False, False]
    # tree_by_block: the records by key, in the tree's order; merge_profile: the records as they are
    by_block = RawMap.tree_by_block(merges, refs, keys)
    assert sorted(by_block) == [1, 2]
    assert by_block[1].tolist() == [[10, 11, 800], [11, 12, 600]] and by_block[2].tolist() == [[14, 15, 450]]
    assert {k: v.tolist() for k, v in RawMap.tree_by_block(raw[2], LISTED, KEYS).items()} == \
        {k: v.tolist() for k, v in by_block.items()}
    assert RawMap.merge_profile(merges, nodes=5) == [{"permille": 800, "merges": 1, "n_clusters": 4},
                                                     {"permille": 600, "merges": 2, "n_clusters": 3},
                                                     {"permille": 450, "merges": 3, "n_clusters": 2}]
    # one call per dense_tree_within, whatever the list's shape
    calls = len(m._lib.calls)
    again = m.dense_tree_within(LISTED[::-1], KEYS[::-1], 300, 2)
    assert len(m._lib.calls) == calls + 1 and m._lib.calls[-1]["listed"] == refs.tolist()
    assert all(np.array_equal(x, y) for x, y in zip(again, (refs, keys, labels, core, merges)))
    _unstub(m)


# ---- the truth, against itself

_CASES = {}


def oracle_truth(kind, n, modulus):
    """(the blocked truth under reference % modulus, the plain truth that shares its tokenisations and pairs, the list, the
    keys), made once."""
    if (kind, n, modulus) not in _CASES:
        hay, off, _ = oracle_case_inputs(kind, n)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        listed = np.arange(1, n + 1, dtype=np.uint32)
        blocks = (listed % modulus).astype(np.uint32)
        truth = blocked(held, listed, blocks)
        _CASES[kind, n, modulus] = (truth, unblocked(truth), listed, blocks)
    return _CASES[kind, n, modulus]


def capped_edges(t, truth, listed):
    """A CoreTreeTruth's tree edges again: (lo, hi, H) by index into truth.refs, from its core heights."""
    lo, hi, h = CT.edges(truth, listed, t.p)
    tree = (t.c[lo] >= 0) & (t.c[hi] >= 0)
    lo, hi, h = lo[tree], hi[tree], h[tree]
    return lo, hi, np.minimum(h, np.minimum(t.c[lo], t.c[hi]))


def boruvka(n, lo, hi, H):
    """Boruvka over weighted edges under the total order (H descending, lo ascending, hi ascending): every round each
    component takes the best edge that leaves it.  Returns (the forest as a set of (lo, hi, H), the rounds that
    merged something)."""
    key = ((1000 - H).astype(np.uint64) << np.uint64(2 * CT.BITS)) | (lo.astype(np.uint64) << np.uint64(CT.BITS)) | \
        hi.astype(np.uint64)
    comp = np.arange(n)
    forest, rounds = set(), 0
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    while True:
        cl, ch = comp[lo], comp[hi]
        out = cl != ch
        if not out.any():
            return forest, rounds
        best = np.full(n, none, dtype=np.uint64)
        np.minimum.at(best, cl[out], key[out])
        np.minimum.at(best, ch[out], key[out])
        chosen = np.unique(best[best != none])
        rounds += 1
        parent = list(range(n))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for k in chosen.tolist():
            a, b = (k >> CT.BITS) & CT.MASK, k & CT.MASK
            ra, rb = find(int(comp[a])), find(int(comp[b]))
            assert ra != rb                                   # (distinct keys: the chosen edges hold no cycle)
            parent[max(ra, rb)] = min(ra, rb)
            forest.add((a, b, 1000 - (k >> (2 * CT.BITS))))
        comp = np.array([find(int(c)) for c in comp.tolist()])


# (haystack, n, modulus, floor, min_degree, merges, heights, clusters, edges, core edges, cores, the records of
# cluster_tree_within's truth on the same input, the Boruvka rounds): the figures of DESIGN.md section 44
TABLE = [("words", 5000, 3, 200, 2, 222, 9, 134, 873, 311, 356, 784, 3),
         ("words", 5000, 3, 200, 3, 71, 6, 55, 873, 102, 126, 784, 2),
         ("geonames", 8000, 3, 500, 5, 2780, 74, 74, 72710, 70270, 2854, 4257, None),
         ("geonames", 8000, 64, 300, 3, 2687, 101, 168, 13206, 11624, 2855, 3966, None),
         ("skewed", 6000, 3, 500, 3, 59, 4, 41, 640, 84, 100, 575, None)]


@pytest.mark.parametrize("kind,n,modulus,p,min_degree,merges,heights,clusters,edges,core_edges,cores,plain_records,rounds",
                         TABLE, ids=[f"{c[0]}-{c[2]}-{c[3]}-{c[4]}" for c in TABLE])
def test_the_truth_on_the_oracle_haystacks_has_the_designs_figures_and_agrees_with_itself(
        kind, n, modulus, p, min_degree, merges, heights, clusters, edges, core_edges, cores, plain_records, rounds):
    truth, plain, listed, blocks = oracle_truth(kind, n, modulus)
    t = CT.CoreTreeTruth(truth, listed, p, min_degree)
    got_heights = np.unique(t.merges[:, 2]).tolist()
    print(f"merges {len(t.merges)}, heights {len(got_heights)}, clusters {t.n_clusters}, edges {t.n_edges}, "
          f"core edges {t.n_core_edges}, cores {int((t.c >= 0).sum())}")
    assert (len(t.merges), len(got_heights), t.n_clusters, t.n_edges, t.n_core_edges, int((t.c >= 0).sum())) == \
        (merges, heights, clusters, edges, core_edges, cores)
    assert len(t.merges) == cores - clusters
    # the records in the total order, none across two keys
    rows = t.merges.tolist()
    keys = [(-h, a, b) for a, b, h in rows]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and all(a < b for a, b, _ in rows)
    assert all(a % modulus == b % modulus for a, b, _ in rows)
    # cuts at the floor and at about five of the heights, and one per mille above each: the blocked cores' truth there
    at = [got_heights[i] for i in sorted({int(i) for i in np.linspace(0, len(got_heights) - 1, 5).round()})]
    for f in [p] + [f for h in at for f in (h, h + 1)]:
        if f > 1000:
            continue
        is_core, label_of, n_clusters = t.cut(f)
        want = CoresWithinEdges(plain, listed, blocks, f, least=p).cores(min_degree)
        want_core = {r for r, k in want.kind_of.items() if k == CORE}
        assert set(truth.refs[is_core].tolist()) == want_core, f
        assert label_of == {r: want.label_of[r] for r in want_core}, f
        assert n_clusters == want.n_clusters, f
        if f == p:
            assert (want.n_clusters, want.n_edges, want.n_core_edges) == (clusters, edges, core_edges)
        cut, core = RawMap.cut_core_tree(listed, t.labels, t.core_permille, t.merges, f, min_permille=p)
        assert set(listed[core].tolist()) == want_core and dict(zip(listed[core].tolist(), cut[core].tolist())) == label_of
    by_block = RawMap.tree_by_block(t.merges, listed, blocks)
    assert sum(len(v) for v in by_block.values()) == merges and all(k < modulus for k in by_block)
    # the keys tell, and so do the cores: other records than the unblocked core tree's and than the blocked plain tree's
    whole = CT.CoreTreeTruth(unblocked(truth), listed, p, min_degree)
    assert whole.merges.tobytes() != t.merges.tobytes() and whole.n_edges > edges
    single = TT.kruskal(truth, listed, p)
    assert len(single) == plain_records and single.tobytes() != t.merges.tobytes()
    # min_degree 0 and 1 are the blocked plain tree
    for md in (0, 1):
        low = CT.CoreTreeTruth(truth, listed, p, md)
        assert low.merges.tobytes() == single.tobytes()
        assert md or ((low.core_permille == 1000).all() and (low.n_edges, low.n_core_edges) == (edges, edges))
    # a Boruvka over the capped edges finds the Kruskal forest
    index = {int(r): i for i, r in enumerate(truth.refs.tolist())}
    forest, took = boruvka(len(truth.refs), *capped_edges(t, truth, listed))
    assert forest == {(index[a], index[b], h) for a, b, h in rows}
    print("rounds", took)
    if rounds is not None:
        assert took == rounds                                 # (what the GPU file's rounds test stands on)
    # one core tree per block over the plain truth, put back, is the whole (last: a block's list takes the pairs' place)
    labels, core, records, counts = per_block(plain, listed, blocks, p, min_degree)
    assert np.array_equal(labels, t.labels) and np.array_equal(core, t.core_permille)
    assert np.array_equal(records, t.merges) and counts == (clusters, edges, core_edges)


def test_all_keys_equal_is_the_core_tree_and_all_keys_distinct_has_no_core():
    truth, plain, listed, _ = oracle_truth("words", 5000, 3)
    same = CT.CoreTreeTruth(blocked_over(plain, listed, np.full(len(listed), 9)), listed, 200, 2)
    whole = CT.CoreTreeTruth(plain, listed, 200, 2)
    for k in ("labels", "core_permille", "merges"):
        assert getattr(same, k).tobytes() == getattr(whole, k).tobytes()
    assert (same.n_clusters, same.n_edges, same.n_core_edges) == (whole.n_clusters, whole.n_edges, whole.n_core_edges)
    assert len(whole.merges) > 0
    for md in (1, 3):
        alone = CT.CoreTreeTruth(blocked_over(plain, listed, listed[::-1].copy()), listed, 200, md)
        assert alone.merges.shape == (0, 3) and (alone.core_permille == NO_CORE).all()
        assert np.array_equal(alone.labels, listed)
        assert (alone.n_clusters, alone.n_edges, alone.n_core_edges) == (0, 0, 0)

