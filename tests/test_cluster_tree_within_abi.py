"""The cluster tree within blocks, without a GPU: blurrily_storage_cluster_tree_within is exported with its ten argtypes
set, its prototype agrees with the reference's storage.h in one translation unit and alone, a drifted prototype does not
compile, every argument error -- a reference listed under two block keys and n = 2^27 + 1 among them -- is EINVAL before
a GPU is asked for and leaves all five outputs as they were, valid calls fail loudly (ENODEV) where no GPU is usable, the
Python surface checks its arguments, hands the right pointers and shapes canned arrays rightly, and tree_by_block --
numpy over the records -- splits them by key and refuses what it cannot place.  The blocked truth's two spanning forests
(Kruskal's and Boruvka's of tests/cluster_tree_truth.py over tests/cluster_tree_within_truth.py's pairs) agree on the
blocked inputs the GPU tests use, and need the rounds those tests rely on."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, RawMap, _native
import cluster_tree_truth as TT
from cluster_tree_within_truth import blocked, per_block
from cluster_truth import Truth
from helpers import ORACLE_CASES, compile_c, einval, oracle_case_inputs, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster_tree_within.c")
NO = _native.NO_CLUSTER


def test_the_cluster_tree_within_symbol_is_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert " T blurrily_storage_cluster_tree_within\n" in out
    fn = lib.blurrily_storage_cluster_tree_within
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10
    assert "blurrily_storage_cluster_tree_within" in _native.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "blurrily_storage.h")).read()
    assert ("int blurrily_storage_cluster_tree_within(trigram_map haystack, const uint32_t* references, "
            "const uint32_t* blocks,\n"
            "                                         size_t n, uint32_t min_permille, uint32_t* labels,\n"
            "                                         blurrily_cluster_merge_t* merges, uint32_t* n_merges,\n"
            "                                         uint32_t* n_clusters, uint64_t* n_edges);") in header


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_cluster_tree_within_prototype_compiles_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_tree_within_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("was,now", [("const uint32_t*, const uint32_t*, size_t, uint32_t,",
                                      "const uint32_t*, size_t, uint32_t,"),
                                     ("const uint32_t*, size_t, uint32_t,", "const uint32_t*, uint32_t, uint32_t,"),
                                     ("uint32_t*, blurrily_cluster_merge_t*,", "uint32_t*, uint32_t*,"),
                                     ("uint32_t*, uint64_t*) =", "uint32_t*, uint32_t*) =")],
                         ids=["no_blocks", "n_as_a_word", "merges_as_words", "edges_as_a_word"])
def test_a_drifted_cluster_tree_within_prototype_does_not_compile(tmp_path, was, now):
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
    labels = np.full(8, 7, dtype=np.uint32)
    merges = np.full((8, 3), 7, dtype=np.uint32)
    n_merges, n_clusters, n_edges = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint64(7)
    counts = (ctypes.byref(n_merges), ctypes.byref(n_clusters), ctypes.byref(n_edges))
    call = lib.blurrily_storage_cluster_tree_within
    r, k, lab, mer = refs.ctypes.data, keys.ctypes.data, labels.ctypes.data, merges.ctypes.data
    einval(lambda: call(None, r, k, 3, 500, lab, mer, *counts))                     # no map
    einval(lambda: call(m.handle, r, k, 3, 1001, lab, mer, *counts))                # min_permille > 1000
    einval(lambda: call(m.handle, None, None, 0, 1001, None, None, *counts))        # ... with nothing listed too
    einval(lambda: call(m.handle, None, k, 3, 500, lab, mer, *counts))              # references NULL, n > 0
    einval(lambda: call(m.handle, r, None, 3, 500, lab, mer, *counts))              # blocks NULL, n > 0
    einval(lambda: call(m.handle, r, k, 3, 500, None, mer, *counts))                # labels NULL, n > 0
    einval(lambda: call(m.handle, r, k, 3, 500, lab, None, *counts))                # merges NULL, n > 0
    einval(lambda: call(m.handle, r, k, (1 << 27) + 1, 500, lab, mer, *counts))     # more than the key's 27 bits number
    einval(lambda: call(m.handle, r, k, 0xFFFFFFF1, 500, lab, mer, *counts))
    einval(lambda: call(m.handle, r, k, 2**64 - 1, 500, lab, mer, *counts))
    einval(lambda: call(m.handle, r, k, 3, 1001, lab, mer, None, None, None))       # the counts are optional
    # a reference listed twice under different keys: in a shuffled list, and side by side
    sh, two = np.array(SHUFFLED, dtype=np.uint32), np.array(KEYS_TWO, dtype=np.uint32)
    einval(lambda: call(m.handle, sh.ctypes.data, two.ctypes.data, len(sh), 500, lab, mer, *counts))
    pair, pk = np.array([4, 4], dtype=np.uint32), np.array([0, 1], dtype=np.uint32)
    einval(lambda: call(m.handle, pair.ctypes.data, pk.ctypes.data, 2, 500, lab, mer, None, None, None))
    einval(lambda: call(m.handle, pair.ctypes.data, pk.ctypes.data, 2, 0, lab, mer, *counts))
    assert (n_merges.value, n_clusters.value, n_edges.value) == (7, 7, 7)           # nothing written
    assert (labels == 7).all() and (merges == 7).all()
    with pytest.raises(OSError) as e:
        m.cluster_tree_within(SHUFFLED, KEYS_TWO, 500)
    assert e.value.errno == errno.EINVAL
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster_tree_within.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    refs, keys = np.array([1, 2, 3], dtype=np.uint32), np.array([5, 5, 6], dtype=np.uint32)
    labels, merges = np.zeros(8, dtype=np.uint32), np.zeros((8, 3), dtype=np.uint32)
    n_merges, n_clusters, n_edges = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
    call = lib.blurrily_storage_cluster_tree_within
    r, k, lab, mer = refs.ctypes.data, keys.ctypes.data, labels.ctypes.data, merges.ctypes.data
    # the shuffled list with its repeats under consistent keys is a valid call: ENODEV here, not EINVAL
    sh, same = np.array(SHUFFLED, dtype=np.uint32), np.array(KEYS_SAME, dtype=np.uint32)
    for one in (lambda: call(m.handle, r, k, 3, 500, lab, mer, ctypes.byref(n_merges), ctypes.byref(n_clusters),
                             ctypes.byref(n_edges)),
                lambda: call(m.handle, r, k, 3, 0, lab, mer, None, None, None),
                lambda: call(m.handle, r, k, 3, 1000, lab, mer, None, None, None),
                lambda: call(m.handle, sh.ctypes.data, same.ctypes.data, len(sh), 500, lab, mer, None, None, None),
                lambda: call(m.handle, None, None, 0, 500, None, None, None, None, None)):
        ctypes.set_errno(0)
        assert one() == -1
        assert ctypes.get_errno() == errno.ENODEV
    for one in (lambda: m.cluster_tree_within([1, 2], [0, 0], 700), lambda: m.cluster_tree_within([], [], 0),
                lambda: m.cluster_tree_within(SHUFFLED, KEYS_SAME, 1000)):
        with pytest.raises(OSError) as e:
            one()
        assert e.value.errno == errno.ENODEV
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    with pytest.raises(ValueError):
        m.cluster_tree_within([1], [0], 1001)
    with pytest.raises(OverflowError):
        m.cluster_tree_within([1], [0], -1)
    with pytest.raises(OverflowError):
        m.cluster_tree_within([-1], [0], 500)
    with pytest.raises(OverflowError):
        m.cluster_tree_within([1 << 32], [0], 500)
    with pytest.raises(OverflowError):
        m.cluster_tree_within([1], [1 << 32], 500)
    with pytest.raises(OverflowError):
        m.cluster_tree_within([1], [-3], 500)
    with pytest.raises(ValueError):
        m.cluster_tree_within([[1, 2]], [0], 500)
    with pytest.raises(ValueError):
        m.cluster_tree_within([1, 2], [0], 500)                   # a key per reference
    m.close()
    with pytest.raises(RawMap.ClosedError):
        m.cluster_tree_within([1], [0], 500)


class _StubLib:
    """Stands where the library stands in a RawMap: records what blurrily_storage_cluster_tree_within is handed and
    fills the outputs from canned arrays (no GPU is asked for)."""

    def __init__(self, canned):
        self.canned, self.calls = canned, []

    def blurrily_storage_cluster_tree_within(self, handle, refs, keys, n, mp, labels, merges, n_merges, n_clusters,
                                             n_edges):
        u32 = ctypes.POINTER(ctypes.c_uint32)
        seen = lambda p: np.ctypeslib.as_array(ctypes.cast(p, u32), shape=(n,)).tolist() if n else []
        self.calls.append(dict(refs=refs, keys=keys, n=n, mp=mp, labels=labels, merges=merges, listed=seen(refs),
                               listed_keys=seen(keys)))
        c = self.canned
        if labels:
            out = np.array([c["label_of"].get(r, NO) for r in self.calls[-1]["listed"]], dtype=np.uint32)
            ctypes.memmove(labels, out.ctypes.data, 4 * n)
        rows = np.array(c["merges"], dtype=np.uint32).reshape(-1, 3)
        if merges and len(rows):
            assert len(rows) <= n                                                   # (room for n records was handed)
            ctypes.memmove(merges, rows.ctypes.data, rows.nbytes)
        n_merges._obj.value, n_clusters._obj.value, n_edges._obj.value = len(rows), c["n_clusters"], c["n_edges"]
        return 0


# block 1: {10, 11} together at 800; block 2: {14, 15} together at 900; 17 alone in block 3; 99 is absent
RECORDS = [(14, 15, 900), (10, 11, 800)]
CANNED = dict(label_of={10: 10, 11: 10, 14: 14, 15: 14, 17: 17}, merges=RECORDS, n_clusters=3, n_edges=2)


def _stubbed():
    m = RawMap()
    m._real, m._lib = m._lib, _StubLib(CANNED)
    return m


def _unstub(m):
    m._lib = m._real
    m.close()


def test_cluster_tree_within_hands_every_pointer_and_shapes_the_outputs():
    m = _stubbed()
    labels, merges, n_clusters, n_edges = m.cluster_tree_within(SHUFFLED, KEYS_SAME, 700)
    call = m._lib.calls[-1]
    assert all(call[k] for k in ("refs", "keys", "labels", "merges"))
    assert (call["n"], call["mp"]) == (8, 700)
    assert (call["listed"], call["listed_keys"]) == (SHUFFLED, KEYS_SAME)
    assert labels.dtype == np.uint32 and labels.shape == (8,)
    assert labels.tolist() == [14, 10, 17, 10, 14, 14, NO, 10]
    assert merges.dtype == np.uint32 and merges.shape == (2, 3) and merges.tolist() == [list(e) for e in RECORDS]
    assert (n_clusters, n_edges) == (3, 2) and isinstance(n_clusters, int) and isinstance(n_edges, int)
    # cut_tree and merge_profile serve the result as they are
    assert RawMap.cut_tree(SHUFFLED, labels, merges, 801, min_permille=700).tolist() == [14, 10, 17, 11, 14, 14, NO, 11]
    assert RawMap.merge_profile(merges, nodes=5) == [{"permille": 900, "merges": 1, "n_clusters": 4},
                                                     {"permille": 800, "merges": 2, "n_clusters": 3}]
    # arrays of the right type go as they are; nothing listed hands no pointer
    labels, merges, _, _ = m.cluster_tree_within(np.array(SHUFFLED, dtype=np.uint32),
                                                 np.array(KEYS_SAME, dtype=np.uint32), 0)
    assert labels.tolist() == [14, 10, 17, 10, 14, 14, NO, 10] and m._lib.calls[-1]["mp"] == 0
    m._lib.canned = dict(label_of={}, merges=[], n_clusters=0, n_edges=0)
    out = m.cluster_tree_within([], [], 1000)
    last = m._lib.calls[-1]
    assert last["n"] == 0 and not any(last[k] for k in ("refs", "keys", "labels", "merges"))
    assert out[0].shape == (0,) and out[0].dtype == np.uint32 and out[1].shape == (0, 3) and out[1].dtype == np.uint32
    assert out[2:] == (0, 0)
    _unstub(m)


def test_tree_by_block_splits_canned_records_by_key_in_the_trees_order():
    records = [(14, 15, 900), (10, 11, 800), (14, 20, 800), (11, 12, 300)]
    refs, keys = [20, 14, 10, 17, 11, 15, 14, 99, 12], [2, 2, 1, 3, 1, 2, 2, 5, 1]
    got = RawMap.tree_by_block(records, refs, keys)
    assert sorted(got) == [1, 2] and all(v.dtype == np.uint32 and v.shape[1] == 3 for v in got.values())
    assert got[1].tolist() == [[10, 11, 800], [11, 12, 300]] and got[2].tolist() == [[14, 15, 900], [14, 20, 800]]
    assert all(isinstance(k, int) for k in got)
    # arrays go as they are; the greatest key is a key like any other
    got = RawMap.tree_by_block(np.array(records[:1], dtype=np.uint32), np.array([14, 15], dtype=np.uint32),
                               np.array([0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32))
    assert list(got) == [0xFFFFFFFF] and got[0xFFFFFFFF].tolist() == [[14, 15, 900]]
    assert RawMap.tree_by_block([], refs, keys) == {} and RawMap.tree_by_block([], [], []) == {}
    with pytest.raises(ValueError):
        RawMap.tree_by_block([(14, 10, 500)], refs, keys)         # a record whose ends carry two keys
    with pytest.raises(ValueError):
        RawMap.tree_by_block([(14, 16, 500)], refs, keys)         # ... names a reference that is not listed
    with pytest.raises(ValueError):
        RawMap.tree_by_block([(14, 100, 500)], refs, keys)        # ... one above every listed reference
    with pytest.raises(ValueError):
        RawMap.tree_by_block([(14, 15, 500)], [], [])
    with pytest.raises(ValueError):
        RawMap.tree_by_block(records, refs, keys[:-1])            # a key per reference
    with pytest.raises(ValueError):
        RawMap.tree_by_block([(14, 15)], refs, keys)              # rows of three


def _agree(held, listed, blocks, floor):
    """The blocked truth's two forests are one; its records in the total order, none across two keys, cut at their own
    floor they give the blocked components; they are the per-block trees merged.  Returns (records, rounds)."""
    listed, blocks = np.asarray(listed, dtype=np.uint32), np.asarray(blocks, dtype=np.uint32)
    truth = blocked(held, listed, blocks)
    records = TT.kruskal(truth, listed, floor)
    forest, rounds = TT.boruvka(truth, listed, floor)
    assert set(map(tuple, records.tolist())) == forest and len(forest) == len(records)
    keys = [(-p, a, b) for a, b, p in records.tolist()]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and all(a < b for a, b, _ in records.tolist())
    key_of = dict(zip(listed.tolist(), blocks.tolist()))
    assert all(key_of[a] == key_of[b] for a, b, _ in records.tolist())
    labels, n_clusters, _, of_ref = truth.cluster(listed, floor)
    assert len(records) == len(of_ref) - n_clusters
    assert np.array_equal(TT.cut(records, labels, listed, floor), labels)
    assert np.array_equal(RawMap.cut_tree(listed, labels, records, floor, min_permille=floor), labels)
    # one plain tree per block, merged under the total order
    plain = Truth(held)
    own = [TT.kruskal(plain, listed[blocks == k], floor) for k in np.unique(blocks)]
    assert np.array_equal(per_block(own), records)
    by_block = RawMap.tree_by_block(records, listed, blocks)
    assert sum(len(v) for v in by_block.values()) == len(records)
    for k, rows in zip(np.unique(blocks).tolist(), own):
        assert np.array_equal(by_block.get(k, np.zeros((0, 3), dtype=np.uint32)), rows)
    return records, rounds


def _words():
    kind, n, _ = ORACLE_CASES[0]
    assert (kind, n) == ("words", 5000)
    hay, off, _ = oracle_case_inputs(kind, n)
    return {i + 1: s for i, s in enumerate(W.unpack(hay, off))}, np.arange(1, n + 1, dtype=np.uint32)


def test_the_blocked_forests_agree_on_the_words_haystack_under_three_keys_and_need_three_rounds():
    held, listed = _words()
    records, rounds = _agree(held, listed, listed % 3, 200)
    print("keys % 3 at 200:", rounds, "rounds,", len(records), "merges")
    assert rounds >= 3                                        # (what the GPU file's rounds test stands on)
    assert len(records) < len(TT.kruskal(Truth(held), listed, 200))   # (the keys cut edges the plain tree keeps)


def test_the_blocked_forests_agree_on_blocks_of_every_size_and_need_three_rounds():
    held, listed = _words()
    sizes = [1, 2, 15, 16, 17, 33, 255, 256, 257, 600]
    rng = np.random.default_rng(29)                           # (as tests/test_gpu_cluster_within.py's _sized_blocks)
    picked = rng.permutation(listed)[:sum(sizes)].astype(np.uint32)
    keys = np.repeat(rng.permutation(np.arange(1000, 1000 + len(sizes), dtype=np.uint32)), sizes).astype(np.uint32)
    records, rounds = _agree(held, picked, keys, 100)
    print("sized blocks at 100:", rounds, "rounds,", len(records), "merges")
    assert rounds >= 3


def test_the_blocked_forests_agree_on_ties_in_one_block_and_split_across_two():
    same = b"tied strings"
    held = {1: same, 2: same, 3: same, 4: same}
    records, rounds = _agree(held, [1, 2, 3, 4], [9, 9, 9, 9], 1000)
    assert records.tolist() == [[1, 2, 1000], [1, 3, 1000], [1, 4, 1000]] and rounds == 1
    records, rounds = _agree(held, [1, 2, 3, 4], [9, 9, 8, 8], 1000)
    assert records.tolist() == [[1, 2, 1000], [3, 4, 1000]] and rounds == 1
