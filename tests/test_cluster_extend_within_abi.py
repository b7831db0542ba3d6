"""Cluster extend within blocks, without a GPU: blurrily_storage_cluster_extend_within is exported with its thirteen
argtypes set, its prototype agrees with the reference's storage.h in one translation unit and alone, a drifted prototype
does not compile, every argument error -- a reference listed under two block keys inside the old list, inside the new
list and across the two among them -- is EINVAL before a GPU is asked for and leaves all four outputs as they were,
valid calls fail loudly (ENODEV) where no GPU is usable while a call with nothing listed succeeds, and the Python
surface checks its arguments, hands the right pointers and shapes canned arrays rightly (cluster_changes serves the
result as it is).  The block plan (cluster_plan.h: plan_extend_within_blocks) is checked by a stand-alone program,
tests/cpp/cluster_extend_within_plan_check.cpp, built and run plainly and under the sanitizers.  The truth the GPU tests
compare with (cluster_extend_within_truth.py) is checked here against itself and by hand."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, RawMap, _native
from cluster_extend_truth import ExtendTruth
from cluster_extend_within_truth import ORACLE_TABLE, ExtendWithinTruth, contract_figures
from cluster_truth import Truth
from cluster_within_truth import WithinTruth
from helpers import compile_c, einval, oracle_case_inputs, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster_extend_within.c")
NAME = "blurrily_storage_cluster_extend_within"
NO = _native.NO_CLUSTER


def test_the_cluster_extend_within_symbol_is_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert f" T {NAME}\n" in out
    fn = getattr(lib, NAME)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
    vp, sz, u32, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    assert list(fn.argtypes[1:]) == [vp, vp, vp, sz, vp, vp, sz, ctypes.c_uint32, vp, vp, u32, u64]
    assert NAME in _native.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "blurrily_storage.h")).read()
    assert "int blurrily_storage_cluster_extend_within(trigram_map haystack,\n" in header
    assert "const uint32_t* old_refs, const uint32_t* old_blocks, const uint32_t* old_labels, size_t n_old,\n" in header
    assert "const uint32_t* new_refs, const uint32_t* new_blocks, size_t n_new,\n" in header
    assert "uint32_t* labels_old, uint32_t* labels_new, uint32_t* n_clusters, uint64_t* n_edges);" in header


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_cluster_extend_within_prototype_compiles_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_extend_within_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("was,now", [("const uint32_t*, const uint32_t*, const uint32_t*, size_t, const uint32_t*,",
                                      "const uint32_t*, const uint32_t*, size_t, const uint32_t*,"),
                                     ("                  const uint32_t*, size_t, uint32_t, uint32_t*,",
                                      "                  size_t, uint32_t, uint32_t*,"),
                                     ("uint32_t*, uint32_t*, uint32_t*, uint64_t*) =",
                                      "uint32_t*, uint32_t*, uint32_t*, uint32_t*) ="),
                                     ("uint32_t*, uint32_t*, uint32_t*, uint64_t*) =", "uint32_t*, uint32_t*, uint64_t*) ="),
                                     ("const uint32_t*, const uint32_t*, const uint32_t*, size_t,",
                                      "const uint32_t*, const uint64_t*, const uint32_t*, size_t,"),
                                     ("                  const uint32_t*, size_t, uint32_t,",
                                      "                  const uint32_t*, uint32_t, uint32_t,")],
                         ids=["no_old_blocks", "no_new_blocks", "edges_as_a_word", "one_label_array", "keys_of_64_bits",
                              "n_new_as_a_word"])
def test_a_drifted_cluster_extend_within_prototype_does_not_compile(tmp_path, was, now):
    write_recorded_storage_h(tmp_path)
    text = open(SRC).read()
    drifted = text.replace(was, now)
    assert drifted != text
    src = tmp_path / "drifted.c"
    src.write_text(drifted)
    assert compile_c(tmp_path, src).returncode != 0


def _u32(x):
    return np.array(x, dtype=np.uint32)


def test_argument_errors_are_einval_before_any_gpu_and_write_nothing():
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    old, okeys, seeds, new, nkeys = _u32([1, 2]), _u32([5, 5]), _u32([1, 1]), _u32([3]), _u32([5])
    labels_old, labels_new = np.full(8, 7, dtype=np.uint32), np.full(8, 7, dtype=np.uint32)
    n_clusters, n_edges = ctypes.c_uint32(7), ctypes.c_uint64(7)
    counts = (ctypes.byref(n_clusters), ctypes.byref(n_edges))
    call = getattr(lib, NAME)
    o, ok, s, w, wk, lo, ln = (a.ctypes.data for a in (old, okeys, seeds, new, nkeys, labels_old, labels_new))
    einval(lambda: call(None, o, ok, s, 2, w, wk, 1, 500, lo, ln, *counts))                  # no map
    einval(lambda: call(m.handle, o, ok, s, 2, w, wk, 1, 1001, lo, ln, *counts))             # min_permille > 1000
    einval(lambda: call(m.handle, None, None, None, 0, None, None, 0, 1001, None, None, *counts))   # ... with nothing listed
    einval(lambda: call(m.handle, None, ok, s, 2, w, wk, 1, 500, lo, ln, *counts))           # old_refs NULL, n_old > 0
    einval(lambda: call(m.handle, o, None, s, 2, w, wk, 1, 500, lo, ln, *counts))            # old_blocks NULL
    einval(lambda: call(m.handle, o, ok, None, 2, w, wk, 1, 500, lo, ln, *counts))           # old_labels NULL
    einval(lambda: call(m.handle, o, ok, s, 2, w, wk, 1, 500, None, ln, *counts))            # labels_old NULL
    einval(lambda: call(m.handle, o, ok, s, 2, None, wk, 1, 500, lo, ln, *counts))           # new_refs NULL, n_new > 0
    einval(lambda: call(m.handle, o, ok, s, 2, w, None, 1, 500, lo, ln, *counts))            # new_blocks NULL
    einval(lambda: call(m.handle, o, ok, s, 2, w, wk, 1, 500, lo, None, *counts))            # labels_new NULL
    einval(lambda: call(m.handle, o, ok, s, 0xFFFFFFF0, w, wk, 1, 500, lo, ln, *counts))     # the two together: too many
    einval(lambda: call(m.handle, o, ok, s, 2, w, wk, 0xFFFFFFEF, 500, lo, ln, *counts))
    einval(lambda: call(m.handle, o, ok, s, 0xFFFFFFF1, None, None, 0, 500, lo, None, *counts))
    einval(lambda: call(m.handle, None, None, None, 0, w, wk, 0xFFFFFFF1, 500, None, ln, *counts))
    einval(lambda: call(m.handle, o, ok, s, 2**64 - 1, w, wk, 2, 500, lo, ln, *counts))      # (a sum that wraps round)
    einval(lambda: call(m.handle, o, ok, s, 2, w, wk, 1, 1001, lo, ln, None, None))          # the counts are optional
    # a reference under two keys: inside the old list (side by side, and apart in a shuffled list) ...
    two, twok, twos = _u32([4, 4]), _u32([0, 1]), _u32([4, 4])
    einval(lambda: call(m.handle, two.ctypes.data, twok.ctypes.data, twos.ctypes.data, 2, w, wk, 1, 500, lo, ln, *counts))
    einval(lambda: call(m.handle, two.ctypes.data, twok.ctypes.data, twos.ctypes.data, 2, None, None, 0, 500, lo, None,
                        *counts))
    sh, shk = _u32([14, 10, 17, 11, 15, 14, 99, 11]), _u32([2, 1, 3, 1, 2, 7, 5, 1])
    einval(lambda: call(m.handle, sh.ctypes.data, shk.ctypes.data, sh.ctypes.data, 8, w, wk, 1, 500, lo, ln, *counts))
    # ... inside the new list
    einval(lambda: call(m.handle, o, ok, s, 2, two.ctypes.data, twok.ctypes.data, 2, 500, lo, ln, *counts))
    einval(lambda: call(m.handle, None, None, None, 0, sh.ctypes.data, shk.ctypes.data, 8, 0, None, ln, None, None))
    # ... and across the two lists: 2 is old under 5 and new under 6
    cross, crossk = _u32([3, 2]), _u32([5, 6])
    einval(lambda: call(m.handle, o, ok, s, 2, cross.ctypes.data, crossk.ctypes.data, 2, 500, lo, ln, *counts))
    assert n_clusters.value == 7 and n_edges.value == 7                              # nothing written
    assert (labels_old == 7).all() and (labels_new == 7).all()
    for lists in (([4, 4], [0, 1], [4, 4], [3], [5]), ([1, 2], [5, 5], [1, 1], [4, 4], [0, 1]),
                  ([1, 2], [5, 5], [1, 1], [3, 2], [5, 6])):
        with pytest.raises(OSError) as e:
            m.cluster_extend_within(*lists, 500)
        assert e.value.errno == errno.EINVAL
    m.close()


def test_nothing_listed_is_success_with_the_counts_given_and_nothing_else_written():
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    call = getattr(lib, NAME)
    labels = np.full(2, 7, dtype=np.uint32)
    n_clusters, n_edges = ctypes.c_uint32(7), ctypes.c_uint64(7)
    assert call(m.handle, None, None, None, 0, None, None, 0, 500, None, None, None, None) == 0
    assert call(m.handle, None, None, None, 0, None, None, 0, 1000, labels.ctypes.data, labels.ctypes.data,
                ctypes.byref(n_clusters), None) == 0
    assert (n_clusters.value, n_edges.value) == (0, 7) and (labels == 7).all()
    assert call(m.handle, None, None, None, 0, None, None, 0, 0, None, None, None, ctypes.byref(n_edges)) == 0
    assert n_edges.value == 0
    out = m.cluster_extend_within([], [], [], [], [], 0)
    assert [a.shape for a in out[:2]] == [(0,), (0,)] and out[2:] == (0, 0)
    assert [a.dtype for a in out[:2]] == [np.uint32, np.uint32]
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster_extend_within.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    old, okeys, seeds, new, nkeys = _u32([1, 2]), _u32([5, 6]), _u32([1, 1]), _u32([3]), _u32([5])
    labels_old, labels_new = np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
    n_clusters, n_edges = ctypes.c_uint32(0), ctypes.c_uint64(0)
    call = getattr(lib, NAME)
    o, ok, s, w, wk, lo, ln = (a.ctypes.data for a in (old, okeys, seeds, new, nkeys, labels_old, labels_new))
    # a shuffled list with repeats under consistent keys, also across the lists, is a valid call: ENODEV, not EINVAL
    sh, shk = _u32([14, 10, 17, 11, 15, 14, 99, 11]), _u32([2, 1, 3, 1, 2, 2, 5, 1])
    for one in (lambda: call(m.handle, o, ok, s, 2, w, wk, 1, 500, lo, ln, ctypes.byref(n_clusters), ctypes.byref(n_edges)),
                lambda: call(m.handle, o, ok, s, 2, w, wk, 1, 0, lo, ln, None, None),
                lambda: call(m.handle, o, ok, s, 2, None, None, 0, 1000, lo, None, None, None),
                lambda: call(m.handle, None, None, None, 0, w, wk, 1, 500, None, ln, None, None),
                lambda: call(m.handle, sh.ctypes.data, shk.ctypes.data, sh.ctypes.data, 8, sh.ctypes.data, shk.ctypes.data,
                             8, 500, lo, ln, None, None)):
        ctypes.set_errno(0)
        assert one() == -1
        assert ctypes.get_errno() == errno.ENODEV
    # a seed across two keys is no error either: it does not exist
    with pytest.raises(OSError) as e:
        m.cluster_extend_within([1, 2], [5, 6], [1, 1], [3], [5], 700)
    assert e.value.errno == errno.ENODEV
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    ext = m.cluster_extend_within
    with pytest.raises(ValueError):
        ext([1], [0], [1], [2], [0], 1001)
    with pytest.raises(OverflowError):
        ext([1], [0], [1], [2], [0], -1)
    with pytest.raises(OverflowError):
        ext([-1], [0], [1], [2], [0], 500)
    with pytest.raises(OverflowError):
        ext([1], [1 << 32], [1], [2], [0], 500)
    with pytest.raises(OverflowError):
        ext([1], [0], [1 << 32], [2], [0], 500)
    with pytest.raises(OverflowError):
        ext([1], [0], [1], [-2], [0], 500)
    with pytest.raises(OverflowError):
        ext([1], [0], [1], [2], [-3], 500)
    with pytest.raises(ValueError):
        ext([[1, 2]], [0], [1], [2], [0], 500)
    with pytest.raises(ValueError):
        ext([1, 2], [0], [1, 1], [3], [0], 500)                   # a key per old reference
    with pytest.raises(ValueError):
        ext([1, 2], [0, 0], [1], [3], [0], 500)                   # a label per old reference
    with pytest.raises(ValueError):
        ext([1, 2], [0, 0], [1, 1], [3], [0, 0], 500)             # a key per new reference
    with pytest.raises(ValueError):
        ext([1, 2], [0, 0], [1, 1], [3, 4], [], 500)
    m.close()
    with pytest.raises(RawMap.ClosedError):
        ext([1], [0], [1], [2], [0], 500)


class _StubLib:
    """Stands where the library stands in a RawMap: records what blurrily_storage_cluster_extend_within is handed and
    fills the outputs from canned arrays (no GPU is asked for)."""

    def __init__(self, canned):
        self.canned, self.calls = canned, []

    def blurrily_storage_cluster_extend_within(self, handle, old, old_keys, seeds, n_old, new, new_keys, n_new, mp,
                                               labels_old, labels_new, n_clusters, n_edges):
        u32 = ctypes.POINTER(ctypes.c_uint32)
        seen = lambda p, n: np.ctypeslib.as_array(ctypes.cast(p, u32), shape=(n,)).tolist() if n else []
        self.calls.append(dict(old=old, old_keys=old_keys, seeds=seeds, n_old=n_old, new=new, new_keys=new_keys,
                               n_new=n_new, mp=mp, labels_old=labels_old, labels_new=labels_new,
                               listed_old=seen(old, n_old), listed_old_keys=seen(old_keys, n_old),
                               listed_seeds=seen(seeds, n_old), listed_new=seen(new, n_new),
                               listed_new_keys=seen(new_keys, n_new)))
        c = self.canned
        for ptr, refs in ((labels_old, self.calls[-1]["listed_old"]), (labels_new, self.calls[-1]["listed_new"])):
            if ptr:
                out = np.array([c["label_of"].get(r, NO) for r in refs], dtype=np.uint32)
                ctypes.memmove(ptr, out.ctypes.data, 4 * len(refs))
        n_clusters._obj.value, n_edges._obj.value = c["n_clusters"], c["n_edges"]
        return 0


# key 1: old groups {10, 11} and {14, 15}, which the new 12 joins; key 2: 17 alone, the new 20 alone; 99 is absent
CANNED = dict(label_of={10: 10, 11: 10, 14: 10, 15: 10, 17: 17, 12: 10, 20: 20}, n_clusters=3, n_edges=2)
OLD, OLD_KEYS, SEEDS = [10, 11, 14, 15, 17, 99], [1, 1, 1, 1, 2, 2], [10, 10, 14, 14, 17, NO]
NEW, NEW_KEYS = [12, 20], [1, 2]


def _stubbed():
    m = RawMap()
    m._real, m._lib = m._lib, _StubLib(CANNED)
    return m


def _unstub(m):
    m._lib = m._real
    m.close()


def test_cluster_extend_within_hands_every_pointer_and_shapes_the_outputs():
    m = _stubbed()
    labels_old, labels_new, n_clusters, n_edges = m.cluster_extend_within(OLD, OLD_KEYS, SEEDS, NEW, NEW_KEYS, 700)
    call = m._lib.calls[-1]
    assert all(call[k] for k in ("old", "old_keys", "seeds", "new", "new_keys", "labels_old", "labels_new"))
    assert (call["n_old"], call["n_new"], call["mp"]) == (6, 2, 700)
    assert (call["listed_old"], call["listed_old_keys"], call["listed_seeds"]) == (OLD, OLD_KEYS, SEEDS)
    assert (call["listed_new"], call["listed_new_keys"]) == (NEW, NEW_KEYS)
    assert labels_old.dtype == labels_new.dtype == np.uint32
    assert labels_old.tolist() == [10, 10, 10, 10, 17, NO] and labels_new.tolist() == [10, 20]
    assert (n_clusters, n_edges) == (3, 2) and all(isinstance(x, int) for x in (n_clusters, n_edges))
    # an empty side hands no pointer for it
    out = m.cluster_extend_within([], [], [], NEW, NEW_KEYS, 0)
    last = m._lib.calls[-1]
    assert last["n_old"] == 0 and not any(last[k] for k in ("old", "old_keys", "seeds", "labels_old")) and last["new"]
    assert out[0].shape == (0,) and out[1].tolist() == [10, 20]
    out = m.cluster_extend_within(_u32(OLD), _u32(OLD_KEYS), _u32(SEEDS), [], [], 1000)
    last = m._lib.calls[-1]
    assert last["n_new"] == 0 and not any(last[k] for k in ("new", "new_keys", "labels_new")) and last["old"]
    assert out[1].shape == (0,) and out[0].tolist() == [10, 10, 10, 10, 17, NO]
    # cluster_changes serves the result as it is
    moved, now = m.cluster_changes(OLD, SEEDS, labels_old)
    assert (moved.tolist(), now.tolist()) == ([14, 15], [10, 10])
    _unstub(m)


SANITIZED = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("sanitize", [[], SANITIZED], ids=["plain", "sanitized"])
def test_the_block_plan_matches_what_was_written_down(tmp_path, sanitize):
    # (built the way tests/test_find_choice.py builds the other tests/cpp checks: a stand-alone program)
    exe = str(tmp_path / "cluster_extend_within_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *sanitize,
           "-I", os.path.join(ROOT, "blurrily_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "cluster_extend_within_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "cluster_extend_within_plan: 0 expectations failed", r.stdout + r.stderr


# ---- the truth, by hand and against itself

def test_the_truth_on_canned_strings_by_hand():
    # three strings without a letter in common: references share trigrams exactly when they hold the same string
    S = [b"abcde", b"fghij", b"klmno"]
    held = {1: S[0], 2: S[0], 3: S[1], 4: S[1], 5: S[0], 6: S[2], 7: S[1], 8: S[0]}
    truth = Truth(held)
    # old 1, 2 (key 1), 3, 4 (key 2), 100 (not held); new 5 (key 1: joins 1 and 2), 7 (key 3: its twins 3 and 4 are
    # under key 2), 8 (key 3: its twins are under key 1, 7 is no twin), 6 (key 2: no twin at all), 101 (not held)
    t = ExtendWithinTruth(truth, [1, 2, 3, 4, 100], [1, 1, 2, 2, 2], [1, 1, 3, 3, 100], [5, 7, 8, 6, 101],
                          [1, 3, 3, 2, 1], 1000)
    assert t.labels_old.tolist() == [1, 1, 3, 3, NO] and t.labels_new.tolist() == [1, 7, 8, 6, NO]
    assert (t.n_clusters, t.n_edges, t.new_new_edges, t.n_seeds) == (5, 2, 0, 2)
    assert t.cross_key_edges == 2 + 3 and not t.spans_two_keys()       # 7-3, 7-4; 8-1, 8-2, 8-5
    # a seed across two keys does not exist; a chain of must-links inside a key does; a label that is new does not
    t = ExtendWithinTruth(truth, [1, 3, 6, 4], [1, 2, 2, 2], [3, 6, 4, 5], [5], [1], 1001)
    assert (t.n_seeds, t.cross_key_seeds, t.n_edges) == (2, 1, 0)
    assert t.labels_old.tolist() == [1, 3, 3, 3] and t.labels_new.tolist() == [5] and t.n_clusters == 3
    # a reference both lists name is new: its seed goes, its edges are looked at
    t = ExtendWithinTruth(truth, [1, 2], [1, 1], [1, 1], [2, 5], [1, 1], 1000)
    assert (t.n_seeds, t.n_edges, t.new_new_edges) == (0, 3, 1) and t.labels_old.tolist() == [1, 1]


_CASES = {}


def oracle_truth(kind, n):
    if (kind, n) not in _CASES:
        hay, off, _ = oracle_case_inputs(kind, n)
        held = {i + 1: s for i, s in enumerate(W.unpack(hay, off))}
        _CASES[kind, n] = WithinTruth(held), np.arange(1, n + 1, dtype=np.uint32)
    return _CASES[kind, n]


TABLE = ORACLE_TABLE                                          # (the figures of the issue)


@pytest.mark.parametrize("kind,n,modulus,p,figures", TABLE, ids=[f"{c[0]}-{c[2]}-{c[3]}" for c in TABLE])
def test_the_truth_on_the_oracle_haystacks_is_telling_and_agrees_with_itself(kind, n, modulus, p, figures):
    truth, listed = oracle_truth(kind, n)
    new, old = listed[listed % 7 == 0], listed[listed % 7 != 0]
    t, seeds, old_edges, got = contract_figures(truth, old, old % modulus, new, new % modulus, p, least=p)
    print(f"{kind} % {modulus} at {p}: {got}")
    assert got == figures and min(got) >= 1 and not t.spans_two_keys()
    # the contract: cluster_within over both lists, the keys concatenated
    both = np.concatenate([old, new])
    labels, n_clusters, n_edges, _ = truth.cluster_within(both, both % modulus, p, least=p)
    assert np.array_equal(np.concatenate([t.labels_old, t.labels_new]), labels)
    assert (t.n_clusters, t.n_edges) == (n_clusters, n_edges - old_edges)
    # all keys equal: ExtendTruth
    if modulus == 3:
        plain_seeds = truth.cluster(old, p, least=p)[0]
        same = ExtendWithinTruth(truth, old, np.zeros_like(old), plain_seeds, new, np.zeros_like(new), p, least=p)
        plain = ExtendTruth(truth, old, plain_seeds, new, p, least=p)
        assert np.array_equal(same.labels_old, plain.labels_old) and np.array_equal(same.labels_new, plain.labels_new)
        assert (same.n_clusters, same.n_edges, same.cross_key_edges) == (plain.n_clusters, plain.n_edges, 0)
