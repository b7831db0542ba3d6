"""Cluster edges extend and between without a GPU: blurrily_storage_cluster_edges_extend and
blurrily_storage_cluster_edges_between are exported with their nine argtypes set, their prototypes agree with the
reference's storage.h in one translation unit and alone, drifted prototypes do not compile, every argument error --
n_edges NULL and the two n together above 2^27 among them -- is EINVAL before a GPU is asked for and leaves the buffer and
the count as they were, valid calls fail loudly (ENODEV) where no GPU is usable, the Python surface checks its
arguments, hands the right pointers, grows once on ERANGE and hands no buffer to count; ``merge_edges`` merges, and
refuses lists out of order and records present twice; the side that sweeps is cluster_plan.h's pure function
(tests/cpp/cluster_edges_extend_plan_check.cpp, built and run plainly and under the sanitizers); and the truth of
tests/cluster_edges_extend_truth.py is checked against itself on the oracle haystacks split as the GPU tests split them,
with the figures those tests stand on."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, RawMap, _native
import cluster_edges_truth as CE
from cluster_edges_extend_truth import Split
from cluster_truth import Truth
from helpers import ORACLE_CASES, compile_c, einval, oracle_case_inputs, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "header_compat_cluster_edges_extend.c")
EXTEND, BETWEEN = "blurrily_storage_cluster_edges_extend", "blurrily_storage_cluster_edges_between"
# (haystack: the floors, and per floor the old-old, old-new and new-new edges of the split mod 7, from a CPU run of the
# truth; tests/test_gpu_cluster_extend.py records the same new-new figures)
ORACLE_FLOORS = {"words": ((200, 300), ((1888, 667, 63), (123, 47, 5))),
                 "geonames": ((500, 700), ((2520173, 828073, 67597), (1084014, 338450, 26229))),
                 "skewed": ((500,), ((16287, 5302, 403),))}


def test_the_two_symbols_are_exported_with_argtypes():
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name in (EXTEND, BETWEEN):
        assert f" T {name}\n" in out
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
        assert name in _native.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "blurrily_storage.h")).read()
    assert ("int blurrily_storage_cluster_edges_extend(trigram_map haystack, const uint32_t* old_refs, size_t n_old,\n"
            "                                          const uint32_t* new_refs, size_t n_new, uint32_t min_permille,\n"
            "                                          blurrily_cluster_merge_t* edges, uint64_t capacity, uint64_t* n_edges);"
            ) in header
    assert ("int blurrily_storage_cluster_edges_between(trigram_map haystack, const uint32_t* left_refs, size_t n_left,\n"
            "                                           const uint32_t* right_refs, size_t n_right, uint32_t min_permille,\n"
            "                                           blurrily_cluster_merge_t* edges, uint64_t capacity, uint64_t* n_edges);"
            ) in header
    assert "an extend form" not in header


@pytest.mark.parametrize("order", ["reference_first", "ours_alone"])
def test_the_prototypes_compile_beside_the_reference_header(tmp_path, order):
    src = SRC
    if order == "ours_alone":
        text = open(SRC).read().replace('#include "storage.h"', "/* (reference header left out) */")
        src = tmp_path / "cluster_edges_extend_alone.c"
        src.write_text(text)
    else:
        write_recorded_storage_h(tmp_path)
    r = compile_c(tmp_path, src)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("was,now", [
    ("(*f_extend)(trigram_map, const uint32_t*, size_t, const uint32_t*, size_t, uint32_t,",
     "(*f_extend)(trigram_map, const uint32_t*, size_t, uint32_t,"),
    ("(*f_between)(trigram_map, const uint32_t*, size_t, const uint32_t*, size_t, uint32_t,",
     "(*f_between)(trigram_map, const uint32_t*, size_t, const uint32_t*, uint32_t, uint32_t,"),
    ("blurrily_cluster_merge_t*, uint64_t, uint64_t*) = blurrily_storage_cluster_edges_extend",
     "uint32_t*, uint64_t, uint64_t*) = blurrily_storage_cluster_edges_extend"),
    ("blurrily_cluster_merge_t*, uint64_t, uint64_t*) = blurrily_storage_cluster_edges_between",
     "blurrily_cluster_merge_t*, uint32_t, uint64_t*) = blurrily_storage_cluster_edges_between"),
    ("blurrily_cluster_merge_t*, uint64_t, uint64_t*) = blurrily_storage_cluster_edges_between",
     "blurrily_cluster_merge_t*, uint64_t, uint32_t*) = blurrily_storage_cluster_edges_between")],
    ids=["one_list", "n_right_as_a_word", "edges_as_words", "capacity_as_a_word", "count_as_a_word"])
def test_a_drifted_prototype_does_not_compile(tmp_path, was, now):
    write_recorded_storage_h(tmp_path)
    text = " ".join(open(SRC).read().split())                 # (one line: the prototypes' line breaks do not matter)
    assert text.count(was) == 1
    src = tmp_path / "drifted.c"
    src.write_text(text.replace(was, now).replace('#include "storage.h" #include "blurrily_storage.h"',
                                                  '#include "storage.h"\n#include "blurrily_storage.h"\n'))
    assert compile_c(tmp_path, src).returncode != 0
    whole = tmp_path / "not_drifted.c"
    whole.write_text(text.replace('#include "storage.h" #include "blurrily_storage.h"',
                                  '#include "storage.h"\n#include "blurrily_storage.h"\n'))
    r = compile_c(tmp_path, whole)                            # (the drift alone is what does not compile)
    assert r.returncode == 0, r.stderr


def test_argument_errors_are_einval_before_any_gpu_and_write_nothing():
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    one, two = np.array([1, 2, 3], dtype=np.uint32), np.array([4, 5], dtype=np.uint32)
    edges = np.full((8, 3), 7, dtype=np.uint32)
    n_edges = ctypes.c_uint64(7)
    a, b, e, count = one.ctypes.data, two.ctypes.data, edges.ctypes.data, ctypes.byref(n_edges)
    top = 1 << 27
    for fn in (getattr(lib, EXTEND), getattr(lib, BETWEEN)):
        einval(lambda: fn(None, a, 3, b, 2, 500, e, 8, count))                      # no map
        einval(lambda: fn(m.handle, a, 3, b, 2, 1001, e, 8, count))                 # min_permille > 1000
        einval(lambda: fn(m.handle, None, 0, None, 0, 1001, None, 0, count))        # ... with nothing listed too
        einval(lambda: fn(m.handle, None, 3, b, 2, 500, e, 8, count))               # the first list NULL, its n > 0
        einval(lambda: fn(m.handle, a, 3, None, 2, 500, e, 8, count))               # the second list NULL, its n > 0
        einval(lambda: fn(m.handle, a, 3, b, 2, 500, e, 8, None))                   # n_edges is required
        einval(lambda: fn(m.handle, a, 3, b, 2, 500, None, 0, None))                # ... to count only, too
        einval(lambda: fn(m.handle, None, 0, None, 0, 500, None, 0, None))          # ... and with nothing listed
        einval(lambda: fn(m.handle, a, top, b, 1, 500, e, 8, count))                # the two n together above 2^27
        einval(lambda: fn(m.handle, a, 1, b, top, 500, e, 8, count))
        einval(lambda: fn(m.handle, a, top // 2 + 1, b, top // 2, 500, None, 0, count))
        einval(lambda: fn(m.handle, a, top + 1, None, 0, 500, e, 8, count))
        einval(lambda: fn(m.handle, None, 0, b, top + 1, 500, e, 8, count))
        einval(lambda: fn(m.handle, a, 2**64 - 1, b, 2, 500, None, 0, count))       # (no wrap-around in the sum)
        einval(lambda: fn(m.handle, a, 2**64 - 1, b, 2**64 - 1, 500, None, 0, count))
        einval(lambda: fn(m.handle, a, 3, b, 2**64 - 2, 500, None, 0, count))
    assert n_edges.value == 7 and (edges == 7).all()                                # nothing written
    m.close()


def test_valid_calls_without_a_gpu_are_enodev(has_gpu):
    if has_gpu:
        pytest.skip("a GPU is usable here: tests/test_gpu_cluster_edges_extend.py covers the calls")
    lib = _native.lib()
    m = RawMap()
    m.put(b"san jose", 1, 0)
    one, two = np.array([1, 2, 3], dtype=np.uint32), np.array([3, 5], dtype=np.uint32)
    edges = np.zeros((8, 3), dtype=np.uint32)
    n_edges = ctypes.c_uint64(0)
    a, b, e, count = one.ctypes.data, two.ctypes.data, edges.ctypes.data, ctypes.byref(n_edges)
    for fn in (getattr(lib, EXTEND), getattr(lib, BETWEEN)):
        for call in (lambda: fn(m.handle, a, 3, b, 2, 500, e, 8, count),
                     lambda: fn(m.handle, a, 3, b, 2, 0, None, 0, count),           # count only
                     lambda: fn(m.handle, a, 3, b, 2, 1000, e, 0, count),
                     lambda: fn(m.handle, None, 0, b, 2, 500, e, 8, count),         # one list empty
                     lambda: fn(m.handle, a, 3, None, 0, 500, None, 0, count),
                     lambda: fn(m.handle, None, 0, None, 0, 500, None, 0, count),   # both n 0
                     lambda: fn(m.handle, None, 0, None, 0, 500, e, 8, count)):
            ctypes.set_errno(0)
            assert call() == -1
            assert ctypes.get_errno() == errno.ENODEV
    for call in (lambda: m.cluster_edges_extend([1, 2], [3], 700), lambda: m.cluster_edges_extend([], [], 0),
                 lambda: m.cluster_edge_count_extend([1, 2], [3], 700), lambda: m.cluster_edges_between([1, 2], [3], 700),
                 lambda: m.cluster_edges_between([], [], 0), lambda: m.cluster_edge_count_between([], [3], 1000)):
        with pytest.raises(OSError) as err:
            call()
        assert err.value.errno == errno.ENODEV
    m.close()


def test_the_python_surface_checks_its_arguments():
    m = Map()
    m.put("san jose", 1)
    for call in (m.cluster_edges_extend, m.cluster_edge_count_extend, m.cluster_edges_between, m.cluster_edge_count_between):
        with pytest.raises(ValueError):
            call([1], [2], 1001)
        with pytest.raises(OverflowError):
            call([1], [2], -1)
        with pytest.raises(OverflowError):
            call([-1], [2], 500)
        with pytest.raises(OverflowError):
            call([1], [1 << 32], 500)
        with pytest.raises(ValueError):
            call([[1, 2]], [3], 500)
        with pytest.raises(ValueError):
            call([1], [[2, 3]], 500)
    for call in (m.cluster_edges_extend, m.cluster_edges_between):
        with pytest.raises(OverflowError):
            call([1], [2], 500, capacity=-1)
        with pytest.raises(OverflowError):
            call([1], [2], 500, capacity=1 << 64)
    m.close()
    for call in (m.cluster_edges_extend, m.cluster_edge_count_extend, m.cluster_edges_between, m.cluster_edge_count_between):
        with pytest.raises(RawMap.ClosedError):
            call([1], [2], 500)


class _StubLib:
    """Stands where the library stands in a RawMap: records what the two entries are handed and answers from canned
    records as the library would (the count always, ERANGE where the room is too small, the records where it is not)."""

    def __init__(self, records):
        self.records, self.calls = np.array(records, dtype=np.uint32).reshape(-1, 3), []

    def _answer(self, symbol, first, n_first, second, n_second, mp, edges, capacity, n_edges):
        u32 = ctypes.POINTER(ctypes.c_uint32)
        seen = lambda p, n: np.ctypeslib.as_array(ctypes.cast(p, u32), shape=(n,)).tolist() if n and p else []
        self.calls.append(dict(symbol=symbol, first=first, second=second, n_first=n_first, n_second=n_second, mp=mp,
                               edges=edges, capacity=capacity, listed=(seen(first, n_first), seen(second, n_second))))
        n_edges._obj.value = len(self.records)
        if not edges:
            return 0
        if capacity < len(self.records):
            ctypes.set_errno(errno.ERANGE)
            return -1
        if len(self.records):
            ctypes.memmove(edges, self.records.ctypes.data, self.records.nbytes)
        return 0

    def blurrily_storage_cluster_edges_extend(self, handle, *args):
        return self._answer("extend", *args)

    def blurrily_storage_cluster_edges_between(self, handle, *args):
        return self._answer("between", *args)


RECORDS = [(14, 15, 900), (10, 11, 800), (11, 17, 800), (10, 17, 705)]
FIRST, SECOND = [14, 10, 17, 14], [11, 15, 99, 11, 15]


def _stubbed(records=RECORDS):
    m = RawMap()
    m._real, m._lib = m._lib, _StubLib(records)
    return m


def _unstub(m):
    m._lib = m._real
    m.close()


def test_the_methods_hand_every_pointer_shape_the_records_and_pick_the_symbol():
    m = _stubbed()
    for method, symbol in ((m.cluster_edges_extend, "extend"), (m.cluster_edges_between, "between")):
        m._lib.calls.clear()
        edges = method(FIRST, SECOND, 700)
        call = m._lib.calls[-1]
        assert len(m._lib.calls) == 1 and call["symbol"] == symbol and call["first"] and call["second"] and call["edges"]
        assert (call["n_first"], call["n_second"], call["mp"], call["capacity"]) == (4, 5, 700, 1024)
        assert call["listed"] == (FIRST, SECOND)
        assert edges.dtype == np.uint32 and edges.shape == (4, 3) and edges.tolist() == [list(e) for e in RECORDS]
        # the first room: the caller's, or max(1024, 8 (n + n))
        method(np.arange(1, 201, dtype=np.uint32), list(range(201, 301)), 0)
        assert m._lib.calls[-1]["capacity"] == 2400 and m._lib.calls[-1]["mp"] == 0
        method(FIRST, SECOND, 500, capacity=4)
        assert m._lib.calls[-1]["capacity"] == 4
        # an empty list hands no pointer, and still a buffer: the call is no count
        method([], SECOND, 1000)
        last = m._lib.calls[-1]
        assert last["n_first"] == 0 and not last["first"] and last["second"] and last["edges"]
        method(FIRST, [], 1000)
        last = m._lib.calls[-1]
        assert last["n_second"] == 0 and not last["second"] and last["first"] and last["listed"] == (FIRST, [])
    m._lib.records = np.zeros((0, 3), dtype=np.uint32)
    out = m.cluster_edges_between([], [], 1000)
    assert out.shape == (0, 3) and out.dtype == np.uint32 and not m._lib.calls[-1]["first"]
    _unstub(m)


def test_the_methods_grow_once_to_the_reported_count():
    m = _stubbed()
    for method, symbol in ((m.cluster_edges_extend, "extend"), (m.cluster_edges_between, "between")):
        m._lib.calls.clear()
        edges = method(FIRST, SECOND, 700, capacity=3)
        assert [(c["symbol"], c["capacity"]) for c in m._lib.calls] == [(symbol, 3), (symbol, 4)]
        assert edges.tolist() == [list(e) for e in RECORDS]
        m._lib.calls.clear()
        assert method(FIRST, SECOND, 700, capacity=0).shape == (4, 3)
        assert [c["capacity"] for c in m._lib.calls] == [0, 4]
    _unstub(m)


def test_the_count_methods_hand_no_buffer():
    m = _stubbed()
    for method, symbol in ((m.cluster_edge_count_extend, "extend"), (m.cluster_edge_count_between, "between")):
        m._lib.calls.clear()
        count = method(FIRST, SECOND, 700)
        call = m._lib.calls[-1]
        assert count == 4 and isinstance(count, int) and len(m._lib.calls) == 1 and call["symbol"] == symbol
        assert not call["edges"] and call["capacity"] == 0 and call["listed"] == (FIRST, SECOND)
    _unstub(m)


def test_merge_edges_merges_under_the_total_order_and_refuses_disorder_and_duplicates():
    # two interleaved lists
    one = [(14, 15, 900), (11, 17, 800), (10, 17, 705)]
    two = [(3, 4, 1000), (10, 11, 800), (1, 2, 705), (10, 18, 705)]
    got = RawMap.merge_edges(one, two)
    assert got.dtype == np.uint32 and got.shape == (7, 3)
    assert got.tolist() == [[3, 4, 1000], [14, 15, 900], [10, 11, 800], [11, 17, 800], [1, 2, 705], [10, 17, 705],
                            [10, 18, 705]]
    assert RawMap.merge_edges(two, one).tobytes() == got.tobytes()
    assert RawMap.merge_edges(np.array(one, dtype=np.uint32), np.array(two, dtype=np.uint32)).tobytes() == got.tobytes()
    # equal heights broken by a, then b -- across three lists
    got = RawMap.merge_edges([(2, 9, 500)], [(2, 3, 500), (7, 8, 500)], [(1, 9, 500), (2, 4, 500)])
    assert got.tolist() == [[1, 9, 500], [2, 3, 500], [2, 4, 500], [2, 9, 500], [7, 8, 500]]
    # an empty list, only empty lists, no list, one list
    assert RawMap.merge_edges(one, []).tolist() == [list(r) for r in one]
    assert RawMap.merge_edges([], np.zeros((0, 3), dtype=np.uint32), one).tolist() == [list(r) for r in one]
    for nothing in (RawMap.merge_edges(), RawMap.merge_edges([]), RawMap.merge_edges([], [])):
        assert nothing.shape == (0, 3) and nothing.dtype == np.uint32
    assert RawMap.merge_edges(two).tolist() == [list(r) for r in two]
    # agrees with the truth's merge
    assert RawMap.merge_edges(one, two).tobytes() == CE.merged([one, two]).tobytes()
    # an unordered list: heights ascending, a descending at one height, b descending at one height and a
    for bad in ([(10, 17, 705), (14, 15, 900)], [(11, 17, 800), (10, 11, 800)], [(10, 18, 705), (10, 17, 705)]):
        with pytest.raises(ValueError):
            RawMap.merge_edges(bad)
        with pytest.raises(ValueError):
            RawMap.merge_edges(two, bad)
    # a record present twice: in one list, and in two
    with pytest.raises(ValueError):
        RawMap.merge_edges([(14, 15, 900), (14, 15, 900)])
    with pytest.raises(ValueError):
        RawMap.merge_edges(one, two, [(11, 17, 800)])
    with pytest.raises(ValueError):
        RawMap.merge_edges(one, one)
    # rows of three, values of 32 bits
    with pytest.raises(ValueError):
        RawMap.merge_edges([(10, 11)])
    with pytest.raises(OverflowError):
        RawMap.merge_edges([(10, 1 << 32, 500)])


SANITIZED = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("sanitize", [[], SANITIZED], ids=["plain", "sanitized"])
def test_the_side_that_sweeps_matches_what_was_written_down(tmp_path, sanitize):
    # (built the way tests/test_find_choice.py builds the other tests/cpp checks: a stand-alone program)
    exe = str(tmp_path / "cluster_edges_extend_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *sanitize,
           "-I", os.path.join(ROOT, "blurrily_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "cluster_edges_extend_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "cluster_edges_extend_plan: 0 expectations failed", r.stdout + r.stderr


def test_the_truth_on_canned_strings_by_hand():
    # five parts without a letter in common: strings share trigrams exactly when they share a part
    S = [b"abcde", b"fghij", b"klmno"]
    held = {1: S[0], 2: S[0], 3: S[1], 4: S[1], 5: S[0], 6: S[2], 7: S[1]}
    truth = Truth(held)
    s = Split(truth, [1, 2, 3, 4, 100], [5, 7, 6, 101], 1000).check_itself()
    assert s.whole.tolist() == [[1, 2, 1000], [1, 5, 1000], [2, 5, 1000], [3, 4, 1000], [3, 7, 1000], [4, 7, 1000]]
    assert s.extend.tolist() == [[1, 5, 1000], [2, 5, 1000], [3, 7, 1000], [4, 7, 1000]]
    assert s.between.tolist() == s.extend.tolist() and s.figures() == (2, 4, 0)
    # a reference in both lists is new (on the right) only; both twins new
    s = Split(truth, [1, 2, 3, 4], [2, 5], 1000).check_itself()
    assert s.first_only.tolist() == [1, 3, 4] and s.figures() == (1, 2, 1)       # 3-4; 1-2 and 1-5; 2-5
    assert s.extend.tolist() == [[1, 2, 1000], [1, 5, 1000], [2, 5, 1000]]
    assert s.between.tolist() == [[1, 2, 1000], [1, 5, 1000]] and s.new_new.tolist() == [[2, 5, 1000]]
    # nothing old: the second list's own records; nothing new: none
    s = Split(truth, [], [1, 2, 5], 1000).check_itself()
    assert s.extend.tobytes() == CE.records(truth, [1, 2, 5], 1000).tobytes() and len(s.between) == 0
    s = Split(truth, [1, 2, 5], [], 1000).check_itself()
    assert len(s.extend) == 0 and len(s.between) == 0 and len(s.whole) == 3


@pytest.mark.parametrize("kind,n,_limit", ORACLE_CASES)
def test_the_truth_is_sound_on_the_oracle_haystacks_split_mod_seven_and_every_split_is_telling(kind, n, _limit):
    hay, off, _ = oracle_case_inputs(kind, n)
    truth = Truth({i + 1: s for i, s in enumerate(W.unpack(hay, off))})
    listed = np.arange(1, n + 1, dtype=np.uint32)
    old, new = listed[listed % 7 != 0], listed[listed % 7 == 0]
    floors, figures = ORACLE_FLOORS[kind]
    for floor, figure in zip(floors, figures):
        s = Split(truth, old, new, floor, floors[0]).check_itself()
        print(f"{kind} at {floor}: old-old, old-new, new-new edges: {s.figures()}")
        assert min(s.figures()) >= 1 and s.figures() == figure, (floor, s.figures())
        # the other way round the between records are the same bytes (the lists are disjoint)
        assert Split(truth, new, old, floor, floors[0]).between.tobytes() == s.between.tobytes()
        assert RawMap.merge_edges(s.held_before, s.extend).tobytes() == s.whole.tobytes()
        assert RawMap.merge_edges(s.between, s.among_second).tobytes() == s.extend.tobytes()
