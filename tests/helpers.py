"""Test-side access to the checkers under oracle/ (never imported by the product)."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
REF_SO = os.path.join(ORACLE_DIR, "_ref", "libblurrily_ref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")


class Match(C.Structure):
    _pack_ = 1
    _fields_ = [("reference", C.c_uint32), ("matches", C.c_uint32), ("weight", C.c_uint32)]


def _rows(buf, n):
    return [[buf[k].reference, buf[k].matches, buf[k].weight] for k in range(n)]


class Oracle:
    """oracle/blurrily_oracle.c -- CPU restatement of the reference algorithm."""

    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            L = C.CDLL(os.path.join(ORACLE_DIR, "liboracle.so"))
            L.oracle_new.restype = C.c_void_p
            L.oracle_free.argtypes = [C.c_void_p]
            L.oracle_put.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32]
            L.oracle_delete.argtypes = [C.c_void_p, C.c_uint32]
            L.oracle_find.argtypes = [C.c_void_p, C.c_char_p, C.c_uint16, C.c_void_p]
            L.oracle_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            L.oracle_tokenise.argtypes = [C.c_char_p, C.c_void_p]
            L.oracle_nb_entries.argtypes = [C.c_void_p, C.c_char_p]
            L.oracle_nb_entries.restype = C.c_uint64
            L.oracle_put_many.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
            L.oracle_put_many.restype = C.c_long
            L.oracle_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint16,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
            L.oracle_normalize_ascii.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p]
            L.oracle_normalize_ascii.restype = C.c_long
            cls._lib = L
        return cls._lib

    def __init__(self):
        self.L = self.lib()
        self.h = self.L.oracle_new()
        self._gen = 0                                            # bumped by every mutation (batch_upto's kept answer)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.oracle_free(self.h)
            self.h = None

    def put(self, needle, ref, weight=0):
        self._gen += 1
        return self.L.oracle_put(self.h, needle, ref, weight)

    def put_many(self, packed, offsets, refs=None):
        self._gen += 1
        return self.L.oracle_put_many(self.h, packed.ctypes.data, offsets.ctypes.data,
                                      None if refs is None else refs.ctypes.data, len(offsets) - 1)

    def delete(self, ref):
        self._gen += 1
        return self.L.oracle_delete(self.h, ref)

    def find(self, needle, limit=10):
        buf = (Match * max(limit, 1))()
        n = self.L.oracle_find(self.h, needle, limit, buf)
        return _rows(buf, n)

    def stats(self):
        a, b = C.c_uint32(), C.c_uint32()
        self.L.oracle_stats(self.h, C.byref(a), C.byref(b))
        return {"references": a.value, "trigrams": b.value}

    def nb_entries(self, needle):
        return int(self.L.oracle_nb_entries(self.h, needle))

    def batch(self, packed, offsets, idx=None, limit=10, find=True, nb=False, ntri=False, threads=None):
        """oracle_find / oracle_nb_entries / distinct-trigram count for needles ``idx`` (all when
        None) of a packed batch, on ``threads`` host threads (the oracle is read-only once built).
        Returns a dict with rows uint32[n, limit, 3] + counts, nb uint64[n], ntri uint32[n]."""
        n = len(offsets) - 1 if idx is None else len(idx)
        threads = threads or min(os.cpu_count() or 1, 64)
        packed = np.ascontiguousarray(packed)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        idx_a = None if idx is None else np.ascontiguousarray(idx, dtype=np.uint32)
        out = {}
        rows = counts = nb_a = nt_a = None
        if find:
            rows = np.zeros((n, max(limit, 1), 3), dtype=np.uint32)
            counts = np.zeros(n, dtype=np.uint32)
            out["rows"], out["counts"] = rows, counts
        if nb:
            nb_a = out["nb"] = np.zeros(n, dtype=np.uint64)
        if ntri:
            nt_a = out["ntri"] = np.zeros(n, dtype=np.uint32)
        ptr = lambda a: None if a is None else a.ctypes.data
        self.L.oracle_batch(self.h, packed.ctypes.data, offsets.ctypes.data, ptr(idx_a), n, limit,
                            ptr(rows), ptr(counts), ptr(nb_a), ptr(nt_a), threads)
        return out

    def batch_upto(self, packed, offsets, limit, upto, spot=96):
        """``batch(packed, offsets, limit=limit)`` for a test that asks the SAME needles of the SAME oracle at several
        limits: the answer at ``limit`` is the head of the answer at ``upto`` >= limit (storage.c:568-573 truncates one
        total order -- matches, weight, reference -- to the limit), so the oracle runs once at ``upto`` and later
        limits are cut from it.  The first ``spot`` needles are asked at ``limit`` itself every time and must agree
        with the cut.  The kept answer is dropped when the oracle or the batch changes (caller's arrays are held)."""
        assert limit <= upto
        key = (id(packed), id(offsets), upto, self._gen)
        if getattr(self, "_upto_key", None) != key:
            self._upto_key, self._upto_hold = key, (packed, offsets)
            self._upto_ans = self.batch(packed, offsets, limit=upto)
        rows = self._upto_ans["rows"][:, :max(limit, 1)].copy()
        counts = np.minimum(self._upto_ans["counts"], limit).astype(np.uint32)
        n_spot = min(spot, len(offsets) - 1)
        if n_spot and limit != upto:
            d = self.batch(packed, offsets, idx=np.arange(n_spot, dtype=np.uint32), limit=limit)
            assert np.array_equal(d["counts"], counts[:n_spot])
            live = np.arange(max(limit, 1))[None, :] < counts[:n_spot, None].astype(np.int64)
            assert np.array_equal(np.where(live[:, :, None], d["rows"], 0), np.where(live[:, :, None], rows[:n_spot], 0))
        return {"rows": rows, "counts": counts}

    @classmethod
    def tokenise(cls, needle):
        out = (C.c_uint16 * (len(needle) + 1))()
        n = cls.lib().oracle_tokenise(needle, out)
        return list(out[:n])

    @classmethod
    def normalize_ascii(cls, raw):
        """oracle/normalize_oracle.c: Blurrily::Map#normalize_string restated from the Ruby text
        (lib/blurrily/map.rb:40-47), ASCII input only (None for input with a byte >= 0x80)."""
        out = C.create_string_buffer(len(raw) + 1)
        n = cls.lib().oracle_normalize_ascii(raw, len(raw), out)
        return None if n < 0 else out.raw[:n]


class Reference:
    """The reference's own C compiled in place (oracle/_ref), bound lazily via ref_shim."""

    _shim = None

    @classmethod
    def available(cls):
        return os.path.exists(REF_SO) and os.path.exists(os.path.join(ORACLE_DIR, "libref_shim.so"))

    @classmethod
    def shim(cls):
        if cls._shim is None:
            S = C.CDLL(os.path.join(ORACLE_DIR, "libref_shim.so"))
            assert S.ref_open(REF_SO.encode()) == 0
            S.ref_find.argtypes = [C.c_void_p, C.c_char_p, C.c_uint16, C.c_void_p]
            S.ref_save.argtypes = [C.c_void_p, C.c_char_p]
            S.ref_stats.argtypes = [C.c_void_p, C.c_void_p]
            S.ref_tokenise.argtypes = [C.c_char_p, C.c_void_p]
            S.ref_find_many.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint16, C.c_void_p, C.c_void_p]
            S.ref_find_many.restype = C.c_long
            cls._shim = S
        return cls._shim

    def __init__(self, path):
        """Load a .trigrams file with the reference's blurrily_storage_load."""
        self.S = self.shim()
        self.h = C.c_void_p()
        res = self.S.ref_load(C.byref(self.h), os.fsencode(path))
        if res < 0:
            raise OSError(C.get_errno(), "reference load failed")

    def close(self):
        if self.h:
            self.S.ref_close(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def find(self, needle, limit=10):
        buf = (Match * max(limit, 1))()
        n = self.S.ref_find(self.h, needle, limit, buf)
        return _rows(buf, n)

    def save(self, path):
        return self.S.ref_save(self.h, os.fsencode(path))

    def stats(self):
        st = (C.c_uint32 * 2)()
        self.S.ref_stats(self.h, st)
        return {"references": st[0], "trigrams": st[1]}

    @classmethod
    def tokenise(cls, needle):
        out = (C.c_uint16 * (len(needle) + 1))()
        n = cls.shim().ref_tokenise(needle, out)
        return list(out[:n])


def block_digests(rows, counts, block):
    """SHA-256 per block of `block` consecutive needles: for each needle its count (u32), then its
    first `count` rows (u32 reference, matches, weight), little endian.  rows: uint32[n, limit, 3]."""
    import hashlib
    rows = np.ascontiguousarray(rows, dtype="<u4")
    counts = np.ascontiguousarray(counts, dtype="<u4")
    out = []
    for lo in range(0, len(counts), block):
        h = hashlib.sha256()
        for q in range(lo, min(len(counts), lo + block)):
            c = int(counts[q])
            h.update(counts[q:q + 1].tobytes())
            h.update(rows[q, :c].tobytes())
        out.append(h.hexdigest())
    return out


def build_pair(strings, refs=None, weights=None):
    """The same haystack in the product (RawMap) and in the oracle."""
    from blurrily_amd import RawMap
    m, o = RawMap(), Oracle()
    refs = list(range(1, len(strings) + 1)) if refs is None else refs
    weights = [0] * len(strings) if weights is None else weights
    for s, r, w in zip(strings, refs, weights):
        a = m.put(s, r, w)
        b = o.put(s, r, w)
        assert a == b, (s, r, w, a, b)
    return m, o


def golden_haystack(h):
    """Rebuild the seeded haystack a tests/golden/ref_find_*.json fixture was generated from:
    returns (packed, offsets, refs uint32[n], weights uint32[n] or None).  Shared by
    tools/make_golden.py so generator and tests cannot drift apart."""
    import workloads as W
    n = h["n"]
    if h["kind"] == "words":
        hay, off = W.words(n, h["seed"])
    elif h["kind"] == "geonames":
        hay, off = W.geonames(n, max(500, n // 10), h["seed"])
    else:
        hay, off = W.skewed(n, h["seed"])
    rng = np.random.default_rng(h["ref_seed"])
    refs = np.arange(1, n + 1, dtype=np.uint32)
    if h["refs"] == "sparse":
        refs = (rng.choice(2**31 - 2, size=n, replace=False) + 1).astype(np.uint32)
    weights = None
    if h["weights"] == "small":
        weights = rng.integers(0, 4, size=n).astype(np.uint32)
    return hay, off, refs, weights


def load_golden(name):
    import json
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def golden_find_files():
    return sorted(f for f in os.listdir(GOLDEN) if f.startswith("ref_find_") and f.endswith(".json"))


# ---- the reference's answers, recorded (tests/golden/ref_recorded.json, ref_abi.json: tools/make_golden.py) ----
# The inputs below are rebuilt from seeds by the generator and the tests alike; the fixtures hold only what the
# reference's own C answered for them, so that no test needs the reference tree or oracle/_ref.

RECORDED = "ref_recorded.json"
ABI = "ref_abi.json"


def rows_digest(rows):
    """First 16 hex digits of the SHA-256 of find rows [[reference, matches, weight], ...] as little-endian u32."""
    import hashlib
    return hashlib.sha256(np.asarray(rows, dtype="<u4").reshape(-1, 3).tobytes()).hexdigest()[:16]


def codes_digest(codes):
    """The same for a tokeniser's codes, as little-endian u16."""
    import hashlib
    return hashlib.sha256(np.asarray(codes, dtype="<u2").tobytes()).hexdigest()[:16]


def tokeniser_needles():
    """2000 seeded needles over a small alphabet with spaces, '*', capitals and a UTF-8 lead byte."""
    rng = np.random.default_rng(3)
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz   *Q\xc3", dtype=np.uint8)
    return [bytes(rng.choice(alphabet, size=int(rng.integers(0, 60))).tolist()) for _ in range(2000)]


# (kind, strings, limit) of the oracle's seeded comparisons and of the HIP path's larger ones
ORACLE_CASES = [("words", 5000, 10), ("geonames", 30000, 10), ("skewed", 20000, 100)]
HIP_CASES = [("geonames", 300000, 10), ("skewed", 200000, 100), ("words", 235886, 10)]


def case_key(kind, n, limit):
    return f"{kind}-{n}-{limit}"


def oracle_case_inputs(kind, n):
    """Haystack (seed 7) and needles (150 queries, seed 8, the empty needle and one letter) of ORACLE_CASES."""
    import workloads as W
    hay, off = {"words": W.words, "skewed": W.skewed}.get(kind, lambda n, s: W.geonames(n, 2000, s))(n, 7)
    q, qo = W.queries(hay, off, 150, 8)
    return hay, off, W.unpack(q, qo) + [b"", b"q"]


def hip_case_inputs(kind, n):
    """Haystack (seed 17) and needles (300 queries, seed 18) of HIP_CASES."""
    import workloads as W
    hay, off = {"words": W.words, "skewed": W.skewed}.get(kind, lambda n, s: W.geonames(n, 30000, s))(n, 17)
    q, qo = W.queries(hay, off, 300, 18)
    return hay, off, W.unpack(q, qo)


HEAD_LIMITS = (1, 10, 64)


def head_case_inputs(kind):
    """Haystack and 400 needles (seed 19) of the limit-head check (tests/test_oracle_pinning.py); the reference's
    rows are recorded for the first 60 needles at each of HEAD_LIMITS."""
    import workloads as W
    hay, off = W.geonames(30000, 4000, 17) if kind == "geonames" else W.skewed(30000, 18)
    q, qo = W.queries(hay, off, 400, 19)
    return hay, off, q, qo


def tiny_haystack_cases(count=200, seed=5):
    """Tiny adversarial haystacks: up to 40 distinct strings of up to 12 bytes over alphabets of 2, 3, 5 or 26
    letters (the last with spaces), weights 0..5 -- near-duplicates, tiny weights, ties everywhere -- a needle of up
    to 10 letters and a limit of 1..12.  Returns [(entries [(string, weight)], needle, limit)]."""
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(count):
        k = int(rng.choice([2, 3, 5, 27]))
        entries, seen = [], set()
        for _ in range(int(rng.integers(1, 41))):
            raw = rng.integers(0, 256, size=int(rng.integers(0, 13))).tolist()
            s = bytes(32 if x % k == 26 else 97 + x % k for x in raw)
            w = int(rng.integers(0, 6))
            if s not in seen:
                seen.add(s)
                entries.append((s, w))
        needle = bytes(97 + x % min(k, 26) for x in rng.integers(0, 256, size=int(rng.integers(0, 11))).tolist())
        cases.append((entries, needle, int(rng.integers(1, 13))))
    return cases


def resave_haystack():
    """The map whose saved file the reference loads and saves again (tests/test_host_index.py): 20 000 seeded
    geonames strings, every seventh reference deleted, one put after the deletions."""
    import workloads as W
    from blurrily_amd import RawMap
    hay, off = W.geonames(20000, 2000, 3)
    m = RawMap()
    m.put_many_packed(hay, off, np.arange(1, 20001, dtype=np.uint32))
    for r in range(1, 20001, 7):                   # deletions leave 0xFF-scribbled tail slots
        m.delete(r)
    m.put("after the deletions", 900001, 0)
    return m


# ---- the C-ABI tests' shared pieces (tests/test_*_abi.py, test_ruby_glue_syntax.py) ----
# the gem's own flags (ext/blurrily/extconf.rb:4-16), -Werror kept
FLAGS = ["-std=c99", "-Wall", "-Wextra", "-Werror", "-DPLATFORM_LINUX", "-D_XOPEN_SOURCE=700", "-D_GNU_SOURCE=1",
         "-D_FILE_OFFSET_BITS=64"]


def compile_c(tmp_path, src):
    """gcc over one C file with the gem's flags, headers from `tmp_path` (the recorded storage.h) and include/;
    the finished process (returncode, stderr)."""
    import subprocess
    cmd = ["gcc", *FLAGS, "-I", str(tmp_path), "-I", os.path.join(ROOT, "include"), "-c", str(src),
           "-o", str(tmp_path / "out.o")]
    return subprocess.run(cmd, capture_output=True, text=True)


def einval(call):
    """`call()`, an entry point given a bad argument, answers -1 with errno EINVAL."""
    import errno
    C.set_errno(0)
    assert call() == -1
    assert C.get_errno() == errno.EINVAL


def write_recorded_storage_h(directory):
    """A stand-in for the gem's ext/blurrily/storage.h, made from what tests/golden/ref_abi.json recorded of it:
    this repository's types, held to the recorded typedefs and row layout, and the nine functions declared with the
    reference's own prototypes.  C accepts a second declaration only if it is compatible with the first, so a
    translation unit that includes it compiles only while include/blurrily_storage.h agrees with the reference."""
    abi = load_golden(ABI)
    lines = ["#ifndef BLURRILY_RECORDED_STORAGE_H", "#define BLURRILY_RECORDED_STORAGE_H",
             '#include "blurrily_storage.h"', "#include <stddef.h>",
             "#define RECORDED_ASSERT(cond, name) typedef char recorded_##name[(cond) ? 1 : -1]"]
    for i, (name, target) in enumerate(sorted(abi["typedefs"].items())):
        lines.append(f"RECORDED_ASSERT(__builtin_types_compatible_p({name}, {target}), typedef_{i});")
    for i, (expr, value) in enumerate(sorted(abi["layout"].items())):
        lines.append(f"RECORDED_ASSERT(({expr}) == {value}, layout_{i});")
    lines += abi["prototypes"]
    lines.append("#endif")
    path = os.path.join(str(directory), "storage.h")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path
