"""The needle-major step's unit descriptors (needle_major.inc: BLURRILY_DESC) against the oracle,
row for row.  The manager publishes the bounds of a step's first 64 units, one per lane; a worker reads its own in one
LDS read and takes the units from 64 on, where a step has them, from the slice table as before.  What can go wrong
sits at the unit counts where the dealing (unit k to worker k mod 15) and the descriptor array end: a step of 0, 1,
14, 15, 16, 30, 63, 64, 65 and about 80 units, in the even window alone and over the even and the odd window together.

Haystacks of two and of three windows (70 000 and 140 000 strings of up to three four-letter words; the weights put
65 536 references into every window but the last).  One word is hot -- in six strings of ten -- so that its slices hold
more than 32 768 postings of window 0: more than 64 units in ONE slice.  The words' frequencies differ per window and
span four orders of magnitude; the needles are found by a seeded search over words of the haystack and over nonsense
words that share exactly one trigram with it, and the unit counts they give a step are worked out here from the
haystack's slice sizes (slice_units: postings padded to 8, / 512, rounded up) and ASSERTED.  The two-window haystack
holds strings of more than 15 trigrams in window 0, so needles of more than 15 trigrams are swept with byte counters
there; on the three-window one they take windows 0 and 1 as a 4-bit pair and window 2 -- the last pair's even window,
alone -- with byte counters.

Every batch runs under the plain sweep and under the one that leaves dense slices out (the options bench.py --force-sweep
1 and 3 set).  On images this small the second is mostly the same walk: a step's table is published while the step
before is counted, so a sweep of two or three steps has published its last before it has a threshold to leave anything
out by -- what it still changes is the pool's split and the pending lists' room.  Steps that do leave slices out, over
the same descriptors, are tests/test_gpu_leave.py's and tests/test_gpu_find_boundaries.py's."""
import itertools

import numpy as np
import pytest

from blurrily_amd import RawMap
from helpers import Oracle

pytestmark = pytest.mark.gpu

WINDOW_RANKS, NUM_CODES = 65536, 28 * 28 * 28
TARGETS = (0, 1, 14, 15, 16, 30, 63, 64, 65)
ABOUT_80 = range(75, 91)
LOW, HIGH = b"abcdefghijklmnop", b"rstuvwxyz"                  # the haystack's letters; letters of no haystack word
PLAIN = dict(ws_autotune=0, small_sweep=0, wsweep=0, nm_cmin=0)                        # nothing left out
LEAVE = dict(ws_autotune=0, small_sweep=0, wsweep=0, nm_min_windows=0, nm_cmin=3)       # dense slices left out


def slice_units(postings):
    return ((postings + 7) // 8 + 63) // 64


def _pack(strings):
    off = np.zeros(len(strings) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in strings])
    return np.frombuffer(b"".join(strings), dtype=np.uint8), off


def _codes(s):
    return sorted(set(Oracle.tokenise(s)))


class Case:
    """strings, weights, refs; units[window][code]; nib_windows; the needles and, per needle, its steps' (even, odd) units."""

    def __init__(self, n, seed, long_strings):
        rng = np.random.default_rng(seed)
        self.n, self.n_win = n, (n + WINDOW_RANKS - 1) // WINDOW_RANKS
        words = set()
        while len(words) < 160:
            words.add(bytes(rng.choice(list(LOW), size=4).tolist()))
        self.words = words = sorted(words)
        self.hot = hot = b"hhop"
        win = np.arange(n) // WINDOW_RANKS
        # Every string holds two words (and the hot one in front, in six of ten strings of the EVEN windows: units of an
        # even window alone).  In every window 24 words are heavy -- drawn for 1, 2, .. 24 units of postings each, one
        # word slot of a full window holding 128 units in all -- and the others rare (a unit at most) or, seven of ten in
        # an odd window and three of ten in an even one, absent.
        strings = [None] * n
        for w in range(self.n_win):
            lo, hi = w * WINDOW_RANKS, min(n, (w + 1) * WINDOW_RANKS)
            p = np.where(rng.random(len(words)) < (0.7 if w % 2 else 0.3), 0.0, 0.05)
            heavy = rng.permutation(len(words))[:16]
            p[heavy] = np.arange(2, 34, 2)
            pick = rng.choice(len(words), size=(hi - lo, 2), p=p / p.sum())
            front = rng.random(hi - lo) < (0.0 if w % 2 else 0.6)
            for i in range(lo, hi):
                a, b = pick[i - lo]
                parts = ([hot] if front[i - lo] else []) + [words[a], words[b]]
                if long_strings and i % 97 == 0:                # more than 15 trigrams: byte counters for window 0
                    parts = parts + [words[int(k)] for k in rng.integers(len(words), size=2)]
                strings[i] = b" ".join(parts)
        self.strings = strings
        self.refs = np.arange(1, n + 1, dtype=np.uint32)
        self.weights = (win + 1).astype(np.uint32)              # rank = index: window w holds strings [65 536 w, 65 536 (w + 1))
        self.packed, self.offsets = _pack(strings)
        lists = [Oracle.tokenise(s) for s in strings]
        ntri = np.array([len(set(x)) for x in lists], dtype=np.int64)
        owner = np.repeat(win, [len(x) for x in lists])
        flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists])
        pairs = np.unique(np.stack([np.repeat(np.arange(n), [len(x) for x in lists]), flat]), axis=1)   # a string holds a trigram once
        postings = np.bincount(win[pairs[0]] * NUM_CODES + pairs[1], minlength=self.n_win * NUM_CODES).reshape(self.n_win, NUM_CODES)
        del owner
        self.postings, self.units = postings, slice_units(postings)
        wmt = np.zeros(self.n_win, dtype=np.int64)
        np.maximum.at(wmt, win, ntri)
        self.nib_windows = 0                                    # device_index.hip: pairs of windows of at most 15 trigrams a reference
        while self.nib_windows + 1 < self.n_win and wmt[self.nib_windows] <= 15 and wmt[self.nib_windows + 1] <= 15:
            self.nib_windows += 2
        self.rng = rng

    def steps(self, needle):
        """(even, odd) units of every step of the needle's sweep: windows in pairs with 4-bit counters (every window for
        up to 15 trigrams, the leading `nib_windows` for more), one window a step with byte counters."""
        codes = _codes(needle)
        u = self.units[:, codes].sum(axis=1) if codes else np.zeros(self.n_win, dtype=np.int64)
        nib_end = self.n_win if len(codes) <= 15 else min(self.nib_windows, self.n_win)
        out = [(int(u[w]), int(u[w + 1]) if w + 1 < nib_end else 0) for w in range(0, nib_end, 2)]
        return out + [(int(u[w]), 0) for w in range(nib_end, self.n_win)], len(codes)

    def core(self, atoms):
        """a needle that shares exactly the trigrams `atoms` (three letters of the haystack each) with the haystack: the
        atoms between letters the haystack does not use -- 4 k + 2 trigrams for k atoms"""
        out = b"r"
        for i, t in enumerate(atoms):
            out += t + HIGH[1 + i % 8:2 + i % 8]
        return out if atoms else b"rstu"

    def padded(self, core, t_want):
        """the core with letters the haystack does not use appended until it has t_want distinct trigrams (None: it has
        more already) -- a string of n bytes has up to n + 1 trigrams, spaces and all"""
        s, have = core, len(_codes(core))
        if have > t_want:
            return None
        if have < t_want and core:
            s, have = core + b" ", len(_codes(core + b" "))
        for _ in range(400):
            if have == t_want:
                return s
            if have > t_want:
                return None
            nxt = s + bytes([int(self.rng.choice(list(HIGH)))])
            t = len(_codes(nxt))
            if have < t <= t_want:
                s, have = nxt, t
        return None

    def needles(self):
        """For every class of needle (up to 15 trigrams; exactly 16, 31, 64) and every unit count wanted -- in an even
        window alone, over an even and an odd window together --, a needle one of whose steps has it: a seeded search over
        sets of up to six of the haystack's letter trigrams.  Returns the needles, what was found -- {(class, 'alone' |
        'both', count): needle} -- and what was wanted."""
        rng = self.rng
        letters = set(LOW)
        atoms = sorted({w[i:i + 3] for s in self.strings[::7] for w in s.split() for i in range(len(w) - 2)} | {self.hot[:3], self.hot[1:]})
        assert all(set(a) <= letters for a in atoms)
        # (of r + atom + z only the atom is a trigram of the haystack)
        code = np.array([next(c for c in _codes(b"r" + a + b"z") if self.postings[:, c].sum() > 0) for a in atoms])
        U = self.units[:, code]                                             # [window][atom]
        top = np.argsort(-U.max(axis=0))[:40]
        found, needles = {}, []
        wanted = [(m, t) for m in ("alone", "both") for t in list(TARGETS) + [80] if not (m == "both" and t < 2)]
        for cls in (15, 16, 31, 64):
            nib_end = self.n_win if cls <= 15 else min(self.nib_windows, self.n_win)
            for k in (0, 1, 2, 3, 4, 5, 6):
                if 4 * k + 2 > cls:
                    break
                # (sets of any atoms, and sets of the forty atoms of most units -- every one of up to three: the large counts are sums of those)
                idx = np.stack([rng.permutation(len(atoms))[:k] for _ in range(1 if k == 0 else 3000)] +
                               ([top[list(c)] for c in itertools.combinations(range(len(top)), k)] if 0 < k <= 3 else
                                [top[rng.permutation(len(top))[:k]] for _ in range(0 if k == 0 else 6000)]))
                u = U[:, idx].sum(axis=2)                                   # [window][candidate]
                for w in list(range(0, nib_end, 2)) + list(range(nib_end, self.n_win)):
                    odd = u[w + 1] if w < nib_end and w + 1 < nib_end else np.zeros_like(u[w])
                    for mode, t in wanted:
                        if (cls, mode, t) in found:
                            continue
                        tot = u[w] + odd
                        ok = (odd == 0) if mode == "alone" else (odd > 0) & (u[w] > 0)
                        ok &= ((tot >= ABOUT_80[0]) & (tot <= ABOUT_80[-1])) if t == 80 else tot == t
                        hit = np.nonzero(ok)[0]
                        if len(hit):
                            core = self.core([atoms[j] for j in idx[hit[0]]])
                            s = self.padded(core, cls) if cls != 15 else core
                            if s is not None:
                                found[cls, mode, t] = s
                                needles.append(s)
        return needles, found, wanted

    def reachable(self, cls, mode):
        """steps over two windows exist where the needle's class is swept in 4-bit pairs"""
        return mode == "alone" or cls <= 15 or self.nib_windows >= 2


class Built:
    def __init__(self, n, seed, long_strings):
        c = self.case = Case(n, seed, long_strings)
        self.needles, self.found, self.wanted = c.needles()
        self.m = RawMap()
        self.m.set_option("dense_min", 1024)
        self.m.put_many_packed(c.packed, c.offsets, c.refs, c.weights)
        self.m.sync_device()
        self.o = Oracle()
        for s, r, w in zip(c.strings, c.refs.tolist(), c.weights.tolist()):
            self.o.put(s, r, w)
        # the batches: every needle found, repeated to 1 024 (the throughput launch) and the first 40 (latency mode's ranges)
        # (... and strings of the haystack itself, hot word and heavy words and all: many matches, a threshold, slices to leave out)
        own = c.strings[::max(1, c.n // 90)][:90]
        reps = (1024 - len(own) + len(self.needles) - 1) // len(self.needles)
        self.big = _pack((self.needles * reps)[:1024 - len(own)] + own)
        self.few = _pack(self.needles[::max(1, len(self.needles) // 30)][:30] + own[:10])
        self._want = {}

    def want(self, which, limit):
        if (which, limit) not in self._want:
            self._want[which, limit] = self.o.batch(*getattr(self, which), limit=limit)
        return self._want[which, limit]

    def check(self, which, limit):
        """the batch twice: rows against the oracle's and against each other"""
        packed, off = getattr(self, which)
        want = self.want(which, limit)
        live = np.arange(limit)[None, :] < want["counts"][:, None].astype(np.int64)
        first = None
        for _ in range(2):
            rows, counts = self.m.find_batch_packed(packed, off, limit)
            assert np.array_equal(counts, want["counts"])
            got = np.where(live[:, :, None], rows, 0)
            bad = np.nonzero((got != np.where(live[:, :, None], want["rows"], 0)).any(axis=(1, 2)))[0]
            if len(bad):
                q = int(bad[0])
                nd = bytes(packed[int(off[q]):int(off[q + 1])])
                raise AssertionError((len(bad), q, nd, self.case.steps(nd), rows[q, :counts[q]].tolist()[:4],
                                      want["rows"][q, :counts[q]].tolist()[:4]))
            assert first is None or np.array_equal(first, got)
            first = got
        return self.m.last_kernels()


@pytest.fixture(scope="module", params=["two", "three"])
def built(request):
    b = Built(70000, 341, True) if request.param == "two" else Built(140000, 342, False)
    b.name = request.param
    yield b
    b.m.close()


def test_the_needles_give_their_steps_the_unit_counts_wanted(built):
    c = built.case
    assert c.n_win == (2 if built.name == "two" else 3)
    assert c.nib_windows == (0 if built.name == "two" else 2)
    assert c.postings[0].max() > 32768 and c.units[0].max() > 64           # one slice of more than 64 units
    info = built.m.device_info()
    assert info["n_windows"] == c.n_win, info
    missing = [(cls, m, t) for cls in (15, 16, 31, 64) for m, t in built.wanted
               if c.reachable(cls, m) and (cls, m, t) not in built.found]
    assert not missing, missing
    for (cls, mode, tot), s in built.found.items():                          # ... as worked out again from the slice sizes
        st, t = c.steps(s)
        assert (t <= 15) if cls == 15 else t == cls
        sums = [e if o == 0 else e + o for e, o in st if (o == 0) == (mode == "alone") and (e or mode == "alone")]
        assert any((x in ABOUT_80) if tot == 80 else x == tot for x in sums), (cls, mode, tot, s, st)
    if built.name == "three":                                                # the last pair has an even window only
        assert any(len(c.steps(s)[0]) == 2 and c.steps(s)[1] <= 15 for s in built.needles)


@pytest.mark.parametrize("limit", [1, 10, 64])
@pytest.mark.parametrize("sweep", ["plain", "leave"])
def test_the_throughput_launch(built, sweep, limit):
    for k, v in (PLAIN if sweep == "plain" else LEAVE).items():
        built.m.set_option(k, v)
    kernels = built.check("big", limit)
    assert built.m.get_option("last_sweep") == (1 if sweep == "plain" else 3)
    assert kernels[0] == "find_kernel<uint8_t,1024,false,true>", kernels


@pytest.mark.parametrize("limit", [1, 10, 64])
def test_latency_modes_ranges(built, limit):
    for k, v in PLAIN.items():
        built.m.set_option(k, v)
    built.m.set_option("mid_max", 0)                            # (not over the pinned page, where find_one_kernel may serve them)
    try:
        kernels = built.check("few", limit)
    finally:
        built.m.set_option("mid_max", 128)
    print(built.name, limit, kernels)
    if built.name == "three":                                   # (three windows are the smallest image that is cut into ranges)
        assert kernels[0] == "find_kernel<uint8_t,1024,true,true>", kernels


def test_tombstones_and_pending_puts():
    """(last, on a map of its own: deletes since the image was built, and puts since then -- the delta image)"""
    b = Built(70000, 341, True)
    try:
        m, o, c = b.m, b.o, b.case
        for ref in range(1, 60000, 211):
            assert m.delete(ref) == o.delete(ref)
        for k, s in enumerate(c.strings[:200]):
            assert m.put(s + b" zq", 900000 + k, 1) == o.put(s + b" zq", 900000 + k, 1)
        for opts in (PLAIN, LEAVE):
            for k, v in opts.items():
                m.set_option(k, v)
            b.check("big", 10)
        assert m.device_info()["base_builds"] == 1
    finally:
        b.m.close()
