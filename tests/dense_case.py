"""The map tests/test_gpu_dense_floor_sweeps.py runs the floor sweeps on: one small haystack on which the parts of a
sweep that the other haystacks never reach are all reached -- more than 64 dense slices for one (needle, window),
16-bit counters with slices left out, neighbours in the upper half window of a wide needle, and a needle's windows
shared among two workgroups.

70 000 pseudo-words (references 1 ..) and 15 families of glued words (references 200 000 ..): 12, 25, 45, 70 and 110
random words of the haystack joined by spaces, three families of each, six members a family -- the string twice, with
b" zq" behind it, without its last two bytes, without its first fifth, and with its words reversed.  Weights are random,
so ranks are unrelated to length and a family's members fall into both windows and both halves of the first.  With
"dense_min" at 64 (set before the first put) every family head has more than 64 dense trigrams in window 0.

`host()` is everything the host knows (numpy and Oracle.tokenise, nothing of the library); `build()` adds the map and
asserts the conditions on the inputs that the tests rely on.  If a re-seeded generator ever breaks one of them, change
the seeds, not the assertion."""
import numpy as np

import workloads as W
from cluster_truth import Truth

WINDOW_RANKS = 65520                                           # device_index.h: ranks per window
HALF = 32768                                                   # a wide needle counts a window in two halves of this many ranks
MAX_DENSE = 64                                                 # dense slices of a (needle, window) a sweep can list
DENSE_MIN = 64
NUM_CODES = 28 * 28 * 28
N_WORDS = 70000
FAMILY_WORDS = (12, 25, 45, 70, 110)
FAMILY_REF0 = 200000
MEMBERS = 6


def family_of(words):
    s = b" ".join(words)
    return [s, s, s + b" zq", s[:-2], s[len(s) // 5:], b" ".join(reversed(words))]


def locate(refs, weights):
    """{reference: (window, in-window rank)}: ranks ascend in (weight, reference), WINDOW_RANKS to a window."""
    refs, weights = np.asarray(refs, dtype=np.int64), np.asarray(weights, dtype=np.int64)
    order = np.lexsort((refs, weights))
    rank = np.zeros(len(refs), dtype=np.int64)
    rank[order] = np.arange(len(refs))
    return {int(r): (int(k) // WINDOW_RANKS, int(k) % WINDOW_RANKS) for r, k in zip(refs, rank)}


def postings_of(truth, loc):
    """[window][code]: the held strings of the window with that code (truth: a cluster_truth.Truth over them)."""
    win = np.array([loc[int(r)][0] for r in truth.refs], dtype=np.int64)
    owner = np.repeat(win, truth.R)
    flat = np.concatenate(truth.codes)
    n_windows = int(win.max()) + 1
    return np.bincount(owner * NUM_CODES + flat, minlength=n_windows * NUM_CODES).reshape(n_windows, NUM_CODES)


class Host:
    """held {reference: string}; refs (ascending), strings and weights side by side; truth (cluster_truth.Truth);
    loc {reference: (window, rank)}; postings[window][code]; heads: the 15 families' first references; family(head):
    its six references; T(reference); dense(reference, window): its certainly dense codes there."""

    def __init__(self, held, weights, heads, dense_min):
        self.held, self.heads = held, heads
        self.refs = np.array(sorted(held), dtype=np.uint32)
        self.strings = [held[int(r)] for r in self.refs]
        self.weights = np.asarray(weights, dtype=np.uint32)
        self.truth = Truth(held)
        self.loc = locate(self.refs, self.weights)
        self.postings = postings_of(self.truth, self.loc)
        self.dense_min = dense_min
        self._at = {int(r): i for i, r in enumerate(self.refs)}

    def family(self, head):
        return list(range(head, head + MEMBERS))

    def codes(self, ref):
        return self.truth.codes[self._at[ref]]

    def T(self, ref):
        return int(self.truth.R[self._at[ref]])

    def dense(self, ref, window):
        return int((self.postings[window][self.codes(ref)] >= self.dense_min).sum())

    def dense_padded(self, ref, window):
        """... by the index's own rule: a slice is dense when its postings, padded to a multiple of 8, reach the bar."""
        return int(((self.postings[window][self.codes(ref)] + 7) // 8 * 8 >= self.dense_min).sum())

    def n_dense_pairs(self):
        return int((self.postings >= self.dense_min).sum())

    def permille(self, a, b):
        A, B = set(self.codes(a).tolist()), set(self.codes(b).tolist())
        return 1000 * len(A & B) // len(A | B)


_HOST = {}


def host():
    if "h" in _HOST:
        return _HOST["h"]
    hay, off = W.words(N_WORDS, seed=17)
    words = W.unpack(hay, off)
    held = {i + 1: s for i, s in enumerate(words)}
    rng = np.random.default_rng(61)
    heads, ref = [], FAMILY_REF0
    for k in FAMILY_WORDS:
        for _ in range(3):
            heads.append(ref)
            for s in family_of([words[int(i)] for i in rng.integers(0, N_WORDS, size=k)]):
                held[ref] = s
                ref += 1
    weights = np.random.default_rng(23).integers(1, 1 << 20, size=len(held)).astype(np.uint32)   # ranks unrelated to length
    h = _HOST["h"] = Host(held, weights, heads, DENSE_MIN)
    assert_inputs(h)
    return h


def assert_inputs(h):
    """The conditions on the inputs that the host can tell."""
    assert max(w for w, _ in h.loc.values()) == 1
    assert h.n_dense_pairs() > 1000
    narrow = [x for x in h.heads if h.T(x) <= 255 and h.dense(x, 0) > MAX_DENSE]
    wide = [x for x in h.heads if h.T(x) > 255 and h.dense(x, 0) > MAX_DENSE]
    assert len(narrow) >= 3 and len(wide) >= 3, (len(narrow), len(wide))
    both_up = across = windows = False
    for head in h.heads:
        at = [h.loc[r] for r in h.family(head)]
        in0 = [r for w, r in at if w == 0]
        if h.T(head) > 255:
            both_up |= sum(r >= HALF for r in in0) >= 2
            across |= any(r >= HALF for r in in0) and any(r < HALF for r in in0)
        windows |= len(in0) not in (0, MEMBERS)
    assert both_up, "no family with T > 255 has two members in window 0 at ranks >= 32768"
    assert across, "no family with T > 255 has a member on either side of rank 32768"
    assert windows, "no family has a member in window 1 and a member in window 0"


DEFAULT_DENSE_MIN = 1024                                       # device_index.h: kDenseMin
DEFAULT_WORDS = 40000
DEFAULT_FAMILIES = {1001: "low", 32766: "across", 36001: "up"}   # head reference: where its six ranks lie in the window


def host_default():
    """The second haystack, for the default "dense_min": 40 000 words and three families of 70 glued words in one
    window, weight = reference, so that rank = reference - 1: one family below rank HALF, one on both sides of it and
    one above it.  The words take the references the families leave."""
    if "d" in _HOST:
        return _HOST["d"]
    hay, off = W.words(DEFAULT_WORDS, seed=3)
    words = W.unpack(hay, off)
    rng = np.random.default_rng(67)
    held = {}
    for head in DEFAULT_FAMILIES:
        for j, s in enumerate(family_of([words[int(i)] for i in rng.integers(0, DEFAULT_WORDS, size=70)])):
            held[head + j] = s
    free = [r for r in range(1, DEFAULT_WORDS + len(held) + 1) if r not in held]
    held.update(zip(free, words))
    assert sorted(held) == list(range(1, DEFAULT_WORDS + 3 * MEMBERS + 1))
    h = _HOST["d"] = Host(held, np.array(sorted(held), dtype=np.uint32), list(DEFAULT_FAMILIES), DEFAULT_DENSE_MIN)
    assert all(h.loc[r] == (0, r - 1) for r in h.held)
    for head, where in DEFAULT_FAMILIES.items():
        ranks = [h.loc[r][1] for r in h.family(head)]
        assert h.T(head) > 255 and h.dense(head, 0) >= 1, (head, h.T(head), h.dense(head, 0))
        assert {"low": max(ranks) < HALF, "across": min(ranks) < HALF <= max(ranks), "up": min(ranks) >= HALF}[where]
    return h


def build_default():
    """(the map with every option at its default, the Host).  The caller closes the map."""
    from blurrily_amd import RawMap
    from blurrily_amd.map import _pack
    h = host_default()
    m = RawMap()
    m.put_many_packed(*_pack(h.strings), h.refs, h.weights)
    m.sync_device()
    info = m.device_info()
    assert info["n_windows"] == 1 and info["n_bitmaps"] >= h.n_dense_pairs() >= 1, (info, h.n_dense_pairs())
    assert m.get_option("dense_min") == DEFAULT_DENSE_MIN
    return m, h


def build():
    """(the map, the Host).  The caller closes the map."""
    from blurrily_amd import RawMap
    from blurrily_amd.map import _pack
    h = host()
    m = RawMap()
    m.set_option("dense_min", DENSE_MIN)                       # before the first put: changing it later forces a rebuild
    m.put_many_packed(*_pack(h.strings), h.refs, h.weights)
    m.sync_device()
    info = m.device_info()
    assert info["n_windows"] == 2, info["n_windows"]
    assert info["n_bitmaps"] >= h.n_dense_pairs() > 1000, (info["n_bitmaps"], h.n_dense_pairs())
    return m, h
