"""The inputs tests/test_gpu_find_boundaries.py runs the core find on: needles of an EXACT distinct-trigram count T at
every count where the kernels change their way, references that put a counter exactly on its
ceiling, and two maps over the same strings whose 4-bit window prefix ("nib_windows") differs by one reference's weight.

Needles.  One string per class T of CLASSES, built from space-separated words of a 3 000-word vocabulary and ending in a
space (see `class_needle`), plus the LENGTHS needles, where the count and the byte length -- which the host decides by --
fall on different sides of 64 and 127.

References.  Every class needle C has, under CLASS_REF0 + 8 * (its index) + k:
  k = 0  an exact twin: matches == T, the counter sits on `need` and, at T = 15 / 127, on its ceiling;
  k = 1  a near twin, T - 1 matches (none for T = 1);
  k = 2  a superstring: its trigram set contains C's;
  k = 3  for T >= 16, a whole-word prefix of C of exactly 15 distinct trigrams, all of them C's: a 4-bit counter
         reaches 15 under a needle that is not a <= 15 needle.
The LENGTHS needles have an exact twin each (LENGTH_REF0 + index).  Those of these strings that have at most 15 trigrams
take references at the end of the weight-1 block instead, so that they lie among the fillers (`Case.ref_at` knows
where), and X (below) takes X_REF.

Map A.  Everything of at most 15 trigrams has weight 1, everything else weight 2; ranks ascend in (weight, reference),
WINDOW_RANKS to a window.  The fillers -- one or two vocabulary words, the hot word HOT in front of one in sixteen -- top
the weight-1 strings up to exactly 2 * WINDOW_RANKS, so the first reference of more than 15 trigrams sits at rank
2 * 65 520 exactly: three windows, "nib_windows" 2.  Behind the long strings window 2 holds N_WEIGHT3 more hot fillers of
weight 3 (references WEIGHT3_REF0 ..).  The hot fillers make the four slices of "qua " dense in every window at
"dense_min" 64; every class needle of 15 and more trigrams starts with HOT.  That is what lets the needle-major sweep
leave slices out for them (tests/test_gpu_find_boundaries.py: test_slices_left_out): whichever window a sweep starts in,
a later window has dense slices AND a reference -- the twin, the superstring -- that reaches the threshold with
matches in those slices.

Map B.  The same strings.  X -- the twin of the T = 16 class needle, reference X_REF, the highest among the weight-1
ones -- swaps weights with the last filler: X lands on the LAST rank of window 1, the pair (0, 1) is no longer a pair of
<= 15 windows, "nib_windows" is 0.

Map C (`Case.long()`; tests/test_gpu_find_boundaries.py: test_slices_left_out_of_a_4_bit_sweep).  A needle of at most 15
trigrams sweeps three windows in TWO steps of a window pair, and a step is published while the step before is counted: the
second is out before the first has given a threshold, so nothing can be left out for it there.  Map C is map A with
weight-3 fillers up to exactly four windows, then -- window 4 -- N_WEIGHT4 hot fillers and N_WEIGHT4 fillers that start
with "a" under weight 4 and a second twin of every class needle of at most 64 trigrams under weight 5 (LATE_REF0 + its
index): five windows, three 4-bit steps, dense slices and a full match in the last.

`case()` is everything the host knows (numpy and helpers.Oracle, nothing of the library) and asserts, in `conditions`,
every fact about the inputs that the tests rely on.  If a re-seeded generator ever breaks one, change the seed, not the
assertion."""
import numpy as np

import workloads as W
from helpers import Oracle

WINDOW_RANKS = 65520                                           # device_index.h: ranks per window
NUM_CODES = 28 * 28 * 28
DENSE_MIN = 64
CLASSES = (1, 2, 15, 16, 17, 64, 65, 127, 128, 129, 255, 256, 257, 1200)
LENGTHS = ((63, 64), (64, 64), (64, 65), (126, 127), (127, 127), (300, 5))     # (bytes, distinct trigrams)
HOT = b"qua"
N_WEIGHT1 = 2 * WINDOW_RANKS                                   # references of weight 1 in map A: windows 0 and 1, full
CLASS_REF0 = 200000
LENGTH_REF0 = 210000
WEIGHT3_REF0 = 300000
N_WEIGHT3 = 256                                                # hot fillers of weight 3: they make HOT's slices dense in window 2
LONG_REF0 = 400000                                             # map C: weight-3 fillers up to four full windows ...
WEIGHT4_REF0 = 600000                                          # ... N_WEIGHT4 hot fillers and as many that start with "a", weight 4 ...
N_WEIGHT4 = 128
LATE_REF0 = 700000                                             # ... and the second twins, weight 5
X_REF = N_WEIGHT1 + 1                                          # above every other weight-1 reference, below every weight-2 one
LETTERS = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz ", dtype=np.uint8)


def T_of(s):
    return len(Oracle.tokenise(s))


def _needle_of(rng, t, length=None):
    """A string of exactly t distinct trigrams (of exactly `length` bytes, when given)."""
    while True:
        if length is not None:
            s = bytes(rng.choice(LETTERS, size=length).tolist())
            if T_of(s) == t and b"\0" not in s:
                return s
            continue
        s = bytes(rng.choice(LETTERS, size=t + 40).tolist())
        if T_of(s) >= t:
            for k in range(0, len(s) + 1):
                if T_of(s[:k]) == t:
                    return s[:k]


def class_needle(rng, t, vocab):
    """(C, P): a needle of exactly t distinct trigrams made of vocabulary words and, for t >= 16, its whole-word prefix P
    of exactly 15.  C = s + b" " where s has t - 1 and ends in a letter: the space turns s's last code (y, z, end) into
    the same (y, z, ' ') and adds (z, ' ', end), so s itself is the near twin.  A whole-word prefix keeps its codes
    inside a longer string for the same reason, hence P's set is a subset of C's."""
    if t == 1:
        return b"", None
    if t == 2:
        return b"a", None
    hot = t >= 15
    for _ in range(200000):
        pick = lambda: vocab[int(rng.integers(0, len(vocab)))]
        s, p = (HOT if hot else pick()), None
        if t >= 16:
            while T_of(s) < 15:
                s += b" " + pick()
            if T_of(s) != 15:
                continue
            p = s
        while T_of(s) < t - 1:
            s += b" " + pick()
        lo = len(p) if p else 1
        for k in range(lo, len(s) + 1):
            head = s[:k]
            if head[-1:] != b" " and (p is None or k == len(p) or k >= len(p) + 2) and T_of(head) == t - 1:
                c = head + b" "
                if T_of(c) == t:
                    return c, p
    raise AssertionError(f"no class needle of {t} trigrams")


def near_twin(c):
    return {b"": None, b"a": b"ab"}.get(c, c[:-1])


def superstring(c):
    return c + b" zq"


def locate(refs, weights):
    """rank of every reference, ascending in (weight, reference)."""
    refs, weights = np.asarray(refs, dtype=np.int64), np.asarray(weights, dtype=np.int64)
    order = np.lexsort((refs, weights))
    rank = np.zeros(len(refs), dtype=np.int64)
    rank[order] = np.arange(len(refs))
    return rank


def nib_windows_of(rank, ntri):
    """device_index.hip: windows are taken in PAIRS while both hold no reference of more than 15 trigrams."""
    n_win = (len(rank) + WINDOW_RANKS - 1) // WINDOW_RANKS
    wmt = np.zeros(n_win, dtype=np.int64)
    np.maximum.at(wmt, rank // WINDOW_RANKS, ntri)
    nib = 0
    while nib + 1 < n_win and wmt[nib] <= 15 and wmt[nib + 1] <= 15:
        nib += 2
    return nib, wmt


class Case:
    """needles: the class needles then the LENGTHS needles; T[i] their counts; classes {T: index}; prefix15 {T: string};
    refs, strings (side by side, references ascending), ntri; weights_a / weights_b; rank_a / rank_b; role {reference:
    (needle index, k)}; oracle_a / oracle_b (built on first use)."""

    def __init__(self):
        rng = np.random.default_rng(20260)
        vhay, voff = W.words(3000, seed=9)
        self.vocab = vocab = [w for w in W.unpack(vhay, voff) if 2 <= len(w) <= 9]
        self.needles, self.T, self.classes, self.prefix15, self.role = [], [], {}, {}, {}
        special = {}                                           # reference: string
        for i, t in enumerate(CLASSES):
            c, p = class_needle(rng, t, vocab)
            self.classes[t] = i
            self.needles.append(c)
            self.T.append(t)
            if p is not None:
                self.prefix15[t] = p
            for k, s in enumerate((c, near_twin(c), superstring(c), p)):
                if s is not None:
                    special[CLASS_REF0 + 8 * i + k] = s
                    self.role[CLASS_REF0 + 8 * i + k] = (i, k)
        for j, (length, t) in enumerate(LENGTHS):
            s = (b"ab" * 150) if length == 300 else _needle_of(rng, t, length)
            self.needles.append(s)
            self.T.append(T_of(s))
            special[LENGTH_REF0 + j] = s
            self.role[LENGTH_REF0 + j] = (len(CLASSES) + j, 0)
        x_old = CLASS_REF0 + 8 * self.classes[16]              # X: the T = 16 needle's twin, moved to X_REF
        special[X_REF] = special.pop(x_old)
        self.role[X_REF] = self.role.pop(x_old)
        # fillers: one word, two words, HOT + word; at most 14 bytes, hence at most 15 trigrams; distinct
        n_small = sum(1 for s in special.values() if T_of(s) <= 15 and s is not special[X_REF])
        n_fill = N_WEIGHT1 - n_small + N_WEIGHT3
        a = rng.integers(0, len(vocab), size=3 * n_fill)
        b = rng.integers(0, len(vocab), size=3 * n_fill)
        kind = rng.integers(0, 16, size=3 * n_fill)
        seen, fillers = set(special.values()), []
        for x, y, k in zip(a.tolist(), b.tolist(), kind.tolist()):
            s = HOT + b" " + vocab[x][:6] + vocab[y][:4] if k == 0 else vocab[x][:6] + b" " + vocab[y][:7]
            if s not in seen:
                seen.add(s)
                fillers.append(s)
                if len(fillers) == n_fill:
                    break
        assert len(fillers) == n_fill, len(fillers)
        hot_at = [i for i, f in enumerate(fillers) if f.startswith(HOT + b" ")][:N_WEIGHT3]
        heavy = [fillers[i] for i in hot_at]
        fillers = [f for i, f in enumerate(fillers) if i not in set(hot_at)]
        assert len(heavy) == N_WEIGHT3
        small = sorted(r for r, s in special.items() if T_of(s) <= 15)
        # references: the fillers 1 .., with the small specials spliced in at the END of the weight-1 block but for its
        # very last reference, which stays a filler (map B moves it to weight 2)
        held = {}
        for r, s in enumerate(fillers[:-1], start=1):
            held[r] = s
        at = len(fillers)
        self.small_ref = {}
        for r in small:
            held[at] = special[r]
            self.small_ref[r] = at
            self.role[at] = self.role.pop(r)
            at += 1
        held[at] = fillers[-1]
        self.last_filler = at
        assert at == N_WEIGHT1
        for r, s in special.items():
            if r not in self.small_ref:
                held[r] = s
        for k, s in enumerate(heavy):
            held[WEIGHT3_REF0 + k] = s
        self.refs = np.array(sorted(held), dtype=np.uint32)
        self.strings = [held[int(r)] for r in self.refs]
        self.packed = np.frombuffer(b"".join(self.strings), dtype=np.uint8)
        self.offsets = np.zeros(len(self.strings) + 1, dtype=np.uint64)
        self.offsets[1:] = np.cumsum([len(s) for s in self.strings])
        self.ntri = Oracle().batch(self.packed, self.offsets, find=False, ntri=True)["ntri"].astype(np.int64)
        self.weights_a = np.where(self.refs >= WEIGHT3_REF0, 3, np.where(self.ntri <= 15, 1, 2)).astype(np.uint32)
        self.weights_b = self.weights_a.copy()
        self._at = {int(r): i for i, r in enumerate(self.refs)}
        self.weights_b[self._at[X_REF]] = 1
        self.weights_b[self._at[self.last_filler]] = 2
        self.rank_a = locate(self.refs, self.weights_a)
        self.rank_b = locate(self.refs, self.weights_b)
        self._oracles = {}
        self.n_class = len(CLASSES)
        self._seen = seen

    def long(self):
        """Map C."""
        if not hasattr(self, "_long"):
            self._long = Long(self)
        return self._long

    def ref_at(self, i, k):
        """the reference of needle i's k-th special string (0 twin, 1 near twin, 2 superstring, 3 15-trigram prefix)."""
        for r, (ii, kk) in self.role.items():
            if ii == i and kk == k:
                return r
        return None

    def ref_of(self, t, k):
        """... of class t's."""
        return self.ref_at(self.classes[t], k)

    def codes(self, s):
        return set(Oracle.tokenise(s))

    def weights(self, which):
        return self.weights_a if which == "a" else self.weights_b

    def rank(self, which):
        return self.rank_a if which == "a" else self.rank_b

    def oracle(self, which):
        if which not in self._oracles:
            src = self.long() if which == "c" else self
            o = Oracle()
            for s, r, w in zip(src.strings, src.refs.tolist(), src.weights(which).tolist()):
                o.put(s, r, w)
            self._oracles[which] = o
        return self._oracles[which]

    def pack(self, needles):
        off = np.zeros(len(needles) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for s in needles])
        return np.frombuffer(b"".join(needles), dtype=np.uint8), off

    def postings(self, which):
        """[window][code]: references of the window that hold the code."""
        if not hasattr(self, "_flat"):
            lists = [Oracle.tokenise(s) for s in self.strings]
            assert [len(x) for x in lists] == self.ntri.tolist()
            self._flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists])
        win = self.rank(which) // WINDOW_RANKS
        n_win = int(win.max()) + 1
        owner = np.repeat(win, self.ntri)
        return np.bincount(owner * NUM_CODES + self._flat, minlength=n_win * NUM_CODES).reshape(n_win, NUM_CODES)


class Long:
    """Map C: refs, strings, packed, offsets, ntri, weights("c"), rank."""

    def __init__(self, c):
        rng = np.random.default_rng(20261)
        vocab = c.vocab
        n_more = 4 * WINDOW_RANKS - len(c.refs)                # weight-3 fillers up to the end of window 3
        seen, more, hot, a_first = set(c._seen), [], [], []
        draws = rng.integers(0, len(vocab), size=(3 * n_more, 3)).tolist()
        for x, y, k in draws:
            if len(more) == n_more and len(hot) == N_WEIGHT4 and len(a_first) == N_WEIGHT4:
                break
            s = HOT + b" " + vocab[x][:6] + vocab[y][:4] if k % 16 == 0 else vocab[x][:6] + b" " + vocab[y][:7]
            if s in seen:
                continue
            seen.add(s)
            if k % 16 == 0 and len(hot) < N_WEIGHT4:
                hot.append(s)
            elif s[:1] == b"a" and len(a_first) < N_WEIGHT4:
                a_first.append(s)
            elif len(more) < n_more:
                more.append(s)
        assert len(more) == n_more and len(hot) == N_WEIGHT4 == len(a_first)
        late = [(LATE_REF0 + i, c.needles[i]) for t, i in c.classes.items() if t <= 64]
        self.late = dict((i - LATE_REF0, i) for i, _ in late)  # needle index: its second twin's reference
        self.refs = np.concatenate([c.refs, LONG_REF0 + np.arange(n_more), WEIGHT4_REF0 + np.arange(2 * N_WEIGHT4),
                                    [r for r, _ in late]]).astype(np.uint32)
        self.strings = c.strings + more + hot + a_first + [s for _, s in late]
        self._weights = np.concatenate([c.weights_a, np.full(n_more, 3), np.full(2 * N_WEIGHT4, 4),
                                        np.full(len(late), 5)]).astype(np.uint32)
        self.packed = np.frombuffer(b"".join(self.strings), dtype=np.uint8)
        self.offsets = np.zeros(len(self.strings) + 1, dtype=np.uint64)
        self.offsets[1:] = np.cumsum([len(s) for s in self.strings])
        self.ntri = Oracle().batch(self.packed, self.offsets, find=False, ntri=True)["ntri"].astype(np.int64)
        self.rank = locate(self.refs, self._weights)
        conditions_long(c, self)

    def weights(self, which="c"):
        return self._weights


def conditions_long(c, L):
    """Map C: five windows, "nib_windows" 2; window 4 starts with the weight-4 fillers and ends with the second twins; HOT's
    four codes and (start, start, 'a') are dense in it."""
    nib, wmt = nib_windows_of(L.rank, L.ntri)
    assert len(wmt) == 5 and nib == 2 and wmt[3] <= 15 and wmt[4] == 64, wmt
    assert (L.rank[L._weights >= 4] >= 4 * WINDOW_RANKS).all() and (L.rank[L._weights < 4] < 4 * WINDOW_RANKS).all()
    in4 = [s for s, r in zip(L.strings, L.rank) if r >= 4 * WINDOW_RANKS]
    hot = c.codes(HOT + b" x") & c.codes(HOT + b" y")
    first_a = (c.codes(b"a") & c.codes(b"ab")).pop()           # (start, start, 'a')
    for code in sorted(hot) + [first_a]:
        assert sum(1 for s in in4 if code in c.codes(s)) >= 2 * DENSE_MIN, code
    assert sorted(L.late) == sorted(i for t, i in c.classes.items() if t <= 64)


def conditions(c):
    """Every fact about the inputs that the tests rely on, from numpy and the oracle's tokeniser alone."""
    # ---- the needles: exact counts; byte length against count
    for t, i in c.classes.items():
        assert T_of(c.needles[i]) == t == c.T[i], (t, T_of(c.needles[i]))
    for j, (length, t) in enumerate(LENGTHS):
        s = c.needles[c.n_class + j]
        assert len(s) == length and T_of(s) == t == c.T[c.n_class + j], (length, t, len(s), T_of(s))
    assert T_of(c.needles[c.n_class + 5]) <= 15 and len(c.needles[c.n_class + 5]) > 255
    # (the host's rule is by bytes: > 63 "maybe mid", > 126 "maybe long"; it is SAFE because a string of n bytes has at
    # most n + 1 distinct trigrams -- the four needles that sit on that edge, and the two it misjudges harmlessly)
    by_len = {(len(s), t) for s, t in zip(c.needles, c.T)}
    assert {(63, 64), (64, 64), (64, 65), (126, 127), (127, 127), (300, 5)} <= by_len
    assert all(t <= len(s) + 1 for s, t in zip(c.needles, c.T))
    # ---- the references of every class
    for t, i in c.classes.items():
        C = c.codes(c.needles[i])
        at = lambda k: c.strings[c._at[c.ref_of(t, k)]] if c.ref_of(t, k) is not None else None
        assert at(0) == c.needles[i]
        if t >= 2:
            assert len(C & c.codes(at(1))) == t - 1, t
        else:
            assert at(1) is None
        assert C <= c.codes(at(2)) and len(c.codes(at(2))) > t
        if t >= 16:
            P = c.codes(at(3))
            assert len(P) == 15 and P <= C and c.needles[i].startswith(at(3) + b" ")
        else:
            assert at(3) is None
    # ---- the maps: weights by trigram count, ranks, the windows' bounds, nib_windows
    assert int((c.weights_a == 1).sum()) == N_WEIGHT1 == int((c.weights_b == 1).sum())
    assert ((c.ntri > 15) == (c.weights_a == 2)).all() and int((c.weights_a == 3).sum()) == N_WEIGHT3
    nib_a, wmt_a = nib_windows_of(c.rank_a, c.ntri)
    nib_b, wmt_b = nib_windows_of(c.rank_b, c.ntri)
    assert len(wmt_a) == 3 == len(wmt_b)
    assert wmt_a[0] == 15 and wmt_a[1] == 15 and wmt_a[2] > 1200 and nib_a == 2
    assert wmt_b[0] == 15 and wmt_b[1] == 16 and wmt_b[2] > 1200 and nib_b == 0
    x = c._at[X_REF]
    assert c.ntri[x] == 16 and c.strings[x] == c.needles[c.classes[16]]
    assert c.rank_a[x] == 2 * WINDOW_RANKS                     # map A: the first rank of window 2
    assert c.rank_b[x] == 2 * WINDOW_RANKS - 1                 # map B: the last rank of window 1
    assert c.rank_b[c._at[c.last_filler]] == 2 * WINDOW_RANKS and c.ntri[c._at[c.last_filler]] <= 15
    first_long = int(c.rank_a[c.ntri > 15].min())
    assert first_long == 2 * WINDOW_RANKS
    # the 15-trigram prefixes and the twins of the <= 15 classes lie among the fillers, in a 4-bit window
    for t in c.classes:
        for k in range(4):
            r = c.ref_of(t, k)
            if r is not None and c.ntri[c._at[r]] <= 15:
                assert c.rank_a[c._at[r]] < 2 * WINDOW_RANKS and c.weights_a[c._at[r]] == 1
    # ---- dense slices: HOT's four codes are dense in every window of both maps, and every class needle of 15 and more
    # trigrams holds them; so do its twin and its superstring
    hot = sorted(c.codes(HOT + b" x") & c.codes(HOT + b" y"))
    assert len(hot) == 4
    for which in ("a", "b"):
        post = c.postings(which)
        assert (post[0][hot] >= 1024).all() and (post[1][hot] >= 1024).all(), (post[0][hot], post[1][hot])
        assert (post[2][hot] >= N_WEIGHT3).all() and N_WEIGHT3 >= 2 * DENSE_MIN
    for t, i in c.classes.items():
        if t >= 15:
            assert set(hot) <= c.codes(c.needles[i]), t


_CASE = {}


def case():
    if "c" not in _CASE:
        c = Case()
        conditions(c)
        _CASE["c"] = c
    return _CASE["c"]
