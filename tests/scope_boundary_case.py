"""The inputs of tests/test_gpu_scope_sweeps.py and tests/test_gpu_scope_direct.py: SCOPES over
the three maps of tests/boundary_case.py, chosen so that a scope's mask -- a tombstone bitmap with nearly every bit set --
takes away exactly what a sweep leans on, and a small map of its own that puts the direct select on its edges.

Scopes (`scope(case, which, name)`: the references, uint32, of the named scope on map `which`):
  no_twins      every reference but each needle's twin and near twin: the row that sets the unscoped threshold is out;
  no_prefix15   every reference but the 15-trigram prefixes of the class needles from 16 trigrams on: a prefix lies in
                window 0 or 1 -- not where a longer needle's sweep starts --, starts with the hot word, and is among the
                needle's first ten rows with 15 matches, four of them in the slices a leaving sweep does not count: a
                non-member that would pass BY the left-out slices (as the second twins do that `no_late` leaves out);
  specials      the special references only (a few dozen: fewer members than most limits); specials_255 those of at most
                255 trigrams -- the direct form's ceiling for a member;
  hot           the references that start with the hot word: their matches with a needle of 15 .. 64 trigrams include the
                hot word's four codes, which lie in the slices a leaving sweep does not count; hot_w1: window 1's alone;
                hot_255: those of at most 255 trigrams (every class needle from 15 trigrams on starts with the hot word, so
                `hot` holds the twins and superstrings of the 256 .. 1 200 classes: no direct form);
  window0       the first 57 344 ranks of window 0 (kScopeMaxMembers exactly), window0_plus one more, window0_all the
                whole window: no member in window 1 or 2, so no needle of two or more bytes has one in its own window;
  rank_65519, rank_65520, rank_131039, rank_131040   ONE member, at a window's last and first rank (65 520 ranks are
                2 047.5 mask words: 65 519 and 65 520 share a word); edge_ranks all four;
  alternate     every reference of even rank;
  late_only / no_late (map C)   the second twins of window 4 / everything but them.

`ScopedTruth(case, which)` is tests/scope_truth.py over a whole map: the matches of every needle of the case with every
reference once, then any scope's rows from a subset of them.

`direct_case()` is the small map: members of exactly 255 and 256 trigrams, 600 copies of one string interleaved in member
order with 600 strings that share no trigram with it, fillers for scopes of any size, and the needles -- empty, 1 200
trigrams, b"ab" * 150, three with embedded NULs.

`conditions(sc)` asserts every fact the GPU tests rely on (tests/test_scope_boundary_case.py runs it without a GPU).  If a
re-seeded generator ever breaks one, change the seed, not the assertion."""
import numpy as np

import boundary_case as B
from helpers import Oracle
from scope_truth import Truth, c_prefix

MAX_MEMBERS = 57344                                            # find_kernels.h: kScopeMaxMembers
MAX_MEMBER_CODES = 255                                         # kScopeMaxMemberCodes
MAX_KEEP = 256                                                 # kScopeMaxKeep
EDGE_RANKS = (B.WINDOW_RANKS - 1, B.WINDOW_RANKS, 2 * B.WINDOW_RANKS - 1, 2 * B.WINDOW_RANKS)
SCOPES_A = ("no_twins", "no_prefix15", "specials", "specials_255", "hot", "hot_255", "hot_w1", "window0", "window0_plus", "window0_all",
            "rank_65519", "rank_65520", "rank_131039", "rank_131040", "edge_ranks", "alternate")
SCOPES_C = ("late_only", "no_late", "hot")


class View:
    """One map as arrays side by side: refs, weights, rank, ntri (int64), strings, and the flat code list."""
    _flat = {}

    def __init__(self, case, which):
        src = case.long() if which == "c" else case
        self.which = which
        self.refs = src.refs.astype(np.int64)
        self.weights = src.weights(which).astype(np.int64)
        self.rank = np.asarray(src.rank if which == "c" else src.rank(which), dtype=np.int64)
        self.ntri = np.asarray(src.ntri, dtype=np.int64)
        self.strings = src.strings
        key = "c" if which == "c" else "ab"                    # (maps A and B hold the same strings)
        if key not in View._flat:
            View._flat[key] = np.concatenate([np.asarray(Oracle.tokenise(s), dtype=np.int64) for s in self.strings])
        self.flat = View._flat[key]
        assert len(self.flat) == int(self.ntri.sum())
        self.starts = np.zeros(len(self.refs), dtype=np.int64)
        self.starts[1:] = np.cumsum(self.ntri)[:-1]
        self.at = {int(r): i for i, r in enumerate(self.refs)}
        self.is_hot = np.array([s.startswith(B.HOT + b" ") for s in self.strings])

    def index(self, refs):
        return np.array([self.at[int(r)] for r in refs], dtype=np.int64)


_VIEWS = {}


def view(case, which):
    if which not in _VIEWS:
        _VIEWS[which] = View(case, which)
    return _VIEWS[which]


def scope(case, which, name):
    """The references (uint32, ascending) of scope `name` on map `which`."""
    v = view(case, which)
    n = len(v.refs)
    if name == "no_twins":
        out = {case.ref_at(i, k) for i in range(len(case.needles)) for k in (0, 1)} - {None}
        keep = ~np.isin(v.refs, sorted(out))
    elif name == "no_prefix15":
        out = [case.ref_of(t, 3) for t in case.classes if t >= 16]
        keep = ~np.isin(v.refs, sorted(out))
    elif name == "specials":
        keep = np.isin(v.refs, sorted(case.role))
    elif name == "specials_255":
        keep = np.isin(v.refs, sorted(case.role)) & (v.ntri <= MAX_MEMBER_CODES)
    elif name == "hot":
        keep = v.is_hot
    elif name == "hot_255":
        keep = v.is_hot & (v.ntri <= MAX_MEMBER_CODES)
    elif name == "hot_w1":
        keep = v.is_hot & (v.rank // B.WINDOW_RANKS == 1)
    elif name == "window0":
        keep = v.rank < MAX_MEMBERS
    elif name == "window0_plus":
        keep = v.rank < MAX_MEMBERS + 1
    elif name == "window0_all":
        keep = v.rank < B.WINDOW_RANKS
    elif name.startswith("rank_"):
        keep = v.rank == int(name[5:])
    elif name == "edge_ranks":
        keep = np.isin(v.rank, EDGE_RANKS)
    elif name == "alternate":
        keep = v.rank % 2 == 0
    elif name == "late_only":
        keep = v.refs >= B.LATE_REF0
    elif name == "no_late":
        keep = v.refs < B.LATE_REF0
    elif name == "all":
        keep = np.ones(n, dtype=bool)
    else:
        raise KeyError(name)
    return v.refs[keep].astype(np.uint32)


class ScopedTruth:
    """tests/scope_truth.py over a whole map: `matches[i]` of needle i of the case with every reference (computed once,
    left unchanged), `rows(refs, i, limit)` of any scope, `batch(refs, limit)` as (rows[n, limit, 3], counts[n])."""

    def __init__(self, case, which):
        self.case, self.v = case, view(case, which)
        v = self.v
        mem = (v.refs, v.weights, v.flat, v.starts)
        self.matches = [Truth.matches(mem, nd) for nd in case.needles]
        self._batches = {}

    def rows(self, refs, i, limit):
        idx = self.v.index(refs) if not isinstance(refs, Subset) else refs.idx
        if len(idx) == 0 or limit == 0:
            return []
        return Truth.ranked(self.v.refs[idx], self.v.weights[idx], self.matches[i][idx], limit)

    def subset(self, refs):
        return Subset(self.v.index(refs))

    def batch(self, key, refs, limit):
        """the needle list's rows within `refs` at `limit`, as (rows[n, limit, 3], counts[n]) uint32.  A scope's ranking
        is computed once per `key` (its name) -- up to 1 025 rows, or up to 65 535 when a limit asks for more -- and every
        limit is a head of it: one total order, truncated (left unchanged)."""
        tier = 1025 if limit <= 1025 else 65535
        if (key, tier) not in self._batches:
            sub = self.subset(refs)
            self._batches[(key, tier)] = [
                Truth.ranked_array(self.v.refs[sub.idx], self.v.weights[sub.idx], self.matches[i][sub.idx], tier).astype(np.uint32)
                for i in range(len(self.case.needles))]
        full = self._batches[(key, tier)]
        rows, counts = np.zeros((len(full), limit, 3), dtype=np.uint32), np.zeros(len(full), dtype=np.uint32)
        for i, r in enumerate(full):
            counts[i] = min(len(r), limit)
            rows[i, :counts[i]] = r[:limit]
        return rows, counts


class Subset:
    def __init__(self, idx):
        self.idx = idx


# ---- the small map of the direct select --------------------------------------------------------------------------------
N_COPIES = 600
COPY_REF0, OTHER_REF0, PREFIX_REF0, FILL_REF0 = 10000, 20000, 30000, 40000
REF_255A, REF_255B, REF_256 = 50, 51, 52
COPIED = b"abc defg hij klm"                                   # letters a .. m; the others are spelt in n .. z
COPIED_PREFIX = b"abc def"                                    # (cut inside a word: its last code is not the copied string's)
N_FILL = 2400
SELECT_MEMBERS = 300                                           # the scope the select's boundary limits are taken on


class DirectCase:
    """strings / refs / weights of the small map (one window); `truth`, a scope_truth.Truth over it; the scopes and the
    needles of tests/test_gpu_scope_direct.py."""

    def __init__(self):
        c = B.case()
        rng = np.random.default_rng(20262)
        self.m255 = c.needles[c.classes[255]]
        self.m256 = c.needles[c.classes[256]]
        self.super255 = B.superstring(self.m255)
        ent = [(self.m255, REF_255A, 7), (self.m255, REF_255B, 9), (self.m256, REF_256, 8)]
        late = np.frombuffer(b"nopqrstuvwxyz", dtype=np.uint8)
        others = set()
        while len(others) < N_COPIES:
            others.add(bytes(rng.choice(late, size=8).tolist()))
        self.others = sorted(others)
        # member order is (weight, reference): copy k at weight 100 + 2k, other k at 101 + 2k
        for k in range(N_COPIES):
            ent.append((COPIED, COPY_REF0 + k, 100 + 2 * k))
            ent.append((self.others[k], OTHER_REF0 + k, 101 + 2 * k))
        for k in range(3):                                     # the prefix itself: above every copy under the prefix needle
            ent.append((COPIED_PREFIX, PREFIX_REF0 + k, 20 + k))
        seen = {s for s, _, _ in ent}
        fill = []
        while len(fill) < N_FILL:
            x, y = rng.integers(0, len(c.vocab), size=2).tolist()
            s = c.vocab[x][:6] + b" " + c.vocab[y][:7]
            if s not in seen:
                seen.add(s)
                fill.append(s)
        wf = rng.integers(1, 40, size=N_FILL).tolist()
        for k, s in enumerate(fill):
            ent.append((s, FILL_REF0 + k, wf[k]))
        self.strings = [e[0] for e in ent]
        self.refs = np.array([e[1] for e in ent], dtype=np.uint32)
        self.weights = np.array([e[2] for e in ent], dtype=np.uint32)
        self.truth = Truth()
        for s, r, w in ent:
            self.truth.put(s, int(r), int(w))
        self.fill_refs = np.arange(FILL_REF0, FILL_REF0 + N_FILL, dtype=np.uint32)
        self.ties = np.concatenate([COPY_REF0 + np.arange(N_COPIES), OTHER_REF0 + np.arange(N_COPIES)]).astype(np.uint32)
        self.ties_plus = np.concatenate([self.ties, PREFIX_REF0 + np.arange(3)]).astype(np.uint32)
        # needles: the empty one, 1 200 trigrams, b"ab" * 150, and three cut at an embedded NUL -- at byte 0, in the
        # middle, at byte 300 -- each with a SECOND NUL exactly 256 bytes behind the first: the kernel's 256 threads look
        # for NULs in a stride of 256, so ONE thread meets both, the nearer one first
        a300 = (b"abc defg hij " * 24)[:300]
        tail = (b"nop qrs tuv " * 22)[:255]
        self.long_needle = c.needles[c.classes[1200]]
        self.nul_needles = [b"\0" + tail + b"\0zzz", fill[0] + b"\0" + tail + b"\0" + fill[1], a300 + b"\0" + tail + b"\0zzz"]
        self.needles = [b"", self.long_needle, b"ab" * 150] + self.nul_needles
        # six needles for the select's boundary: two fillers, a filler's first word, the copied string, a common prefix
        self.select_needles = [fill[3], fill[4] + b" " + fill[5], fill[6].split(b" ")[0], COPIED, b"s", b"co"]

    def members(self, refs):
        return self.truth.members(refs)

    def rows(self, mem, needle, limit):
        return Truth.rows(mem, c_prefix(needle), limit)


_DIRECT = {}


def direct_case():
    if "d" not in _DIRECT:
        d = DirectCase()
        direct_conditions(d)
        _DIRECT["d"] = d
    return _DIRECT["d"]


def direct_conditions(d):
    T = B.T_of
    assert T(d.m255) == 255 and T(d.m256) == 256 and set(Oracle.tokenise(d.m255)) <= set(Oracle.tokenise(d.super255))
    copied = set(Oracle.tokenise(COPIED))
    for s in d.others:
        assert not (copied & set(Oracle.tokenise(s))), s
    assert len(set(Oracle.tokenise(COPIED_PREFIX)) & copied) == T(COPIED_PREFIX) - 1 < T(COPIED)
    # member order of the interleaved scope: copies at the even member indices, across five ballot chunks of 256
    mem = d.members(d.ties)
    order = np.lexsort((mem[0], mem[1]))
    assert len(order) == 2 * N_COPIES > 4 * 256
    assert (mem[0][order][0::2] >= COPY_REF0).all() and (mem[0][order][0::2] < COPY_REF0 + N_COPIES).all()
    assert (mem[0][order][1::2] >= OTHER_REF0).all()
    assert len(d.strings) < B.WINDOW_RANKS and all(T(s) <= 255 for s in d.strings if s is not d.m256)
    # the select's boundary: every needle has members that pass, few enough for limits around their count
    sel = d.members(d.fill_refs[:SELECT_MEMBERS])
    for nd in d.select_needles:
        passing = int((Truth.matches(sel, nd) >= 1).sum())
        assert 2 <= passing < MAX_KEEP, (nd, passing)
    # the needles
    assert T(d.long_needle) == 1200 and d.needles[0] == b""
    firsts = [nd.index(b"\0") for nd in d.nul_needles]
    assert firsts[0] == 0 and 0 < firsts[1] < 64 and firsts[2] == 300
    for nd, f in zip(d.nul_needles, firsts):
        assert nd[f + 256] == 0 and nd.count(b"\0") == 2
        assert T(c_prefix(nd)) != T(nd.replace(b"\0", b" ")[:f + 256])      # (cut at the second NUL: another code set)


# ---- what the GPU tests rely on ----------------------------------------------------------------------------------------
def conditions(case, truth_of):
    """truth_of(which) -> ScopedTruth.  Every scope's conditions, from numpy and the oracle's tokeniser alone."""
    c = case
    a, ta = view(c, "a"), truth_of("a")
    win = a.rank // B.WINDOW_RANKS
    assert np.bincount(win).tolist() == [B.WINDOW_RANKS, B.WINDOW_RANKS, 294] and len(a.refs) == 131334
    short = [i for t, i in c.classes.items() if 16 <= t <= 64]
    hot_codes = sorted(c.codes(B.HOT + b" x") & c.codes(B.HOT + b" y"))
    # no_twins: the unscoped first row is out; more than a pass of rows is left
    for which in ("a", "b"):
        t = truth_of(which)
        members = set(scope(c, which, "no_twins").tolist())
        everything = scope(c, which, "all")
        for i in range(c.n_class):
            first = t.rows(everything, i, 1)[0]
            assert first[0] == c.ref_at(i, 0) and first[0] not in members, (which, c.T[i], first)
        counts = t.batch("no_twins", scope(c, which, "no_twins"), 65535)[1]
        for tt in (15, 16, 64, 65, 127, 128, 1200):
            assert counts[c.classes[tt]] > 1024, (which, tt, counts[c.classes[tt]])
    # no_prefix15: what it leaves out is hot, in window 0 or 1, and among the first ten unscoped rows with 15 matches
    for which in ("a", "b"):
        v, t = view(c, which), truth_of(which)
        members = set(scope(c, which, "no_prefix15").tolist())
        for i in short:
            p = c.ref_of(c.T[i], 3)
            k = v.at[p]
            assert p not in members and v.is_hot[k] and v.rank[k] < 2 * B.WINDOW_RANKS and v.ntri[k] == 15
            assert [p, 15, 1] in t.rows(scope(c, which, "all"), i, 10), (which, c.T[i])
    # specials: fewer members than the limits 149 and 1 024; a member of 256 or more trigrams, specials_255 has none
    sp, sp255 = scope(c, "a", "specials"), scope(c, "a", "specials_255")
    assert len(sp) == 58 and len(sp255) == 49 and len(sp) < 149
    assert (a.ntri[a.index(sp)] >= 256).any() and (a.ntri[a.index(sp255)] <= 255).all()
    # hot: 8 673 members, 4 009 / 4 375 / 289 a window; every 16 .. 64 class needle has at least 150 of them with four or
    # more matches in windows 0 and 1, and the hot word's four codes are among every member's
    hot = a.index(scope(c, "a", "hot"))
    assert np.bincount(win[hot]).tolist() == [4009, 4375, 289] and len(hot) == 8673
    assert len(scope(c, "a", "hot_w1")) == 4375
    # ... among them the special strings of the classes from 15 trigrams on, up to 1 200 trigrams: `hot` has no direct
    # form, `hot_255` -- without the few of 256 trigrams and more -- has
    long_hot = int((a.ntri[hot] > MAX_MEMBER_CODES).sum())
    assert 0 < long_hot < 40 and len(scope(c, "a", "hot_255")) == len(hot) - long_hot
    assert (a.ntri[a.index(scope(c, "a", "hot_255"))] <= MAX_MEMBER_CODES).all()
    for i in short:
        for w in (0, 1):
            assert int(((ta.matches[i][hot] >= 4) & (win[hot] == w)).sum()) >= 150, (c.T[i], w)
        assert set(hot_codes) <= c.codes(c.needles[i])
    for k in hot[:: 97].tolist() + hot[-3:].tolist():
        assert set(hot_codes) <= c.codes(a.strings[k])
    assert a.is_hot[hot].all()                                 # (they start with HOT + b" ": the four codes, always)
    # window0*: sizes; no member in windows 1 or 2, where every needle of two or more bytes has its own window
    for name, size in (("window0", MAX_MEMBERS), ("window0_plus", MAX_MEMBERS + 1), ("window0_all", B.WINDOW_RANKS)):
        idx = a.index(scope(c, "a", name))
        assert len(idx) == size and (win[idx] == 0).all(), name
    assert (a.weights[win == 0] == 1).all() and all(len(nd) >= 2 for nd in c.needles[2:])
    # edge ranks: one member each, matched by at least one needle
    for which in ("a", "b"):
        v, t = view(c, which), truth_of(which)
        for r in EDGE_RANKS:
            refs = scope(c, which, f"rank_{r}")
            assert len(refs) == 1 and v.rank[v.at[int(refs[0])]] == r
            assert any(t.rows(refs, i, 1) for i in range(len(c.needles))), (which, r)
        assert len(scope(c, which, "edge_ranks")) == 4
    assert int(scope(c, "b", "rank_131039")[0]) == B.X_REF
    # alternate
    alt = a.index(scope(c, "a", "alternate"))
    assert (a.rank[alt] % 2 == 0).all() and len(alt) == (len(a.refs) + 1) // 2
    # map C
    L = c.long()
    late = scope(c, "c", "late_only")
    assert sorted(late.tolist()) == sorted(L.late.values())
    assert len(scope(c, "c", "no_late")) + len(late) == len(L.refs)
    vc = view(c, "c")
    assert (vc.rank[vc.index(late)] >= 4 * B.WINDOW_RANKS).all()
