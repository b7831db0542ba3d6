"""The host's truths and inputs on tests/dense_case.py's map that the dense GPU files share
(tests/test_gpu_dense_floor_sweeps.py, tests/test_gpu_dense_cluster_within.py, tests/test_gpu_dense_scoped_finds.py) and
tests/test_dense_scoped_case.py proves without a GPU: the threshold and the similarity find restated for needles with tens
of thousands of rows (ArrayAbove, FlooredSimilar), their scoped forms, and the lists, block keys, family pair and scopes
of the blocked clustering and the scoped finds.  numpy and Oracle.tokenise alone, nothing of the library."""
from types import SimpleNamespace

import numpy as np

import above_truth
import dense_case as D
import similar_truth
from helpers import Oracle

LEAST = 200                                                    # every floor is at least this: the truths keep no pair below it
FIXED_FLOORS = (200, 350, 600)
# the family pair whose permille p* gives the last two floors, p* and p* + 1: of the thirteenth family (110 words),
# the string without its first fifth and the one with its words reversed
PAIR_FAMILY, PAIR_MEMBERS = 12, (4, 5)


class FlooredSimilar(similar_truth.Truth):
    """similar_truth.Truth for floors of at least `least`: only the candidates at or above `least` are ranked -- the
    rows at or above a floor p >= least are the same prefix of either ranking -- which spares a glued needle the exact
    fractions of the tens of thousands of references it shares a trigram with."""

    def __init__(self, strings, refs, weights, least):
        super().__init__(strings, refs, weights)
        self.least = least

    def rows(self, needle, limit, p):
        assert p >= self.least
        codes = Oracle.tokenise(needle)
        T = len(codes)
        if needle not in self._ranked:
            mask = np.zeros(similar_truth.NUM_CODES, dtype=bool)
            mask[codes] = True
            matches = np.add.reduceat(mask[self.flat].astype(np.int64), self.starts)
            matches[self.R == 0] = 0
            i = np.nonzero((matches >= 1) & (1000 * matches >= self.least * (T + self.R - matches)))[0]
            cands = zip(self.refs[i].tolist(), matches[i].tolist(), self.weights[i].tolist(), self.R[i].tolist())
            self._ranked[needle] = similar_truth.ranked(cands, T)
        return similar_truth.cut(self._ranked[needle], T, limit, p)


class ArrayAbove(above_truth.Truth):
    """above_truth.Truth with a needle's matches kept from one bar to the next and its rows as an array: the glued
    needles have tens of thousands of rows at the low bars."""

    def __init__(self, strings, refs, weights):
        super().__init__(strings, refs, weights)
        self._matches = {}

    def rows(self, needle, mm, mp):
        codes = Oracle.tokenise(needle)
        T = len(codes)
        t = above_truth.bar(T, mm, mp)
        if T == 0 or t > T:
            return np.zeros((0, 3), dtype=np.uint32)
        if needle not in self._matches:
            mask = np.zeros(above_truth.NUM_CODES, dtype=bool)
            mask[codes] = True
            matches = np.add.reduceat(mask[self.flat].astype(np.int64), self.starts)
            matches[~self.has] = 0
            self._matches[needle] = matches.astype(np.int16)      # (a string of these maps has under 2^15 trigrams)
        matches = self._matches[needle].astype(np.int64)
        keep = np.nonzero(matches >= t)[0]
        order = keep[np.lexsort((self.refs[keep], self.weights[keep], -matches[keep]))]
        return np.stack([self.refs[order], matches[order], self.weights[order]], axis=1).astype(np.uint32)


def floor_bar(T, p):
    """The bar of matches a sweep holds a needle of T trigrams to at floor p."""
    return max(1, (p * T + 999) // 1000)


def _same_bytes(one, other):
    for x, y in zip(one, other):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        else:
            assert x == y


# ---- the scoped forms ------------------------------------------------------------------------------------------------

def live_of(truth, scope):
    """The scope's live set: its references that the truth's map holds (sorted int64; kept per truth and scope)."""
    kept = truth.__dict__.setdefault("_live", {})
    key = np.asarray(scope, dtype=np.int64).tobytes()
    if key not in kept:
        kept[key] = np.intersect1d(np.asarray(scope, dtype=np.int64), truth.refs)
    return kept[key]


class ScopedAbove:
    """The scoped threshold find on an ArrayAbove: a needle's rows over the whole map at its bar, in order, kept where
    the reference is in the scope's live set (scope None: the whole map).  A threshold find has no cut."""

    def __init__(self, above):
        self.above = above

    def rows(self, needle, scope, mm, mp):
        rows = self.above.rows(needle, mm, mp)
        if scope is None:
            return rows
        return rows[np.isin(rows[:, 0].astype(np.int64), live_of(self.above, scope))]


class ScopedSimilar:
    """The scoped similarity find on a FlooredSimilar: the needle's ranked candidates (those at or above `least`)
    filtered to the scope's live set FIRST, then similar_truth.cut with the real limit and floor -- a row the whole-map
    find cuts off at its limit comes back when the rows in front of it are no members."""

    def __init__(self, similar):
        self.similar = similar

    def rows(self, needle, scope, limit, p):
        assert p >= self.similar.least
        self.similar.rows(needle, 1, self.similar.least)             # (ranks the needle's candidates once)
        ranked = self.similar._ranked[needle]
        if scope is not None and ranked:
            keep = np.isin(np.array([r[0] for r in ranked], dtype=np.int64), live_of(self.similar, scope))
            ranked = [r for r, k in zip(ranked, keep.tolist()) if k]
        return similar_truth.cut(ranked, len(Oracle.tokenise(needle)), limit, p)


# ---- the lists, the keys, the pair and the scopes --------------------------------------------------------------------

def key_pairs(refs):
    """(ref // 2) % 2: a family's two identical strings, head and head + 1, share a key, and so does the pair."""
    return ((np.asarray(refs, dtype=np.uint32) // 2) % 2).astype(np.uint32)


def key_parity(refs):
    """ref % 2: the pair's members lie under different keys."""
    return (np.asarray(refs, dtype=np.uint32) % 2).astype(np.uint32)


def key_families(refs):
    """Each family under a key of its own (10 + its index), the words under three (by ref // 7: the lists take every
    97th and every 9th word, and a key by ref % 3 would give all of the latter one key)."""
    refs = np.asarray(refs, dtype=np.uint32)
    family = refs >= D.FAMILY_REF0
    return np.where(family, 10 + (refs - np.where(family, D.FAMILY_REF0, 0)) // D.MEMBERS, (refs // 7) % 3).astype(np.uint32)


def inputs(h):
    """The lists, the pair and the scopes on dense_case.host()'s Host h: lists {"short", "long"}; pair (low, high) by
    position and its permille p_star; floors; family (the 90 references); scopes {name: references}."""
    family = np.array([r for head in h.heads for r in h.family(head)], dtype=np.uint32)
    words = h.refs[:D.N_WORDS]
    assert int(words[-1]) < D.FAMILY_REF0 <= int(h.refs[D.N_WORDS])
    lists = {"short": np.concatenate([words[::97], family]), "long": np.concatenate([words[::9], family])}
    head = h.heads[PAIR_FAMILY]
    low, high = (head + k for k in PAIR_MEMBERS)
    if h.loc[low][1] > h.loc[high][1]:
        low, high = high, low
    p_star = h.permille(low, high)
    floors = tuple(sorted(FIXED_FLOORS + (p_star, p_star + 1)))
    short = lists["short"]
    firsts = np.array([x + k for x in h.heads for k in (0, 1)], dtype=np.uint32)
    window = np.array([h.loc[int(r)][0] for r in h.refs], dtype=np.int64)
    rank = np.array([h.loc[int(r)][1] for r in h.refs], dtype=np.int64)
    scopes = {
        "short": short,
        "nofirst": short[~np.isin(short, firsts)],               # without each family's two identical strings
        "half": h.refs[key_pairs(h.refs) == 0],                  # every second pair of references of the whole map
        "upper": h.refs[(window == 1) | (rank >= D.HALF)],       # the second half window of window 0, and window 1
        "nolow": short[short != low],                            # without the pair's member at the lower position
        "words97": words[::97],                                  # words alone: the one scope with a direct form
    }
    return SimpleNamespace(lists=lists, pair=(low, high), p_star=p_star, floors=floors, family=family, scopes=scopes,
                           words=words)


def wide_members(h, scope):
    """How many of a scope's family members have more than 255 trigrams (such a member leaves a scope no direct form)."""
    return sum(1 for r in np.asarray(scope).tolist() if r >= D.FAMILY_REF0 and h.T(r) > 255)


def within_edges(truth, listed, blocks, p, least=LEAST):
    """The within-block edges (blocks None: the plain ones) of a list at floor p as a set of sorted reference pairs, from
    a cluster_truth.Truth's pairs."""
    nodes, a, b, m = truth.pairs(listed, least)
    edge = 1000 * m >= p * (truth.R[a] + truth.R[b] - m)
    if blocks is not None:
        key_of = dict(zip(np.asarray(listed).tolist(), np.asarray(blocks).tolist()))
        key = np.array([key_of.get(int(r), -1) for r in truth.refs], dtype=np.int64)
        edge &= key[a] == key[b]
    ra, rb = truth.refs[a[edge]].tolist(), truth.refs[b[edge]].tolist()
    return {(min(x, y), max(x, y)) for x, y in zip(ra, rb)}


def handmade():
    """The hand-made case of tests/test_gpu_dense_floor_sweeps.py: seventy copies of a word and, at the highest position,
    the word glued to another -- the word's six trigrams are the glued string's only dense slices, the bar at floor 500 is
    6 of its 12, and a copy shares exactly those six: (held {reference: string}, refs, weights, glued, word, other)."""
    word, other = b"klmno", b"pqrst"
    glued = word + b" " + other
    held = {1: glued, 100: other, 101: b"uvwxy"}
    held.update({r: word for r in range(2, 72)})
    refs = np.array(sorted(held), dtype=np.uint32)
    weights = np.where(refs == 1, 100, 1).astype(np.uint32)        # (the glued string last: the edges are its to find)
    h = D.Host(held, weights, [], D.DENSE_MIN)
    assert set(h.codes(2).tolist()) < set(h.codes(1).tolist()) and (h.T(2), h.T(1)) == (6, 12)
    assert h.loc[1] == (0, len(held) - 1) and floor_bar(12, 500) == 6 and h.permille(1, 2) == 500
    assert h.dense_padded(1, 0) == h.dense(1, 0) == 6 and sorted(h.postings[0][h.codes(2)].tolist()) == [71] * 6
    return SimpleNamespace(held=held, refs=refs, weights=weights, glued=glued, word=word, other=other, h=h)
