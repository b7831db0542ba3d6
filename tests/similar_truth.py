"""The numpy restatement of the similarity find that tests/test_gpu_similar.py and tests/test_gpu_dense_floor_sweeps.py
compare blurrily_storage_find_batch_similar with on haystacks too large for the oracle's complete find: from the
strings' tokenisations alone (Oracle.tokenise) and exact fractions, nothing of the library.  The tests anchor it on the
oracle for a few needles."""
from fractions import Fraction

import numpy as np

from helpers import Oracle

NUM_CODES = 28 * 28 * 28


def ranked(cands, T):
    """cands: (ref, m, weight, R) of every reference with m >= 1 -> [ref, m, weight, R] rows in result order: J
    descending (exact fractions), then matches descending, weight ascending, reference ascending."""
    keys = sorted((-Fraction(m, T + R - m), -m, w, ref, R) for ref, m, w, R in cands if m >= 1)
    return [[ref, -nm, w, R] for _, nm, w, ref, R in keys]


def cut(rows, T, limit, p):
    """The rows at or above the floor (J >= p / 1000 is a prefix of the ranked rows), cut at `limit`."""
    out = []
    if T == 0:
        return out
    for r in rows:
        if len(out) == limit or 1000 * r[1] < p * (T + r[3] - r[1]):
            break
        out.append(r)
    return out


class Truth:
    """The map's contents restated in numpy: m is the needle's distinct codes among a reference's own, R the count of
    its own."""

    def __init__(self, strings, refs, weights):
        self.refs = np.asarray(refs, dtype=np.int64)
        self.weights = np.array([w if w else len(s) for s, w in zip(strings, weights)], dtype=np.int64)
        codes = [Oracle.tokenise(s) for s in strings]
        self.R = np.array([len(c) for c in codes], dtype=np.int64)
        self.flat = np.array([c for cs in codes for c in cs], dtype=np.int64)
        self.starts = np.zeros(len(codes), dtype=np.int64)
        self.starts[1:] = np.cumsum(self.R)[:-1]
        self._ranked = {}

    def rows(self, needle, limit, p):
        codes = Oracle.tokenise(needle)
        if needle not in self._ranked:
            mask = np.zeros(NUM_CODES, dtype=bool)
            mask[codes] = True
            matches = np.add.reduceat(mask[self.flat].astype(np.int64), self.starts)
            matches[self.R == 0] = 0
            i = np.nonzero(matches >= 1)[0]
            cands = zip(self.refs[i].tolist(), matches[i].tolist(), self.weights[i].tolist(), self.R[i].tolist())
            self._ranked[needle] = ranked(cands, len(codes))
        return cut(self._ranked[needle], len(codes), limit, p)
