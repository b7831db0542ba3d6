"""The numpy restatement of the threshold find that tests/test_gpu_above.py and tests/test_gpu_dense_floor_sweeps.py
compare blurrily_storage_find_batch_above with on haystacks too large for the oracle's complete find: from the strings'
tokenisations alone (Oracle.tokenise), nothing of the library.  The tests anchor it on the oracle for a few needles."""
import numpy as np

from helpers import Oracle

NUM_CODES = 28 * 28 * 28


def bar(T, mm, mp):
    return max(1, mm, (mp * T + 999) // 1000)


class Truth:
    """The map's contents restated in numpy: a reference's matches are the needle's distinct codes among its own; rows
    by (matches desc, weight asc, reference asc)."""

    def __init__(self, strings, refs, weights):
        self.refs = np.asarray(refs, dtype=np.int64)
        self.weights = np.array([w if w else len(s) for s, w in zip(strings, weights)], dtype=np.int64)
        codes = [Oracle.tokenise(s) for s in strings]
        lens = np.array([len(c) for c in codes], dtype=np.int64)
        self.flat = np.array([c for cs in codes for c in cs], dtype=np.int64)
        self.starts = np.zeros(len(codes), dtype=np.int64)
        self.starts[1:] = np.cumsum(lens)[:-1]
        self.has = lens > 0

    def rows(self, needle, mm, mp):
        codes = Oracle.tokenise(needle)
        T = len(codes)
        t = bar(T, mm, mp)
        if T == 0 or t > T:
            return []
        mask = np.zeros(NUM_CODES, dtype=bool)
        mask[codes] = True
        matches = np.add.reduceat(mask[self.flat].astype(np.int64), self.starts)
        matches[~self.has] = 0
        keep = np.nonzero(matches >= t)[0]
        order = keep[np.lexsort((self.refs[keep], self.weights[keep], -matches[keep]))]
        return [[int(self.refs[i]), int(matches[i]), int(self.weights[i])] for i in order]
