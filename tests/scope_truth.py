"""The scoped top-k find restated in numpy (shared by tests/test_gpu_scope.py, tests/scope_boundary_case.py and the
files that run on the latter's inputs): a member's matches are the needle's distinct codes among its own; rows by
(matches desc, weight asc, reference asc), matches >= 1, truncated to the limit.  Anchored on helpers.Oracle where the
scope is the whole map (tests/test_gpu_scope.py, tests/test_scope_boundary_case.py)."""
import numpy as np

from helpers import Oracle

NUM_CODES = 28 * 28 * 28


def c_prefix(needle):
    """The needle as the library reads it: a C string within its bytes (storage.c:480)."""
    return needle.split(b"\0", 1)[0]


class Truth:
    """The map's contents (reference -> (string, weight)) and the scoped find restated in numpy: a member's matches are
    the needle's distinct codes among its own; rows by (matches desc, weight asc, reference asc), matches >= 1."""

    def __init__(self):
        self.entries = {}

    def put(self, s, ref, weight):
        if ref not in self.entries:
            self.entries[ref] = (s, weight if weight else len(s))

    def delete(self, ref):
        self.entries.pop(ref, None)

    def members(self, scope):
        refs = sorted({int(r) for r in scope if int(r) in self.entries})
        codes = [Oracle.tokenise(self.entries[r][0]) for r in refs]
        lens = np.array([len(c) for c in codes], dtype=np.int64)
        flat = np.array([c for cs in codes for c in cs], dtype=np.int64)
        starts = np.zeros(len(refs), dtype=np.int64)
        if len(refs):
            starts[1:] = np.cumsum(lens)[:-1]
        return (np.array(refs, dtype=np.int64), np.array([self.entries[r][1] for r in refs], dtype=np.int64),
                flat, starts)

    @staticmethod
    def matches(mem, needle):
        """every member's matches (int64[len(members)]): one boolean table of the needle's codes, summed over the flat
        code list member by member."""
        refs, weights, flat, starts = mem
        mask = np.zeros(NUM_CODES, dtype=bool)
        mask[Oracle.tokenise(needle)] = True
        return np.add.reduceat(mask[flat].astype(np.int64), starts)

    @staticmethod
    def ranked_array(refs, weights, matches, limit):
        """the rows of members (refs, weights) with these matches, int64[k, 3]."""
        keep = np.nonzero(matches >= 1)[0]
        order = keep[np.lexsort((refs[keep], weights[keep], -matches[keep]))][:limit]
        return np.stack([refs[order], matches[order], weights[order]], axis=1).astype(np.int64)

    @staticmethod
    def ranked(refs, weights, matches, limit):
        return Truth.ranked_array(refs, weights, matches, limit).tolist()

    @staticmethod
    def rows(mem, needle, limit):
        refs, weights, flat, starts = mem
        if len(refs) == 0 or limit == 0:
            return []
        return Truth.ranked(refs, weights, Truth.matches(mem, needle), limit)
