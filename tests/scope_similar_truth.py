"""The scoped similarity find restated for tests/test_gpu_scope_similar.py, on similar_truth.Truth (numpy and exact
fractions over the strings' tokenisations, nothing of the library): a needle's full ranked rows over the whole map,
the rows of references outside the scope's live set removed, then similar_truth.cut with the real limit and floor.
The test anchors it on the oracle for a whole-map scope."""
from helpers import Oracle
from similar_truth import Truth, cut


class ScopedTruth:
    """The map's contents (reference -> (string, weight)), mutable as the map is."""

    def __init__(self):
        self.entries = {}
        self._truth = None

    def put(self, s, ref, weight):
        if ref not in self.entries:                       # (a put of a held reference changes nothing)
            self.entries[ref] = (s, weight)
            self._truth = None

    def delete(self, ref):
        if self.entries.pop(ref, None) is not None:
            self._truth = None

    def truth(self):
        if self._truth is None:
            refs = sorted(self.entries)
            self._truth = Truth([self.entries[r][0] for r in refs], refs, [self.entries[r][1] for r in refs])
        return self._truth

    def rows(self, needle, scope, limit, p):
        """[ref, m, weight, R] rows of `needle` among `scope` (an iterable of references; None: the whole map)."""
        full = self.truth().rows(needle, 10 ** 9, 0)
        if scope is not None:
            live = {int(r) for r in scope} & self.entries.keys()
            full = [r for r in full if r[0] in live]
        return cut(full, len(Oracle.tokenise(needle)), limit, p)

    def by_reference(self, ref, scope, limit, p):
        """... of the string `ref` was put with; none for a reference the map does not hold."""
        if ref not in self.entries:
            return []
        return self.rows(self.entries[ref][0], scope, limit, p)
