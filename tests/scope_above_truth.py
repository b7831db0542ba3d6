"""The scoped threshold find restated for tests/test_gpu_scope_above.py, on above_truth.Truth (numpy over the strings'
tokenisations, nothing of the library): a needle's rows over the whole map at its bar, in order, the rows of references
outside the scope's live set removed -- a threshold find has no cut, so that is all.  The test anchors it on the oracle
for a whole-map scope."""
from above_truth import Truth


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

    def live(self, scope):
        """the scope's references the map holds now"""
        return {int(r) for r in scope} & self.entries.keys()

    def rows(self, needle, scope, mm, mp):
        """[ref, m, weight] rows of `needle` among `scope` (an iterable of references; None: the whole map)."""
        full = self.truth().rows(needle, mm, mp)
        if scope is None:
            return full
        live = self.live(scope)
        return [r for r in full if r[0] in live]

    def by_reference(self, ref, scope, mm, mp):
        """... of the string `ref` was put with; none for a reference the map does not hold."""
        if ref not in self.entries:
            return []
        return self.rows(self.entries[ref][0], scope, mm, mp)
