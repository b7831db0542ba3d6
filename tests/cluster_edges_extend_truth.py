"""The truth tests/test_gpu_cluster_edges_extend.py compares blurrily_storage_cluster_edges_extend and
blurrily_storage_cluster_edges_between with, on the host from cluster_edges_truth.records over both lists alone: of every
record among the listed, held references, the ones with at least one end named by the second list (extend) or with
exactly one (between).  A reference both lists name is on the second list's side only.  Nothing of the library under
test is used."""
import numpy as np

import cluster_edges_truth as CE


class Split:
    """The records over first ++ second at `floor`, and each record's side: how many of its ends the second list names."""

    def __init__(self, truth, first, second, floor, least=None):
        first, second = (np.asarray(x, dtype=np.uint32).reshape(-1) for x in (first, second))
        self.first, self.second = first, second
        self.whole = CE.records(truth, np.concatenate([first, second]), floor, least)
        new_ends = np.isin(self.whole[:, :2], second).sum(axis=1) if len(self.whole) else np.zeros(0, dtype=np.int64)
        self.old_old, self.old_new, self.new_new = (self.whole[new_ends == k] for k in (0, 1, 2))
        self.extend = self.whole[new_ends >= 1]               # (a subsequence: still in the total order)
        self.between = self.old_new
        # the old references that are not new, alone: what a caller holds before the second list arrives
        self.first_only = first[~np.isin(first, second)]
        self.held_before = CE.records(truth, self.first_only, floor, least)
        self.among_second = CE.records(truth, second, floor, least)

    def figures(self):
        return len(self.old_old), len(self.old_new), len(self.new_new)

    def check_itself(self):
        """Merged with the old-only records the extend records are the whole; between and the second list's own records
        are the extend records; the three sides are disjoint and everything."""
        assert self.held_before.tobytes() == self.old_old.tobytes()
        assert self.among_second.tobytes() == self.new_new.tobytes()
        assert CE.merged([self.held_before, self.extend]).tobytes() == self.whole.tobytes()
        assert CE.merged([self.between, self.among_second]).tobytes() == self.extend.tobytes()
        assert sum(self.figures()) == len(self.whole) and len(self.extend) == len(self.old_new) + len(self.new_new)
        return self
