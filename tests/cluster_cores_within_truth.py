"""The truth tests/test_gpu_cluster_cores_within.py compares blurrily_storage_cluster_cores_within with:
cluster_cores_truth.CoresEdges' edges (numpy over the strings' tokenisations, the edge test in integers) kept where
both ends carry the same block key, and the degrees counted again over what is kept.  Everything per min_degree -- the
cores, the components of the core-core edges, the anchors, the kinds, the labels, the three counts -- is
cluster_cores_truth.CoresTruth over those edges as it stands.  Nothing of the library under test is used."""
import numpy as np

from cluster_cores_truth import CoresEdges, CoresTruth
from cluster_truth import NO_CLUSTER


class CoresWithinEdges(CoresEdges):
    """One list with its keys at one floor: blocks[i] is listed[i]'s key, the same wherever a reference is repeated."""

    def __init__(self, truth, listed, blocks, p, least=0):
        super().__init__(truth, listed, p, least)
        assert len(self.listed) == len(blocks)
        self.key_of = dict(zip(self.listed, (int(k) for k in np.asarray(blocks).tolist())))
        key = np.array([self.key_of.get(int(r), -1) for r in truth.refs], dtype=np.int64)
        same = key[self.a] == key[self.b]
        self.a, self.b = self.a[same], self.b[same]
        self.degree = np.zeros(len(truth.refs), dtype=np.int64)
        np.add.at(self.degree, self.a, 1)
        np.add.at(self.degree, self.b, 1)
        self.n_edges = len(self.a)
        self.key = key                                            # by index into truth.refs (-1: not listed)


def per_block(truth, listed, blocks, p, min_degree, least=0):
    """One CoresTruth per block over that block's elements alone, put back in place: (labels, degrees, kinds in the
    order of `listed`, and the three counts summed)."""
    listed, blocks = np.asarray(listed, dtype=np.int64), np.asarray(blocks, dtype=np.int64)
    labels = np.full(len(listed), NO_CLUSTER, dtype=np.uint32)
    degrees = np.zeros(len(listed), dtype=np.uint32)
    kinds = np.zeros(len(listed), dtype=np.uint8)
    counts = [0, 0, 0]
    for k in np.unique(blocks).tolist():
        at = np.flatnonzero(blocks == k)
        t = CoresTruth(CoresEdges(truth, listed[at], p, least), min_degree)
        labels[at], degrees[at], kinds[at] = t.labels, t.degrees, t.kinds
        for i, c in enumerate((t.n_clusters, t.n_edges, t.n_core_edges)):
            counts[i] += c
    return labels, degrees, kinds, tuple(counts)


def telling(blocked, unblocked):
    """A case tells blocked cores from the plain ones (two CoresTruth over the same list, floor and min_degree): it has
    clusters of three or more cores, borders, noise with an edge, borders whose core neighbours lie in two clusters,
    and labels and kinds that differ from the unblocked truth."""
    return bool(blocked.big_clusters and blocked.n_borders and blocked.noise_with_an_edge and blocked.torn_borders and
                (blocked.labels != unblocked.labels).any() and (blocked.kinds != unblocked.kinds).any())


def dense_lists(t):
    """dense_duplicates' lists from a CoresTruth: cores and borders, each ascending, ordered by label."""
    groups = {}
    for r, kind in t.kind_of.items():
        if kind >= 2:
            groups.setdefault(t.label_of[r], []).append(r)
    return [sorted(groups[k]) for k in sorted(groups)]
