"""The truth tests/test_gpu_cluster_tree_within.py compares blurrily_storage_cluster_tree_within with: cluster_truth.Truth
whose pairs() drops every pair whose ends carry different block keys.  cluster_tree_truth's kruskal, boruvka and cut, and
Truth.cluster, then give the blocked records, rounds and labels as they stand, since all of them see the graph through
pairs() alone.  Nothing of the library under test is used."""
import numpy as np

from cluster_truth import Truth


class BlockedTruth(Truth):
    """held: {reference: string} -- the map's contents as they should be now; key_of: {reference: block key} for every
    reference that will be listed (a reference without a key is in a block of its own)."""

    def __init__(self, held, key_of):
        super().__init__(held)
        own = -1 - np.arange(len(self.refs), dtype=np.int64)     # (no 32-bit key is negative)
        self.key = np.array([key_of.get(int(r), own[i]) for i, r in enumerate(self.refs)], dtype=np.int64)

    def pairs(self, listed, least=0):
        nodes, a, b, m = super().pairs(listed, least)
        same = self.key[a] == self.key[b]
        return nodes, a[same], b[same], m[same]


def blocked(held, listed, blocks):
    """The truth for a list and its keys (the same key wherever a reference is repeated)."""
    return BlockedTruth(held, dict(zip(np.asarray(listed).tolist(), np.asarray(blocks).tolist())))


def unblocked(truth):
    """The plain Truth over the same strings, sharing what `truth` has tokenised and the pairs it has found."""
    plain = Truth.__new__(Truth)
    plain.__dict__ = truth.__dict__
    return plain


def per_block(records_of):
    """Per-block trees as one: the records of every block's own tree, uint32[k, 3] each, concatenated and sorted under the
    total order (height descending, then the lower reference, then the higher)."""
    rows = [np.asarray(r, dtype=np.uint32).reshape(-1, 3) for r in records_of]
    rows = np.concatenate(rows) if rows else np.zeros((0, 3), dtype=np.uint32)
    return rows[np.lexsort((rows[:, 1], rows[:, 0], 1000 - rows[:, 2].astype(np.int64)))]
