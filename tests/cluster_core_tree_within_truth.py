"""The truth tests/test_gpu_cluster_core_tree_within.py compares blurrily_storage_cluster_core_tree_within with.  It
only composes: cluster_core_tree_truth.CoreTreeTruth sees the graph through truth.pairs() alone, and
cluster_tree_within_truth.BlockedTruth's pairs() drops every pair whose ends carry different block keys, so
CoreTreeTruth over a BlockedTruth ranks, caps and spans the within-block edges and nothing else.  per_block builds the
same from one CoreTreeTruth per block over the plain truth.  Nothing of the library under test is used."""
import numpy as np

from cluster_core_tree_truth import NO_CORE, CoreTreeTruth
from cluster_truth import NO_CLUSTER
from cluster_tree_within_truth import BlockedTruth, blocked, per_block as merged_records, unblocked


def blocked_over(truth, listed, blocks):
    """The blocked truth for a list and its keys over the strings a cluster_truth.Truth has tokenised already (the
    tokenisations are shared, the pairs are kept apart)."""
    t = BlockedTruth.__new__(BlockedTruth)
    t.__dict__ = dict(truth.__dict__)
    t._pairs = {}
    key_of = dict(zip(np.asarray(listed).tolist(), np.asarray(blocks).tolist()))
    own = -1 - np.arange(len(t.refs), dtype=np.int64)         # (no 32-bit key is negative)
    t.key = np.array([key_of.get(int(r), own[i]) for i, r in enumerate(t.refs)], dtype=np.int64)
    return t


def within(held, listed, blocks, p, min_degree, least=None):
    """The truth for a list, its keys (the same key wherever a reference is repeated), a floor and a min_degree."""
    return CoreTreeTruth(blocked(held, listed, blocks), listed, p, min_degree, least)


def per_block(truth, listed, blocks, p, min_degree, least=None):
    """One CoreTreeTruth per block over that block's elements alone (truth: a plain cluster_truth.Truth, or a blocked one,
    whose keys then change nothing), put back: (labels, core_permille in the order of `listed`, the records merged under
    the total order, and n_clusters, n_edges, n_core_edges summed)."""
    listed, blocks = np.asarray(listed, dtype=np.int64), np.asarray(blocks, dtype=np.int64)
    labels = np.full(len(listed), NO_CLUSTER, dtype=np.uint32)
    core = np.full(len(listed), NO_CORE, dtype=np.uint32)
    records, counts = [], [0, 0, 0]
    for k in np.unique(blocks).tolist():
        at = np.flatnonzero(blocks == k)
        t = CoreTreeTruth(truth, listed[at], p, min_degree, least)
        labels[at], core[at] = t.labels, t.core_permille
        records.append(t.merges)
        for i, c in enumerate((t.n_clusters, t.n_edges, t.n_core_edges)):
            counts[i] += c
    return labels, core, merged_records(records), tuple(counts)


__all__ = ["within", "per_block", "blocked", "blocked_over", "unblocked", "NO_CORE"]
