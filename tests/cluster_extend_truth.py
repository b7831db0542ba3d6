"""The truth tests/test_gpu_cluster_extend.py compares blurrily_storage_cluster_extend with, computed on the host in
numpy on top of cluster_truth.Truth: Truth.pairs gives every pair of listed, held references that share a trigram with
its m; here the integer edge test is applied and only the pairs with a new end are kept (the similarity edges), the
seed edges are the pairs (old reference, its label) whose two ends are both held, listed and old, and the components
of the two kinds of edges together come from lowest-label propagation.  Nothing of the library under test is used."""
import numpy as np

from cluster_truth import NO_CLUSTER


class ExtendTruth:
    """labels_old, labels_new (in the lists' order), n_clusters, n_edges; of_ref {reference: label} of the nodes; and
    what the tests assert a split has: new_new_edges, old_new_edges, n_seeds (seed edges that exist, a node's own label
    apart)."""

    def __init__(self, truth, old_refs, old_labels, new_refs, p, least=0):
        assert p >= least
        refs, R = truth.refs, truth.R.astype(np.int64)
        n = len(refs)
        old = np.asarray(old_refs, dtype=np.int64).reshape(-1)
        seeds = np.asarray(old_labels, dtype=np.int64).reshape(-1)
        new = np.asarray(new_refs, dtype=np.int64).reshape(-1)
        assert len(old) == len(seeds)
        nodes, a, b, m = truth.pairs(np.concatenate([old, new]), least)
        node = np.zeros(n, dtype=bool)
        node[nodes] = True
        is_new = node & np.isin(refs, new)                       # named by new_refs, whatever old_refs says of it
        a, b, m = a.astype(np.int64), b.astype(np.int64), m.astype(np.int64)
        edge = 1000 * m >= p * (R[a] + R[b] - m)
        a, b = a[edge], b[edge]
        has_new = is_new[a] | is_new[b]                          # pairs of two old nodes are not looked at
        a, b = a[has_new], b[has_new]
        self.n_edges = len(a)
        self.new_new_edges = int((is_new[a] & is_new[b]).sum())
        self.old_new_edges = self.n_edges - self.new_new_edges

        def number(x):
            """(index into refs, whether it is an old node) of each reference of x."""
            if n == 0:
                return np.zeros(len(x), dtype=np.int64), np.zeros(len(x), dtype=bool)
            i = np.minimum(np.searchsorted(refs, x), n - 1)
            return i, (refs[i] == x) & node[i] & ~is_new[i]

        (ia, oka), (il, okl) = number(old), number(seeds)
        ok = oka & okl & (ia != il)
        sa, sb = ia[ok], il[ok]
        self.n_seeds = len(sa)
        ea, eb = np.concatenate([a, sa]), np.concatenate([b, sb])
        label = np.arange(n, dtype=np.int64)                      # (refs ascend: the lowest index is the lowest reference)
        while True:
            low = np.minimum(label[ea], label[eb])
            nxt = label.copy()
            np.minimum.at(nxt, ea, low)
            np.minimum.at(nxt, eb, low)
            nxt = nxt[nxt]
            if np.array_equal(nxt, label):
                break
            label = nxt
        self.of_ref = dict(zip(refs[nodes].tolist(), refs[label[nodes]].tolist()))
        self.n_clusters = len(set(self.of_ref.values()))
        self.labels_old = np.array([self.of_ref.get(int(r), NO_CLUSTER) for r in old], dtype=np.uint32)
        self.labels_new = np.array([self.of_ref.get(int(r), NO_CLUSTER) for r in new], dtype=np.uint32)
        self.is_new_ref = set(refs[is_new].tolist())
        # the similarity edges as pairs of references, for the tests that ask where their ends lie
        self.edge_refs = (refs[a], refs[b])
