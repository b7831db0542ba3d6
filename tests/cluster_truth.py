"""The truth tests/test_gpu_cluster.py compares blurrily_storage_cluster with, computed on the host in numpy from the
strings alone (Oracle.tokenise gives a string's distinct trigram codes): every pair of listed, held references that
share a trigram, with its m; the edge test in integers; components by lowest-label propagation; label = the smallest
reference of the component.  Nothing of the library under test is used."""
import numpy as np

from helpers import Oracle

NO_CLUSTER = 0xFFFFFFFF


class Truth:
    """held: {reference: string} -- the map's contents as they should be now."""

    def __init__(self, held):
        self.refs = np.array(sorted(held), dtype=np.int64)
        self.codes = [np.array(Oracle.tokenise(held[int(r)]), dtype=np.int64) for r in self.refs]
        self.R = np.array([len(c) for c in self.codes], dtype=np.int32)
        self._pairs = {}

    def pairs(self, listed, least=0):
        """(a, b, m) of every pair a > b (indices into self.refs) of listed, held references with m >= 1 -- with `least`,
        only the pairs that are edges at that floor (what a haystack with too many pairs to keep is asked for)."""
        nodes = np.nonzero(np.isin(self.refs, np.asarray(listed, dtype=np.int64)) & (self.R > 0))[0]
        key = (nodes.tobytes(), least)
        if key in self._pairs:
            return self._pairs[key]
        # postings: for every code the nodes holding it, ascending
        owner = np.repeat(nodes, self.R[nodes]).astype(np.int32)
        flat = np.concatenate([self.codes[i] for i in nodes]) if len(nodes) else np.zeros(0, dtype=np.int64)
        order = np.argsort(flat, kind="stable")
        flat, owner = flat[order], owner[order]
        starts = np.searchsorted(flat, np.arange(28 * 28 * 28 + 1))
        A, B, M = [], [], []
        for a in nodes.tolist():
            parts = []
            for c in self.codes[a].tolist():
                post = owner[starts[c]:starts[c + 1]]
                parts.append(post[:np.searchsorted(post, a)])      # the nodes in front of a
            both = np.concatenate(parts)
            if both.size == 0:
                continue
            b, m = np.unique(both, return_counts=True)
            if least:
                keep = 1000 * m >= least * (self.R[a] + self.R[b] - m)
                b, m = b[keep], m[keep]
            A.append(np.full(len(b), a, dtype=np.int32))
            B.append(b.astype(np.int32))
            M.append(m.astype(np.int32))
        cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, dtype=np.int32)
        self._pairs = {key: (nodes, cat(A), cat(B), cat(M))}      # (one list's pairs are kept)
        return self._pairs[key]

    def cluster(self, listed, p, least=0):
        """(labels in the order of `listed`, n_clusters, n_edges, the nodes' labels {reference: label}); p >= least."""
        assert p >= least
        nodes, a, b, m = self.pairs(listed, least)
        edge = 1000 * m >= p * (self.R[a] + self.R[b] - m)            # (below 2^31: m, R < 2^15)
        a, b = a[edge], b[edge]
        label = np.arange(len(self.refs), dtype=np.int64)         # (refs ascending: the lowest index is the lowest reference)
        while True:
            low = np.minimum(label[a], label[b])
            nxt = label.copy()
            np.minimum.at(nxt, a, low)
            np.minimum.at(nxt, b, low)
            nxt = nxt[nxt]
            if np.array_equal(nxt, label):
                break
            label = nxt
        of_ref = dict(zip(self.refs[nodes].tolist(), self.refs[label[nodes]].tolist()))
        labels = np.array([of_ref.get(int(r), NO_CLUSTER) for r in listed], dtype=np.uint32)
        return labels, len(set(of_ref.values())), int(edge.sum()), of_ref


def shape(of_ref):
    """(components, components of three or more nodes, singletons) of a labelling."""
    _, sizes = np.unique(np.array(list(of_ref.values()), dtype=np.int64), return_counts=True)
    return len(sizes), int((sizes >= 3).sum()), int((sizes == 1).sum())
