"""The truth tests/test_gpu_cluster_cores.py compares blurrily_storage_cluster_cores with, computed on the host in
numpy: cluster_truth.Truth.pairs gives every pair of listed, held references that share a trigram with its m, once per
list and floor; here the integer edge test is applied, the degrees are counted at both ends of every edge, and then per
min_degree: the cores, the components of the core-core edges by lowest-label propagation, every other node's anchor by
the maximum of (degree, -reference) over its core neighbours, the kinds, the labels and the three counts.  Nothing of
the library under test is used."""
import numpy as np

from cluster_truth import NO_CLUSTER

NONE, NOISE, BORDER, CORE = 0, 1, 2, 3


class CoresEdges:
    """One list at one floor: the nodes, the edges (a, b: indices into truth.refs, which ascend) and the degrees."""

    def __init__(self, truth, listed, p, least=0):
        assert p >= least
        self.truth, self.listed = truth, [int(r) for r in np.asarray(listed).tolist()]
        nodes, a, b, m = truth.pairs(listed, least)
        R = truth.R.astype(np.int64)
        edge = 1000 * m.astype(np.int64) >= p * (R[a] + R[b] - m)
        self.nodes, self.a, self.b = nodes, a[edge].astype(np.int64), b[edge].astype(np.int64)
        self.degree = np.zeros(len(truth.refs), dtype=np.int64)
        np.add.at(self.degree, self.a, 1)
        np.add.at(self.degree, self.b, 1)
        self.n_edges = len(self.a)

    def cores(self, min_degree):
        return CoresTruth(self, min_degree)


class CoresTruth:
    """One min_degree over a CoresEdges.  Per element of the list: labels, degrees, kinds; n_clusters, n_edges,
    n_core_edges; and per node (dicts by reference): label_of, degree_of, kind_of."""

    def __init__(self, e, min_degree):
        refs, nodes, a, b, degree = e.truth.refs, e.nodes, e.a, e.b, e.degree
        n = len(refs)
        node = np.zeros(n, dtype=bool)
        node[nodes] = True
        core = node & (degree >= min_degree)
        cc = core[a] & core[b]
        self.n_edges, self.n_core_edges = e.n_edges, int(cc.sum())
        ca, cb = a[cc], b[cc]
        label = np.arange(n, dtype=np.int64)                      # (refs ascend: the lowest index is the lowest reference)
        while True:
            low = np.minimum(label[ca], label[cb])
            nxt = label.copy()
            np.minimum.at(nxt, ca, low)
            np.minimum.at(nxt, cb, low)
            nxt = nxt[nxt]
            if np.array_equal(nxt, label):
                break
            label = nxt
        self.n_clusters = len(set(label[core].tolist()))
        # anchors: over the edges with exactly one core end, the other end's best (degree, -index) among its core ends
        one = core[a] != core[b]
        x = np.where(core[a[one]], b[one], a[one])                # the end that is no core
        c = np.where(core[a[one]], a[one], b[one])                # its core neighbour
        key = degree[c] * (n + 1) + (n - c)                       # (degree first, then the lower index)
        best = np.zeros(n, dtype=np.int64)
        np.maximum.at(best, x, key)
        border = node & ~core & (best > 0)
        anchor = n - best % (n + 1)
        label[border] = label[anchor[border]]
        kind = np.zeros(n, dtype=np.uint8)
        kind[node] = NOISE
        kind[border] = BORDER
        kind[core] = CORE
        # (what the tests assert a haystack has)
        sizes = np.bincount(label[core], minlength=n)
        self.big_clusters = int((sizes >= 3).sum())
        self.n_borders = int(border.sum())
        self.noise_with_an_edge = int(((kind == NOISE) & (degree >= 1)).sum())
        lo = np.full(n, n, dtype=np.int64)
        hi = np.full(n, -1, dtype=np.int64)
        np.minimum.at(lo, x, label[c])
        np.maximum.at(hi, x, label[c])
        self.torn_borders = int((border & (lo != hi)).sum())      # borders whose core neighbours lie in two clusters
        self.label_of = dict(zip(refs[nodes].tolist(), refs[label[nodes]].tolist()))
        self.degree_of = dict(zip(refs[nodes].tolist(), degree[nodes].tolist()))
        self.kind_of = dict(zip(refs[nodes].tolist(), kind[nodes].tolist()))
        self.labels = np.array([self.label_of.get(r, NO_CLUSTER) for r in e.listed], dtype=np.uint32)
        self.degrees = np.array([self.degree_of.get(r, 0) for r in e.listed], dtype=np.uint32)
        self.kinds = np.array([self.kind_of.get(r, NONE) for r in e.listed], dtype=np.uint8)
