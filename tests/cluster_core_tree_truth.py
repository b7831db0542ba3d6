"""The truth tests/test_gpu_cluster_core_tree.py compares blurrily_storage_cluster_core_tree with, on the host in numpy
from cluster_truth.Truth.pairs alone: each pair's height h = 1000 m // (Ra + Rb - m), the pairs with h >= p as edges;
per node its core height c, the min_degree-th largest h among its edges, by sorting them (no core height with fewer
edges; 1000 for every node with min_degree == 0); the edges whose ends both have one, at H = min(h, c[a], c[b]);
Kruskal under the total order (H descending, lower reference ascending, higher reference ascending), whose accepted
edges in the order they are taken are the expected records; the labels and the four counts.  Nothing of the library
under test is used."""
import numpy as np

from cluster_truth import NO_CLUSTER

NO_CORE = 0xFFFFFFFF
BITS = 27
MASK = (1 << BITS) - 1


def edges(truth, listed, p, least=None):
    """(lo, hi, h): indices into truth.refs with lo < hi and the height of every edge at floor p.  `least` (default: p)
    is the floor the truth's pairs are asked at, so that several floors share one list of pairs."""
    _, a, b, m = truth.pairs(listed, p if least is None else least)
    a, b, m = a.astype(np.int64), b.astype(np.int64), m.astype(np.int64)
    h = 1000 * m // (truth.R[a].astype(np.int64) + truth.R[b] - m)
    keep = h >= p
    return b[keep], a[keep], h[keep]                          # (pairs() gives a > b)


def core_heights(n, nodes, lo, hi, h, min_degree):
    """c[index]: the min_degree-th largest height among the node's edges, -1 without one."""
    c = np.full(n, -1, dtype=np.int64)
    if min_degree == 0:
        c[nodes] = 1000
        return c
    # every edge at both its ends, sorted by node and, within a node, by height descending: one word per entry
    key = np.concatenate([lo, hi]).astype(np.uint64) << np.uint64(10) | (1000 - np.concatenate([h, h])).astype(np.uint64)
    key.sort()
    end, height = (key >> np.uint64(10)).astype(np.int64), 1000 - (key & np.uint64(1023)).astype(np.int64)
    first = np.searchsorted(end, np.arange(n))
    degree = np.bincount(end, minlength=n)
    has = nodes[degree[nodes] >= min_degree]
    c[has] = height[first[has] + min_degree - 1]
    return c


def forest(n, lo, hi, h):
    """Kruskal: (lo, hi, h) of the accepted edges in the total order, and every index's root (the lowest index of its
    component)."""
    key = ((1000 - h).astype(np.uint64) << np.uint64(2 * BITS)) | (lo.astype(np.uint64) << np.uint64(BITS)) | hi.astype(np.uint64)
    key.sort()
    lo = ((key >> np.uint64(BITS)) & np.uint64(MASK)).astype(np.int64)
    hi = (key & np.uint64(MASK)).astype(np.int64)
    h = 1000 - (key >> np.uint64(2 * BITS)).astype(np.int64)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    out = []
    at, step = 0, 4096
    while at < len(lo):                                       # in growing runs: the edges whose ends were together when the
        root = np.array([find(x) for x in range(n)], dtype=np.int64)   # run began are dropped without a loop
        l, g, ht = lo[at:at + step], hi[at:at + step], h[at:at + step]
        apart = root[l] != root[g]
        for el, eg, eh in zip(l[apart].tolist(), g[apart].tolist(), ht[apart].tolist()):
            rl, rg = find(el), find(eg)
            if rl != rg:
                parent[max(rl, rg)] = min(rl, rg)
                out.append((el, eg, eh))
        at, step = at + step, step * 2
    return out, np.array([find(x) for x in range(n)], dtype=np.int64)


class CoreTreeTruth:
    """One list at one (p, min_degree).  Per element of the list: labels, core_permille; merges [k, 3]; n_clusters,
    n_edges, n_core_edges; per index into truth.refs: c (-1: no core height) and node."""

    def __init__(self, truth, listed, p, min_degree, least=None):
        assert len(truth.refs) <= MASK
        self.truth, self.listed, self.p, self.min_degree = truth, [int(r) for r in np.asarray(listed).tolist()], p, min_degree
        refs, n = truth.refs, len(truth.refs)
        nodes = np.nonzero(np.isin(refs, np.asarray(listed, dtype=np.int64)) & (truth.R > 0))[0]
        lo, hi, h = edges(truth, listed, p, least)
        self.node = np.zeros(n, dtype=bool)
        self.node[nodes] = True
        self.c = c = core_heights(n, nodes, lo, hi, h, min_degree)
        tree = (c[lo] >= 0) & (c[hi] >= 0)
        lo, hi, h = lo[tree], hi[tree], h[tree]
        H = np.minimum(h, np.minimum(c[lo], c[hi]))
        kept, root = forest(n, lo, hi, H)
        self.merges = np.array([(refs[a], refs[b], ht) for a, b, ht in kept], dtype=np.uint32).reshape(-1, 3)
        self.n_edges, self.n_core_edges = len(tree), int(tree.sum())
        self.n_clusters = int((c >= 0).sum()) - len(kept)
        assert self.n_clusters == len(set(root[c >= 0].tolist()))
        label_of = dict(zip(refs[nodes].tolist(), refs[root[nodes]].tolist()))   # (a node without a core height: its own root)
        core_of = dict(zip(refs[nodes].tolist(), np.where(c[nodes] >= 0, c[nodes], NO_CORE).tolist()))
        self.labels = np.array([label_of.get(r, NO_CLUSTER) for r in self.listed], dtype=np.uint32)
        self.core_permille = np.array([core_of.get(r, NO_CORE) for r in self.listed], dtype=np.uint32)

    def cut(self, floor):
        """(is_core per index into truth.refs, {reference: label} of the cores, n_clusters) at `floor` >= p, by a
        plain union-find over the records with permille >= floor."""
        assert floor >= self.p
        refs = self.truth.refs
        is_core = self.c >= floor
        parent = {int(r): int(r) for r in refs[is_core].tolist()}

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for a, b, ht in self.merges.tolist():
            if ht >= floor:
                ra, rb = find(a), find(b)                     # (KeyError: a record at this floor names no core)
                assert ra != rb                               # (a forest)
                parent[max(ra, rb)] = min(ra, rb)
        label_of = {r: find(r) for r in parent}
        return is_core, label_of, len(set(label_of.values()))
