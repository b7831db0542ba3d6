"""The truth tests/test_gpu_cluster_tree_extend.py compares blurrily_storage_cluster_tree_extend with, on the host, on top
of cluster_truth.Truth.pairs and cluster_tree_truth.edges (every pair of listed, held references with its height).  The
candidate edges are (a) the old records at or above the floor whose two ends are both nodes and both not new, at the
height the record states, and (b) the similarity edges at or above the floor with at least one new end; the expected
records are what Kruskal's algorithm keeps when it takes the candidates in the total order (height descending, lower
reference ascending, higher reference ascending), in the order it takes them.  Nothing of the library under test is
used."""
import numpy as np

import cluster_tree_truth as TT
from cluster_truth import NO_CLUSTER


def forest(n, lo, hi, h):
    """Kruskal over edges (lo, hi, h) between indices below n, lo < hi: (the kept edges as int64 [k, 3] rows in the total
    order, each index's root: the lowest index of its component)."""
    lo, hi, h = (np.asarray(x, dtype=np.int64) for x in (lo, hi, h))
    order = np.lexsort((hi, lo, -h))
    lo, hi, h = lo[order], hi[order], h[order]
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
    return np.array(out, dtype=np.int64).reshape(-1, 3), np.array([find(x) for x in range(n)], dtype=np.int64)


def boruvka_rounds(n, lo, hi, h):
    """The rounds of a synchronous Boruvka over the same edges that merge something (every component picks the best edge
    leaving it, all picked edges are united, again), and the forest it ends with as a set of (lo, hi, h)."""
    lo, hi, h = (np.asarray(x, dtype=np.int64) for x in (lo, hi, h))
    assert n <= TT.MASK
    key = (h.astype(np.uint64) << np.uint64(2 * TT.BITS)) | ((TT.MASK - lo).astype(np.uint64) << np.uint64(TT.BITS)) | \
        (TT.MASK - hi).astype(np.uint64)
    comp = np.arange(n, dtype=np.int64)
    chosen, rounds = set(), 0
    while True:
        out = comp[lo] != comp[hi]
        lo, hi, key = lo[out], hi[out], key[out]              # (an edge inside a component stays inside)
        if len(lo) == 0:
            return rounds, chosen
        best = np.zeros(n, dtype=np.uint64)
        np.maximum.at(best, comp[lo], key)
        np.maximum.at(best, comp[hi], key)
        picked = np.unique(best[best != 0])
        pl = TT.MASK - ((picked >> np.uint64(TT.BITS)) & np.uint64(TT.MASK)).astype(np.int64)
        ph = TT.MASK - (picked & np.uint64(TT.MASK)).astype(np.int64)
        chosen.update(zip(pl.tolist(), ph.tolist(), (picked >> np.uint64(2 * TT.BITS)).astype(np.int64).tolist()))
        rounds += 1
        _, root = forest(n, comp[pl], comp[ph], np.zeros(len(pl), dtype=np.int64))   # the picked edges united
        comp = root[comp]


class TreeExtendTruth:
    """records (uint32 [k, 3], references), labels_old, labels_new (in the lists' order), n_clusters, n_edges (the edges
    of (b), each once), of_ref {reference: label} of the nodes; and what the tests assert a case has: n_old_candidates
    (records that are candidates), dropped (candidate records the forest leaves out), new_new_edges, old_new_edges;
    candidates (n, lo, hi, h: indices into truth.refs and heights) for boruvka_rounds."""

    def __init__(self, truth, old_refs, old_records, new_refs, floor, least=None):
        refs = truth.refs
        n = len(refs)
        old = np.asarray(old_refs, dtype=np.int64).reshape(-1)
        new = np.asarray(new_refs, dtype=np.int64).reshape(-1)
        rec = np.asarray(old_records, dtype=np.int64).reshape(-1, 3)
        listed = np.concatenate([old, new])
        node = np.zeros(n, dtype=bool)
        node[TT.nodes_of(truth, listed)] = True
        is_new = node & np.isin(refs, new)                        # named by new_refs, whatever old_refs says of it
        # (b) the similarity edges with a new end
        lo, hi, h = TT.edges(truth, listed, floor, least)
        has_new = is_new[lo] | is_new[hi]
        lo, hi, h = lo[has_new], hi[has_new], h[has_new]
        self.n_edges = len(lo)
        self.new_new_edges = int((is_new[lo] & is_new[hi]).sum())
        self.old_new_edges = self.n_edges - self.new_new_edges
        # (a) the old records between two old nodes, at or above the floor
        if n and len(rec):
            ia = np.minimum(np.searchsorted(refs, rec[:, 0]), n - 1)
            ib = np.minimum(np.searchsorted(refs, rec[:, 1]), n - 1)
            ok = (refs[ia] == rec[:, 0]) & (refs[ib] == rec[:, 1]) & node[ia] & node[ib] & ~is_new[ia] & ~is_new[ib] & \
                (rec[:, 2] >= floor)
            assert (rec[:, 0] < rec[:, 1]).all()
            ra, rb, rh = ia[ok], ib[ok], rec[ok, 2]
        else:
            ra = rb = rh = np.zeros(0, dtype=np.int64)
        self.n_old_candidates = len(ra)
        self.candidates = (n, np.concatenate([ra, lo]), np.concatenate([rb, hi]), np.concatenate([rh, h]))
        kept, root = forest(*self.candidates)
        self.records = np.stack([refs[kept[:, 0]], refs[kept[:, 1]], kept[:, 2]], axis=1).astype(np.uint32).reshape(-1, 3)
        have = set(map(tuple, self.records.tolist()))
        candidates = set(zip(refs[ra].tolist(), refs[rb].tolist(), rh.tolist()))
        self.dropped = sorted(candidates - have)
        nodes = np.nonzero(node)[0]
        self.of_ref = dict(zip(refs[nodes].tolist(), refs[root[nodes]].tolist()))
        self.n_clusters = len(set(self.of_ref.values()))
        self.labels_old = np.array([self.of_ref.get(int(r), NO_CLUSTER) for r in old], dtype=np.uint32)
        self.labels_new = np.array([self.of_ref.get(int(r), NO_CLUSTER) for r in new], dtype=np.uint32)
