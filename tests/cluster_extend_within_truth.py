"""The truth tests/test_gpu_cluster_extend_within.py compares blurrily_storage_cluster_extend_within with, computed on
the host in numpy on top of cluster_truth.Truth: Truth.pairs gives every pair of listed, held references that share a
trigram with its m; here the integer edge test is applied and only the pairs whose ends carry the same key and of which
at least one end is new are kept (the similarity edges), the seed edges are the pairs (old reference, its label) whose
two ends are both held, listed, old and under one key, and the components of the two kinds of edges together come from
lowest-label propagation.  Nothing of the library under test is used."""
import numpy as np

from cluster_truth import NO_CLUSTER


class ExtendWithinTruth:
    """labels_old, labels_new (in the lists' order), n_clusters, n_edges; of_ref {reference: label} of the nodes; and
    what the tests assert a case has: new_new_edges, old_new_edges, n_seeds (seed edges that exist, a node's own label
    apart), cross_key_seeds (seeds that do not exist only because their ends' keys differ) and cross_key_edges (pairs
    with a new end that pass the floor under different keys: what the key test is there to drop)."""

    def __init__(self, truth, old_refs, old_blocks, old_labels, new_refs, new_blocks, p, least=0):
        assert p >= least
        refs, R = truth.refs, truth.R.astype(np.int64)
        n = len(refs)
        old = np.asarray(old_refs, dtype=np.int64).reshape(-1)
        seeds = np.asarray(old_labels, dtype=np.int64).reshape(-1)
        new = np.asarray(new_refs, dtype=np.int64).reshape(-1)
        old_keys = np.asarray(old_blocks, dtype=np.int64).reshape(-1)
        new_keys = np.asarray(new_blocks, dtype=np.int64).reshape(-1)
        assert len(old) == len(seeds) == len(old_keys) and len(new) == len(new_keys)
        key_of = dict(zip(old.tolist(), old_keys.tolist()))
        for r, k in zip(new.tolist(), new_keys.tolist()):
            assert key_of.setdefault(r, k) == k                  # (a reference under two keys is an error, not a case)
        assert all(key_of[r] == k for r, k in zip(old.tolist(), old_keys.tolist()))
        key = np.array([key_of.get(int(r), -1) for r in refs], dtype=np.int64)
        nodes, a, b, m = truth.pairs(np.concatenate([old, new]), least)
        node = np.zeros(n, dtype=bool)
        node[nodes] = True
        is_new = node & np.isin(refs, new)                       # named by new_refs, whatever old_refs says of it
        a, b, m = a.astype(np.int64), b.astype(np.int64), m.astype(np.int64)
        edge = 1000 * m >= p * (R[a] + R[b] - m)                 # the edge test, in integers
        a, b = a[edge], b[edge]
        has_new = is_new[a] | is_new[b]                          # pairs of two old nodes are not looked at
        a, b = a[has_new], b[has_new]
        same = key[a] == key[b]
        self.cross_key_edges = int((~same).sum())
        a, b = a[same], b[same]
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
        self.cross_key_seeds = int((ok & (key[ia] != key[il])).sum())
        ok &= key[ia] == key[il]
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
        self.key_of = key_of
        self.n_clusters = len(set(self.of_ref.values()))
        self.labels_old = np.array([self.of_ref.get(int(r), NO_CLUSTER) for r in old], dtype=np.uint32)
        self.labels_new = np.array([self.of_ref.get(int(r), NO_CLUSTER) for r in new], dtype=np.uint32)
        self.is_new_ref = set(refs[is_new].tolist())

    def spans_two_keys(self):
        """Whether some component holds nodes under different keys (never, by construction of the edges)."""
        return any(self.key_of[r] != self.key_of[lab] for r, lab in self.of_ref.items())


# (haystack, n, modulus, floor, (components merging old groups, old labels moved, new-new edges, cross-key edges with a
# new end)): what a CPU run of this truth gave on the oracle haystacks, new being reference % 7 == 0 and the key
# reference % modulus
ORACLE_TABLE = [("words", 5000, 3, 200, (33, 180, 22, 469)), ("words", 5000, 3, 300, (1, 8, 3, 34)),
                ("geonames", 8000, 3, 500, (9, 330, 1533, 39608)), ("geonames", 8000, 3, 700, (4, 268, 558, 15561)),
                ("geonames", 8000, 64, 500, (22, 192, 71, 58354)), ("geonames", 8000, 64, 700, (1, 91, 26, 22952)),
                ("skewed", 6000, 3, 500, (21, 116, 11, 371))]


def contract_figures(within_truth, old, old_keys, new, new_keys, p, least=0):
    """What the issue's table counts for a split under the contract (seeds = cluster_within(old)): (the truth, the
    components that merge two or more old groups, the old labels that moved, new-new edges, cross-key edges with a new
    end).  within_truth is a cluster_within_truth.WithinTruth."""
    seeds, _, old_edges, _ = within_truth.cluster_within(old, old_keys, p, least)
    t = ExtendWithinTruth(within_truth, old, old_keys, seeds, new, new_keys, p, least)
    held = seeds != NO_CLUSTER
    groups_of = {}
    for was, now in zip(seeds[held].tolist(), t.labels_old[held].tolist()):
        groups_of.setdefault(now, set()).add(was)
    merging = sum(len(g) >= 2 for g in groups_of.values())
    moved = int((seeds != t.labels_old).sum())
    return t, seeds, old_edges, (merging, moved, t.new_new_edges, t.cross_key_edges)
