"""The truth tests/test_gpu_cluster_within.py compares blurrily_storage_cluster_within with: cluster_truth.Truth's pairs
(numpy over the strings' tokenisations), kept where both ends carry the same block key, the edge test in integers,
components by lowest-label propagation, label = the smallest reference of the component.  Nothing of the library under
test is used."""
import numpy as np

from cluster_truth import NO_CLUSTER, Truth


class WithinTruth(Truth):
    """held: {reference: string} -- the map's contents as they should be now."""

    def cluster_within(self, listed, blocks, p, least=0):
        """(labels in the order of `listed`, n_clusters, n_edges, the nodes' labels {reference: label}); blocks[i] is
        listed[i]'s key, the same wherever a reference is repeated; p >= least."""
        assert p >= least and len(listed) == len(blocks)
        key_of = dict(zip(np.asarray(listed).tolist(), np.asarray(blocks).tolist()))
        key = np.array([key_of.get(int(r), -1) for r in self.refs], dtype=np.int64)
        nodes, a, b, m = self.pairs(listed, least)
        edge = (1000 * m >= p * (self.R[a] + self.R[b] - m)) & (key[a] == key[b])
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


def telling(blocked, unblocked):
    """A floor tells blocked clustering from the plain one: the labellings {reference: label} differ on a node, some
    within-block component has three or more nodes, and a singleton exists."""
    _, sizes = np.unique(np.array(list(blocked.values()), dtype=np.int64), return_counts=True)
    differ = any(blocked[r] != unblocked[r] for r in blocked)
    return bool(differ and (sizes >= 3).any() and (sizes == 1).any())
