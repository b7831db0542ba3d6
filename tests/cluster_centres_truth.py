"""The truth tests/test_gpu_cluster_centres.py compares blurrily_storage_cluster_centres with, computed on the host in
numpy: cluster_truth.Truth gives every pair of listed, held references that share a trigram with its m, and the labels
and counts; here the integer edge test is applied once more, the degrees are counted at both ends of every edge, a
component's centre is its member of the highest degree (the smallest reference among equals), and a node is attached
when it is that centre or the edge list holds the pair of them.  Nothing of the library under test is used."""
import numpy as np

from cluster_truth import NO_CLUSTER


class CentresTruth:
    """One list at one floor.  Per element of `listed`: labels, degrees, centres, attached; n_clusters, n_edges; and
    per node (dicts by reference): label_of, degree_of, centre_of, attached_of."""

    def __init__(self, truth, listed, p, least=0):
        nodes, a, b, m = truth.pairs(listed, least)
        R = truth.R.astype(np.int64)
        edge = 1000 * m.astype(np.int64) >= p * (R[a] + R[b] - m)
        a, b = a[edge], b[edge]
        degree = np.zeros(len(truth.refs), dtype=np.int64)        # (by index into truth.refs, which ascend)
        np.add.at(degree, a, 1)
        np.add.at(degree, b, 1)
        self.labels, self.n_clusters, self.n_edges, self.label_of = truth.cluster(listed, p, least)
        assert self.n_edges == len(a)
        refs = truth.refs
        label = np.array([self.label_of[int(r)] for r in refs[nodes].tolist()], dtype=np.int64)
        # a component's centre: the highest degree first, the smallest reference among equals
        order = np.lexsort((refs[nodes], -degree[nodes], label))
        first = np.ones(len(order), dtype=bool)
        first[1:] = label[order][1:] != label[order][:-1]
        centre_of_label = dict(zip(label[order][first].tolist(), nodes[order][first].tolist()))
        centre = np.full(len(refs), -1, dtype=np.int64)               # (index of the node's centre)
        centre[nodes] = [centre_of_label[x] for x in label.tolist()]
        attached = np.zeros(len(refs), dtype=np.uint8)
        attached[nodes] = centre[nodes] == nodes
        attached[a[centre[a] == b]] = 1
        attached[b[centre[b] == a]] = 1
        self.degree_of = dict(zip(refs[nodes].tolist(), degree[nodes].tolist()))
        self.centre_of = dict(zip(refs[nodes].tolist(), refs[centre[nodes]].tolist()))
        self.attached_of = dict(zip(refs[nodes].tolist(), attached[nodes].tolist()))
        asked = [int(r) for r in np.asarray(listed).tolist()]
        self.degrees = np.array([self.degree_of.get(r, 0) for r in asked], dtype=np.uint32)
        self.centres = np.array([self.centre_of.get(r, NO_CLUSTER) for r in asked], dtype=np.uint32)
        self.attached = np.array([self.attached_of.get(r, 0) for r in asked], dtype=np.uint8)

    def telling(self):
        """(a component of four or more with an unattached member, a star of three or more, a singleton) -- which of
        them this floor has."""
        size, loose = {}, {}
        for r, lab in self.label_of.items():
            size[lab] = size.get(lab, 0) + 1
            loose[lab] = loose.get(lab, 0) + (1 - self.attached_of[r])
        chain = any(size[k] >= 4 and loose[k] >= 1 for k in size)
        star = any(size[k] >= 3 and loose[k] == 0 for k in size)
        return chain, star, any(v == 1 for v in size.values())
