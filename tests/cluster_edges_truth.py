"""The truth tests/test_gpu_cluster_edges.py compares blurrily_storage_cluster_edges and
blurrily_storage_cluster_edges_within with, on the host from cluster_truth.Truth.pairs and cluster_tree_truth.edges alone:
every pair of listed, held references at or above the floor, once, as a record (a, b, permille) in references with
a < b, in the total order (height descending, lower reference ascending, higher reference ascending).  The blocked form
is the same over cluster_tree_within_truth.blocked's truth, whose pairs() drops the pairs under two keys.  And what the
records are turned into: the adjacency rows of a list, and the labels after uniting them.  Nothing of the library under
test is used."""
import numpy as np

import cluster_tree_truth as TT
import cluster_tree_within_truth as TW


def order(rows):
    """Records under the total order."""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, 3)
    return rows[np.lexsort((rows[:, 1], rows[:, 0], 1000 - rows[:, 2].astype(np.int64)))]


def records(truth, listed, floor, least=None):
    """uint32[E, 3]: all edges at `floor` among `listed`, in the total order.  `least` as cluster_tree_truth.edges'."""
    lo, hi, h = TT.edges(truth, listed, floor, least)
    assert (lo < hi).all()                                    # (truth.refs ascend: the lower index is the lower reference)
    rows = np.stack([truth.refs[lo], truth.refs[hi], h], axis=1) if len(lo) else np.zeros((0, 3))
    return order(rows.astype(np.uint32))


def blocked_records(held, listed, blocks, floor, least=None):
    """The same within blocks: (records, the blocked truth)."""
    truth = TW.blocked(held, listed, blocks)
    return records(truth, listed, floor, least), truth


def merged(records_of):
    """Several record lists (one per block, say) as one, under the total order."""
    return TW.per_block(records_of)


def adjacency(rows, listed):
    """(row_off, neighbour, permille) of a record list, a row per element of `listed`, neighbours in the records' order:
    by a plain loop over the records."""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, 3).tolist()
    of = {}
    for a, b, p in rows:
        of.setdefault(a, []).append((b, p))
        of.setdefault(b, []).append((a, p))
    row_off, neighbour, permille = [0], [], []
    for r in np.asarray(listed).tolist():
        for b, p in of.get(int(r), []):
            neighbour.append(b)
            permille.append(p)
        row_off.append(len(neighbour))
    return (np.array(row_off, dtype=np.uint64), np.array(neighbour, dtype=np.uint32), np.array(permille, dtype=np.uint32))


def labels(rows, listed, held_refs):
    """The labels of `listed` after uniting every record's ends: the lowest reference of each component, 0xFFFFFFFF for
    a reference that is not in held_refs.  (cluster_tree_truth.cut, every height taken.)"""
    held = set(int(r) for r in held_refs)
    marks = [0 if int(r) in held else 0xFFFFFFFF for r in np.asarray(listed).tolist()]
    return TT.cut(rows, marks, listed, 0)
