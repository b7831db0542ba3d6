"""What a caller does with cluster results once it holds them: cutting a tree, telling what an update changed, splitting
and merging record lists, neighbour lists, the profile a cut is chosen by, the groups of a labelling.  Numpy over arrays
the cluster methods returned (``map_clusters.py``): no function here needs a map or a GPU.  ``RawMap`` carries each
under its name as a static method.
"""
import numpy as np

from . import _native
from ._marshal import _permille, _records


def groups(refs, labels, member, min_size=1):
    """The groups of a labelling as lists: of the distinct ascending ``refs`` those that ``member`` marks, gathered by
    label -- a list of lists of references, each ascending, ordered by label, groups of fewer than ``min_size`` left
    out."""
    refs, labels = refs[member], labels[member]
    order = np.argsort(labels, kind="stable")               # (refs ascending within a label)
    _, starts, sizes = np.unique(labels[order], return_index=True, return_counts=True)
    return [refs[order[s:s + k]].tolist() for s, k in zip(starts.tolist(), sizes.tolist()) if k >= min_size]


def cut_tree(references, labels, merges, floor, min_permille=0):
    """The labels ``cluster(references, floor)`` would give, from a ``cluster_tree`` result alone: union-find in
    numpy over the merges with ``permille >= floor``.  ``labels`` are the tree's (they tell which references the
    map holds), ``min_permille`` the floor the tree was made at: the tree knows no edge below it, so a cut there
    is refused (ValueError), as is one above 1000.  Needs no map and no GPU."""
    floor, low = _permille(floor), _permille(min_permille)
    if floor < low:
        raise ValueError(f"floor {floor} below the tree's {low}: its edges are not in the tree")
    refs, labels = np.asarray(references, dtype=np.uint32), np.asarray(labels, dtype=np.uint32)
    merges = np.asarray(merges, dtype=np.uint32).reshape(-1, 3)
    if refs.ndim != 1 or labels.shape != refs.shape:
        raise ValueError("references and labels must be one-dimensional and of one length")
    held = labels != _native.NO_CLUSTER
    nodes = np.unique(refs[held])                             # ascending: the lowest index is the lowest reference
    kept = merges[merges[:, 2] >= floor]
    a, b = np.searchsorted(nodes, kept[:, 0]), np.searchsorted(nodes, kept[:, 1])
    if len(kept) and (max(a.max(), b.max()) >= len(nodes) or (nodes[a] != kept[:, 0]).any() or (nodes[b] != kept[:, 1]).any()):
        raise ValueError("a merge names a reference that the labels do not hold")
    label = np.arange(len(nodes), dtype=np.int64)
    while len(kept):                                          # lowest-label propagation with pointer jumping
        low_of = np.minimum(label[a], label[b])
        nxt = label.copy()
        np.minimum.at(nxt, a, low_of)
        np.minimum.at(nxt, b, low_of)
        nxt = nxt[nxt]
        if np.array_equal(nxt, label):
            break
        label = nxt
    out = np.full(len(refs), _native.NO_CLUSTER, dtype=np.uint32)
    out[held] = nodes[label[np.searchsorted(nodes, refs[held])]]
    return out


def cut_core_tree(references, labels, core_permille, merges, floor, min_permille=0):
    """What ``cluster_cores(references, floor, min_degree)`` says of the cores, from a ``cluster_core_tree`` result
    alone: ``(labels_at_floor, is_core)``.  A reference is a core at ``floor`` when its core height is at least
    ``floor``; the cores are labelled by the smallest reference of their component under the merges with
    ``permille >= floor``, every other node by its own reference (its anchor needs its degree at that floor,
    which the tree does not hold), and a reference that is no node keeps ``NO_CLUSTER``.  ``min_permille`` is the
    floor the tree was made at; a cut below it or above 1000 is refused (ValueError).  Needs no map and no GPU."""
    core = np.asarray(core_permille, dtype=np.uint32)
    refs = np.asarray(references, dtype=np.uint32)
    if core.shape != refs.shape:
        raise ValueError("references and core_permille must be of one length")
    cut = cut_tree(refs, labels, merges, floor, min_permille)   # (checks the rest)
    is_core = (core != _native.NO_CORE) & (core >= _permille(floor)) & (cut != _native.NO_CLUSTER)
    merges = np.asarray(merges, dtype=np.uint32).reshape(-1, 3)
    kept = merges[merges[:, 2] >= floor]
    if not np.isin(kept[:, :2], refs[is_core]).all():
        raise ValueError("a merge at this floor names a reference that is no core there")
    held = cut != _native.NO_CLUSTER
    return np.where(is_core | ~held, cut, refs), is_core


def tree_changes(old_merges, merges):
    """What a database update after ``cluster_tree_extend`` needs: ``(removed, added)``, uint32[r, 3] and
    uint32[s, 3] -- the records of ``old_merges`` that ``merges`` no longer holds and the records of ``merges``
    that ``old_merges`` did not hold, whole rows compared, each in the tree's order (height descending, then a,
    then b).  Needs no map and no GPU."""
    was, now = _records(old_merges, "old_merges"), _records(merges, "merges")
    # equal rows get one number: whole records are compared, the height included
    _, number = np.unique(np.concatenate([was, now]), axis=0, return_inverse=True)
    number = number.reshape(-1)
    gone = ~np.isin(number[:len(was)], number[len(was):])
    come = ~np.isin(number[len(was):], number[:len(was)])

    def ordered(rows):
        return rows[np.lexsort((rows[:, 1], rows[:, 0], 1000 - rows[:, 2].astype(np.int64)))]

    return ordered(was[gone]), ordered(now[come])


def tree_by_block(merges, references, blocks):
    """A ``cluster_tree_within`` result split by block, for the caller who stores a tree per block:
    ``{key: merges rows}``, uint32[k, 3] each, in the tree's order (the order the records come in).  Only keys with
    a record appear.  ValueError for a record whose ends carry two keys or name a reference that is not listed.
    Needs no map and no GPU."""
    rows = _records(merges, "merges")
    refs, keys = np.asarray(references, dtype=np.uint32), np.asarray(blocks, dtype=np.uint32)
    if refs.ndim != 1 or keys.shape != refs.shape:
        raise ValueError("references and blocks must be one-dimensional and of one length")
    if not len(rows):
        return {}
    listed, at = np.unique(refs, return_index=True)
    ends = np.searchsorted(listed, rows[:, :2])
    if len(listed) == 0 or (listed[np.minimum(ends, len(listed) - 1)] != rows[:, :2]).any():
        raise ValueError("a record names a reference that is not listed")
    key = keys[at][ends]
    if (key[:, 0] != key[:, 1]).any():
        raise ValueError("a record joins references under two keys")
    return {int(k): rows[key[:, 0] == k] for k in np.unique(key[:, 0]).tolist()}


def merge_edges(*record_lists):
    """Edge record lists, each in ``cluster_edges``' total order (permille descending, then a, then b), as one
    list in that order: uint32[E, 3].  How a caller keeps an edge list current:
    ``merge_edges(held, cluster_edges_extend(old, new, floor))``.  ValueError for a list that is not in order or
    for a record present twice, in one list or in two.  Needs no map and no GPU."""
    lists = [_records(rows, "edges") for rows in record_lists]
    for rows in lists:
        if len(rows) > 1:
            prev, nxt = rows[:-1], rows[1:]
            eq = lambda c: prev[:, c] == nxt[:, c]
            before = (prev[:, 2] > nxt[:, 2]) | (eq(2) & ((prev[:, 0] < nxt[:, 0]) | (eq(0) & (prev[:, 1] < nxt[:, 1]))))
            if not before.all():
                raise ValueError("a record list is not in order (permille descending, then a, then b), or holds "
                                 "a record twice")
    if not sum(len(rows) for rows in lists):
        return np.zeros((0, 3), dtype=np.uint32)
    rows = np.concatenate(lists)
    rows = np.ascontiguousarray(rows[np.lexsort((rows[:, 1], rows[:, 0], -rows[:, 2].astype(np.int64)))])
    if len(rows) > 1 and (rows[1:] == rows[:-1]).all(axis=1).any():
        raise ValueError("a record is present twice")
    return rows


def adjacency(edges, references):
    """``cluster_edges`` records (``cluster_edges_extend``'s and ``cluster_edges_between``'s too: of a left row's
    neighbours the first is its best link) as neighbour lists, what a caller's own graph code starts from:
    ``(row_off uint64[n + 1], neighbour uint32[2 E], permille uint32[2 E])``, one row per element of ``references``
    -- element i's neighbours are ``neighbour[row_off[i]:row_off[i + 1]]`` with their similarities beside them, in
    the records' order.  A repeated reference gets the same row each time it is listed (so the rows add up to more
    than 2 E then); one that no record names gets an empty row.  ValueError for a record that names a reference
    which is not listed.  Needs no map and no GPU."""
    rows = _records(edges, "edges")
    refs = np.asarray(references, dtype=np.uint32)
    if refs.ndim != 1:
        raise ValueError("references must be one-dimensional")
    listed = np.unique(refs)
    ends = np.searchsorted(listed, rows[:, :2])
    if len(rows) and (len(listed) == 0 or (listed[np.minimum(ends, len(listed) - 1)] != rows[:, :2]).any()):
        raise ValueError("a record names a reference that is not listed")
    # every record twice, once from each end, kept in the records' order per end
    src = np.concatenate([ends[:, 0], ends[:, 1]]) if len(rows) else np.zeros(0, dtype=np.int64)
    dst = np.concatenate([rows[:, 1], rows[:, 0]])
    sim = np.concatenate([rows[:, 2], rows[:, 2]])
    at = np.concatenate([np.arange(len(rows)), np.arange(len(rows))])
    order = np.lexsort((at, src))
    dst, sim = dst[order], sim[order]
    start = np.zeros(len(listed) + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=len(listed)), out=start[1:])
    if len(listed) == len(refs) and (listed == refs).all():    # (the list is its own numbering: nothing to gather)
        return start.astype(np.uint64), dst.astype(np.uint32), sim.astype(np.uint32)
    node = np.searchsorted(listed, refs)
    size = start[node + 1] - start[node]
    row_off = np.zeros(len(refs) + 1, dtype=np.int64)
    np.cumsum(size, out=row_off[1:])
    pick = np.repeat(start[node] - row_off[:-1], size) + np.arange(row_off[-1])
    return row_off.astype(np.uint64), dst[pick].astype(np.uint32), sim[pick].astype(np.uint32)


def merge_profile(merges, nodes=None):
    """What a caller slides the cut by: per distinct height of a ``cluster_tree`` result, highest first,
    ``{permille, merges, n_clusters}`` -- the merges at or above it and the clusters a cut there leaves among
    ``nodes`` references (default: the references the merges name, so singletons are left out).  (It counts
    records: for ``cluster_edges`` records, which are no forest, ``merges`` is the edges at or above each height
    and ``n_clusters`` means nothing.)"""
    merges = np.asarray(merges, dtype=np.uint32).reshape(-1, 3)
    if nodes is None:
        nodes = len(np.unique(merges[:, :2]))
    heights, counts = np.unique(merges[:, 2], return_counts=True)
    done = np.cumsum(counts[::-1])
    return [{"permille": int(h), "merges": int(k), "n_clusters": int(nodes) - int(k)}
            for h, k in zip(heights[::-1].tolist(), done.tolist())]
