"""The cluster surface of ``RawMap`` (no reference counterpart): the methods that call a ``blurrily_storage_cluster*``
entry, and the numpy conveniences over them.  ``RawMap`` inherits them; what they do with a result afterwards, without
a map, is in ``cluster_records.py``.

Every C-calling method reads as the methods of ``map.py`` do: check open, convert the arguments -- the scalars first,
in the order the tests pin --, call the C function by name, shape the result.
"""
import numpy as np

from . import _native
from ._marshal import (_byrefs, _check, _counters, _edge_count, _edge_records, _floors, _ints, _merged, _merges,
                       _permille, _ptr, _records, _refs, _refs_with_keys, _u32)
from .cluster_records import groups


class ClusterMethods:
    """Connected components of the similarity self-join and what was built on them.  A mixin: `_lib`, `_h` and
    `_check_open` are ``RawMap``'s."""

    def cluster(self, references, min_permille):
        """Single-linkage clusters of the stored references under "J >= min_permille / 1000" (blurrily_storage_cluster).
        Returns (labels[n] uint32: the smallest reference of each reference's component, ``_native.NO_CLUSTER`` for
        one the map does not hold; the number of components; the number of edges, each pair once)."""
        self._check_open()
        mp = _permille(min_permille)
        refs = _refs(references)
        n = len(refs)
        labels = np.zeros(n, dtype=np.uint32)
        counts = _counters(32, 64)                              # n_clusters, n_edges
        _check(self._lib.blurrily_storage_cluster(self._h, _ptr(refs), n, mp, _ptr(labels), *_byrefs(counts)))
        return (labels,) + _ints(counts)

    def cluster_levels(self, references, floors):
        """``cluster`` at several floors (strictly ascending, at most ``_native.CLUSTER_MAX_LEVELS``) from one sweep of
        the device (blurrily_storage_cluster_levels).  Returns (labels[K, n] uint32, n_clusters[K] int64, n_edges[K]
        int64): row k is what ``cluster(references, floors[k])`` returns."""
        self._check_open()
        fl = _floors(floors)
        refs = _refs(references)
        n, k = len(refs), len(fl)
        labels = np.zeros((k, n), dtype=np.uint32)
        n_clusters, n_edges = np.zeros(k, dtype=np.uint32), np.zeros(k, dtype=np.uint64)
        _check(self._lib.blurrily_storage_cluster_levels(self._h, _ptr(refs), n, fl.ctypes.data, k, _ptr(labels),
                                                         n_clusters.ctypes.data, n_edges.ctypes.data))
        return labels, n_clusters.astype(np.int64), n_edges.astype(np.int64)

    def cluster_profile(self, references, floors):
        """What a caller picks a floor by: per floor ``{floor, n_clusters, n_edges, largest, singletons}`` -- the
        components, the edges, the nodes of the largest component and the components of one node -- from one
        ``cluster_levels`` call and numpy over its labels."""
        floors = list(floors)
        refs = np.unique(_refs(references))                    # (a reference listed twice is one node)
        labels, n_clusters, n_edges = self.cluster_levels(refs, floors)
        profile = []
        for k, floor in enumerate(floors):
            _, sizes = np.unique(labels[k][labels[k] != _native.NO_CLUSTER], return_counts=True)
            profile.append({"floor": int(floor), "n_clusters": int(n_clusters[k]), "n_edges": int(n_edges[k]),
                            "largest": int(sizes.max()) if len(sizes) else 0, "singletons": int((sizes == 1).sum())})
        return profile

    def cluster_centres(self, references, min_permille, attached=True):
        """``cluster`` with what tells a tight group from a chain (blurrily_storage_cluster_centres).  Returns (labels[n],
        degrees[n] uint32: each reference's edges; centres[n] uint32: the reference with the most edges in its
        component, the smallest among equals, ``_native.NO_CLUSTER`` for one the map does not hold; attached[n] uint8:
        1 for a centre and for a reference that shares an edge with its centre -- None with ``attached=False``, which
        spares the device its second sweep; the number of components; the number of edges)."""
        self._check_open()
        mp = _permille(min_permille)
        refs = _refs(references)
        n = len(refs)
        labels, degrees, centres = (np.zeros(n, dtype=np.uint32) for _ in range(3))
        att = np.zeros(n, dtype=np.uint8) if attached else None
        counts = _counters(32, 64)                              # n_clusters, n_edges
        _check(self._lib.blurrily_storage_cluster_centres(self._h, _ptr(refs), n, mp, _ptr(labels), _ptr(degrees),
                                                          _ptr(centres), _ptr(att), *_byrefs(counts)))
        return (labels, degrees, centres, att) + _ints(counts)

    def cluster_shapes(self, references, min_permille):
        """The components of two or more references, ordered by label: ``{label, size, edges, centre, attached, star}``
        each -- its nodes, its edges, its centre, how many of its nodes are the centre or share an edge with it, and
        whether all do (a star: every member is directly similar to the centre; otherwise a chain to look at again).
        Numpy over one ``cluster_centres`` call."""
        refs = np.unique(_refs(references))                    # (a reference listed twice is one node)
        labels, degrees, centres, att, _, _ = self.cluster_centres(refs, min_permille)
        held = labels != _native.NO_CLUSTER
        labels, degrees, centres, att = labels[held], degrees[held], centres[held], att[held]
        uniq, first, which, sizes = np.unique(labels, return_index=True, return_inverse=True, return_counts=True)
        edges = np.bincount(which, weights=degrees.astype(np.float64), minlength=len(uniq)).astype(np.int64) // 2
        marked = np.bincount(which, weights=att.astype(np.float64), minlength=len(uniq)).astype(np.int64)
        return [{"label": int(uniq[k]), "size": int(sizes[k]), "edges": int(edges[k]), "centre": int(centres[first[k]]),
                 "attached": int(marked[k]), "star": bool(marked[k] == sizes[k])}
                for k in np.nonzero(sizes >= 2)[0].tolist()]

    # The four listings below end alike (``cluster_records.groups``) and differ in the list the library sees, which is
    # the n of its call: ``duplicates`` and ``duplicates_within`` hand the list with its repeats and drop them from
    # the labels afterwards, ``dense_duplicates`` drops them first, ``dense_duplicates_within`` hands the repeats (each
    # has its key) and drops them afterwards.
    def duplicates(self, references, min_permille):
        """The clusters of two or more references: a list of lists of references, each ascending, ordered by label."""
        refs = _refs(references)
        labels, _, _ = self.cluster(refs, min_permille)
        refs, at = np.unique(refs, return_index=True)
        labels = labels[at]
        return groups(refs, labels, labels != _native.NO_CLUSTER, 2)

    def cluster_cores(self, references, min_permille, min_degree):
        """Density-based clusters over ``cluster``'s edges (blurrily_storage_cluster_cores): a reference with at least
        ``min_degree`` edges is a core, only edges between cores unite, a reference that is no core joins the cluster
        of its core neighbour with the most edges (the smallest among equals) as a border, or is noise.  Returns
        (labels[n] uint32: the smallest core of the cluster, a noise reference itself, ``_native.NO_CLUSTER`` for one
        the map does not hold; degrees[n] uint32; kinds[n] uint8: ``_native.KIND_NONE``, ``KIND_NOISE``,
        ``KIND_BORDER``, ``KIND_CORE``; the number of clusters; the number of edges; the edges between cores)."""
        self._check_open()
        mp = _permille(min_permille)
        md = _u32(min_degree, "min_degree")
        refs = _refs(references)
        n = len(refs)
        labels, degrees = (np.zeros(n, dtype=np.uint32) for _ in range(2))
        kinds = np.zeros(n, dtype=np.uint8)
        counts = _counters(32, 64, 64)                          # n_clusters, n_edges, n_core_edges
        _check(self._lib.blurrily_storage_cluster_cores(self._h, _ptr(refs), n, mp, md, _ptr(labels), _ptr(degrees),
                                                        _ptr(kinds), *_byrefs(counts)))
        return (labels, degrees, kinds) + _ints(counts)

    def dense_duplicates(self, references, min_permille, min_degree):
        """The clusters of ``cluster_cores``: a list of lists of references, cores and borders, each ascending,
        ordered by label; noise is left out.  Numpy over one ``cluster_cores`` call."""
        refs = np.unique(_refs(references))                    # (a reference listed twice is one node)
        labels, _, kinds, _, _, _ = self.cluster_cores(refs, min_permille, min_degree)
        return groups(refs, labels, kinds >= _native.KIND_BORDER)

    def cluster_extend(self, old_refs, old_labels, new_refs, min_permille):
        """The clusters of ``old_refs`` and ``new_refs`` together, from the labels the caller holds for the old ones
        (blurrily_storage_cluster_extend): only the new references sweep the map, the old ones start from
        ``old_labels``.  With ``old_labels`` from ``cluster(old_refs, min_permille)`` on the map as it is now and the
        lists disjoint, the result is ``cluster``'s over both lists; a group that lost a member to a delete is
        re-clustered on its own first (``cluster`` over its remaining members).  Returns (labels_old[n_old] uint32,
        labels_new[n_new] uint32, the number of components, the number of edges with a new end, each once)."""
        self._check_open()
        mp = _permille(min_permille)
        old, new = _refs(old_refs), _refs(new_refs)
        seeds = _refs(old_labels)
        if len(seeds) != len(old):
            raise ValueError(f"{len(seeds)} old labels for {len(old)} old references")
        labels_old, labels_new = np.zeros(len(old), dtype=np.uint32), np.zeros(len(new), dtype=np.uint32)
        counts = _counters(32, 64)                              # n_clusters, n_edges
        _check(self._lib.blurrily_storage_cluster_extend(self._h, _ptr(old), _ptr(seeds), len(old), _ptr(new), len(new),
                                                         mp, _ptr(labels_old), _ptr(labels_new), *_byrefs(counts)))
        return (labels_old, labels_new) + _ints(counts)

    def cluster_changes(self, old_refs, old_labels, labels_old):
        """What a database update after ``cluster_extend`` or ``cluster_extend_within`` needs: (the old references
        whose label moved, their new labels), in the list's order.  Numpy only."""
        old, was, now = _refs(old_refs), _refs(old_labels), _refs(labels_old)
        if not len(old) == len(was) == len(now):
            raise ValueError("old_refs, old_labels and labels_old differ in length")
        moved = was != now
        return old[moved], now[moved]

    def cluster_within(self, references, blocks, min_permille):
        """``cluster`` within blocks (blurrily_storage_cluster_within): ``blocks[i]`` is a 32-bit key for
        ``references[i]``, and only references under one key are ever joined.  One call serves all blocks.  Returns
        (labels[n] uint32, the number of components over all blocks, the number of within-block edges): what one
        ``cluster`` call per block gives, the counts summed."""
        self._check_open()
        mp = _permille(min_permille)
        refs, keys = _refs_with_keys(references, blocks)
        n = len(refs)
        labels = np.zeros(n, dtype=np.uint32)
        counts = _counters(32, 64)                              # n_clusters, n_edges
        _check(self._lib.blurrily_storage_cluster_within(self._h, _ptr(refs), _ptr(keys), n, mp, _ptr(labels),
                                                         *_byrefs(counts)))
        return (labels,) + _ints(counts)

    def cluster_extend_within(self, old_refs, old_blocks, old_labels, new_refs, new_blocks, min_permille):
        """``cluster_extend`` within blocks (blurrily_storage_cluster_extend_within): ``old_blocks[i]`` is a 32-bit key
        for ``old_refs[i]``, ``new_blocks[j]`` for ``new_refs[j]``; a seed and an edge need both ends under one key,
        and only the new references of a block are scored against it.  With ``old_labels`` from
        ``cluster_within(old_refs, old_blocks, min_permille)`` on the map as it is now and the lists disjoint, the
        result is ``cluster_within``'s over both lists with the keys concatenated; a group that lost a member to a
        delete is re-clustered on its own first (``cluster_within`` over its remaining members).  Returns
        (labels_old[n_old] uint32, labels_new[n_new] uint32, the number of components, the number of within-block
        edges with a new end, each once).  ``cluster_changes`` serves the result as it is."""
        self._check_open()
        mp = _permille(min_permille)
        old, old_keys = _refs_with_keys(old_refs, old_blocks)
        new, new_keys = _refs_with_keys(new_refs, new_blocks)
        seeds = _refs(old_labels)
        if len(seeds) != len(old):
            raise ValueError(f"{len(seeds)} old labels for {len(old)} old references")
        labels_old, labels_new = np.zeros(len(old), dtype=np.uint32), np.zeros(len(new), dtype=np.uint32)
        counts = _counters(32, 64)                              # n_clusters, n_edges
        _check(self._lib.blurrily_storage_cluster_extend_within(self._h, _ptr(old), _ptr(old_keys), _ptr(seeds), len(old),
                                                                _ptr(new), _ptr(new_keys), len(new), mp,
                                                                _ptr(labels_old), _ptr(labels_new), *_byrefs(counts)))
        return (labels_old, labels_new) + _ints(counts)

    def duplicates_within(self, references, blocks, min_permille):
        """The within-block clusters of two or more references, as ``duplicates`` gives them: a list of lists of
        references, each ascending, ordered by label."""
        refs = _refs(references)
        labels, _, _ = self.cluster_within(refs, blocks, min_permille)
        refs, at = np.unique(refs, return_index=True)
        labels = labels[at]
        return groups(refs, labels, labels != _native.NO_CLUSTER, 2)

    def cluster_cores_within(self, references, blocks, min_permille, min_degree):
        """``cluster_cores`` within blocks (blurrily_storage_cluster_cores_within): ``blocks[i]`` is a 32-bit key for
        ``references[i]``, an edge needs both ends under one key, and a degree counts those edges only, so a core, a
        border's anchor and a cluster never reach across a key.  One call serves all blocks.  Returns (labels[n]
        uint32, degrees[n] uint32, kinds[n] uint8, the number of clusters, the number of within-block edges, the edges
        between cores) as ``cluster_cores`` gives them: what one ``cluster_cores`` call per block gives, put back in
        place, the counts summed."""
        self._check_open()
        mp = _permille(min_permille)
        md = _u32(min_degree, "min_degree")
        refs, keys = _refs_with_keys(references, blocks)
        n = len(refs)
        labels, degrees = (np.zeros(n, dtype=np.uint32) for _ in range(2))
        kinds = np.zeros(n, dtype=np.uint8)
        counts = _counters(32, 64, 64)                          # n_clusters, n_edges, n_core_edges
        _check(self._lib.blurrily_storage_cluster_cores_within(self._h, _ptr(refs), _ptr(keys), n, mp, md, _ptr(labels),
                                                               _ptr(degrees), _ptr(kinds), *_byrefs(counts)))
        return (labels, degrees, kinds) + _ints(counts)

    def dense_duplicates_within(self, references, blocks, min_permille, min_degree):
        """The clusters of ``cluster_cores_within``, as ``dense_duplicates`` gives them: a list of lists of references,
        cores and borders, each ascending, ordered by label; noise is left out.  Numpy over one call."""
        refs = _refs(references)
        labels, _, kinds, _, _, _ = self.cluster_cores_within(refs, blocks, min_permille, min_degree)
        refs, at = np.unique(refs, return_index=True)           # (a reference listed twice is one node)
        return groups(refs, labels[at], kinds[at] >= _native.KIND_BORDER)

    def cluster_tree(self, references, min_permille):
        """The single-linkage dendrogram of ``cluster`` at per-mille resolution (blurrily_storage_cluster_tree): the
        maximum spanning forest of the edges at or above ``min_permille``, an edge's height being its similarity in
        whole per mille, rounded down.  Returns (labels[n] uint32, n_clusters and n_edges as ``cluster`` gives them at
        ``min_permille``, and between them merges[k, 3] uint32: rows ``[a, b, permille]`` with a < b, sorted by height
        descending, then a, then b; k is the nodes minus the components) as ``(labels, merges, n_clusters, n_edges)``.
        ``cut_tree`` gives the labels at any higher floor without another call."""
        self._check_open()
        mp = _permille(min_permille)
        refs = _refs(references)
        n = len(refs)
        labels = np.zeros(n, dtype=np.uint32)
        merges, counts = _merges(n), _counters(32, 32, 64)      # (counts: n_merges, n_clusters, n_edges)
        _check(self._lib.blurrily_storage_cluster_tree(self._h, _ptr(refs), n, mp, _ptr(labels), _ptr(merges),
                                                       *_byrefs(counts)))
        return (labels,) + _merged(merges, counts)

    def cluster_tree_extend(self, old_refs, old_merges, new_refs, min_permille):
        """The tree of ``old_refs`` and ``new_refs`` together, from the records the caller holds for the old ones
        (blurrily_storage_cluster_tree_extend): only the new references sweep the map, the old ones are spoken for by
        ``old_merges``.  With ``old_merges`` from ``cluster_tree(old_refs, f)`` for some ``f <= min_permille`` on old
        rows unchanged since, the lists disjoint and every reference held, the result is ``cluster_tree``'s over both
        lists at ``min_permille``; a component that lost a member to a delete is re-treed on its own first.  Returns
        ``(labels_old, labels_new, merges, n_clusters, n_edges)``: merges[k, 3] uint32 as ``cluster_tree`` gives them,
        n_edges the edges with a new end, each once.  ``cut_tree`` and ``merge_profile`` take the records as they
        are; ``tree_changes`` tells which of the caller's to delete and to insert."""
        self._check_open()
        mp = _permille(min_permille)
        old, new = _refs(old_refs), _refs(new_refs)
        records = _records(old_merges, "old_merges")
        if len(records) > len(old):
            raise ValueError(f"{len(records)} old records for {len(old)} old references: a forest has fewer")
        if len(records) and ((records[:, 0] >= records[:, 1]).any() or (records[:, 2] > 1000).any()):
            raise ValueError("an old record needs a < b and permille <= 1000")
        labels_old, labels_new = np.zeros(len(old), dtype=np.uint32), np.zeros(len(new), dtype=np.uint32)
        merges, counts = _merges(len(old) + len(new)), _counters(32, 32, 64)   # (n_merges, n_clusters, n_edges)
        _check(self._lib.blurrily_storage_cluster_tree_extend(self._h, _ptr(old), len(old), _ptr(records), len(records),
                                                              _ptr(new), len(new), mp, _ptr(labels_old),
                                                              _ptr(labels_new), _ptr(merges), *_byrefs(counts)))
        return (labels_old, labels_new) + _merged(merges, counts)

    def cluster_core_tree(self, references, min_permille, min_degree):
        """The dendrogram of ``cluster_cores``' cores at every floor from ``min_permille`` up
        (blurrily_storage_cluster_core_tree).  A node's core height is the ``min_degree``-th largest height among its
        edges, and an edge between two nodes that have one joins them at the least of its own height and theirs.
        Returns ``(labels, core_permille, merges, n_clusters, n_edges, n_core_edges)``: labels[n] and core_permille[n]
        uint32 (``_native.NO_CORE`` for a reference the map does not hold or a node of fewer than ``min_degree`` edges),
        merges[k, 3] uint32 rows ``[a, b, permille]`` as ``cluster_tree`` gives them, and ``cluster_cores``' three
        counts at ``(min_permille, min_degree)``.  ``cut_core_tree`` gives the cores and their labels at any higher
        floor without another call."""
        self._check_open()
        mp = _permille(min_permille)
        md = _u32(min_degree, "min_degree")
        refs = _refs(references)
        n = len(refs)
        labels, core_permille = (np.zeros(n, dtype=np.uint32) for _ in range(2))
        merges, counts = _merges(n), _counters(32, 32, 64, 64)  # (n_merges, n_clusters, n_edges, n_core_edges)
        _check(self._lib.blurrily_storage_cluster_core_tree(self._h, _ptr(refs), n, mp, md, _ptr(labels),
                                                            _ptr(core_permille), _ptr(merges), *_byrefs(counts)))
        return (labels, core_permille) + _merged(merges, counts)

    def cluster_tree_within(self, references, blocks, min_permille):
        """``cluster_tree`` within blocks (blurrily_storage_cluster_tree_within): ``blocks[i]`` is a 32-bit key for
        ``references[i]``, and only references under one key are ever joined.  One call serves all blocks.  Returns
        ``(labels, merges, n_clusters, n_edges)``: labels[n] uint32, n_clusters and n_edges as ``cluster_within`` gives
        them at ``min_permille``, and merges[k, 3] uint32 as ``cluster_tree`` gives them -- what one ``cluster_tree``
        call per block gives, the records merged into one list in the tree's order.  ``cut_tree`` gives
        ``cluster_within``'s labels at any higher floor without another call, ``merge_profile`` takes the records as
        they are, and ``tree_by_block`` splits them by key."""
        self._check_open()
        mp = _permille(min_permille)
        refs, keys = _refs_with_keys(references, blocks)
        n = len(refs)
        labels = np.zeros(n, dtype=np.uint32)
        merges, counts = _merges(n), _counters(32, 32, 64)      # (counts: n_merges, n_clusters, n_edges)
        _check(self._lib.blurrily_storage_cluster_tree_within(self._h, _ptr(refs), _ptr(keys), n, mp, _ptr(labels),
                                                              _ptr(merges), *_byrefs(counts)))
        return (labels,) + _merged(merges, counts)

    def cluster_core_tree_within(self, references, blocks, min_permille, min_degree):
        """``cluster_core_tree`` within blocks (blurrily_storage_cluster_core_tree_within): ``blocks[i]`` is a 32-bit key
        for ``references[i]``, an edge needs both ends under one key, and a core height ranks those edges only, so no
        record joins two keys.  One call serves all blocks.  Returns ``(labels, core_permille, merges, n_clusters,
        n_edges, n_core_edges)`` as ``cluster_core_tree`` gives them, the counts being ``cluster_cores_within``'s at
        ``(min_permille, min_degree)`` -- what one ``cluster_core_tree`` call per block gives, the records merged into
        one list in the tree's order.  ``cut_core_tree`` gives ``cluster_cores_within``'s cores and their labels at any
        higher floor without another call, ``merge_profile`` takes the records as they are, and ``tree_by_block``
        splits them by key."""
        self._check_open()
        mp = _permille(min_permille)
        md = _u32(min_degree, "min_degree")
        refs, keys = _refs_with_keys(references, blocks)
        n = len(refs)
        labels, core_permille = (np.zeros(n, dtype=np.uint32) for _ in range(2))
        merges, counts = _merges(n), _counters(32, 32, 64, 64)  # (n_merges, n_clusters, n_edges, n_core_edges)
        _check(self._lib.blurrily_storage_cluster_core_tree_within(self._h, _ptr(refs), _ptr(keys), n, mp, md,
                                                                   _ptr(labels), _ptr(core_permille), _ptr(merges),
                                                                   *_byrefs(counts)))
        return (labels, core_permille) + _merged(merges, counts)

    def _cluster_edges_call(self, references, min_permille, blocks):
        """What the two edge methods share: ``(call(rows, cap, n_edges), n)`` for the unblocked symbol
        (``blocks`` None) or the blocked one."""
        self._check_open()
        mp = _permille(min_permille)
        if blocks is None:
            refs = _refs(references)
            return (lambda rows, cap, n_edges: self._lib.blurrily_storage_cluster_edges(
                self._h, _ptr(refs), len(refs), mp, rows, cap, n_edges)), len(refs)
        refs, keys = _refs_with_keys(references, blocks)
        return (lambda rows, cap, n_edges: self._lib.blurrily_storage_cluster_edges_within(
            self._h, _ptr(refs), _ptr(keys), len(refs), mp, rows, cap, n_edges)), len(refs)

    def cluster_edges(self, references, min_permille, blocks=None, capacity=None):
        """The edges of ``cluster``'s graph themselves (blurrily_storage_cluster_edges), or with ``blocks`` of
        ``cluster_within``'s (blurrily_storage_cluster_edges_within): edges[E, 3] uint32, one row ``[a, b, permille]``
        per pair of listed references at or above ``min_permille``, a < b, permille the similarity in whole per mille
        rounded down, sorted as ``cluster_tree``'s merges are (height descending, then a, then b).  E is ``cluster``'s
        n_edges.  The first call has room for ``capacity`` records (default ``max(1024, 8 n)``); if there are more, one
        more call is made with the room the first reported.  OSError EOVERFLOW when the edges outnumber option
        "cluster_edges_max": raise the floor, block or split the list.  ``tree_by_block``, ``cut_tree`` (with
        ``cluster``'s labels) and ``merge_profile`` take the records as they are; ``adjacency`` turns them into
        neighbour lists."""
        call, n = self._cluster_edges_call(references, min_permille, blocks)
        return _edge_records(call, n, capacity)

    def cluster_edge_count(self, references, min_permille, blocks=None):
        """How many records ``cluster_edges`` would return, without sorting or fetching them: no buffer is handed."""
        call, _ = self._cluster_edges_call(references, min_permille, blocks)
        return _edge_count(call)

    def _cluster_edges_two_call(self, symbol, first, second, min_permille):
        """What the extend and between methods share: ``(call(rows, cap, n_edges), n)`` over two lists."""
        self._check_open()
        mp = _permille(min_permille)
        one, two = _refs(first), _refs(second)
        fn = getattr(self._lib, symbol)
        return (lambda rows, cap, n_edges: fn(self._h, _ptr(one), len(one), _ptr(two), len(two), mp, rows, cap,
                                              n_edges)), len(one) + len(two)

    def cluster_edges_extend(self, old_refs, new_refs, min_permille, capacity=None):
        """The ``cluster_edges`` records over both lists that have at least one end in ``new_refs``, each once
        (blurrily_storage_cluster_edges_extend): only the new references sweep the map.  A reference both lists name
        is new.  ``merge_edges(cluster_edges(old minus new), this)`` is ``cluster_edges(old and new)`` byte for byte:
        how an edge list is kept current after a put.  E is ``cluster_extend``'s n_edges.  Records, order, ``capacity``
        and EOVERFLOW are ``cluster_edges``'; ``adjacency``, ``cut_tree`` and ``merge_profile`` take the records as
        they are."""
        call, n = self._cluster_edges_two_call("blurrily_storage_cluster_edges_extend", old_refs, new_refs, min_permille)
        return _edge_records(call, n, capacity)

    def cluster_edge_count_extend(self, old_refs, new_refs, min_permille):
        """How many records ``cluster_edges_extend`` would return: no buffer is handed, nothing is sorted."""
        call, _ = self._cluster_edges_two_call("blurrily_storage_cluster_edges_extend", old_refs, new_refs, min_permille)
        return _edge_count(call)

    def cluster_edges_between(self, left, right, min_permille, capacity=None):
        """Record linkage: the ``cluster_edges`` records with exactly one end in ``left`` and one in ``right``
        (blurrily_storage_cluster_edges_between).  A reference both lists name is on the right only.  The side with
        fewer distinct references sweeps the map, whichever way round the lists are given, and for disjoint lists
        both ways round give identical bytes.  ``cluster_edges_extend(l, r)`` is this merged with ``cluster_edges(r)``.
        Records, order, ``capacity`` and EOVERFLOW are ``cluster_edges``'.  ``adjacency(records, left + right)`` takes
        them as they are: a left row's first neighbour is its best link (the records come best first); ``cut_tree``
        and ``merge_profile`` take them too."""
        call, n = self._cluster_edges_two_call("blurrily_storage_cluster_edges_between", left, right, min_permille)
        return _edge_records(call, n, capacity)

    def cluster_edge_count_between(self, left, right, min_permille):
        """How many records ``cluster_edges_between`` would return: no buffer is handed, nothing is sorted."""
        call, _ = self._cluster_edges_two_call("blurrily_storage_cluster_edges_between", left, right, min_permille)
        return _edge_count(call)
