"""The truth tests/test_gpu_cluster_tree.py compares blurrily_storage_cluster_tree with, on the host from
cluster_truth.Truth.pairs alone (every pair of listed, held references with its m): each pair's height
floor(1000 m / (T + R - m)), the pairs at or above the floor as edges, and the maximum spanning forest under the total
order (height descending, lower reference ascending, higher reference ascending) made twice over: by Kruskal's
algorithm, whose accepted edges in the order they are taken ARE the expected records, and by a synchronous Boruvka
(every component picks the best edge leaving it, all picked edges are united, again), which also tells how many
rounds merge something.  Nothing of the library under test is used."""
import numpy as np

BITS = 27
MASK = (1 << BITS) - 1


def edges(truth, listed, floor, least=None):
    """(lo, hi, h) of every edge at `floor`: indices into truth.refs with lo < hi, heights in whole per mille.  `least`
    (default: the floor) is the floor the truth's pairs are asked at, so that several floors share one list of pairs."""
    _, a, b, m = truth.pairs(listed, floor if least is None else least)
    a, b, m = a.astype(np.int64), b.astype(np.int64), m.astype(np.int64)
    union = truth.R[a].astype(np.int64) + truth.R[b] - m
    h = 1000 * m // union
    keep = h >= floor                                         # (h >= f exactly when 1000 m >= f (T + R - m))
    assert np.array_equal(keep, 1000 * m >= floor * union)
    return b[keep], a[keep], h[keep]                          # (pairs() gives a > b)


def nodes_of(truth, listed):
    return np.nonzero(np.isin(truth.refs, np.asarray(listed, dtype=np.int64)) & (truth.R > 0))[0]


def kruskal(truth, listed, floor, least=None):
    """The expected records: uint32 [k, 3] rows (a, b, permille) as references, in the total order."""
    lo, hi, h = edges(truth, listed, floor, least)
    assert len(truth.refs) <= MASK                            # the total order as one word, ascending: sorted in one pass
    key = ((1000 - h).astype(np.uint64) << np.uint64(2 * BITS)) | (lo.astype(np.uint64) << np.uint64(BITS)) | hi.astype(np.uint64)
    key.sort()
    lo = ((key >> np.uint64(BITS)) & np.uint64(MASK)).astype(np.int64)
    hi = (key & np.uint64(MASK)).astype(np.int64)
    h = 1000 - (key >> np.uint64(2 * BITS)).astype(np.int64)
    parent = list(range(len(truth.refs)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    out = []
    at, step = 0, 4096
    while at < len(lo):                                       # in growing runs: the edges whose ends were together when the
        root = np.array([find(x) for x in range(len(parent))], dtype=np.int64)   # run began are dropped without a loop
        l, g, ht = lo[at:at + step], hi[at:at + step], h[at:at + step]
        apart = root[l] != root[g]
        for el, eg, eh in zip(l[apart].tolist(), g[apart].tolist(), ht[apart].tolist()):
            rl, rg = find(el), find(eg)
            if rl != rg:
                parent[max(rl, rg)] = min(rl, rg)
                out.append((int(truth.refs[el]), int(truth.refs[eg]), eh))
        at, step = at + step, step * 2
    return np.array(out, dtype=np.uint32).reshape(-1, 3)


def boruvka(truth, listed, floor, least=None):
    """(the forest's edges as a set of (a, b, permille) in references, the rounds that merged something)."""
    lo, hi, h = edges(truth, listed, floor, least)
    assert len(truth.refs) <= MASK
    key = (h.astype(np.uint64) << np.uint64(2 * BITS)) | ((MASK - lo).astype(np.uint64) << np.uint64(BITS)) | \
        (MASK - hi).astype(np.uint64)
    comp = np.arange(len(truth.refs), dtype=np.int64)
    chosen, rounds = set(), 0
    while True:
        out = comp[lo] != comp[hi]
        lo, hi, key = lo[out], hi[out], key[out]              # (an edge inside a component stays inside)
        if len(lo) == 0:
            break
        best = np.zeros(len(comp), dtype=np.uint64)
        np.maximum.at(best, comp[lo], key)
        np.maximum.at(best, comp[hi], key)
        picked = np.unique(best[best != 0])
        pl = MASK - ((picked >> np.uint64(BITS)) & np.uint64(MASK)).astype(np.int64)
        ph = MASK - (picked & np.uint64(MASK)).astype(np.int64)
        pk = (picked >> np.uint64(2 * BITS)).astype(np.int64)
        before = len(chosen)
        chosen.update(zip(truth.refs[pl].tolist(), truth.refs[ph].tolist(), pk.tolist()))
        assert len(chosen) == before + len(picked)            # (an edge is picked in one round only)
        rounds += 1
        parent = list(range(len(comp)))                       # the picked edges united, component by component

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for cl, ch in zip(comp[pl].tolist(), comp[ph].tolist()):
            rl, rh = find(cl), find(ch)
            assert rl != rh                                   # (the picked edges of a round form no cycle)
            parent[max(rl, rh)] = min(rl, rh)
        comp = np.array([find(x) for x in range(len(comp))], dtype=np.int64)[comp]
    return chosen, rounds


def boruvka_rounds(truth, listed, floor, least=None):
    """boruvka() that also tells which edge was picked in which round and what the components were after each:
    ({(a, b, permille) in references: round, counted from 1}, the rounds that merged something, [after round k, k = 1 ..:
    every index's component as an index into truth.refs, the lowest of the component])."""
    lo, hi, h = edges(truth, listed, floor, least)
    assert len(truth.refs) <= MASK
    key = (h.astype(np.uint64) << np.uint64(2 * BITS)) | ((MASK - lo).astype(np.uint64) << np.uint64(BITS)) | \
        (MASK - hi).astype(np.uint64)
    comp = np.arange(len(truth.refs), dtype=np.int64)
    picked_in, after = {}, []
    while True:
        out = comp[lo] != comp[hi]
        lo, hi, key = lo[out], hi[out], key[out]
        if len(lo) == 0:
            break
        best = np.zeros(len(comp), dtype=np.uint64)
        np.maximum.at(best, comp[lo], key)
        np.maximum.at(best, comp[hi], key)
        picked = np.unique(best[best != 0])
        pl = MASK - ((picked >> np.uint64(BITS)) & np.uint64(MASK)).astype(np.int64)
        ph = MASK - (picked & np.uint64(MASK)).astype(np.int64)
        pk = (picked >> np.uint64(2 * BITS)).astype(np.int64)
        for e in zip(truth.refs[pl].tolist(), truth.refs[ph].tolist(), pk.tolist()):
            assert e not in picked_in                         # (an edge is picked in one round only)
            picked_in[e] = len(after) + 1
        low = comp.copy()                                     # the picked edges united: the lowest index spreads
        while True:
            nxt = low.copy()
            m = np.minimum(low[comp[pl]], low[comp[ph]])
            np.minimum.at(nxt, comp[pl], m)
            np.minimum.at(nxt, comp[ph], m)
            nxt = nxt[nxt]
            if np.array_equal(nxt, low):
                break
            low = nxt
        comp = low[comp]
        after.append(comp.copy())
    return picked_in, len(after), after


def cut(records, listed_labels, listed, floor):
    """The labels of `listed` after uniting the records with permille >= floor, by a plain union-find (the check of
    RawMap.cut_tree that shares no code with it).  listed_labels tell which references are held."""
    held = sorted({int(r) for r, l in zip(listed, listed_labels) if int(l) != 0xFFFFFFFF})
    parent = {r: r for r in held}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, p in np.asarray(records).reshape(-1, 3).tolist():
        if p >= floor:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(int(r)) if int(r) in parent else 0xFFFFFFFF for r in listed], dtype=np.uint32)
