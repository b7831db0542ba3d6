"""Cluster-cores figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings):

  * against the workaround on section 17's short list (a prefix of the references less those whose rows reach the
    limit): chunks through find_batch_by_reference_similar at limit 65 535, the rows among the listed references turned
    into degrees, cores, labels and kinds by numpy under the rules of the call -- host clock around each path, two
    timed runs after a warm one, both kept (their spread is the margin of the comparison); all outputs must be equal;
  * the whole map (every reference listed) at 900 and 700 per mille, min_degree 3: seconds of
    blurrily_storage_cluster_centres without `attached` and of this call (two timed runs each after one warm call per
    floor), their ratio, the clusters, cores, borders and noise nodes, and the largest cluster beside the largest
    component of the centres call's labels.  A floor is started only while the probe's time budget lasts, and says so
    when it is left out.

Writes the JSON object to --out after every step (a step that runs out of time leaves the ones before it).
Usage: python tools/cluster_cores_probe.py [--scale 1.0] [--prefix 20000 (0: no workaround)] [--floors 900,700]
       [--min-degree 3] [--budget 900] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import workloads as W  # noqa: E402
from cluster_probe import CHUNK, components, timed  # noqa: E402

NOISE, BORDER, CORE = 1, 2, 3


def dbscan(k, a, b, min_degree):
    """(label, degree, kind) per node of the list from its edges, every edge given twice (a[i] -> b[i] and back)."""
    degree = np.bincount(a, minlength=k)
    core = degree >= min_degree
    cc = core[a] & core[b]
    label = components(k, a[cc], b[cc])                       # (a node without a core-core edge: itself)
    to_core = ~core[a] & core[b]
    x, c = a[to_core], b[to_core]
    best = np.zeros(k, dtype=np.int64)
    np.maximum.at(best, x, degree[c] * (k + 1) + (k - c))    # the highest degree, the lowest index among equals
    border = ~core & (best > 0)
    label[border] = label[k - best[border] % (k + 1)]
    kind = np.full(k, NOISE, dtype=np.uint8)
    kind[border] = BORDER
    kind[core] = CORE
    return label, degree, kind, int(cc.sum()) // 2


def largest(labels, member):
    _, sizes = np.unique(labels[member], return_counts=True)
    return int(sizes.max()) if len(sizes) else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--prefix", type=int, default=20000)
    ap.add_argument("--budget", type=float, default=900.0)
    ap.add_argument("--floors", default="900,700")
    ap.add_argument("--min-degree", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_cores_geonames.json"))
    args = ap.parse_args()
    start = time.perf_counter()
    md = args.min_degree
    res = {"haystack": "configs[2] geonames", "scale": args.scale, "min_degree": md}

    def dump():
        W.dump_json(res, args.out)

    m, hay, off, refs, put_s, sync_s = W.bench_map("geonames", args.scale)
    n = len(refs)
    res["references"] = n
    res["build_s"] = round(put_s + sync_s, 2)
    t0 = time.perf_counter()
    m.cluster_cores(refs[:1], 500, md)                        # the first call builds the per-rank table
    res["first_call_s"] = round(time.perf_counter() - t0, 4)
    dump()

    # section 17's short list: a prefix less the references whose rows over the whole map reach the limit at 500
    k = min(args.prefix, n)
    listed = refs[:k]
    if k:
        full = np.concatenate([m.find_batch_by_reference_similar(listed[s:s + CHUNK], 65535, 500)[1]
                               for s in range(0, k, CHUNK)])
        listed = listed[full < 65535]
        res["workaround_list"] = {"prefix": k, "left_out_for_their_rows": int(k - len(listed))}
        k = len(listed)
    node_of = np.full(n + 2, -1, dtype=np.int64)              # reference -> index in the list
    node_of[listed] = np.arange(k)
    for mp in ((700, 500) if k else ()):
        most = [0]

        def workaround():
            ea, eb = [], []
            for s in range(0, k, CHUNK):
                part = listed[s:s + CHUNK]
                rows, counts, _, _ = m.find_batch_by_reference_similar(part, 65535, mp)
                most[0] = max(most[0], int(counts.max()))
                live = np.arange(rows.shape[1])[None, :] < counts[:, None]
                other = node_of[rows[:, :, 0][live]]
                own = np.repeat(np.arange(s, s + len(part)), counts)
                keep = (other >= 0) & (other != own)          # the listed ones among the rows
                ea.append(own[keep])
                eb.append(other[keep])
            a, b = np.concatenate(ea), np.concatenate(eb)     # (every edge twice, once from each end)
            return dbscan(k, a, b, md) + (len(a) // 2,)

        ts_w, (w_label, w_degree, w_kind, w_core_edges, w_edges) = timed(workaround)
        ts_c, (labels, degrees, kinds, n_clusters, n_edges, n_core_edges) = timed(lambda: m.cluster_cores(listed, mp, md))
        ts_p, _ = timed(lambda: m.cluster_centres(listed, mp, attached=False))
        assert most[0] < 65535, "a node's rows were cut: take a smaller prefix"
        res[f"workaround_{mp}"] = {
            "references": k, "most_rows_of_a_node": most[0], "workaround_s": [round(t, 4) for t in ts_w],
            "cores_s": [round(t, 4) for t in ts_c], "centres_without_attached_s": [round(t, 4) for t in ts_p],
            "ratio_best": round(min(ts_w) / min(ts_c), 2),
            "cores_worst_over_workaround_best": round(max(ts_c) / min(ts_w), 4),
            "labels_equal": bool(np.array_equal(labels, listed[w_label])),
            "degrees_equal": bool(np.array_equal(degrees, w_degree)),
            "kinds_equal": bool(np.array_equal(kinds, w_kind)),
            "edges_equal": bool(w_edges == n_edges), "core_edges_equal": bool(w_core_edges == n_core_edges),
            "n_clusters": n_clusters, "n_edges": n_edges, "n_core_edges": n_core_edges,
            "cores_borders_noise": [int((kinds == x).sum()) for x in (CORE, BORDER, NOISE)]}
        dump()

    for mp in [int(f) for f in args.floors.split(",") if f]:
        if time.perf_counter() - start > args.budget:
            res[f"whole_map_{mp}"] = {"left_out": f"the probe's budget of {args.budget:.0f} s was spent before this floor"}
            dump()
            continue
        out = {}
        res[f"whole_map_{mp}"] = out

        def two(fn):
            ts = []
            for _ in range(2):
                t0 = time.perf_counter()
                got = fn()
                ts.append(round(time.perf_counter() - t0, 3))
            return ts, got

        m.cluster_centres(refs, mp, attached=False)           # the floor's warm call
        out["centres_without_attached_s"], base = two(lambda: m.cluster_centres(refs, mp, attached=False))
        dump()
        m.cluster_cores(refs, mp, md)
        out["cores_s"], full = two(lambda: m.cluster_cores(refs, mp, md))
        labels, degrees, kinds, n_clusters, n_edges, n_core_edges = full
        out.update({
            "last_kernels": m.last_kernels(),
            "cores_over_centres": round(min(out["cores_s"]) / min(out["centres_without_attached_s"]), 3),
            "n_clusters": n_clusters, "n_edges": n_edges, "n_core_edges": n_core_edges,
            "edges_and_degrees_equal_the_centres_call": bool(n_edges == base[5] and degrees.tobytes() == base[1].tobytes()),
            "degrees_sum_is_twice_the_edges": bool(int(degrees.sum(dtype=np.uint64)) == 2 * n_edges),
            "cores_borders_noise": [int((kinds == x).sum()) for x in (CORE, BORDER, NOISE)],
            "noise_with_an_edge": int(((kinds == NOISE) & (degrees > 0)).sum()),
            "largest_cluster": largest(labels, kinds >= BORDER),
            "largest_component": largest(base[0], np.ones(len(refs), dtype=bool)), "components": base[4]})
        dump()


if __name__ == "__main__":
    main()
