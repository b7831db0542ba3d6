"""Clustering figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings):

  * against the workaround on a prefix of the references (less those whose rows reach the limit: listed for neither
    path): chunks through find_batch_by_reference_similar at limit 65 535 (no node may reach that many rows:
    asserted), the rows among the listed references joined by a numpy
    lowest-label propagation -- host clock around each path, two timed runs after a warm one, both kept (their spread
    is the margin of the comparison); the labels of both must be equal;
  * the whole map (every reference listed) at 900, 700 and 500 per mille: seconds (best of two after a warm call),
    components, edges and the largest component.  A floor is started only while the probe's time budget lasts, and
    says so when it is left out.

Writes the JSON object to --out after every step (a step that runs out of time leaves the ones before it).
Usage: python tools/cluster_probe.py [--scale 1.0] [--prefix 20000 (0: no workaround)] [--floors 900,700,500]
       [--budget 900] [--out FILE]"""
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

CHUNK = 2000                                                 # needles per workaround call: 65 535 rows of room each


def timed(fn, reps=2):
    """(host-clock seconds of `reps` calls after a warm one, the last call's result)."""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return ts, out


def components(n, a, b):
    """Lowest-index label of each of n nodes under the edges (a[i], b[i])."""
    label = np.arange(n, dtype=np.int64)
    while True:
        low = np.minimum(label[a], label[b])
        nxt = label.copy()
        np.minimum.at(nxt, a, low)
        np.minimum.at(nxt, b, low)
        nxt = nxt[nxt]
        if np.array_equal(nxt, label):
            return label
        label = nxt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--prefix", type=int, default=20000)
    ap.add_argument("--budget", type=float, default=900.0)
    ap.add_argument("--floors", default="900,700,500")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_geonames.json"))
    args = ap.parse_args()
    start = time.perf_counter()
    res = {"haystack": "configs[2] geonames", "scale": args.scale}

    def dump():
        W.dump_json(res, args.out)

    m, hay, off, refs, put_s, sync_s = W.bench_map("geonames", args.scale)
    n = len(refs)
    res["references"] = n
    res["build_s"] = round(put_s + sync_s, 2)
    t0 = time.perf_counter()
    m.cluster(refs[:1], 500)                                  # the first call builds the per-rank table
    res["first_call_s"] = round(time.perf_counter() - t0, 4)
    dump()

    # the workaround on a prefix of the references, less those whose rows over the whole map reach the limit at the
    # lower floor (popular names: they are left out of the list for both paths, so they are no nodes of either)
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
            a, b = np.concatenate(ea), np.concatenate(eb)
            return components(k, a, b), len(a) // 2

        ts_w, (w_label, w_edges) = timed(workaround)
        ts_c, (labels, n_clusters, n_edges) = timed(lambda: m.cluster(listed, mp))
        assert most[0] < 65535, "a node's rows were cut: take a smaller prefix"
        res[f"workaround_{mp}"] = {
            "references": k, "most_rows_of_a_node": most[0], "workaround_s": [round(t, 4) for t in ts_w],
            "cluster_s": [round(t, 4) for t in ts_c], "ratio_best": round(min(ts_w) / min(ts_c), 2),
            "cluster_worst_over_workaround_best": round(max(ts_c) / min(ts_w), 4),
            "labels_equal": bool(np.array_equal(labels, listed[w_label])),
            "edges_equal": bool(w_edges == n_edges), "n_clusters": n_clusters, "n_edges": n_edges}
        dump()

    for mp in [int(f) for f in args.floors.split(",") if f]:
        if time.perf_counter() - start > args.budget:
            res[f"whole_map_{mp}"] = {"left_out": f"the probe's budget of {args.budget:.0f} s was spent before this floor"}
            dump()
            continue
        ts, (labels, n_clusters, n_edges) = timed(lambda: m.cluster(refs, mp))
        _, sizes = np.unique(labels, return_counts=True)
        res[f"whole_map_{mp}"] = {"s": [round(t, 3) for t in ts], "best_s": round(min(ts), 3),
                                  "references_per_s": round(n / min(ts)), "n_clusters": n_clusters, "n_edges": n_edges,
                                  "largest_component": int(sizes.max()), "singletons": int((sizes == 1).sum()),
                                  "last_kernels": m.last_kernels()}
        dump()


if __name__ == "__main__":
    main()
