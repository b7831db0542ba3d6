"""Cluster-centres figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings):

  * against the workaround on section 17's short list (a prefix of the references less those whose rows reach the
    limit): chunks through find_batch_by_reference_similar at limit 65 535, the rows among the listed references turned
    into labels, degrees, centres and attached by numpy -- host clock around each path, two timed runs after a warm
    one, both kept (their spread is the margin of the comparison); all four outputs of both must be equal;
  * the whole map (every reference listed) at 900 and 700 per mille: seconds of blurrily_storage_cluster, of this call
    without `attached` and with it (two timed runs each after one warm call per floor), their ratios, and the share of
    the components of two or more that are stars.  A floor is started only while the probe's time budget lasts, and
    says so when it is left out.

Writes the JSON object to --out after every step (a step that runs out of time leaves the ones before it).
Usage: python tools/cluster_centres_probe.py [--scale 1.0] [--prefix 20000 (0: no workaround)] [--floors 900,700]
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
from cluster_probe import CHUNK, components, timed  # noqa: E402


def centres_of(label, degree):
    """Per node the index of its component's centre: the highest degree, the lowest index among equals."""
    order = np.lexsort((np.arange(len(label)), -degree, label))
    first = np.ones(len(order), dtype=bool)
    first[1:] = label[order][1:] != label[order][:-1]
    best = np.zeros(len(label), dtype=np.int64)
    best[label[order][first]] = order[first]                  # (a label is an index too: the component's lowest)
    return best[label]


def stars(labels, attached):
    """(components of two or more nodes, those of them whose nodes are all attached)."""
    _, which, sizes = np.unique(labels, return_inverse=True, return_counts=True)
    loose = np.bincount(which, weights=(attached == 0), minlength=len(sizes))
    return int((sizes >= 2).sum()), int(((sizes >= 2) & (loose == 0)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--prefix", type=int, default=20000)
    ap.add_argument("--budget", type=float, default=900.0)
    ap.add_argument("--floors", default="900,700")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_centres_geonames.json"))
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
    m.cluster_centres(refs[:1], 500)                          # the first call builds the per-rank table
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
            label = components(k, a, b)
            degree = np.bincount(a, minlength=k)
            centre = centres_of(label, degree)
            attached = (centre == np.arange(k)).astype(np.uint8)
            attached[a[centre[a] == b]] = 1
            return label, degree, centre, attached, len(a) // 2

        ts_w, (w_label, w_degree, w_centre, w_attached, w_edges) = timed(workaround)
        ts_c, (labels, degrees, centres, attached, n_clusters, n_edges) = timed(lambda: m.cluster_centres(listed, mp))
        ts_l, _ = timed(lambda: m.cluster_centres(listed, mp, attached=False))
        ts_p, _ = timed(lambda: m.cluster(listed, mp))
        assert most[0] < 65535, "a node's rows were cut: take a smaller prefix"
        pairs, starred = stars(labels, attached)
        res[f"workaround_{mp}"] = {
            "references": k, "most_rows_of_a_node": most[0], "workaround_s": [round(t, 4) for t in ts_w],
            "centres_s": [round(t, 4) for t in ts_c], "centres_without_attached_s": [round(t, 4) for t in ts_l],
            "cluster_s": [round(t, 4) for t in ts_p], "ratio_best": round(min(ts_w) / min(ts_c), 2),
            "centres_worst_over_workaround_best": round(max(ts_c) / min(ts_w), 4),
            "labels_equal": bool(np.array_equal(labels, listed[w_label])),
            "degrees_equal": bool(np.array_equal(degrees, w_degree)),
            "centres_equal": bool(np.array_equal(centres, listed[w_centre])),
            "attached_equal": bool(np.array_equal(attached, w_attached)),
            "edges_equal": bool(w_edges == n_edges), "n_clusters": n_clusters, "n_edges": n_edges,
            "components_of_two_or_more": pairs, "stars": starred}
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

        base = m.cluster(refs, mp)                            # the floor's warm call
        out["cluster_s"], base = two(lambda: m.cluster(refs, mp))
        dump()
        out["centres_without_attached_s"], lean = two(lambda: m.cluster_centres(refs, mp, attached=False))
        out["last_kernels_without_attached"] = m.last_kernels()
        dump()
        out["centres_s"], full = two(lambda: m.cluster_centres(refs, mp))
        labels, degrees, centres, attached, n_clusters, n_edges = full
        pairs, starred = stars(labels, attached)
        out.update({
            "last_kernels": m.last_kernels(),
            "without_attached_over_cluster": round(min(out["centres_without_attached_s"]) / min(out["cluster_s"]), 3),
            "with_attached_over_cluster": round(min(out["centres_s"]) / min(out["cluster_s"]), 3),
            "n_clusters": n_clusters, "n_edges": n_edges,
            "equals_cluster_call": bool(labels.tobytes() == base[0].tobytes() and (n_clusters, n_edges) == base[1:]
                                        and lean[0].tobytes() == labels.tobytes() and lean[4:] == full[4:]
                                        and lean[1].tobytes() == degrees.tobytes() and lean[2].tobytes() == centres.tobytes()),
            "degrees_sum_is_twice_the_edges": bool(int(degrees.sum(dtype=np.uint64)) == 2 * n_edges),
            "highest_degree": int(degrees.max()), "unattached_nodes": int((attached == 0).sum()),
            "components_of_two_or_more": pairs, "stars": starred,
            "star_share": round(starred / pairs, 4) if pairs else None})
        dump()


if __name__ == "__main__":
    main()
