"""Cluster levels against separate cluster calls at Geonames scale (configs[2]'s haystack, 8 423 769 strings; DESIGN.md
section 18): for every floor set, the levels call and blurrily_storage_cluster at each of its floors, on

  * the short list of section 17 (a prefix of the references less those whose rows reach the workaround's limit), and
  * the whole map (every reference listed),

host clock around each call, two timed runs after a warm one, both kept (their spread is the margin of the
comparison).  A floor's separate call is timed once and shared by the sets that hold it.  Per level the clusters, the
edges and the largest component, and whether labels and counts equal the separate call's.  A step is started only while
the probe's time budget lasts, and says so when it is left out.

Writes the JSON object to --out after every step (a step that runs out of time leaves the ones before it).
Usage: python tools/cluster_levels_probe.py [--scale 1.0] [--sets "700,800,900;500,700,900"] [--prefix 20000 (0: no
       short list)] [--no-whole] [--no-separate] [--budget 900] [--out FILE]"""
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

CHUNK = 2000                                                 # needles per workaround call (cluster_probe.py's)


def timed(fn, reps=2):
    """(host-clock seconds of `reps` calls after a warm one, the last call's result)."""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return ts, out


def largest(labels):
    _, sizes = np.unique(labels, return_counts=True)
    return int(sizes.max()), int((sizes == 1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sets", default="700,800,900;500,700,900")
    ap.add_argument("--prefix", type=int, default=20000)
    ap.add_argument("--no-whole", action="store_true")
    ap.add_argument("--no-separate", action="store_true")
    ap.add_argument("--budget", type=float, default=900.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_levels_geonames.json"))
    args = ap.parse_args()
    start = time.perf_counter()
    sets = [tuple(int(f) for f in s.split(",")) for s in args.sets.split(";") if s]
    res = {"haystack": "configs[2] geonames", "scale": args.scale, "library": os.environ.get("BLURRILY_LIB", "this tree's")}

    def dump():
        W.dump_json(res, args.out)

    m, hay, off, refs, put_s, sync_s = W.bench_map("geonames", args.scale)
    n = len(refs)
    res["references"] = n
    res["build_s"] = round(put_s + sync_s, 2)
    t0 = time.perf_counter()
    m.cluster_levels(refs[:1], sets[0])                       # the first call builds the per-rank table
    res["first_call_s"] = round(time.perf_counter() - t0, 4)
    dump()

    lists = []
    k = min(args.prefix, n)
    if k:                                                     # section 17's short list
        full = np.concatenate([m.find_batch_by_reference_similar(refs[s:s + CHUNK], 65535, 500)[1]
                               for s in range(0, k, CHUNK)])
        lists.append(("short_list", refs[:k][full < 65535]))
    if not args.no_whole:
        lists.append(("whole_map", refs))

    for name, listed in lists:
        separate = {}                                         # floor -> (seconds, labels, n_clusters, n_edges)
        for floors in sets:
            key = f"{name}_{'_'.join(map(str, floors))}"
            if time.perf_counter() - start > args.budget:
                res[key] = {"left_out": f"the probe's budget of {args.budget:.0f} s was spent before this step"}
                dump()
                continue
            ts, (labels, n_clusters, n_edges) = timed(lambda: m.cluster_levels(listed, floors))
            row = {"references": len(listed), "floors": list(floors), "levels_s": [round(t, 4) for t in ts],
                   "last_kernels": m.last_kernels(), "levels": []}
            for i, p in enumerate(floors):
                big, single = largest(labels[i])
                row["levels"].append({"floor": p, "n_clusters": int(n_clusters[i]), "n_edges": int(n_edges[i]),
                                      "largest_component": big, "singletons": single})
            res[key] = row
            dump()
            if args.no_separate:
                continue
            for i, p in enumerate(floors):
                if p not in separate:
                    separate[p] = timed(lambda: m.cluster(listed, p))
                ts_p, (s_labels, s_clusters, s_edges) = separate[p]
                row["levels"][i]["separate_s"] = [round(t, 4) for t in ts_p]
                row["levels"][i]["equals_separate_call"] = bool(
                    np.array_equal(labels[i], s_labels) and (s_clusters, s_edges) == (n_clusters[i], n_edges[i]))
            sums = [sum(separate[p][0][r] for p in floors) for r in range(2)]
            lowest = separate[floors[0]][0]
            row["separate_sum_s"] = [round(t, 4) for t in sums]
            row["levels_worst_over_separate_best"] = round(max(ts) / min(sums), 4)
            row["levels_over_lowest_floor_alone"] = round(min(ts) / min(lowest), 4)
            # the requirement: less than the sum of the separate calls by more than the two runs' spread
            spread = max(max(ts) - min(ts), max(sums) - min(sums))
            row["faster_than_separate_by_more_than_the_spread"] = bool(min(sums) - max(ts) > spread)
            dump()


if __name__ == "__main__":
    main()
