"""The cluster tree against what a caller pays without it, at Geonames scale (configs[2]'s haystack, 8 423 769 strings;
DESIGN.md section 32): for every floor, blurrily_storage_cluster_tree, blurrily_storage_cluster at the same floor and
one eight-floor blurrily_storage_cluster_levels call whose lowest floor it is, on

  * the short list of section 17 (a prefix of the references less those whose rows reach the workaround's limit),
  * a longer prefix (--million, 10^6 references by default), and
  * with --whole, the whole map (every reference listed; a tree call there is one whole-map sweep per round),

host clock around each call, two timed runs after a warm one, both kept.  Per floor the merges, the distinct heights,
the rounds (the sweeps launched, less the last, over images and chunks), whether labels and counts equal the separate
call's, whether cutting the tree at a few of its heights gives the separate call's labels there, and the requirement:
the tree call costs less than ceil(distinct heights / 8) levels calls, which is what the same information costs without
it.  A step is started only while the probe's time budget lasts, and says so when it is left out.

Writes the JSON object to --out after every step (a step that runs out of time leaves the ones before it).
Usage: python tools/cluster_tree_probe.py [--scale 1.0] [--floors 700,500] [--prefix 20000 (0: no short list)]
       [--million 1000000 (0: none)] [--whole] [--cuts 2] [--budget 600] [--out FILE]"""
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
from blurrily_amd import RawMap  # noqa: E402
from cluster_levels_probe import CHUNK, timed  # noqa: E402


def levels_floors(floor):
    """Eight floors from `floor` to 1000, as a caller bisecting the heights above `floor` would ask for first."""
    return sorted({floor + (1000 - floor) * k // 7 for k in range(8)}) if floor < 1000 else [1000]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--floors", default="700,500")
    ap.add_argument("--prefix", type=int, default=20000)
    ap.add_argument("--million", type=int, default=10**6)
    ap.add_argument("--whole", action="store_true")
    ap.add_argument("--cuts", type=int, default=2)
    ap.add_argument("--budget", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_tree_geonames.json"))
    args = ap.parse_args()
    start = time.perf_counter()
    floors = [int(f) for f in args.floors.split(",") if f]
    res = {"haystack": "configs[2] geonames", "scale": args.scale, "library": os.environ.get("BLURRILY_LIB", "this tree's")}

    def dump():
        W.dump_json(res, args.out)

    m, hay, off, refs, put_s, sync_s = W.bench_map("geonames", args.scale)
    n = len(refs)
    res["references"] = n
    res["build_s"] = round(put_s + sync_s, 2)
    t0 = time.perf_counter()
    m.cluster_tree(refs[:1], floors[0])                       # the first call builds the per-rank table
    res["first_call_s"] = round(time.perf_counter() - t0, 4)
    dump()

    lists = []
    k = min(args.prefix, n)
    if k:                                                     # section 17's short list
        full = np.concatenate([m.find_batch_by_reference_similar(refs[s:s + CHUNK], 65535, 500)[1]
                               for s in range(0, k, CHUNK)])
        lists.append(("short_list", refs[:k][full < 65535]))
    if args.million:
        lists.append((f"prefix_{min(args.million, n)}", refs[:min(args.million, n)]))
    if args.whole:
        lists.append(("whole_map", refs))

    for name, listed in lists:
        for floor in floors:
            key = f"{name}_{floor}"
            if time.perf_counter() - start > args.budget:
                res[key] = {"left_out": f"the probe's budget of {args.budget:.0f} s was spent before this step"}
                dump()
                continue
            ts_c, (s_labels, s_clusters, s_edges) = timed(lambda: m.cluster(listed, floor))
            row = {"references": len(listed), "floor": floor, "cluster_s": [round(t, 4) for t in ts_c],
                   "n_clusters": s_clusters, "n_edges": s_edges}
            res[key] = row
            dump()
            ts, (labels, merges, n_clusters, n_edges) = timed(lambda: m.cluster_tree(listed, floor))
            kernels = m.last_kernels()
            images = 1 + (m.device_info()["n_pending"] > 0)
            chunks = -(-len(np.unique(listed)) // (1 << 20))
            heights = np.unique(merges[:, 2])
            row.update({"tree_s": [round(t, 4) for t in ts], "merges": len(merges), "distinct_heights": len(heights),
                        "sweeps": kernels.count("cluster_tree_sweep_kernel"),
                        "rounds": kernels.count("cluster_tree_sweep_kernel") // (images * chunks) - 1,
                        "equals_separate_call": bool(np.array_equal(labels, s_labels) and
                                                     (n_clusters, n_edges) == (s_clusters, s_edges)),
                        "merges_are_nodes_less_clusters": bool(len(merges) == int((labels != 0xFFFFFFFF).sum()) - n_clusters),
                        "profile_head": RawMap.merge_profile(merges, nodes=int((labels != 0xFFFFFFFF).sum()))[:4]})
            row["tree_over_cluster"] = round(min(ts) / min(ts_c), 3)
            dump()
            fl = levels_floors(floor)
            ts_l, (l_labels, _, _) = timed(lambda: m.cluster_levels(listed, fl))
            calls = -(-len(heights) // 8)
            row.update({"levels_floors": fl, "levels_s": [round(t, 4) for t in ts_l], "levels_calls_for_the_heights": calls,
                        "levels_cost_s": round(calls * min(ts_l), 4),
                        "tree_costs_less_than_the_levels_calls": bool(max(ts) < calls * min(ts_l)),
                        "cuts_equal_levels": bool(all(np.array_equal(
                            RawMap.cut_tree(listed, labels, merges, f, min_permille=floor), l_labels[i])
                            for i, f in enumerate(fl)))})
            dump()
            picks = heights[np.unique(np.linspace(0, len(heights) - 1, args.cuts).round().astype(int))] if len(heights) else []
            row["cuts_equal_cluster_calls"] = {
                int(h): bool(np.array_equal(RawMap.cut_tree(listed, labels, merges, int(h), min_permille=floor),
                                            m.cluster(listed, int(h))[0])) for h in picks}
            dump()


if __name__ == "__main__":
    main()
