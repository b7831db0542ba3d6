"""The cluster core tree against what a caller pays without it, at Geonames scale (configs[2]'s haystack; DESIGN.md
section 36): on a prefix of the references (--million, 10^6 by default) at every floor of --floors and one min_degree,

  * blurrily_storage_cluster_core_tree, the same call with min_degree 0 (no height sweep, every node in the forest) and
    with a min_degree no node reaches (the height sweeps and a forest round that returns at once),
  * blurrily_storage_cluster_tree (the single-linkage tree: the rounds without the heights),
  * blurrily_storage_cluster_centres without the attached pass (one degree sweep, what a height sweep is measured by),
  * blurrily_storage_cluster_cores at --cores-calls of the result's distinct heights spread over their range -- the
    workaround is one such call per distinct height, so its cost is given as the mean of the calls timed times the
    distinct heights, and says that it is an extrapolation unless every height was run (--cores-calls 0: all) --

host clock around each call, two timed runs after a warm one, both kept.  Per floor the merges, the cores, the distinct
heights, the height sweeps and the rounds (from the launches' names, over images and chunks), and whether every cut
checked equals the cores call there.  A step is started only while the probe's time budget lasts, and says so when it
is left out.

Writes the JSON object to --out after every step (a step that runs out of time leaves the ones before it).
Usage: python tools/cluster_core_tree_probe.py [--scale 1.0] [--floors 700] [--min-degree 3] [--million 1000000]
       [--cores-calls 3] [--budget 600] [--out FILE]"""
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
from blurrily_amd import RawMap, _native  # noqa: E402
from cluster_levels_probe import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--floors", default="700")
    ap.add_argument("--min-degree", type=int, default=3)
    ap.add_argument("--million", type=int, default=10**6)
    ap.add_argument("--cores-calls", type=int, default=3)
    ap.add_argument("--budget", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_core_tree_geonames.json"))
    args = ap.parse_args()
    start = time.perf_counter()
    floors = [int(f) for f in args.floors.split(",") if f]
    k = args.min_degree
    res = {"haystack": "configs[2] geonames", "scale": args.scale, "min_degree": k,
           "library": os.environ.get("BLURRILY_LIB", "this tree's")}

    def dump():
        W.dump_json(res, args.out)

    def spent():
        return time.perf_counter() - start > args.budget

    m, hay, off, refs, put_s, sync_s = W.bench_map("geonames", args.scale)
    res["references"] = len(refs)
    res["build_s"] = round(put_s + sync_s, 2)
    listed = refs[:min(args.million, len(refs))]
    t0 = time.perf_counter()
    m.cluster_core_tree(refs[:1], floors[0], k)               # the first call builds the per-rank table
    res["first_call_s"] = round(time.perf_counter() - t0, 4)
    dump()

    for floor in floors:
        key = f"prefix_{len(listed)}_{floor}"
        if spent():
            res[key] = {"left_out": f"the probe's budget of {args.budget:.0f} s was spent before this step"}
            dump()
            continue
        ts, (labels, core, merges, n_clusters, n_edges, n_core_edges) = timed(lambda: m.cluster_core_tree(listed, floor, k))
        kernels = m.last_kernels()
        images = 1 + (m.device_info()["n_pending"] > 0)
        chunks = -(-len(np.unique(listed)) // (1 << 20))
        heights = np.unique(merges[:, 2])
        row = {"references": len(listed), "floor": floor, "core_tree_s": [round(t, 4) for t in ts],
               "cores": int((core != _native.NO_CORE).sum()), "merges": len(merges), "distinct_heights": len(heights),
               "n_clusters": n_clusters, "n_edges": n_edges, "n_core_edges": n_core_edges,
               "height_sweeps": kernels.count("cluster_core_height_sweep_kernel") // (images * chunks),
               "rounds": kernels.count("cluster_core_tree_sweep_kernel") // (images * chunks) - 1}
        res[key] = row
        dump()
        ts_0, _ = timed(lambda: m.cluster_core_tree(listed, floor, 0))
        row["core_tree_min_degree_0_s"] = [round(t, 4) for t in ts_0]
        row["rounds_min_degree_0"] = m.last_kernels().count("cluster_core_tree_sweep_kernel") // (images * chunks) - 1
        dump()
        ts_t, (_, t_merges, _, _) = timed(lambda: m.cluster_tree(listed, floor))
        row.update({"tree_s": [round(t, 4) for t in ts_t], "tree_merges": len(t_merges),
                    "tree_rounds": m.last_kernels().count("cluster_tree_sweep_kernel") // (images * chunks) - 1})
        dump()
        ts_d, _ = timed(lambda: m.cluster_centres(listed, floor, attached=False))
        row["centres_degree_sweep_s"] = [round(t, 4) for t in ts_d]
        # a min_degree no node reaches: the height sweeps (the later ones find no bracket to add to) and one round whose
        # workgroups return at once -- the height sweeps' cost, next to that of a degree sweep
        ts_n, none = timed(lambda: m.cluster_core_tree(listed, floor, 0xFFFFFFFF))
        row["core_tree_no_cores_s"] = [round(t, 4) for t in ts_n]
        row["no_cores_has_none"] = bool((none[1] == _native.NO_CORE).all() and len(none[2]) == 0)
        dump()
        picks = heights if args.cores_calls == 0 else \
            heights[np.unique(np.linspace(0, len(heights) - 1, min(args.cores_calls, len(heights))).round().astype(int))] \
            if len(heights) else heights
        each, equal = {}, {}
        for h in picks.tolist():
            if spent():
                break
            ts_c, (c_labels, _, kinds, c_clusters, _, _) = timed(lambda: m.cluster_cores(listed, h, k))
            at, is_core = RawMap.cut_core_tree(listed, labels, core, merges, h, min_permille=floor)
            each[h] = [round(t, 4) for t in ts_c]
            equal[h] = bool(np.array_equal(kinds == _native.KIND_CORE, is_core) and
                            np.array_equal(c_labels[is_core], at[is_core]) and c_clusters == len(np.unique(at[is_core])))
        if each:
            mean = float(np.mean([min(t) for t in each.values()]))
            row.update({"cores_calls_s": each, "cuts_equal_cores_calls": equal,
                        "cores_call_per_height_s": round(mean * len(heights), 2),
                        "cores_call_per_height_is": "measured" if len(each) == len(heights) else
                        f"extrapolated from {len(each)} of {len(heights)} heights",
                        "core_tree_costs_less_than_a_cores_call_per_height": bool(max(ts) < mean * len(heights))})
        dump()


if __name__ == "__main__":
    main()
