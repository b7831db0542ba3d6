"""Cluster-tree-extend figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings): what a
caller who holds a tree over the first --old references (10^6 by default) pays when the next k arrive.

Per floor (700 per mille) and k (10^2, 10^4 and 10^5): old = the first --old references with ``cluster_tree``'s records
at the floor, new = the next k.
  * the only way without the call: ``cluster_tree`` over old ++ new -- host clock, two timed runs after a warm call,
    both kept (their spread is the margin of the comparison);
  * ``cluster_tree_extend(old, records, new)``: two timed runs after a warm call, both kept; the records, both label
    arrays and the components must equal the whole call's, the edges the whole call's minus the old call's; the rounds
    (merge launches less the last, which finds nothing);
  * the requirement, for every k but the largest: the worse extend run costs less than the better whole run; the largest
    k is reported whichever way it falls;
  * where the extend's time goes, each two timed runs after a warm call: ``without_sweep_s`` is the call with no new
    reference (the extraction of the old ones, the node tables, the records' resolve and their rounds, the labels),
    ``without_sweep_or_records_s`` the same with no records either (one round that finds nothing): mostly the
    extraction and the node tables over the old list, the call's fixed cost.
A step is started only while the probe's time budget lasts, and says so when it is left out.

Writes the JSON object to --out after every step (a step that runs out of time leaves the ones before it).
Usage: python tools/cluster_tree_extend_probe.py [--scale 1.0] [--floors 700] [--old 1000000] [--new 100,10000,100000]
       [--budget 600] [--out FILE]"""
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
from cluster_extend_probe import two  # noqa: E402

NONE = np.zeros((0, 3), dtype=np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--floors", default="700")
    ap.add_argument("--old", type=int, default=10**6)
    ap.add_argument("--new", default="100,10000,100000")
    ap.add_argument("--budget", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_tree_extend_geonames.json"))
    args = ap.parse_args()
    start = time.perf_counter()
    res = {"haystack": "configs[2] geonames", "scale": args.scale}

    def dump():
        W.dump_json(res, args.out)

    def spent():
        return time.perf_counter() - start > args.budget

    m, hay, off, refs, put_s, sync_s = W.bench_map("geonames", args.scale)
    n = len(refs)
    res["references"] = n
    res["build_s"] = round(put_s + sync_s, 2)
    t0 = time.perf_counter()
    m.cluster_tree_extend(refs[:1], NONE, refs[1:2], 500)     # the first call builds the per-rank table
    res["first_call_s"] = round(time.perf_counter() - t0, 4)
    dump()

    n_old = min(args.old, n - 1)
    old = refs[:n_old]
    ks = [min(int(k), n - n_old) for k in args.new.split(",") if k]
    for floor in [int(f) for f in args.floors.split(",") if f]:
        out = {"old": n_old}
        res[f"floor_{floor}"] = out
        if spent():
            out["left_out"] = f"the probe's budget of {args.budget:.0f} s was spent before this floor"
            dump()
            continue
        t0 = time.perf_counter()
        _, held, _, old_edges = m.cluster_tree(old, floor)    # the caller's tree (and the whole calls' warm call)
        out.update({"tree_old_s": round(time.perf_counter() - t0, 4), "old_records": len(held), "old_edges": old_edges})
        dump()
        for k in ks:
            one = {"new": k}
            out[f"new_{k}"] = one
            if spent():
                one["left_out"] = f"the probe's budget of {args.budget:.0f} s was spent before this step"
                dump()
                continue
            new = refs[n_old:n_old + k]
            both = np.concatenate([old, new])
            one["tree_all_s"], whole = two(lambda: m.cluster_tree(both, floor), warm=False)
            kernels = m.last_kernels()
            one["tree_all_rounds"] = kernels.count("cluster_tree_merge_kernel") - 1
            dump()
            one["extend_s"], got = two(lambda: m.cluster_tree_extend(old, held, new, floor))
            kernels = m.last_kernels()
            removed, added = RawMap.tree_changes(held, got[2])
            one.update({
                "extend_rounds": kernels.count("cluster_tree_merge_kernel") - 1,
                "extend_sweeps": kernels.count("cluster_tree_extend_sweep_kernel"),
                "records_equal": bool(got[2].tobytes() == whole[1].tobytes()),
                "labels_equal": bool(np.concatenate([got[0], got[1]]).tobytes() == whole[0].tobytes()),
                "clusters_equal": bool(got[3] == whole[2]),
                "edges_equal_whole_minus_old": bool(got[4] == whole[3] - old_edges),
                "records": len(got[2]), "n_edges": got[4], "records_removed": len(removed), "records_added": len(added),
                "extend_worst_under_tree_all_best": bool(max(one["extend_s"]) < min(one["tree_all_s"])),
                "tree_all_best_over_extend_worst": round(min(one["tree_all_s"]) / max(one["extend_s"]), 2),
                "tree_all_best_over_extend_best": round(min(one["tree_all_s"]) / min(one["extend_s"]), 2)})
            dump()
            one["without_sweep_s"], _ = two(lambda: m.cluster_tree_extend(old, held, new[:0], floor))
            one["without_sweep_or_records_s"], _ = two(lambda: m.cluster_tree_extend(old, NONE, new[:0], floor))
            best = {key: min(one[key]) for key in ("extend_s", "without_sweep_s", "without_sweep_or_records_s")}
            one["shares_of_extend_best"] = {
                "sweeps_and_new_extraction": round(1 - best["without_sweep_s"] / best["extend_s"], 3),
                "records_rounds": round((best["without_sweep_s"] - best["without_sweep_or_records_s"]) / best["extend_s"], 3),
                "extraction_tables_labels_copies": round(best["without_sweep_or_records_s"] / best["extend_s"], 3)}
            dump()
    res["probe_s"] = round(time.perf_counter() - start, 1)
    dump()


if __name__ == "__main__":
    main()
