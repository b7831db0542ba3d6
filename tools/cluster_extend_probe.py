"""Cluster-extend figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings): what a job
that has clustered its map pays when k new references arrive.

Per floor (900 and 700 per mille) and k (1 000 and 100 000): old = the first n - k references with ``cluster``'s
labels, new = the last k.
  * the only way without the call: ``cluster`` over all n -- host clock, two timed runs, both kept (their spread is
    the margin of the comparison).  Its warm call is the floor's first ``cluster`` over an old list, the same kernels
    over all but the last k references;
  * ``cluster_extend(old, labels, new)``: two timed runs after a warm call, both kept; both label arrays, the
    components and the edges (the whole call's minus the old call's) must be equal;
  * where the extend's time goes, each two timed runs after a warm call: ``without_sweep_s`` is the call with no new
    reference (the extraction of the n - k old ones, the node tables, the seed kernel and the labels);
    ``without_sweep_or_unions_s`` the same with every old reference its own label (the seed kernel looks nothing up
    and unites nothing): the difference is the seed kernel's work, what is left of the first mostly the extraction;
    the full call less ``without_sweep_s`` is the sweep of the k needles with their extraction.
A step is started only while the probe's time budget lasts, and says so when it is left out.

Writes the JSON object to --out after every step (a step that runs out of time leaves the ones before it).
Usage: python tools/cluster_extend_probe.py [--scale 1.0] [--floors 900,700] [--new 1000,100000] [--budget 600]
       [--out FILE]"""
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


def two(fn, warm=True):
    """(host-clock seconds of two calls, after a warm one unless told otherwise; the last call's result)."""
    if warm:
        fn()
    ts = []
    for _ in range(2):
        t0 = time.perf_counter()
        got = fn()
        ts.append(round(time.perf_counter() - t0, 4))
    return ts, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--floors", default="900,700")
    ap.add_argument("--new", default="1000,100000")
    ap.add_argument("--budget", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_extend_geonames.json"))
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
    m.cluster_extend(refs[:1], refs[:1], refs[1:2], 500)      # the first call builds the per-rank table
    res["first_call_s"] = round(time.perf_counter() - t0, 4)
    dump()

    ks = [min(int(k), n - 1) for k in args.new.split(",") if k]
    for mp in [int(f) for f in args.floors.split(",") if f]:
        out = {}
        res[f"floor_{mp}"] = out
        if spent():
            out["left_out"] = f"the probe's budget of {args.budget:.0f} s was spent before this floor"
            dump()
            continue
        olds = {}
        for k in ks:                                          # the job's labels; the first is the whole call's warm call
            t0 = time.perf_counter()
            labels, _, edges = m.cluster(refs[:n - k], mp)
            olds[k] = (labels, edges, round(time.perf_counter() - t0, 3))
        out["cluster_all_s"], whole = two(lambda: m.cluster(refs, mp), warm=False)
        out["cluster_all"] = {"n_clusters": whole[1], "n_edges": whole[2], "last_kernels": m.last_kernels()}
        dump()
        for k in ks:
            one = {"old": n - k, "new": k, "cluster_old_s": olds[k][2]}
            out[f"new_{k}"] = one
            if spent():
                one["left_out"] = f"the probe's budget of {args.budget:.0f} s was spent before this step"
                dump()
                continue
            old, new, (labels, old_edges, _) = refs[:n - k], refs[n - k:], olds[k]
            one["extend_s"], got = two(lambda: m.cluster_extend(old, labels, new, mp))
            one["last_kernels"] = m.last_kernels()
            moved, _ = m.cluster_changes(old, labels, got[0])
            one.update({
                "labels_equal": bool(np.concatenate([got[0], got[1]]).tobytes() == whole[0].tobytes()),
                "clusters_equal": bool(got[2] == whole[1]),
                "edges_equal_whole_minus_old": bool(got[3] == whole[2] - old_edges),
                "n_edges": got[3], "old_labels_that_moved": int(len(moved)),
                "cluster_all_best_over_extend_worst": round(min(out["cluster_all_s"]) / max(one["extend_s"]), 1),
                "cluster_all_best_over_extend_best": round(min(out["cluster_all_s"]) / min(one["extend_s"]), 1)})
            dump()
            one["without_sweep_s"], _ = two(lambda: m.cluster_extend(old, labels, new[:0], mp))
            one["without_sweep_or_unions_s"], _ = two(lambda: m.cluster_extend(old, old, new[:0], mp))
            one["cluster_new_alone_s"], _ = two(lambda: m.cluster(new, mp))
            best = {key: min(one[key]) for key in ("extend_s", "without_sweep_s", "without_sweep_or_unions_s")}
            one["shares_of_extend_best"] = {
                "sweep_and_new_extraction": round(1 - best["without_sweep_s"] / best["extend_s"], 3),
                "seed_kernel": round((best["without_sweep_s"] - best["without_sweep_or_unions_s"]) / best["extend_s"], 3),
                "extraction_tables_labels_copies": round(best["without_sweep_or_unions_s"] / best["extend_s"], 3)}
            dump()
    res["probe_s"] = round(time.perf_counter() - start, 1)
    dump()


if __name__ == "__main__":
    main()
