"""The cluster core tree within blocks at Geonames scale (configs[2]'s haystack, 8 423 769 strings; DESIGN.md section
44).  Blocks are runs of consecutive references (block key = (reference - 1) // size), the floor 700 per mille,
min_degree 3, the host clock around the calls, two timed runs after a warm call, both kept.

  * workaround: the first 256 blocks of 1 000 references in ONE ``cluster_core_tree_within`` call, against one
    ``cluster_core_tree`` call per block in a loop (labels, core heights, the merged records and the summed counts must
    be equal), and against ``cluster_tree_within`` and ``cluster_cores_within`` on the same input; the height passes
    and the rounds apart, from the same call at min_degree 0 (no height pass: its time is the rounds').
  * one_block_100000: ONE block of the first 10^5 references, "scope_strategy" 2 (direct) against 1 (swept), equal
    results required.
  * keys_1000: the first 10^6 references under 10^3 keys (blocks of 1 000 consecutive references).

A step is started only while the probe's time budget lasts, and says so when it is left out.  Writes the JSON object to
--out after every step.
Usage: python tools/cluster_core_tree_within_probe.py [--scale 1.0] [--floor 700] [--min-degree 3] [--budget 300] [--out FILE]"""
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


def same(one, other):
    return bool(all(a.tobytes() == b.tobytes() for a, b in zip(one[:3], other[:3])) and tuple(one[3:]) == tuple(other[3:]))


def in_order(rows):
    """Record lists as one under the tree's total order (height descending, then a, then b)."""
    rows = np.concatenate(rows) if rows else np.zeros((0, 3), dtype=np.uint32)
    return np.ascontiguousarray(rows[np.lexsort((rows[:, 1], rows[:, 0], 1000 - rows[:, 2].astype(np.int64)))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--floor", type=int, default=700)
    ap.add_argument("--min-degree", type=int, default=3)
    ap.add_argument("--budget", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_core_tree_within_geonames.json"))
    args = ap.parse_args()
    start = time.perf_counter()
    mp, md = args.floor, args.min_degree
    res = {"haystack": "configs[2] geonames", "scale": args.scale, "floor": mp, "min_degree": md}

    def dump():
        W.dump_json(res, args.out)

    def spent(out):
        if time.perf_counter() - start > args.budget:
            out["left_out"] = f"the probe's budget of {args.budget:.0f} s was spent before this step"
            dump()
            return True
        return False

    def shape(got):
        return {"n_merges": int(len(got[2])), "heights": int(len(np.unique(got[2][:, 2]))), "n_clusters": got[3],
                "n_edges": got[4], "n_core_edges": got[5], "cores": int((got[1] != 0xFFFFFFFF).sum())}

    def launches(names):
        return {k: names.count(k) for k in sorted(set(names))}

    m, hay, off, refs, put_s, sync_s = W.bench_map("geonames", args.scale)
    n = len(refs)
    res["references"] = n
    res["build_s"] = round(put_s + sync_s, 2)
    t0 = time.perf_counter()
    m.cluster_core_tree_within(refs[:2], refs[:2] * 0, 500, md)   # the first call builds the per-rank table
    res["first_call_s"] = round(time.perf_counter() - t0, 4)
    res["scope_strategy"] = m.get_option("scope_strategy")
    dump()

    # -- the workaround: a cluster_core_tree call per block --------------------------------------------------------------
    out = res["workaround"] = {}
    size, n_blocks = 1000, min(256, n // 1000)
    listed = refs[:size * n_blocks]
    keys = ((listed - 1) // size).astype(np.uint32)

    def loop():
        labels, core = (np.zeros(len(listed), dtype=np.uint32) for _ in range(2))
        records, sums = [], [0, 0, 0]
        for b in range(n_blocks):
            at = slice(b * size, (b + 1) * size)
            labels[at], core[at], rows, *counts = m.cluster_core_tree(listed[at], mp, md)
            records.append(rows)
            sums = [x + y for x, y in zip(sums, counts)]
        return (labels, core, in_order(records), *sums)

    out.update({"blocks": n_blocks, "members": size})
    out["loop_s"], want = two(loop)
    out["core_tree_within_s"], got = two(lambda: m.cluster_core_tree_within(listed, keys, mp, md))
    out["launches"] = launches(m.last_kernels())
    out["rounds_only_s"], _ = two(lambda: m.cluster_core_tree_within(listed, keys, mp, 0))   # (min_degree 0: no height pass)
    out["cluster_tree_within_s"], tree = two(lambda: m.cluster_tree_within(listed, keys, mp))
    out["cluster_cores_within_s"], cores = two(lambda: m.cluster_cores_within(listed, keys, mp, md))
    out.update(shape(got))
    best = min(out["core_tree_within_s"])
    out.update({"equal_to_the_loop": same(got, want),
                "counts_equal_cluster_cores_within": bool(got[3:] == cores[3:]),
                "edges_equal_cluster_tree_within": bool(got[4] == tree[3]),
                "loop_spread_s": round(abs(out["loop_s"][0] - out["loop_s"][1]), 4),
                "loop_best_over_core_tree_within_worst": round(min(out["loop_s"]) / max(out["core_tree_within_s"]), 1),
                "loop_best_over_core_tree_within_best": round(min(out["loop_s"]) / best, 1),
                "height_passes_s_by_difference": round(best - min(out["rounds_only_s"]), 4),
                "core_tree_within_best_over_cluster_tree_within_best": round(best / min(out["cluster_tree_within_s"]), 2),
                "core_tree_within_best_over_cluster_cores_within_best": round(best / min(out["cluster_cores_within_s"]), 2)})
    dump()

    # -- one block, each strategy forced ---------------------------------------------------------------------------------
    size = 10**5
    out = res[f"one_block_{size}"] = {}
    if size > n:
        out["left_out"] = "the haystack is smaller"
    elif not spent(out):
        listed = refs[:size]
        keys = np.zeros(size, dtype=np.uint32)
        m.set_option("scope_strategy", 1)
        out["sweep_s"], swept = two(lambda: m.cluster_core_tree_within(listed, keys, mp, md))
        out["sweep_launches"] = launches(m.last_kernels())
        m.set_option("scope_strategy", 2)
        out["direct_s"], direct = two(lambda: m.cluster_core_tree_within(listed, keys, mp, md))
        out["direct_launches"] = launches(m.last_kernels())
        m.set_option("scope_strategy", 0)
        out.update(shape(direct))
        out.update({"equal": same(direct, swept), "sweep_best_over_direct_best": round(min(out["sweep_s"]) / min(out["direct_s"]), 1)})
    dump()

    # -- 10^6 references under 10^3 keys ---------------------------------------------------------------------------------
    size, n_keys = 1000, 1000
    out = res[f"keys_{n_keys}"] = {}
    if size * n_keys > n:
        out["left_out"] = "the haystack is smaller"
    elif not spent(out):
        listed = refs[:size * n_keys]
        keys = ((listed - 1) // size).astype(np.uint32)
        out["core_tree_within_s"], got = two(lambda: m.cluster_core_tree_within(listed, keys, mp, md))
        out["launches"] = launches(m.last_kernels())
        out["cluster_cores_within_s"], cores = two(lambda: m.cluster_cores_within(listed, keys, mp, md))
        out.update(shape(got))
        out.update({"references": len(listed), "keys": n_keys, "counts_equal_cluster_cores_within": bool(got[3:] == cores[3:]),
                    "references_per_s": round(len(listed) / min(out["core_tree_within_s"])),
                    "core_tree_within_best_over_cluster_cores_within_best":
                        round(min(out["core_tree_within_s"]) / min(out["cluster_cores_within_s"]), 2)})
    res["probe_s"] = round(time.perf_counter() - start, 1)
    dump()


if __name__ == "__main__":
    main()
