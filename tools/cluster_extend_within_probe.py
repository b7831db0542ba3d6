"""Cluster-extend-within-blocks figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings; DESIGN.md section
45).  Blocks are runs of consecutive references, the floor 700 per mille, the host clock around the calls, the median
of --reps timed calls after a warm one, every timing kept.  The seeds are ``cluster_within``'s labels over the old
rows, so every extend must equal ``cluster_within`` over old ++ new (``equal``).

  * a_many_keys: 10^6 old rows under 10^3 keys, 10^4 new rows spread over the keys, against ``cluster_within`` over the
    union and ``cluster_extend`` (no keys) on the same lists.
  * b_small_blocks: 256 blocks of 10^3 old rows, one new row a block, against ``cluster_within`` over the union.
  * c1_block_1e5, c2_block_1e6: ONE block of 10^5 and of 10^6 old rows with 10^3 new rows, "scope_strategy" 1 (the map
    sweep) and 2 (the direct kernel) forced, against ``cluster_within`` over the union under the default strategy.

Every shape also records ``beginning_s``: the same extend with every key distinct, which numbers, extracts, builds the
node tables, seeds and labels but launches neither blocked kernel -- what ``cluster_within`` over the union pays too,
and what bounds the gain for small blocks.

A step is started only while the probe's time budget lasts, and says so when it is left out.  Writes the JSON object
to --out after every step.
Usage: python tools/cluster_extend_within_probe.py [--scale 1.0] [--floor 700] [--reps 5] [--budget 420] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import workloads as W  # noqa: E402


def timed(fn, reps):
    """({"median_s", "all_s"} of `reps` calls after a warm one, the last call's result)."""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = fn()
        ts.append(round(time.perf_counter() - t0, 5))
    return {"median_s": round(statistics.median(ts), 5), "all_s": ts}, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--floor", type=int, default=700)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget", type=float, default=420.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_extend_within_geonames.json"))
    args = ap.parse_args()
    start = time.perf_counter()
    mp, reps = args.floor, args.reps
    res = {"haystack": "configs[2] geonames", "scale": args.scale, "floor": mp, "reps": reps,
           "clock": "host clock around the call, median of reps after one warm call"}

    def dump():
        W.dump_json(res, args.out)

    def spent(out):
        if time.perf_counter() - start > args.budget:
            out["left_out"] = f"the probe's budget of {args.budget:.0f} s was spent before this step"
            dump()
            return True
        return False

    m, hay, off, refs, put_s, sync_s = W.bench_map("geonames", args.scale)
    n = len(refs)
    res["references"] = n
    res["build_s"] = round(put_s + sync_s, 2)
    m.cluster_within(refs[:2], refs[:2] * 0, 500)             # the first call builds the per-rank table
    res["scope_strategy"] = m.get_option("scope_strategy")
    dump()

    def shape(name, old, okeys, new, nkeys, strategies, with_plain_extend=False):
        out = res[name] = {"old_rows": len(old), "new_rows": len(new),
                           "keys": int(len(np.unique(np.concatenate([okeys, nkeys]))))}
        if len(old) + len(new) > n:
            out["left_out"] = "the haystack is smaller"
            return
        if spent(out):
            return
        both, bkeys = np.concatenate([old, new]), np.concatenate([okeys, nkeys])
        m.set_option("scope_strategy", 0)
        seeds, _, old_edges = m.cluster_within(old, okeys, mp)
        out["within_union"], whole = timed(lambda: m.cluster_within(both, bkeys, mp), reps)
        out["within_union"]["last_kernels"] = m.last_kernels()
        out.update({"n_clusters": whole[1], "n_edges_union": whole[2], "n_edges_old": old_edges})
        dump()
        for s in strategies:
            m.set_option("scope_strategy", s)
            key = f"extend_within_strategy_{s}"
            out[key], got = timed(lambda: m.cluster_extend_within(old, okeys, seeds, new, nkeys, mp), reps)
            out[key].update({"last_kernels": m.last_kernels(), "n_edges": got[3],
                             "equal": bool(np.concatenate([got[0], got[1]]).tobytes() == whole[0].tobytes()
                                           and got[2] == whole[1] and got[3] == whole[2] - old_edges),
                             "within_union_over_this": round(out["within_union"]["median_s"] / out[key]["median_s"], 2)})
            dump()
        m.set_option("scope_strategy", 0)
        # the beginning both calls pay: every key distinct, so no block has a pair and no blocked kernel is launched
        out["beginning"], alone = timed(lambda: m.cluster_extend_within(old, old, seeds, new, new, mp), reps)
        out["beginning"]["last_kernels"] = m.last_kernels()
        assert alone[3] == 0
        if with_plain_extend:
            out["extend_no_keys"], plain = timed(lambda: m.cluster_extend(old, seeds, new, mp), reps)
            out["extend_no_keys"].update({"last_kernels": m.last_kernels(), "n_edges": plain[3]})
        dump()

    # (a) many keys, a night's put spread over them
    old = refs[:10**6]
    new = refs[10**6:10**6 + 10**4]
    shape("a_many_keys", old, ((old - 1) // 1000).astype(np.uint32), new,
          (np.arange(len(new)) % 1000).astype(np.uint32), (0,), with_plain_extend=True)
    # (b) small blocks, one new row each
    old = refs[:256000]
    new = refs[256000:256256]
    shape("b_small_blocks", old, ((old - 1) // 1000).astype(np.uint32), new, np.arange(len(new), dtype=np.uint32), (0,))
    # (c) one large block under either kernel
    for name, size in (("c1_block_1e5", 10**5), ("c2_block_1e6", 10**6)):
        old, new = refs[:size], refs[size:size + 1000]
        shape(name, old, np.zeros(len(old), dtype=np.uint32), new, np.zeros(len(new), dtype=np.uint32), (1, 2))
        out = res[name]
        if "extend_within_strategy_2" in out:
            out["direct_no_slower_than_sweep"] = bool(out["extend_within_strategy_2"]["median_s"]
                                                      <= out["extend_within_strategy_1"]["median_s"])
            dump()
    res["probe_s"] = round(time.perf_counter() - start, 1)
    dump()


if __name__ == "__main__":
    main()
