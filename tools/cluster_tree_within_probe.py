"""Blocked-tree figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings).  Blocks are
runs of consecutive references (block key = (reference - 1) // size), the floor 700 per mille, the host clock around the
calls, two timed runs after a warm call, both kept.

  * per_block_loop: the first 256 blocks of 1 000 references -- the shape of ``cluster_within``'s figure -- timed three
    ways in this one run: ONE ``cluster_tree_within`` call, one ``cluster_tree`` call per block in a loop (what the API
    offered before, the baseline), and ONE ``cluster_within`` call (a single round: the lower bound).  The records of
    the loop, merged under the total order, its labels and its summed counts must equal the one call's.  The new call
    is to take less time than the loop.  Rounds and launches are read from ``last_kernels``.
  * one_block_100000: ONE block of the first 10^5 references under "scope_strategy" 1 (the map sweep every round) and 2
    (the direct kernel every round), equal results required: which side of the direct cap 10^5 lies on for the tree.
  * keys_1000: the first 10^6 references under 10^3 keys (blocks of 1 000), against the plain tree's 10^6 figure
    (profiles/cluster_tree_geonames.json) and one ``cluster_within`` call over the same list.

A step is started only while the probe's time budget lasts, and says so when it is left out.  Writes the JSON object
to --out after every step.
Usage: python tools/cluster_tree_within_probe.py [--scale 1.0] [--floor 700] [--budget 420] [--out FILE]"""
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


def launches(m):
    """What the last call launched: the merging rounds (one more round finds nothing) and every kernel's count."""
    names = m.last_kernels()
    counts = {k: names.count(k) for k in sorted(set(names))}
    return {"rounds_that_merged": counts.get("cluster_tree_merge_kernel", 1) - 1, "launches": len(names), "kernels": counts}


def in_order(rows):
    return rows[np.lexsort((rows[:, 1], rows[:, 0], 1000 - rows[:, 2].astype(np.int64)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--floor", type=int, default=700)
    ap.add_argument("--budget", type=float, default=420.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_tree_within_geonames.json"))
    args = ap.parse_args()
    start = time.perf_counter()
    mp = args.floor
    res = {"haystack": "configs[2] geonames", "scale": args.scale, "floor": mp}

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
    t0 = time.perf_counter()
    m.cluster_tree_within(refs[:2], refs[:2] * 0, 500)        # the first call builds the per-rank table
    res["first_call_s"] = round(time.perf_counter() - t0, 4)
    res["scope_strategy"] = m.get_option("scope_strategy")
    dump()

    # -- one call against a cluster_tree call per block, and against cluster_within's single round ------------------------
    out = res["per_block_loop"] = {}
    size, n_blocks = 1000, min(256, n // 1000)
    listed = refs[:size * n_blocks]
    keys = ((listed - 1) // size).astype(np.uint32)
    loop_rounds, loop_launches = [], []

    def loop():
        labels = np.zeros(len(listed), dtype=np.uint32)
        records, clusters, edges = [], 0, 0
        del loop_rounds[:], loop_launches[:]
        for b in range(n_blocks):
            labels[b * size:(b + 1) * size], rows, k, e = m.cluster_tree(listed[b * size:(b + 1) * size], mp)
            loop_rounds.append(m.last_kernels().count("cluster_tree_merge_kernel") - 1)
            loop_launches.append(len(m.last_kernels()))
            records.append(rows)
            clusters, edges = clusters + k, edges + e
        return labels, in_order(np.concatenate(records)), clusters, edges

    out.update({"blocks": n_blocks, "members": size})
    out["loop_s"], want = two(loop)
    out["loop_rounds_that_merged"] = {"least": int(min(loop_rounds)), "most": int(max(loop_rounds)),
                                      "sum": int(sum(loop_rounds))}
    out["loop_launches"] = int(sum(loop_launches))
    out["tree_within_s"], got = two(lambda: m.cluster_tree_within(listed, keys, mp))
    out["tree_within"] = launches(m)
    out["within_s"], one_round = two(lambda: m.cluster_within(listed, keys, mp))
    spread = abs(out["loop_s"][0] - out["loop_s"][1])
    out.update({"records_equal": bool(got[1].tobytes() == want[1].tobytes()),
                "labels_equal": bool(got[0].tobytes() == want[0].tobytes() == one_round[0].tobytes()),
                "counts_equal": bool(got[2:] == want[2:] == one_round[1:]),
                "n_merges": len(got[1]), "n_clusters": got[2], "n_edges": got[3],
                "heights": len(np.unique(got[1][:, 2])), "loop_spread_s": round(spread, 4),
                "tree_within_faster_than_loop": bool(max(out["tree_within_s"]) < min(out["loop_s"])),
                "loop_best_over_tree_within_worst": round(min(out["loop_s"]) / max(out["tree_within_s"]), 1),
                "tree_within_best_over_within_best": round(min(out["tree_within_s"]) / min(out["within_s"]), 1),
                "loop_ms_per_block": round(1000 * min(out["loop_s"]) / n_blocks, 2)})
    dump()

    # -- one block of 10^5: which side of the direct cap it lies on for the tree -------------------------------------------
    size = 10**5
    out = res[f"one_block_{size}"] = {}
    if size > n:
        out["left_out"] = "the haystack is smaller"
    elif not spent(out):
        listed = refs[:size]
        keys = np.zeros(size, dtype=np.uint32)
        m.set_option("scope_strategy", 1)
        out["sweep_s"], swept = two(lambda: m.cluster_tree_within(listed, keys, mp))
        out["sweep"] = launches(m)
        m.set_option("scope_strategy", 2)
        out["direct_s"], direct = two(lambda: m.cluster_tree_within(listed, keys, mp))
        out["direct"] = launches(m)
        m.set_option("scope_strategy", 0)
        out["auto_s"], auto = two(lambda: m.cluster_tree_within(listed, keys, mp))
        out["auto_kernels"] = sorted(set(m.last_kernels()))
        out["plain_tree_s"], plain = two(lambda: m.cluster_tree(listed, mp))
        out.update({"n_merges": len(swept[1]), "n_clusters": swept[2], "n_edges": swept[3],
                    "equal": bool(all(x.tobytes() == y.tobytes() == z.tobytes() == w.tobytes()
                                      for x, y, z, w in zip(swept[:2], direct[:2], auto[:2], plain[:2]))
                                  and swept[2:] == direct[2:] == auto[2:] == plain[2:]),
                    "direct_no_slower": bool(min(out["direct_s"]) <= min(out["sweep_s"])),
                    "sweep_best_over_direct_best": round(min(out["sweep_s"]) / min(out["direct_s"]), 1)})
    dump()

    # -- 10^6 references under 10^3 keys ---------------------------------------------------------------------------------------
    size, total = 1000, 10**6
    out = res["keys_1000"] = {}
    if total > n:
        out["left_out"] = "the haystack is smaller"
    elif not spent(out):
        listed = refs[:total]
        keys = ((listed - 1) // size).astype(np.uint32)
        out["tree_within_s"], got = two(lambda: m.cluster_tree_within(listed, keys, mp))
        out["tree_within"] = launches(m)
        out["within_s"], one_round = two(lambda: m.cluster_within(listed, keys, mp))
        out.update({"references": total, "blocks": int(keys[-1]) + 1, "n_merges": len(got[1]), "n_clusters": got[2],
                    "n_edges": got[3], "heights": len(np.unique(got[1][:, 2])),
                    "labels_and_counts_equal_cluster_within": bool(got[0].tobytes() == one_round[0].tobytes()
                                                                   and got[2:] == one_round[1:]),
                    "n_merges_is_nodes_minus_clusters": bool(len(got[1]) == int((got[0] != 0xFFFFFFFF).sum()) - got[2]),
                    "no_record_joins_two_keys": bool(((got[1][:, 0] - 1) // size == (got[1][:, 1] - 1) // size).all()),
                    "tree_within_best_over_within_best": round(min(out["tree_within_s"]) / min(out["within_s"]), 1),
                    "references_per_s": round(total / min(out["tree_within_s"]))})
    res["probe_s"] = round(time.perf_counter() - start, 1)
    dump()


if __name__ == "__main__":
    main()
