"""Blocked-clustering figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings).  Blocks
are runs of consecutive references (block key = (reference - 1) // size), the floor 700 per mille, the host clock
around the calls, two timed runs after a warm call, both kept.

  * workaround: the first 256 blocks of 1 000 references, one ``cluster`` call per block in a loop against ONE
    ``cluster_within`` call over the same 256 000 references; labels and the summed counts must be equal.  The new call
    is to be no slower than the loop, the loop's own spread being the margin.
  * whole_map_<size>: every reference, blocks of 1 000 and of 10 000: seconds, components, edges, and the same call with
    every key distinct (``without_kernels_s``: numbering, extraction, node tables, plan, labels and copies -- no block
    has a pair, so neither blocked kernel is launched); the difference is the blocked kernels' share.
  * crossover_<size>: ONE block of the first 10^2 .. 10^6 references, "scope_strategy" 1 (the map sweep) and 2 (the
    direct kernel) forced, equal results required.  A direct run is left out when the size before it says it would
    take longer than --direct-cap seconds (direct work grows with the square of a block).

A step is started only while the probe's time budget lasts, and says so when it is left out.  Writes the JSON object
to --out after every step.
Usage: python tools/cluster_within_probe.py [--scale 1.0] [--floor 700] [--budget 420] [--direct-cap 40] [--out FILE]"""
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
    ap.add_argument("--floor", type=int, default=700)
    ap.add_argument("--budget", type=float, default=420.0)
    ap.add_argument("--direct-cap", type=float, default=40.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_within_geonames.json"))
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
    m.cluster_within(refs[:2], refs[:2] * 0, 500)             # the first call builds the per-rank table
    res["first_call_s"] = round(time.perf_counter() - t0, 4)
    res["scope_strategy"] = m.get_option("scope_strategy")
    dump()

    # -- the workaround: a cluster call per block --------------------------------------------------------------------
    out = res["workaround"] = {}
    size, n_blocks = 1000, min(256, n // 1000)
    listed = refs[:size * n_blocks]
    keys = ((listed - 1) // size).astype(np.uint32)

    def loop():
        labels = np.zeros(len(listed), dtype=np.uint32)
        clusters = edges = 0
        for b in range(n_blocks):
            labels[b * size:(b + 1) * size], k, e = m.cluster(listed[b * size:(b + 1) * size], mp)
            clusters, edges = clusters + k, edges + e
        return labels, clusters, edges

    out.update({"blocks": n_blocks, "members": size})
    out["loop_s"], want = two(loop)
    out["within_s"], got = two(lambda: m.cluster_within(listed, keys, mp))
    spread = abs(out["loop_s"][0] - out["loop_s"][1])
    out.update({"last_kernels": m.last_kernels(), "labels_equal": bool(got[0].tobytes() == want[0].tobytes()),
                "counts_equal": bool(got[1:] == want[1:]), "n_clusters": got[1], "n_edges": got[2],
                "loop_spread_s": round(spread, 4),
                "within_no_slower_than_loop": bool(max(out["within_s"]) <= min(out["loop_s"]) + spread),
                "loop_best_over_within_worst": round(min(out["loop_s"]) / max(out["within_s"]), 1),
                "loop_best_over_within_best": round(min(out["loop_s"]) / min(out["within_s"]), 1)})
    dump()

    # -- the whole map in blocks ---------------------------------------------------------------------------------------
    for size in (1000, 10000):
        out = res[f"whole_map_{size}"] = {}
        if spent(out):
            continue
        keys = ((refs - 1) // size).astype(np.uint32)
        out["s"], got = two(lambda: m.cluster_within(refs, keys, mp))
        out.update({"blocks": int(keys[-1]) + 1, "n_clusters": got[1], "n_edges": got[2],
                    "references_per_s": round(n / min(out["s"])), "last_kernels": m.last_kernels()})
        dump()
        if "without_kernels_s" not in res:                    # (the same for every block size: once)
            res["without_kernels_s"], alone = two(lambda: m.cluster_within(refs, refs, mp))
            res["without_kernels_last_kernels"] = m.last_kernels()
            assert alone[2] == 0
        out["blocked_kernels_share_of_best"] = round(1 - min(res["without_kernels_s"]) / min(out["s"]), 3)
        dump()

    # -- the crossover: one block, each strategy forced ------------------------------------------------------------------
    direct_before = None                                      # (size, best seconds) of the last direct run
    for size in (10**2, 10**3, 10**4, 10**5, 10**6):
        out = res[f"crossover_{size}"] = {}
        if size > n:
            out["left_out"] = "the haystack is smaller"
            continue
        if spent(out):
            continue
        listed = refs[:size]
        keys = np.zeros(size, dtype=np.uint32)
        m.set_option("scope_strategy", 1)
        out["sweep_s"], swept = two(lambda: m.cluster_within(listed, keys, mp))
        out["sweep_kernels"] = m.last_kernels()
        out.update({"n_clusters": swept[1], "n_edges": swept[2]})
        dump()
        if direct_before and direct_before[1] * (size / direct_before[0]) ** 2 > args.direct_cap:
            out["direct_left_out"] = (f"{direct_before[1]:.3f} s at {direct_before[0]} members: the square law puts "
                                      f"a run here above the cap of {args.direct_cap:.0f} s, three runs are timed")
        else:
            m.set_option("scope_strategy", 2)
            out["direct_s"], direct = two(lambda: m.cluster_within(listed, keys, mp))
            out["direct_kernels"] = m.last_kernels()
            out["equal"] = bool(direct[0].tobytes() == swept[0].tobytes() and direct[1:] == swept[1:])
            out["direct_no_slower"] = bool(min(out["direct_s"]) <= min(out["sweep_s"]))
            direct_before = (size, min(out["direct_s"]))
        m.set_option("scope_strategy", 0)
        dump()
    res["probe_s"] = round(time.perf_counter() - start, 1)
    dump()


if __name__ == "__main__":
    main()
