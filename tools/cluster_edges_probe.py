"""Cluster-edges figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings).  The host
clock around each call, the best of two timed calls after a warm one (both kept).

  * count_vs_cluster: the first 10^6 references at 700 per mille: ``cluster_edge_count`` against ``cluster`` on the same
    list in the same run -- the same sweep minus the unions plus the reservation.  The counts must be equal.
  * emit: the lowest of 700, 800, 900, 950 and 1000 per mille at which those references have at most 2^28 edges: the
    emitting call at exactly that capacity beside the count-only call at the same floor (the sweep's share); the
    difference is the sort, the rows kernel and the copy together.  Where no floor fits (a haystack that repeats names
    has that many pairs of identical strings alone), what the call answers at the default bound is recorded, and the
    list is emitted at 700 with option "cluster_edges_max" raised to the next power of two above its count.
  * workaround: the same edges the old way on a prefix of the references whose rows fit 400 M: ``join_above`` at the
    matching per mille plus ``get_batch`` for the R of every end (the host filter and the halving of the pairs left out,
    in the workaround's favour), against ``cluster_edges`` on that prefix.
  * within: 256 blocks of 1 000 consecutive references at 700 per mille: ``cluster_edges`` with blocks against
    ``cluster_within`` on the same input and against one ``cluster_edges`` call per block; equal records required.

A step is started only while the probe's time budget lasts, and says so when it is left out.  Writes the JSON object to
--out after every step.
Usage: python tools/cluster_edges_probe.py [--scale 1.0] [--listed 1000000] [--prefix 20000] [--budget 420] [--out FILE]"""
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

ROOM = 1 << 28                                                # option "cluster_edges_max" at its default
WORKAROUND_ROWS = 400 * 10**6


def two(fn):
    """(host-clock seconds of two calls after a warm one; the last call's result)."""
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
    ap.add_argument("--listed", type=int, default=10**6)
    ap.add_argument("--prefix", type=int, default=20000)
    ap.add_argument("--budget", type=float, default=420.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_edges_geonames.json"))
    args = ap.parse_args()
    start = time.perf_counter()
    res = {"haystack": "configs[2] geonames", "scale": args.scale}

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
    res.update({"references": n, "build_s": round(put_s + sync_s, 2), "cluster_edges_max": m.get_option("cluster_edges_max")})
    t0 = time.perf_counter()
    m.cluster_edge_count(refs[:2], 500)                       # the first call builds the per-rank table
    res["first_call_s"] = round(time.perf_counter() - t0, 4)
    listed = refs[:min(args.listed, n)]
    dump()

    # -- counting against cluster ----------------------------------------------------------------------------------------
    out = res["count_vs_cluster"] = {"references": len(listed), "floor": 700}
    out["cluster_s"], got = two(lambda: m.cluster(listed, 700))
    out["cluster_kernels"] = m.last_kernels()
    out["count_s"], count = two(lambda: m.cluster_edge_count(listed, 700))
    out.update({"count_kernels": m.last_kernels(), "n_edges": count, "counts_equal": bool(count == got[2]),
                "count_best_over_cluster_best": round(min(out["count_s"]) / min(out["cluster_s"]), 3)})
    dump()

    # -- an emitting call ------------------------------------------------------------------------------------------------
    out = res["emit"] = {"references": len(listed), "edges_by_floor": {}}
    floor = None
    for f in (700, 800, 900, 950, 1000):
        e = count if f == 700 else m.cluster_edge_count(listed, f)
        out["edges_by_floor"][str(f)] = e
        if e <= ROOM:
            floor = f
            break
    dump()
    if floor is None:
        # no floor fits the default bound (the haystack repeats names: identical strings alone are that many pairs).
        # What the default answers, then the same list at 700 with the option raised to the next power of two
        floor = 700
        try:
            m.cluster_edges(listed, floor, capacity=count)
            out["at_the_default_bound"] = "filled"
        except OSError as err:
            out["at_the_default_bound"] = os.strerror(err.errno)
        raised = 1 << int(count - 1).bit_length()
        if raised <= 1 << 31:
            m.set_option("cluster_edges_max", raised)
            out["cluster_edges_max"] = raised
        else:
            floor = None
    if floor is not None and not spent(out):
        e = out["edges_by_floor"][str(floor)]
        out["floor"] = floor
        out["count_s"], _ = two(lambda: m.cluster_edge_count(listed, floor))
        out["emit_s"], edges = two(lambda: m.cluster_edges(listed, floor, capacity=e))
        out.update({"emit_kernels": m.last_kernels(), "records": len(edges), "record_bytes": int(edges.nbytes),
                    "sweep_s": min(out["count_s"]),
                    "sort_rows_copy_s": round(min(out["emit_s"]) - min(out["count_s"]), 4),
                    "records_per_s": round(len(edges) / min(out["emit_s"])) if len(edges) else 0,
                    "first": edges[:2].tolist(), "last": edges[-2:].tolist()})
        del edges
        dump()
    m.set_option("cluster_edges_max", ROOM)

    # -- the workaround: join_above plus get_batch ------------------------------------------------------------------------
    out = res["workaround"] = {}
    if floor is not None and not spent(out):
        part = refs[:min(args.prefix, n)]
        while True:
            _, row_off, _ = m.join_above(part, 0, floor)
            if int(row_off[-1]) <= WORKAROUND_ROWS or len(part) <= 1000:
                break
            part = part[:len(part) // 2]

        def workaround():
            held, row_off, rows = m.join_above(part, 0, floor)
            weights, code_off, codes = m.get_batch(np.unique(rows[:, 0]))   # (the R of every end; the filter is left out)
            return int(row_off[-1]), len(code_off) - 1

        out.update({"references": len(part), "floor": floor})
        out["workaround_s"], (n_rows, n_ends) = two(workaround)
        out["edges_s"], edges = two(lambda: m.cluster_edges(part, floor))
        out.update({"rows": n_rows, "ends_fetched": n_ends, "records": len(edges),
                    "workaround_best_over_edges_best": round(min(out["workaround_s"]) / min(out["edges_s"]), 1)})
        dump()

    # -- within blocks ---------------------------------------------------------------------------------------------------
    out = res["within"] = {}
    if not spent(out):
        size, n_blocks = 1000, min(256, n // 1000)
        part = refs[:size * n_blocks]
        keys = ((part - 1) // size).astype(np.uint32)
        out.update({"blocks": n_blocks, "members": size, "floor": 700})
        out["cluster_within_s"], within = two(lambda: m.cluster_within(part, keys, 700))
        out["count_s"], counted = two(lambda: m.cluster_edge_count(part, 700, keys))
        out["edges_s"], edges = two(lambda: m.cluster_edges(part, 700, blocks=keys))
        out["edges_kernels"] = m.last_kernels()

        def loop():
            return [m.cluster_edges(part[b * size:(b + 1) * size], 700) for b in range(n_blocks)]

        out["loop_s"], own = two(loop)
        own = np.concatenate(own)
        own = own[np.lexsort((own[:, 1], own[:, 0], 1000 - own[:, 2].astype(np.int64)))]
        out.update({"records": len(edges), "counts_equal": bool(len(edges) == counted == within[2]),
                    "records_equal_the_loops": bool(own.tobytes() == edges.tobytes()),
                    "edges_best_over_cluster_within_best": round(min(out["edges_s"]) / min(out["cluster_within_s"]), 2),
                    "loop_best_over_edges_best": round(min(out["loop_s"]) / min(out["edges_s"]), 1)})
        dump()
    res["probe_s"] = round(time.perf_counter() - start, 1)
    dump()


if __name__ == "__main__":
    main()
