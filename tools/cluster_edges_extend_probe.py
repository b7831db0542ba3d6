"""Cluster-edges extend and between figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings; DESIGN.md
section 41).  The host clock around each call, two timed calls after a warm one (both kept).

  * extend: the first 10^6 references old, the next 10^4 new, at 700 per mille: ``cluster_edge_count_extend`` and
    ``cluster_edges_extend`` at exactly the count's capacity; the difference is the sort, the rows kernel and the copy.
    The count must equal ``cluster_extend``'s n_edges.
  * whole: what a caller without the extend form pays: ``cluster_edge_count`` over the union, and -- where the device
    and the host have the memory -- ``cluster_edges`` over the union with option "cluster_edges_max" raised to the next
    power of two above the count, plus the host filter (numpy: the records with an end among the new references).  The
    filtered records must be the extend's bytes.
  * between: the 10^4 against the 10^6, both ways round; the records must be identical bytes, and the times should
    match, since the side with fewer references sweeps either way.
  * workaround: ``find_batch_by_reference_similar_each_in`` at limit 65 535 for a prefix of the new references against
    one scope of the old ones (the top 65 535 per needle, cut at the limit, a row of result layout per pair): its
    time, the rows it returns, and how many needles the limit cuts short.

A step is started only while the probe's time budget lasts, and says so when it is left out.  Writes the JSON object to
--out after every step.
Usage: python tools/cluster_edges_extend_probe.py [--scale 1.0] [--old 1000000] [--new 10000] [--prefix 1000]
       [--budget 420] [--whole 1] [--out FILE]"""
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
FLOOR = 700
LIMIT = 65535


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
    ap.add_argument("--old", type=int, default=10**6)
    ap.add_argument("--new", type=int, default=10**4)
    ap.add_argument("--prefix", type=int, default=1000)
    ap.add_argument("--budget", type=float, default=420.0)
    ap.add_argument("--whole", type=int, default=1, help="0: leave the emitting call over the union out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_edges_extend_geonames.json"))
    args = ap.parse_args()
    start = time.perf_counter()
    res = {"haystack": "configs[2] geonames", "scale": args.scale, "floor": FLOOR}

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
    n_old = min(args.old, n - 1)
    old, new = refs[:n_old], refs[n_old:n_old + min(args.new, n - n_old)]
    res.update({"references": n, "old": len(old), "new": len(new), "build_s": round(put_s + sync_s, 2),
                "cluster_edges_max": m.get_option("cluster_edges_max")})
    t0 = time.perf_counter()
    m.cluster_edge_count_extend(refs[:2], refs[2:4], 500)     # the first call builds the per-rank table
    res["first_call_s"] = round(time.perf_counter() - t0, 4)
    dump()

    # -- extend: counting and emitting ----------------------------------------------------------------------------------
    out = res["extend"] = {}
    out["count_s"], count = two(lambda: m.cluster_edge_count_extend(old, new, FLOOR))
    out.update({"count_kernels": m.last_kernels(), "n_edges": count})
    dump()
    out["cluster_extend_s"], got = two(lambda: m.cluster_extend(old, old, new, FLOOR))
    out["count_equals_cluster_extends"] = bool(got[3] == count)
    extend = None
    if count <= ROOM:
        out["emit_s"], extend = two(lambda: m.cluster_edges_extend(old, new, FLOOR, capacity=count))
        out.update({"emit_kernels": m.last_kernels(), "records": len(extend), "record_bytes": int(extend.nbytes),
                    "sort_rows_copy_s": round(min(out["emit_s"]) - min(out["count_s"]), 4),
                    "first": extend[:2].tolist(), "last": extend[-2:].tolist()})
    else:
        out["emit_left_out"] = "more records than the default cluster_edges_max"
    dump()

    # -- between, both ways round ---------------------------------------------------------------------------------------
    out = res["between"] = {}
    if not spent(out):
        out["count_s"], b_count = two(lambda: m.cluster_edge_count_between(old, new, FLOOR))
        out["new_right_s"], one = two(lambda: m.cluster_edges_between(old, new, FLOOR, capacity=b_count))
        out["new_left_s"], other = two(lambda: m.cluster_edges_between(new, old, FLOOR, capacity=b_count))
        out.update({"records": len(one), "kernels": m.last_kernels(),
                    "identical_bytes": bool(one.tobytes() == other.tobytes()),
                    "new_left_best_over_new_right_best": round(min(out["new_left_s"]) / min(out["new_right_s"]), 3)})
        if extend is not None:
            among = m.cluster_edges(new, FLOOR)
            out["merged_with_the_new_lists_own_is_the_extend"] = bool(
                m.merge_edges(one, among).tobytes() == extend.tobytes())
        del one, other
        dump()

    # -- the workaround: a scoped top-k per new reference ---------------------------------------------------------------
    out = res["workaround"] = {}
    if not spent(out):
        part = new[:min(args.prefix, len(new))]
        which = np.zeros(len(part), dtype=np.int64).tolist()
        with m.scope(old) as scope:
            out["scoped_similar_s"], got = two(
                lambda: m.find_batch_by_reference_similar_each_in([scope], which, part, LIMIT, FLOOR))
        counts = got[1]
        out.update({"needles": len(part), "limit": LIMIT, "rows": int(counts.sum()),
                    "needles_cut_at_the_limit": int((counts >= LIMIT).sum()),
                    "result_bytes": int(sum(a.nbytes for a in got[:3]))})
        out["between_same_needles_s"], rows = two(lambda: m.cluster_edges_between(old, part, FLOOR))
        out.update({"between_records": len(rows),
                    "workaround_best_over_between_best": round(min(out["scoped_similar_s"]) / min(out["between_same_needles_s"]), 1)})
        del got, rows
        dump()

    # -- the whole list again, and the host filter ----------------------------------------------------------------------
    out = res["whole"] = {}
    if not spent(out):
        union = np.concatenate([old, new])
        out["count_s"], whole_count = two(lambda: m.cluster_edge_count(union, FLOOR))
        out["n_edges"] = whole_count
        if res["extend"].get("count_s"):
            out["count_best_over_extend_count_best"] = round(min(out["count_s"]) / min(res["extend"]["count_s"]), 1)
        dump()
        raised = 1 << int(max(whole_count, 2) - 1).bit_length()
        if args.whole and raised <= 1 << 31 and not spent(out):
            m.set_option("cluster_edges_max", max(raised, ROOM))
            out["cluster_edges_max"] = max(raised, ROOM)
            try:
                def emit_and_filter():
                    rows = m.cluster_edges(union, FLOOR, capacity=whole_count)
                    t0 = time.perf_counter()
                    kept = rows[(rows[:, 0] >= new[0]) | (rows[:, 1] >= new[0])]   # (the new references are the highest)
                    return kept, time.perf_counter() - t0

                out["emit_and_filter_s"], (kept, filter_s) = two(emit_and_filter)
                out.update({"filter_s": round(filter_s, 4), "kept": len(kept),
                            "kept_is_the_extend": bool(extend is not None and kept.tobytes() == extend.tobytes())})
                if res["extend"].get("emit_s"):
                    out["whole_best_over_extend_best"] = round(min(out["emit_and_filter_s"]) / min(res["extend"]["emit_s"]), 1)
            except (OSError, MemoryError) as err:
                out["emit_failed"] = repr(err)
            m.set_option("cluster_edges_max", ROOM)
            dump()
    res["probe_s"] = round(time.perf_counter() - start, 1)
    dump()


if __name__ == "__main__":
    main()
