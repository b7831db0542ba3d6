"""Threshold-find figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings):

  * batches: the bench's 1 M needles through blurrily_storage_find_batch_above at min_permille 500, 700 and 900 in
    count-only mode (results NULL: the count pass, row_off filled) -- needles/s and rows per needle -- and with the rows
    written (the count pass, the emit pass, the sort and the rows) where they fit ROW_BUDGET, else over the first
    needles whose rows do; blurrily_storage_find_batch at limit 10 over the same needles; host clock around each call
    (needles in from and rows out to host memory on every side), best of two after a warm call;
  * the whole-map self-join at 800 per mille: blurrily_storage_find_references_above over every reference, count only,
    and Map.join_above where the pairs fit ROW_BUDGET; host clock;
  * single finds: blurrily_storage_find_above at 700 per mille, host clock p50 / p90 over 300 needles.

Writes the JSON object to --out after every step (a step that runs out of time leaves the ones before it).
Usage: python tools/above_probe.py [--scale 1.0] [--out FILE] [--skip-join]"""
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
from blurrily_amd import Map, _native  # noqa: E402

ROW_BUDGET = 400_000_000                                     # rows a filled call may return here (12 B each)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "above_geonames.json"))
    ap.add_argument("--skip-join", action="store_true")
    args = ap.parse_args()
    res = {"haystack": "configs[2] geonames", "scale": args.scale}

    def dump():
        W.dump_json(res, args.out)

    m, hay, off, refs, put_s, sync_s = W.bench_map("geonames", args.scale)
    n = len(refs)
    res["references"] = n
    res["build_s"] = round(put_s + sync_s, 2)
    q, qo = W.bench_needles(hay, off, "geonames", args.scale)
    nq = len(qo) - 1
    res["needles"] = nq
    dt, (_, counts) = W.best_of(lambda: m.find_batch_packed(q, qo, 10))
    res["find_batch_limit10"] = {"s": round(dt, 4), "needles_per_s": round(nq / dt), "rows_per_needle":
                                 round(float(counts.mean()), 3)}
    dump()
    lib = _native.lib()
    row_off = np.zeros(nq + 1, dtype=np.uint64)

    def count_only(mp):
        assert lib.blurrily_storage_find_batch_above(m.handle, q.ctypes.data, qo.ctypes.data, nq, 0, mp, None, 0,
                                                     row_off.ctypes.data) == 0
        return row_off.copy()

    for mp in (500, 700, 900):
        dt, offs = W.best_of(lambda: count_only(mp))
        r = {"count_only_s": round(dt, 4), "count_only_needles_per_s": round(nq / dt),
             "rows_per_needle": round(int(offs[-1]) / nq, 3), "rows": int(offs[-1])}
        k = int(np.searchsorted(offs, ROW_BUDGET, side="right")) - 1      # needles whose rows fit the budget
        k = max(1, min(nq, k))
        qk, qok = q[:int(qo[k])], qo[:k + 1]
        dt, (_, ro) = W.best_of(lambda: m.find_batch_above_packed(qk, qok, 0, mp))
        r.update({"filled_needles": k, "filled_s": round(dt, 4), "filled_needles_per_s": round(k / dt),
                  "filled_rows": int(ro[-1]), "last_kernels": m.last_kernels()})
        res[f"above_{mp}"] = r
        dump()
    # single finds at 700 per mille
    needles = W.unpack(q[:int(qo[300])], qo[:301])
    m.find_above(needles[0], 0, 700)
    ts = []
    for s in needles:
        t0 = time.perf_counter()
        m.find_above(s, 0, 700)
        ts.append(time.perf_counter() - t0)
    res["find_above_700_us"] = {"p50": round(float(np.percentile(ts, 50)) * 1e6, 1),
                                "p90": round(float(np.percentile(ts, 90)) * 1e6, 1)}
    dump()
    if not args.skip_join:
        roff = np.zeros(n + 1, dtype=np.uint64)
        t0 = time.perf_counter()
        assert lib.blurrily_storage_find_references_above(m.handle, refs.ctypes.data, n, 0, 800, None, 0,
                                                          roff.ctypes.data, None) == 0
        res["join_above_800"] = {"count_only_s": round(time.perf_counter() - t0, 2), "pairs": int(roff[-1]),
                                 "pairs_without_self": int(roff[-1]) - n}
        dump()
        if int(roff[-1]) <= ROW_BUDGET:
            t0 = time.perf_counter()
            jr, joff, _ = Map.join_above(m, refs, 0, 800)
            res["join_above_800"].update({"s": round(time.perf_counter() - t0, 2), "references": int(len(jr)),
                                          "pairs_filled": int(joff[-1])})
            dump()


if __name__ == "__main__":
    main()
