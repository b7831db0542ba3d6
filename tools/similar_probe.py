"""Similarity-find figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings):

  * batches: the bench's 1 M needles through blurrily_storage_find_batch_similar at limit 10 and min_permille 0, 300,
    500 and 700 -- needles/s and rows per needle -- and blurrily_storage_find_batch at limit 10 over the same needles
    for scale; host clock around each call (needles in from and rows out to host memory), best of two after a warm call;
  * the workaround at 500 and 700 per mille: find_batch_above over the first needles whose rows fit ROW_BUDGET (the
    budget of section 14), plus get_batch for every distinct reference among the rows (each row's R) -- the device
    calls only, host clock, best of two; the host re-rank is not timed (it only adds to the workaround) and is done for
    the first PARITY needles, whose rows must equal the new path's;
  * single finds: blurrily_storage_find_similar at limit 10 and 500 per mille, host clock p50 / p90 over 300 needles.

Writes the JSON object to --out after every step (a step that runs out of time leaves the ones before it).
Usage: python tools/similar_probe.py [--scale 1.0] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import workloads as W  # noqa: E402
from blurrily_amd import _native  # noqa: E402

ROW_BUDGET = 400_000_000                                     # rows a filled threshold call may return (section 14)
PARITY = 1000                                                # needles whose workaround rows are re-ranked and compared
LIMIT = 10


def n_trigrams(s):
    out = (C.c_uint16 * (len(s) + 1))()
    return _native.lib().blurrily_tokeniser_parse_string(s, out)


def rerank(rows, row_off, R, T, limit, mp):
    """The workaround's host step for needles [0, len(T)): J, the floor, the order, the cut -- exact integers."""
    out = []
    for i, t in enumerate(T):
        seg = rows[int(row_off[i]):int(row_off[i + 1])].astype(np.int64)
        r = R[seg[:, 0]]
        m = seg[:, 1]
        u = t + r - m
        keep = 1000 * m >= mp * u
        seg, r, m, u = seg[keep], r[keep], m[keep], u[keep]
        sim = (m << 32) // u                                  # exact and order-preserving (csrc/similar.h)
        order = np.lexsort((seg[:, 0], seg[:, 2], -m, -sim))[:limit]
        out.append([[int(seg[j, 0]), int(m[j]), int(seg[j, 2]), int(r[j])] for j in order])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similar_geonames.json"))
    args = ap.parse_args()
    res = {"haystack": "configs[2] geonames", "scale": args.scale, "limit": LIMIT}

    def dump():
        W.dump_json(res, args.out)

    m, hay, off, refs, put_s, sync_s = W.bench_map("geonames", args.scale)
    n = len(refs)
    res["references"] = n
    res["build_s"] = round(put_s + sync_s, 2)
    q, qo = W.bench_needles(hay, off, "geonames", args.scale)
    nq = len(qo) - 1
    res["needles"] = nq
    t0 = time.perf_counter()
    m.find_batch_similar_packed(q[:int(qo[1])], qo[:2], LIMIT, 0)      # the first call builds the per-rank table
    res["first_call_s"] = round(time.perf_counter() - t0, 4)
    dt, (_, counts) = W.best_of(lambda: m.find_batch_packed(q, qo, LIMIT))
    res["find_batch_limit10"] = {"s": round(dt, 4), "needles_per_s": round(nq / dt),
                                 "rows_per_needle": round(float(counts.mean()), 3)}
    dump()
    got = {}
    for mp in (0, 300, 500, 700):
        dt, out = W.best_of(lambda: m.find_batch_similar_packed(q, qo, LIMIT, mp))
        got[mp] = out
        res[f"similar_{mp}"] = {"s": round(dt, 4), "needles_per_s": round(nq / dt),
                                "rows_per_needle": round(float(out[1].mean()), 3), "last_kernels": m.last_kernels()}
        dump()
    # the workaround, over the needles whose rows fit the budget (counted first, rows not written)
    lib = _native.lib()
    strings = W.unpack(q[:int(qo[PARITY])], qo[:PARITY + 1])
    T = [n_trigrams(s) for s in strings]
    for mp in (500, 700):
        ro = np.zeros(nq + 1, dtype=np.uint64)
        assert lib.blurrily_storage_find_batch_above(m.handle, q.ctypes.data, qo.ctypes.data, nq, 0, mp, None, 0,
                                                     ro.ctypes.data) == 0
        k = max(1, min(nq, int(np.searchsorted(ro, ROW_BUDGET, side="right")) - 1))
        qk, qok = q[:int(qo[k])], qo[:k + 1]

        def workaround():
            rows, row_off = m.find_batch_above_packed(qk, qok, 0, mp)
            refs = np.unique(rows[:, 0])
            _, code_off, _ = m.get_batch(refs)
            return rows, row_off, refs, np.diff(code_off.astype(np.int64))

        dt, (rows, row_off, refs, rr) = W.best_of(workaround)
        dt_new, _ = W.best_of(lambda: m.find_batch_similar_packed(qk, qok, LIMIT, mp))
        R = np.zeros(n + 1, dtype=np.int64)
        R[refs.astype(np.int64)] = rr
        pk = min(PARITY, k)
        want = rerank(rows, row_off, R, T[:pk], LIMIT, mp)
        grows, gcounts, gntri = got[mp]
        same = all(want[i] == [r + [t] for r, t in zip(grows[i, :gcounts[i]].tolist(), gntri[i, :gcounts[i]].tolist())]
                   for i in range(pk))
        res[f"workaround_{mp}"] = {"needles": k, "rows": int(row_off[-1]),
                                   "rows_per_needle": round(int(row_off[-1]) / k, 1),
                                   "s": round(dt, 4), "needles_per_s": round(k / dt),
                                   "similar_same_needles_s": round(dt_new, 4),
                                   "similar_same_needles_per_s": round(k / dt_new),
                                   "speedup": round(dt / dt_new, 2), "parity_needles": pk, "parity": bool(same)}
        del rows, row_off
        dump()
    # single finds
    m.find_similar(strings[0], LIMIT, 500)
    ts = []
    for s in strings[:300]:
        t0 = time.perf_counter()
        m.find_similar(s, LIMIT, 500)
        ts.append(time.perf_counter() - t0)
    res["find_similar_500_us"] = {"p50": round(float(np.percentile(ts, 50)) * 1e6, 1),
                                  "p90": round(float(np.percentile(ts, 90)) * 1e6, 1)}
    dump()


if __name__ == "__main__":
    main()
