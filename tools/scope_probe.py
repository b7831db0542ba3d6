"""Scoped-find figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings, limit 10):

  * scope preparation: the first scoped find of a fresh scope (one needle) against the next one, host clock;
  * batched needles/s through blurrily_storage_find_batch_in_device with each strategy forced (mask, direct), scopes of
    10^2 .. 10^6 references at random and of every reference, for 4 096 and 1 048 576 needles, HIP-event time (best of
    three after a warm call), against the unscoped blurrily_storage_find_batch_device over the same needles; the rows of
    the two strategies compared wherever both run;
  * single scoped finds (blurrily_storage_find_in), host clock p50 / p90 over 300 needles, both strategies;
  * the crossover: the largest scope whose direct batches beat the mask's at both batch sizes, in member codes (the
    figure "scope_direct_max" defaults to).

Prints one JSON object.  Usage: python tools/scope_probe.py [--scale 1.0] [--out FILE] [--kernels-only]
(--kernels-only: one 4 096-needle batch per strategy at 10^3 members and the mask at every reference -- the run to put
under rocprofv3 --kernel-trace --stats)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import workloads as W  # noqa: E402
from blurrily_amd import _native  # noqa: E402

LIMIT = 10


def _events_ms(fn, reps=3):
    fn()                                                     # warm
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return best


class Batch:
    def __init__(self, q, qo, dev):
        self.n = len(qo) - 1
        self.bytes = int(qo[-1])
        self.d_packed = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
        self.d_off = torch.from_numpy(qo.astype(np.int64)).to(dev)
        self.rows = torch.zeros((self.n, LIMIT, 3), dtype=torch.int32, device=dev)
        self.counts = torch.zeros((self.n,), dtype=torch.int32, device=dev)

    def run(self, m, scope=None):
        lib = _native.lib()
        st = torch.cuda.current_stream().cuda_stream
        if scope is None:
            rc = lib.blurrily_storage_find_batch_device(m.handle, self.d_packed.data_ptr(), self.bytes,
                                                        self.d_off.data_ptr(), self.n, LIMIT, self.rows.data_ptr(),
                                                        self.counts.data_ptr(), None, st)
        else:
            rc = lib.blurrily_storage_find_batch_in_device(m.handle, scope._h, self.d_packed.data_ptr(), self.bytes,
                                                           self.d_off.data_ptr(), self.n, LIMIT, self.rows.data_ptr(),
                                                           self.counts.data_ptr(), st)
        assert rc == 0, C.get_errno()

    def result(self):
        torch.cuda.synchronize()
        c = self.counts.cpu().numpy().view(np.uint32).copy()
        r = self.rows.cpu().numpy().view(np.uint32).copy()
        live = np.arange(LIMIT)[None, :] < c[:, None].astype(np.int64)
        return c, np.where(live[:, :, None], r, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    m, hay, off, refs, _, _ = W.bench_map("geonames", args.scale)
    n = len(refs)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(12)
    sizes = sorted({s for s in [10 ** k for k in range(2, 7)] + [30000, 50000] if s < n}) + [n]   # (50 000: near the
    # direct strategy's cap of 57 344 members)
    scopes = {s: (refs if s == n else np.sort(rng.choice(refs, s, replace=False))) for s in sizes}
    batches = {k: Batch(*W.queries(hay, off, k, seed=13 + k % 7), dev) for k in ((4096,) if args.kernels_only
                                                                                  else (4096, 1048576))}
    if args.kernels_only:
        b = batches[4096]
        for s, strategy in ((1000, 1), (1000, 2), (n, 1)):
            m.set_option("scope_strategy", strategy)
            with m.scope(scopes[s]) as sc:
                for _ in range(3):
                    b.run(m, sc)
                torch.cuda.synchronize()
        b.run(m)
        torch.cuda.synchronize()
        m.close()
        return
    out = {"haystack": "configs[2] geonames", "references": n, "limit": LIMIT, "unscoped": {}, "scopes": []}
    for k, b in batches.items():
        ms = _events_ms(lambda: b.run(m))
        out["unscoped"][str(k)] = {"ms": round(ms, 3), "needles_per_s": round(k / ms * 1e3)}
    single = W.unpack(*W.queries(hay, off, 300, seed=21))
    for s in sizes:
        rec = {"members": s}
        _, offs, _ = m.get_batch(scopes[s]) if s <= 100000 else (None, None, None)
        rec["member_codes"] = int(offs[-1]) if offs is not None else None
        # preparation: a fresh scope's first find (one needle) against its second
        m.set_option("scope_strategy", 1)
        sc = m.scope(scopes[s])
        t0 = time.perf_counter()
        m.find_in(sc, single[0], LIMIT)
        t1 = time.perf_counter()
        m.find_in(sc, single[0], LIMIT)
        t2 = time.perf_counter()
        rec["prepare_ms"] = round(1e3 * ((t1 - t0) - (t2 - t1)), 3)
        for k, b in batches.items():
            per = {}
            rows = {}
            for strategy, name in ((1, "mask"), (2, "direct")):
                m.set_option("scope_strategy", strategy)
                b.run(m, sc)
                torch.cuda.synchronize()
                took = "scope_find_kernel" in m.last_kernels()
                if strategy == 2 and not took:
                    per[name] = "declined"
                    continue
                ms = _events_ms(lambda: b.run(m, sc))
                rows[name] = b.result()
                per[name] = {"ms": round(ms, 3), "needles_per_s": round(k / ms * 1e3)}
            if len(rows) == 2:
                per["rows_equal"] = bool(np.array_equal(rows["mask"][0], rows["direct"][0]) and
                                         np.array_equal(rows["mask"][1], rows["direct"][1]))
            rec[str(k)] = per
        for strategy, name in ((1, "mask"), (2, "direct")):
            if s > 100000 and strategy == 2:
                continue
            m.set_option("scope_strategy", strategy)
            m.find_in(sc, single[1], LIMIT)
            if strategy == 2 and "scope_find_kernel" not in m.last_kernels():
                continue
            ts = []
            for nd in single:
                t0 = time.perf_counter()
                m.find_in(sc, nd, LIMIT)
                ts.append(time.perf_counter() - t0)
            rec["single_" + name] = {"p50_us": round(1e6 * float(np.percentile(ts, 50)), 1),
                                     "p90_us": round(1e6 * float(np.percentile(ts, 90)), 1)}
        sc.close()
        out["scopes"].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    m.set_option("scope_strategy", 0)
    # the crossover: the largest scope whose direct batches beat the mask's at both batch sizes
    best = 0
    for rec in out["scopes"]:
        wins = all(isinstance(rec[str(k)].get("direct"), dict) and
                   rec[str(k)]["direct"]["ms"] < rec[str(k)]["mask"]["ms"] for k in batches)
        if wins and rec["member_codes"]:
            best = max(best, rec["member_codes"])
    out["crossover_member_codes"] = best
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    m.close()


if __name__ == "__main__":
    main()
