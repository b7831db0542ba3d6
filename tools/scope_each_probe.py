"""Scope-per-needle figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings, limit 10):

  * mixed batch: 4 096 needles over 256 scopes of 10^3 members each (16 needles a scope, served directly) through
    blurrily_storage_find_batch_each_in_device, against the same needles in ONE 10^3-member scope
    (blurrily_storage_find_batch_in_device) and against 256 find_batch_in_device calls of 16 needles; HIP-event time,
    best of three after a warm call; the rows of the each-in call compared with the 256 calls';
  * small host batch: 32 needles over 32 scopes through blurrily_storage_find_batch_each_in, host clock p50 / p90 over
    200 calls, against 32 find_in calls (the same needles, the same scopes);
  * blocked self-join: blurrily_storage_find_references_each_in over 256 x 10^3 members (and Map.join_within's lists
    beside it), and over a Zipf-sized family of 250 blocks that covers every reference (the largest blocks served
    through the mask), host clock, against the whole-map self-join (blurrily_storage_find_references);
  * preparing 256 stale scopes in one call: the first each-in call over 256 fresh 10^3-member scopes, one needle a
    scope, against the next call; and again after a put (the scopes' device buffers made already).

Prints one JSON object.  Usage: python tools/scope_each_probe.py [--scale 1.0] [--out FILE] [--kernels-only]
(--kernels-only: three mixed batches and three single-scope batches of 4 096 needles -- the run to put under
rocprofv3 --kernel-trace --stats)"""
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
from blurrily_amd import RawMap, _native  # noqa: E402

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


def _host_us(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"p50_us": round(1e6 * float(np.percentile(ts, 50)), 1), "p90_us": round(1e6 * float(np.percentile(ts, 90)), 1)}


class Batch:
    def __init__(self, q, qo, dev):
        self.n = len(qo) - 1
        self.bytes = int(qo[-1])
        self.qo = qo
        self.d_packed = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
        self.d_off = torch.from_numpy(qo.astype(np.int64)).to(dev)
        self.rows = torch.zeros((self.n, LIMIT, 3), dtype=torch.int32, device=dev)
        self.counts = torch.zeros((self.n,), dtype=torch.int32, device=dev)

    def each_in(self, m, scopes, d_which):
        hs = (C.c_void_p * len(scopes))(*[sc._h.value for sc in scopes])
        rc = _native.lib().blurrily_storage_find_batch_each_in_device(
            m.handle, hs, len(scopes), d_which.data_ptr(), self.d_packed.data_ptr(), self.bytes, self.d_off.data_ptr(),
            self.n, LIMIT, self.rows.data_ptr(), self.counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, C.get_errno()

    def find_in(self, m, scope, lo=0, hi=None):
        hi = self.n if hi is None else hi
        rc = _native.lib().blurrily_storage_find_batch_in_device(
            m.handle, scope._h, self.d_packed.data_ptr(), self.bytes, self.d_off[lo:].data_ptr(), hi - lo, LIMIT,
            self.rows[lo:].data_ptr(), self.counts[lo:].data_ptr(), torch.cuda.current_stream().cuda_stream)
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
    rng = np.random.default_rng(31)
    member_sets = [np.sort(rng.choice(refs, 1000, replace=False)) for _ in range(256)]
    scopes = [m.scope(s) for s in member_sets]
    b = Batch(*W.queries(hay, off, 4096, seed=32), dev)
    which = np.repeat(np.arange(256, dtype=np.uint32), 16)          # needle i in scope i // 16
    d_which = torch.from_numpy(which.view(np.int32).copy()).to(dev)
    if args.kernels_only:
        for _ in range(3):
            b.each_in(m, scopes, d_which)
        for _ in range(3):
            b.find_in(m, scopes[0])
        torch.cuda.synchronize()
        m.close()
        return
    out = {"haystack": "configs[2] geonames", "references": n, "limit": LIMIT}

    # preparing 256 stale scopes in one call: one needle a scope, the first call against the next
    one_each = Batch(*W.queries(hay, off, 256, seed=33), dev)
    w256 = torch.from_numpy(np.arange(256, dtype=np.int32)).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    one_each.each_in(m, scopes, w256)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    one_each.each_in(m, scopes, w256)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out["prepare_256_stale"] = {"first_call_ms": round(1e3 * (t1 - t0), 3), "next_call_ms": round(1e3 * (t2 - t1), 3),
                                "prepare_ms": round(1e3 * ((t1 - t0) - (t2 - t1)), 3)}

    # mixed batch
    mixed = _events_ms(lambda: b.each_in(m, scopes, d_which))
    assert m.last_kernels() == ["scope_each_kernel"], m.last_kernels()
    got = b.result()
    one_scope = _events_ms(lambda: b.find_in(m, scopes[0]))

    def serial():
        for j in range(256):
            b.find_in(m, scopes[j], 16 * j, 16 * (j + 1))
    calls = _events_ms(serial)
    want = b.result()
    out["mixed_batch"] = {
        "needles": 4096, "scopes": 256, "members": 1000,
        "each_in_ms": round(mixed, 4), "one_scope_ms": round(one_scope, 4), "serial_256_calls_ms": round(calls, 4),
        "vs_one_scope": round(mixed / one_scope, 3), "speedup_vs_serial": round(calls / mixed, 2),
        "needles_per_s": round(4096 / mixed * 1e3),
        "rows_equal_serial": bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))}
    print(json.dumps(out["mixed_batch"]), file=sys.stderr, flush=True)

    # small host batch: 32 needles over 32 scopes
    small = W.unpack(*W.queries(hay, off, 32, seed=34))
    from blurrily_amd.map import _pack
    sp, so = _pack(small)
    sbuf = np.frombuffer(sp, dtype=np.uint8)
    sw = np.arange(32, dtype=np.uint32)
    r_each, c_each = m.find_batch_each_in(scopes[:32], sw, sbuf, so, LIMIT)
    each_us = _host_us(lambda: m.find_batch_each_in(scopes[:32], sw, sbuf, so, LIMIT), 200)
    singles_us = _host_us(lambda: [m.find_in(scopes[i], small[i], LIMIT) for i in range(32)], 50)
    equal = all(m.find_in(scopes[i], small[i], LIMIT) == r_each[i, :c_each[i]].tolist() for i in range(32))
    out["small_host_batch"] = {"needles": 32, "scopes": 32, "each_in": each_us, "find_in_x32": singles_us,
                               "ratio_p50": round(singles_us["p50_us"] / each_us["p50_us"], 2), "rows_equal": equal}
    print(json.dumps(out["small_host_batch"]), file=sys.stderr, flush=True)

    # preparing 256 stale scopes after a change to the map (their device buffers made already): a put, then the
    # first call against the next
    m.put(b"a string put after the scopes were prepared", n + 1, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    one_each.each_in(m, scopes, w256)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    one_each.each_in(m, scopes, w256)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out["prepare_256_stale_after_put"] = {"first_call_ms": round(1e3 * (t1 - t0), 3),
                                          "next_call_ms": round(1e3 * (t2 - t1), 3),
                                          "prepare_ms": round(1e3 * ((t1 - t0) - (t2 - t1)), 3)}
    m.delete(n + 1)
    print(json.dumps(out["prepare_256_stale_after_put"]), file=sys.stderr, flush=True)

    # blocked self-joins, host clock: the C call (rows as arrays), and for 256 x 10^3 Map.join_within's lists too
    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, time.perf_counter() - t0

    joins = {}
    members = np.concatenate(member_sets)
    which_j = np.repeat(np.arange(256, dtype=np.uint32), 1000)
    RawMap.find_batch_by_reference_each_in(m, scopes, which_j[:1000], members[:1000], LIMIT)       # (warm)
    (_, c256, _), took = timed(lambda: RawMap.find_batch_by_reference_each_in(m, scopes, which_j, members, LIMIT))
    (r, _, _), took_lists = timed(lambda: m.join_within(scopes, LIMIT))
    joins["256x1000"] = {"members": int(len(r)), "call_s": round(took, 4), "members_per_s": round(len(members) / took),
                         "last_kernels": m.last_kernels(), "join_within_with_lists_s": round(took_lists, 4)}
    # a Zipf-sized family of 250 blocks covering the whole map (weights 1 / rank; the largest served through the mask)
    perm = rng.permutation(refs)
    w = 1.0 / np.arange(1, 251)
    cut = np.concatenate([[0], np.round(np.cumsum(w / w.sum()) * n).astype(np.int64)])
    zipf = [np.sort(perm[cut[j]:cut[j + 1]]) for j in range(250)]
    zscopes = [m.scope(z) for z in zipf]
    zmem = np.concatenate(zipf)
    zwhich = np.repeat(np.arange(250, dtype=np.uint32), [len(z) for z in zipf])
    _, took = timed(lambda: RawMap.find_batch_by_reference_each_in(m, zscopes, zwhich, zmem, LIMIT))
    kernels = m.last_kernels()
    _, again = timed(lambda: RawMap.find_batch_by_reference_each_in(m, zscopes, zwhich, zmem, LIMIT))
    codes = [int(m.get_batch(z)[1][-1]) for z in zipf]
    joins["zipf250"] = {"members": int(len(zmem)), "largest_block": int(len(zipf[0])), "smallest_block": int(len(zipf[-1])),
                        "blocks_served_directly_under_auto": int(sum(1 for c, z in zip(codes, zipf)
                                                                     if c <= 150000 and len(z) <= 57344)),
                        "first_call_s": round(took, 4), "call_s": round(again, 4), "members_per_s": round(len(zmem) / again),
                        "kernels": kernels}
    _, took = timed(lambda: RawMap.find_batch_by_reference(m, refs, LIMIT))
    joins["whole_map_self_join_call_s"] = round(took, 4)
    out["blocked_self_join"] = joins
    print(json.dumps(joins), file=sys.stderr, flush=True)
    for sc in zscopes + scopes:
        sc.close()
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    m.close()


if __name__ == "__main__":
    main()
