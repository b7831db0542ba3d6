"""By-reference figures at Geonames scale (configs[2]'s haystack, 8 423 769 strings):

  * single blurrily_storage_get, host clock, p50 / p90 over 300 references at random;
  * extraction of every reference (blurrily_storage_find_references_device at limit 0: the extraction, the per-image
    needle arrays, no sweep), HIP-event time, and the bytes it must read (slice table, postings, bitmaps of every
    window) over that time;
  * the whole-map self-join at limit 10 (find_references_device over all references) against find_batch_device over
    the same references' strings: needles/s of both, and the rows compared;
  * small batches (1, 8, 24 references, limit 10), host clock p50: find by reference -- always the batch path -- against
    the same strings' find / find_batch, which take the single find's copy-free launch.

Prints one JSON object.  Usage: python tools/refs_probe.py [--scale 1.0] [--gets 300] [--extract-only] [--out FILE]
(--extract-only: the whole-map extraction alone, three times -- the run to put under rocprofv3 --kernel-trace --stats,
whose per-kernel averages then describe it)"""
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


def _events_ms(fn, reps=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--gets", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--extract-only", action="store_true")
    args = ap.parse_args()
    m, hay, off, refs, _, sync_s = W.bench_map("geonames", args.scale)
    n = len(refs)
    out = {"haystack": "geonames", "n_refs": n, "build_s": round(sync_s, 2)}
    info = m.device_info()
    out["n_windows"] = info["n_windows"]
    bytes_before = info["device_bytes"]
    lib = _native.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream

    # single get: the first call uploads the reference table
    m.get(1)
    out["ref_table_bytes"] = m.device_info()["device_bytes"] - bytes_before
    rng = np.random.default_rng(1)
    lat = []
    for r in rng.integers(1, n + 1, 0 if args.extract_only else args.gets).tolist():
        t = time.perf_counter()
        m.get(r)
        lat.append((time.perf_counter() - t) * 1e6)
    if lat:
        out["get_p50_us"], out["get_p90_us"] = float(np.percentile(lat, 50)), float(np.percentile(lat, 90))

    # extraction of every reference (limit 0: no sweep)
    d_refs = torch.from_numpy(refs.view(np.int32)).to(dev)
    counts = torch.zeros((n,), dtype=torch.int32, device=dev)
    ntri = torch.zeros((n,), dtype=torch.int32, device=dev)

    def extract():
        assert lib.blurrily_storage_find_references_device(m.handle, d_refs.data_ptr(), n, 0, None, counts.data_ptr(),
                                                           ntri.data_ptr(), stream) == 0, C.get_errno()
    out["extract_all_ms"] = _events_ms(extract)
    # what it must read: every window's slice table row, its postings and bitmaps (the whole image minus side tables)
    read = info["n_windows"] * 21952 * 8 + (info["device_bytes"] - 3 * 4 * n - info["n_windows"] * 21952 * 8)
    out["extract_bytes_read_est"] = int(read)
    out["extract_tb_per_s"] = read / (out["extract_all_ms"] * 1e-3) / 1e12
    out["codes_extracted"] = int(ntri.sum().item())
    if args.extract_only:
        return _emit(out, args.out)

    # small batches: by reference (batch path) against the strings (the single find's launch up to "few_max")
    raw = hay.tobytes()
    for k in (1, 8, 24):
        t_ref, t_str = [], []
        for _ in range(100):
            q = rng.integers(1, n + 1, k).astype(np.uint32)
            strs = [raw[int(off[r - 1]):int(off[r])] for r in q.tolist()]
            t = time.perf_counter()
            rows_b, cnt_b, _ = m.find_batch_by_reference(q, 10)
            t_ref.append((time.perf_counter() - t) * 1e6)
            t = time.perf_counter()
            if k == 1:
                m.find(strs[0], 10)
            else:
                qo = np.zeros(k + 1, dtype=np.uint64)
                qo[1:] = np.cumsum([len(x) for x in strs])
                m.find_batch_packed(np.frombuffer(b"".join(strs), dtype=np.uint8), qo, 10)
            t_str.append((time.perf_counter() - t) * 1e6)
        out[f"by_ref_n{k}_p50_us"] = float(np.percentile(t_ref, 50))
        out[f"strings_n{k}_p50_us"] = float(np.percentile(t_str, 50))

    # whole-map self-join at limit 10, against find_batch_device over the same strings
    limit = 10
    rows_r = torch.zeros((n, limit, 3), dtype=torch.int32, device=dev)
    cnt_r = torch.zeros((n,), dtype=torch.int32, device=dev)

    def join():
        assert lib.blurrily_storage_find_references_device(m.handle, d_refs.data_ptr(), n, limit, rows_r.data_ptr(),
                                                           cnt_r.data_ptr(), None, stream) == 0, C.get_errno()
    join()                                  # (the class's sweep is measured by its first batch)
    out["selfjoin_ms"] = _events_ms(join, reps=2)
    d_packed = torch.from_numpy(hay).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    rows_s = torch.zeros((n, limit, 3), dtype=torch.int32, device=dev)
    cnt_s = torch.zeros((n,), dtype=torch.int32, device=dev)

    def strings():
        assert lib.blurrily_storage_find_batch_device(m.handle, d_packed.data_ptr(), int(off[-1]), d_off.data_ptr(), n,
                                                      limit, rows_s.data_ptr(), cnt_s.data_ptr(), None, stream) == 0
    strings()
    out["strings_ms"] = _events_ms(strings, reps=2)
    out["selfjoin_needles_per_s"] = n / (out["selfjoin_ms"] * 1e-3)
    out["strings_needles_per_s"] = n / (out["strings_ms"] * 1e-3)
    out["selfjoin_vs_strings"] = out["selfjoin_needles_per_s"] / out["strings_needles_per_s"]
    c_r, c_s = cnt_r.cpu().numpy(), cnt_s.cpu().numpy()
    r_r, r_s = rows_r.cpu().numpy(), rows_s.cpu().numpy()
    live = np.arange(limit)[None, :] < c_s[:, None]
    out["rows_equal"] = bool(np.array_equal(c_r, c_s) and
                             np.array_equal(np.where(live[:, :, None], r_r, 0), np.where(live[:, :, None], r_s, 0)))
    _emit(out, args.out)


def _emit(out, path):
    line = json.dumps(out)
    print(line)
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
