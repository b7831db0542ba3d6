"""Scoped similarity find at Geonames scale (configs[2]'s haystack).  Host clock around the calls,
best of two after a warm call:

  * against the workaround: blurrily_storage_find_batch_similar at limit 65 535 and the rows filtered to the scope on
    the host (needles whose row count stays below 65 535, so that the workaround is exact), against
    blurrily_storage_find_batch_similar_in, scopes of 10^3 and 10^5 members; the rows compared;
  * direct against mask: 4 096 needles over scopes of 10^2, 10^3, 10^4 and 5 * 10^4 members, each strategy forced;
  * the blocked similarity self-join: 256 blocks of 10^3 members at 700 per mille (join_similar_within's call), beside
    the blocked self-join by matches on the same blocks (join_within's).

Writes the JSON object after every step.  Usage: python tools/scope_similar_probe.py [--scale 1.0] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import workloads as W  # noqa: E402

LIMIT, FLOOR, ALL = 10, 300, 65535


def _ms(dt):
    return round(dt * 1e3, 3)


def _spread(fn):
    """best and worst of two host-clock repetitions after a warm call, ms, and the last result"""
    import time
    fn()
    ts = []
    for _ in range(2):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return {"best_ms": _ms(min(ts)), "worst_ms": _ms(max(ts))}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scope_similar_geonames.json"))
    args = ap.parse_args()
    m, hay, off, refs, t_put, t_sync = W.bench_map("geonames", args.scale)
    rng = np.random.default_rng(7)
    res = {"haystack": "configs[2] geonames", "scale": args.scale, "strings": int(len(refs)), "limit": LIMIT,
           "min_permille": FLOOR, "clock": "host, best of two after a warm call"}
    q, qo = W.queries(hay, off, 4096, 11)
    m.find_batch_similar_packed(q[:int(qo[1])], qo[:2], LIMIT, 0)       # (the first call builds the per-rank table)

    # -- against the workaround ------------------------------------------------------------------------------------
    nq = 48
    q48, qo48 = q[:int(qo[nq])], qo[:nq + 1]
    rows_all, counts_all, ntri_all = m.find_batch_similar_packed(q48, qo48, ALL, FLOOR)
    exact = np.nonzero(counts_all < ALL)[0]                             # the workaround is exact for these only
    starts = qo48[:-1][exact].astype(np.int64)
    lens = (qo48[1:][exact] - qo48[:-1][exact]).astype(np.int64)
    qe = np.concatenate([q48[s:s + k] for s, k in zip(starts, lens)]) if len(exact) else np.zeros(0, np.uint8)
    qeo = np.zeros(len(exact) + 1, dtype=np.uint64)
    qeo[1:] = np.cumsum(lens)
    res["workaround"] = {"needles": int(len(exact)), "needles_cut_at_65535": int(nq - len(exact))}
    del rows_all, counts_all, ntri_all
    for members in (1000, 100000):
        members = min(members, len(refs))
        scope_refs = np.sort(rng.choice(refs, members, replace=False))

        def workaround():
            rows, counts, ntri = m.find_batch_similar_packed(qe, qeo, ALL, FLOOR)
            out = []
            for i, c in enumerate(counts.tolist()):
                keep = np.nonzero(np.isin(rows[i, :c, 0], scope_refs))[0][:LIMIT]
                out.append(np.concatenate([rows[i, keep], ntri[i, keep, None]], axis=1).tolist())
            return out

        with m.scope(scope_refs) as sc:
            t_old, want = _spread(workaround)
            entry = {"workaround": t_old}
            for strategy, name in ((0, "auto"), (1, "mask"), (2, "direct")):
                m.set_option("scope_strategy", strategy)
                t_new, (rows, counts, ntri) = _spread(lambda: m.find_batch_similar_in_packed(sc, qe, qeo, LIMIT, FLOOR))
                got = [np.concatenate([rows[i, :c], ntri[i, :c, None]], axis=1).tolist() for i, c in enumerate(counts.tolist())]
                entry[name] = dict(t_new, kernels=m.last_kernels(), rows_equal=bool(got == want))
            m.set_option("scope_strategy", 0)
        res["workaround"][f"members_{members}"] = entry
        W.dump_json(res, args.out)

    # -- direct against mask -----------------------------------------------------------------------------------------
    res["direct_vs_mask"] = {"needles": 4096}
    for members in (100, 1000, 10000, 50000):
        members = min(members, len(refs))
        scope_refs = rng.choice(refs, members, replace=False)
        entry = {}
        with m.scope(scope_refs) as sc:
            outs = {}
            for strategy, name in ((1, "mask"), (2, "direct")):
                m.set_option("scope_strategy", strategy)
                t, out = _spread(lambda: m.find_batch_similar_in_packed(sc, q, qo, LIMIT, FLOOR))
                entry[name] = dict(t, kernels=m.last_kernels())
                outs[name] = out
            m.set_option("scope_strategy", 0)
            live = np.arange(LIMIT)[None, :] < outs["mask"][1][:, None].astype(np.int64)
            entry["rows_equal"] = bool(np.array_equal(outs["mask"][1], outs["direct"][1]) and
                                       np.array_equal(np.where(live[:, :, None], outs["mask"][0], 0),
                                                      np.where(live[:, :, None], outs["direct"][0], 0)))
            _, _, _, nb = m.find_batch_by_reference_similar_each_in([sc], np.zeros(len(scope_refs), np.uint32), scope_refs, 1, 1000)
            entry["member_codes"] = int(nb.sum())
        res["direct_vs_mask"][f"members_{members}"] = entry
        W.dump_json(res, args.out)
    res["direct_vs_mask"]["scope_direct_max"] = m.get_option("scope_direct_max")

    # -- the blocked similarity self-join ------------------------------------------------------------------------------
    n_blocks, per = 256, min(1000, len(refs) // 256)
    pool = rng.permutation(refs)[:n_blocks * per].reshape(n_blocks, per)
    scopes = [m.scope(b) for b in pool]
    flat = np.concatenate([sc._refs for sc in scopes]).astype(np.uint32)
    which = np.repeat(np.arange(n_blocks, dtype=np.uint32), per)
    t_sim, out = _spread(lambda: m.find_batch_by_reference_similar_each_in(scopes, which, flat, LIMIT, 700))
    k_sim = m.last_kernels()
    t_cnt, _ = _spread(lambda: m.find_batch_by_reference_each_in(scopes, which, flat, LIMIT))
    res["blocked_self_join"] = {"blocks": n_blocks, "members_per_block": per, "min_permille": 700,
                                "similar_each_in": dict(t_sim, kernels=k_sim, rows=int(out[1].sum())),
                                "each_in_by_matches": dict(t_cnt, kernels=m.last_kernels())}
    for sc in scopes:
        sc.close()
    W.dump_json(res, args.out)
    m.close()


if __name__ == "__main__":
    main()
