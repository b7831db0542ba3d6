"""Scoped threshold find at Geonames scale (configs[2]'s haystack).  Host clock around the calls,
best and worst of two after a warm call:

  * single-scope calls: 41 and 4 096 needles at 700 per mille in scopes of 10^2, 10^3, 10^4 and 5 * 10^4 members --
    direct against mask, each forced, and both against the workaround (blurrily_storage_find_batch_above over the whole
    map, its rows filtered to the scope on the host); the rows compared, the ratios reported;
  * the blocked threshold self-join: 256 blocks of 10^3 members at 700 per mille (join_above_within's call), beside the
    blocked similarity self-join and the blocked self-join by matches on the same blocks.

Writes the JSON object after every step.  Usage: python tools/scope_above_probe.py [--scale 1.0] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import workloads as W  # noqa: E402

BAR, LIMIT = 700, 10


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


def _filter(rows, row_off, scope_sorted):
    """the workaround's host side: the rows whose reference is in the scope, and their offsets"""
    keep = np.isin(rows[:, 0], scope_sorted)
    kept = np.zeros(len(rows) + 1, dtype=np.uint64)
    kept[1:] = np.cumsum(keep)
    return rows[keep], kept[row_off.astype(np.int64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scope_above_geonames.json"))
    args = ap.parse_args()
    m, hay, off, refs, t_put, t_sync = W.bench_map("geonames", args.scale)
    rng = np.random.default_rng(7)
    res = {"haystack": "configs[2] geonames", "scale": args.scale, "strings": int(len(refs)), "min_permille": BAR,
           "clock": "host, best and worst of two after a warm call",
           "scope_direct_max": m.get_option("scope_direct_max")}
    q, qo = W.queries(hay, off, 4096, 11)

    # -- single-scope calls ------------------------------------------------------------------------------------------
    res["single_scope"] = {}
    for nq in (41, 4096):
        qn, qon = q[:int(qo[nq])], qo[:nq + 1]
        t_un, (urows, uoff) = _spread(lambda: m.find_batch_above_packed(qn, qon, 0, BAR))
        block = {"unscoped_call_alone": dict(t_un, rows=int(uoff[-1]))}
        del urows, uoff
        for members in (100, 1000, 10000, 50000):
            members = min(members, len(refs))
            scope_refs = np.sort(rng.choice(refs, members, replace=False))
            entry = {}
            with m.scope(scope_refs) as sc:
                t_old, want = _spread(lambda: _filter(*m.find_batch_above_packed(qn, qon, 0, BAR), scope_refs))
                entry["workaround"] = dict(t_old, rows=int(len(want[0])))
                for strategy, name in ((1, "mask"), (2, "direct"), (0, "auto")):
                    m.set_option("scope_strategy", strategy)
                    t_new, got = _spread(lambda: m.find_batch_above_in_packed(sc, qn, qon, 0, BAR))
                    entry[name] = dict(t_new, kernels=m.last_kernels(),
                                       rows_equal=bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])))
                m.set_option("scope_strategy", 0)
                _, _, nb = m.find_batch_by_reference_above_each_in([sc], np.zeros(members, np.uint32), scope_refs, 0, 1000)
                entry["member_codes"] = int(nb.sum())
            entry["workaround_over_direct"] = round(entry["workaround"]["best_ms"] / entry["direct"]["best_ms"], 1)
            entry["mask_over_direct"] = round(entry["mask"]["best_ms"] / entry["direct"]["best_ms"], 1)
            entry["workaround_over_mask"] = round(entry["workaround"]["best_ms"] / entry["mask"]["best_ms"], 1)
            block[f"members_{members}"] = entry
            res["single_scope"][f"needles_{nq}"] = block
            W.dump_json(res, args.out)

    # -- the blocked threshold self-join ---------------------------------------------------------------------------------
    n_blocks, per = 256, min(1000, len(refs) // 256)
    pool = rng.permutation(refs)[:n_blocks * per].reshape(n_blocks, per)
    scopes = [m.scope(b) for b in pool]
    flat = np.concatenate([sc._refs for sc in scopes]).astype(np.uint32)
    which = np.repeat(np.arange(n_blocks, dtype=np.uint32), per)
    m.find_batch_by_reference_similar_each_in(scopes[:1], which[:1], flat[:1], LIMIT, BAR)   # (builds the per-rank table)
    t_abv, out = _spread(lambda: m.find_batch_by_reference_above_each_in(scopes, which, flat, 0, BAR))
    k_abv = m.last_kernels()
    t_sim, sim = _spread(lambda: m.find_batch_by_reference_similar_each_in(scopes, which, flat, LIMIT, BAR))
    k_sim = m.last_kernels()
    t_cnt, _ = _spread(lambda: m.find_batch_by_reference_each_in(scopes, which, flat, LIMIT))
    res["blocked_self_join"] = {"blocks": n_blocks, "members_per_block": per, "min_permille": BAR,
                                "above_each_in": dict(t_abv, kernels=k_abv, rows=int(out[1][-1])),
                                "similar_each_in_limit10": dict(t_sim, kernels=k_sim, rows=int(sim[1].sum())),
                                "each_in_by_matches_limit10": dict(t_cnt, kernels=m.last_kernels())}
    for sc in scopes:
        sc.close()
    W.dump_json(res, args.out)
    m.close()


if __name__ == "__main__":
    main()
