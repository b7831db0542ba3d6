"""Scoped find on the GPU (scope.hip: scope_prepare / scope_run, kernels/scope.inc): blurrily_storage_find_in and
_find_batch_in[_device] return exactly the unbounded find's rows restricted to the scope's members, truncated to the
limit -- checked against a numpy restatement that is itself anchored on the oracle -- with each strategy forced (mask,
direct) and auto, across scope sizes, limits, needles at the find path's trigram-class boundaries, batch sizes and
entry points, under mutations, and without disturbing the unscoped path's rows, launches or measured choices."""
import ctypes as C

import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, RawMap, _native
from blurrily_amd.map import _pack
from helpers import Oracle
from scope_truth import NUM_CODES, Truth    # noqa: F401

pytestmark = pytest.mark.gpu
STRATEGIES = (0, 1, 2)                # auto, mask, direct
EXACT = (16, 64, 65, 127, 128)       # distinct trigram counts at the find path's class boundaries


def _exact(rng, letters, t):
    while True:
        s = bytes(rng.choice(letters, size=t - 1).tolist())
        if len(Oracle.tokenise(s)) == t:
            return s


def _put(m, t, strings, refs, weights):
    packed, offsets = _pack(strings)
    m.put_many_packed(packed, offsets, np.asarray(refs, dtype=np.uint32), np.asarray(weights, dtype=np.uint32))
    for s, r, w in zip(strings, refs, weights):
        t.put(s, int(r), int(w))


@pytest.fixture(scope="module")
def geo():
    """~300 k strings over five windows, weights at random, references sparse and shuffled, plus needles-to-be of exactly
    16 .. 128 distinct trigrams"""
    hay, off = W.geonames(300000, 50000, 91)
    strings = W.unpack(hay, off)
    rng = np.random.default_rng(92)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    strings += [_exact(rng, letters, t) for t in EXACT for _ in range(2)] + [b"", b"1234 !!", b"a"]
    n = len(strings)
    refs = rng.permutation(np.arange(1, 3 * n, 3, dtype=np.uint32))[:n]
    weights = rng.integers(1, 400, size=n).astype(np.uint32)
    m, t = RawMap(), Truth()
    _put(m, t, strings, refs, weights)
    m.sync_device()
    assert m.device_info()["n_windows"] >= 5
    return m, t, strings, refs


def _needles(strings, rng, n):
    """n needles: stored strings, prefixes, the exact-trigram strings, an empty needle and one without letters"""
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    fixed = [_exact(rng, letters, t) for t in EXACT] + [b"", b"1234 !!"]
    picks = rng.choice(len(strings), size=max(n - len(fixed), 0))
    out = [strings[i][: max(3, len(strings[i]) - int(rng.integers(0, 4)))] for i in picks.tolist()]
    return (fixed + out)[:n]


def _batch_in(m, scope, needles, limit):
    packed, offsets = _pack(needles)
    rows, counts = m.find_batch_in(scope, np.frombuffer(packed, dtype=np.uint8), offsets, limit)
    return rows, counts


def _live(rows, counts):
    """rows past a needle's count are not part of the answer"""
    keep = np.arange(rows.shape[1])[None, :] < counts[:, None].astype(np.int64)
    return np.where(keep[:, :, None], rows, 0)


def _as_lists(rows, counts):
    return [rows[i, :counts[i]].tolist() for i in range(len(counts))]


def _scopes(refs, rng):
    n = len(refs)
    absent = np.arange(2, 3 * n, 3, dtype=np.uint32)[:500]          # never put (references are 1 mod 3)
    return {
        "empty": np.zeros(0, dtype=np.uint32),
        "one": refs[:1],
        "hundred": rng.choice(refs, 100, replace=False),
        "ten_k": np.concatenate([rng.choice(refs, 10000, replace=False), absent[:50]]),
        "half": refs[: n // 2],
        "all": refs,
        "absent": absent,
    }


def test_the_truth_is_the_oracle_when_the_scope_is_everything(geo):
    m, t, strings, refs = geo
    rng = np.random.default_rng(1)
    o = Oracle()
    for r, (s, w) in t.entries.items():
        o.put(s, r, w)
    mem = t.members(refs)
    for nd in _needles(strings, rng, 40):
        for limit in (10, 100):
            assert Truth.rows(mem, nd, limit) == o.find(nd, limit), nd


@pytest.mark.parametrize("scope_name", ["empty", "one", "hundred", "ten_k", "half", "all", "absent"])
def test_rows_equal_the_truth_for_every_strategy_scope_and_limit(geo, scope_name):
    m, t, strings, refs = geo
    rng = np.random.default_rng(2)
    scope_refs = _scopes(refs, rng)[scope_name]
    needles = _needles(strings, rng, 48)
    mem = t.members(scope_refs)
    full = [Truth.rows(mem, nd, 1000) for nd in needles]
    with m.scope(scope_refs) as sc:
        for limit in (1, 10, 120, 121, 1000):
            got = {}
            for strategy in STRATEGIES:
                m.set_option("scope_strategy", strategy)
                rows, counts = _batch_in(m, sc, needles, limit)
                got[strategy] = (rows, counts)
                assert _as_lists(rows, counts) == [f[:limit] for f in full], (scope_name, limit, strategy)
            # mask and direct: byte for byte
            (r1, c1), (r2, c2) = got[1], got[2]
            assert np.array_equal(c1, c2) and np.array_equal(_live(r1, c1), _live(r2, c2))
    m.set_option("scope_strategy", 0)


@pytest.mark.parametrize("n_q", [1, 24, 25, 128, 129, 20000])
def test_batch_sizes_through_the_host_device_and_single_entries(geo, n_q):
    import torch
    m, t, strings, refs = geo
    rng = np.random.default_rng(3 + n_q)
    scope_refs = rng.choice(refs, 2000, replace=False)
    needles = _needles(strings, rng, n_q)
    mem = t.members(scope_refs)
    limit = 10
    want = [Truth.rows(mem, nd, limit) for nd in needles]
    packed, offsets = _pack(needles)
    dev = torch.device("cuda", 0)
    lib = _native.lib()
    default = m.get_option("scope_direct_max")
    with m.scope(scope_refs) as sc:
        for strategy in STRATEGIES:
            m.set_option("scope_strategy", strategy)
            if strategy == 0:
                m.set_option("scope_direct_max", 1 << 30)      # auto takes direct at this size
            rows, counts = m.find_batch_in(sc, np.frombuffer(packed, dtype=np.uint8), offsets, limit)
            assert _as_lists(rows, counts) == want, strategy
            d_packed = torch.from_numpy(np.frombuffer(packed + b"\0", dtype=np.uint8).copy()).to(dev)
            d_off = torch.from_numpy(offsets.astype(np.int64)).to(dev)
            d_rows = torch.zeros((n_q, limit, 3), dtype=torch.int32, device=dev)
            d_counts = torch.zeros((n_q,), dtype=torch.int32, device=dev)
            rc = lib.blurrily_storage_find_batch_in_device(m.handle, sc._h, d_packed.data_ptr(), len(packed),
                                                           d_off.data_ptr(), n_q, limit, d_rows.data_ptr(),
                                                           d_counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, C.get_errno()
            torch.cuda.synchronize()
            assert _as_lists(d_rows.cpu().numpy().view(np.uint32), d_counts.cpu().numpy().view(np.uint32)) == want
            kernels = m.last_kernels()
            assert ("scope_find_kernel" in kernels) == (strategy != 1), (strategy, kernels)
            for i in range(min(n_q, 25)):
                assert m.find_in(sc, needles[i], limit) == want[i], (strategy, needles[i])
    m.set_option("scope_strategy", 0)
    m.set_option("scope_direct_max", default)


def test_auto_scores_small_scopes_directly_and_large_ones_through_the_mask(geo):
    m, t, strings, refs = geo
    default = m.get_option("scope_direct_max")
    assert default > 0
    with m.scope(refs[:300]) as sc:
        m.find_in(sc, strings[0], 10)
        assert m.last_kernels() == ["scope_find_kernel"]
        m.set_option("scope_direct_max", 0)             # auto then always takes the mask
        m.find_in(sc, strings[0], 10)
        assert "scope_find_kernel" not in m.last_kernels()
        m.set_option("scope_direct_max", default)
        m.find_in(sc, strings[0], 300)                  # a limit above the direct strategy's pool
        assert "scope_find_kernel" not in m.last_kernels()
    with m.scope(refs[:50000]) as big:                  # more member codes than the default
        m.find_in(big, strings[0], 10)
        assert "scope_find_kernel" not in m.last_kernels()


def test_mutations_are_seen_by_the_next_scoped_find(tmp_path):
    rng = np.random.default_rng(7)
    hay, off = W.geonames(30000, 5000, 17)
    strings = W.unpack(hay, off)
    n = len(strings)
    refs = np.arange(1, n + 1, dtype=np.uint32)
    weights = rng.integers(1, 50, size=n).astype(np.uint32)
    m, t = RawMap(), Truth()
    _put(m, t, strings, refs, weights)
    m.sync_device()
    scope_refs = np.concatenate([rng.choice(refs, 3000, replace=False), np.array([n + 10, n + 11, n + 12], np.uint32)])
    needles = _needles(strings, rng, 60)
    sc = m.scope(scope_refs)

    def check(what):
        mem = t.members(scope_refs)
        want = [Truth.rows(mem, nd, 20) for nd in needles]
        for strategy in (1, 2):
            m.set_option("scope_strategy", strategy)
            assert _as_lists(*_batch_in(m, sc, needles, 20)) == want, (what, strategy)
            assert m.find_in(sc, needles[7], 20) == want[7], (what, strategy)
        assert sc.members() == len(mem[0])

    check("fresh")
    victims = [int(r) for r in scope_refs[:40]]
    for r in victims:                                  # deleting members
        m.delete(r)
        t.delete(r)
    check("deleted")
    for k, r in enumerate((n + 10, n + 11)):           # members put after the scope was made (pending)
        m.put(strings[k][::-1] + b" new", r, 3)
        t.put(strings[k][::-1] + b" new", r, 3)
    check("pending")
    for r in victims[:10]:                             # deleted and put again, with another string
        s = strings[r % 100] + b" again"
        m.put(s, r, 1)
        t.put(s, r, 1)
    check("re-put")
    bulk = [strings[i] + b" bulk" for i in range(6000)]   # overflows the log: the base is rebuilt
    bulk_refs = list(range(n + 100, n + 100 + len(bulk)))
    before = m.device_info()["base_builds"]
    _put(m, t, bulk, bulk_refs, [2] * len(bulk))
    check("bulk")
    assert m.device_info()["base_builds"] > before
    path = str(tmp_path / "scoped.trigrams")
    m.save(path)
    sc.close()
    m.close()
    m = RawMap.load(path)
    sc = m.scope(scope_refs)
    check("loaded")
    sc.close()
    m.close()


def test_scoped_calls_leave_the_unscoped_path_as_it_was(geo):
    m, t, strings, refs = geo
    rng = np.random.default_rng(11)
    packed, offsets = _pack(_needles(strings, rng, 20000))
    buf = np.frombuffer(packed, dtype=np.uint8)
    for _ in range(2):                                 # (the first batch of a class may measure every sweep)
        rows0, counts0 = m.find_batch_packed(buf, offsets, 10)
    kernels0 = m.last_kernels()
    choice0, tuned0 = m.get_option("ws_choice"), m.get_option("tuned_class")
    with m.scope(rng.choice(refs, 5000, replace=False)) as sc:
        for strategy in STRATEGIES:
            m.set_option("scope_strategy", strategy)
            runs = [m.find_batch_in(sc, buf, offsets, 10) for _ in range(3)]
            for rows, counts in runs[1:]:
                assert np.array_equal(counts, runs[0][1])
                assert np.array_equal(_live(rows, counts), _live(*runs[0]))
        m.set_option("scope_strategy", 1)
        m.find_batch_in(sc, buf, offsets, 64)          # a class the unscoped path has not measured
    m.set_option("scope_strategy", 0)
    assert m.get_option("ws_choice") == choice0 and m.get_option("tuned_class") == tuned0
    rows1, counts1 = m.find_batch_packed(buf, offsets, 10)
    assert m.last_kernels() == kernels0
    assert np.array_equal(counts0, counts1) and np.array_equal(_live(rows0, counts0), _live(rows1, counts1))


def test_map_surface_normalises_and_takes_plain_iterables(geo):
    m, t, strings, refs = geo
    mp = Map()
    mp.put("Saint-Étienne du Rouvray", 10)
    mp.put("saint etienne", 11)
    mp.put("saint malo", 12)
    assert mp.find_in([10, 12], "SAINT Etienne") == [r for r in mp.find("SAINT Etienne") if r[0] in (10, 12)]
    assert mp.find_batch_in({11}, ["saint", "malo"]) == [[r for r in mp.find(s) if r[0] == 11] for s in ("saint", "malo")]
    mp.close()


def test_a_scoped_batch_with_empty_needles_equals_the_single_finds():
    """An empty needle is a valid find (no rows); a batch of nothing but empty needles has no bytes to point to."""
    mp = Map()
    for ref, s in ((1, "san jose"), (2, "san jose california"), (3, "santa cruz")):
        mp.put(s, ref)
    with mp.scope([1, 3]) as held:
        for scope in (held, [1, 3]):
            for needles in (["", "san jose", ""], [""], ["", "", ""], ["  ", "!"]):
                assert mp.find_batch_in(scope, needles) == [mp.find_in(scope, s) for s in needles], needles
        assert mp.find_in(held, "") == [] and mp.find_batch_in(held, ["", "san jose", ""])[1] != []
        rows, counts = RawMap.find_batch_in(mp, held, b"", np.zeros(2, dtype=np.uint64), 10)
        assert rows.shape == (1, 10, 3) and counts.tolist() == [0]
    mp.close()


def test_configs2_scale_every_97th_and_every_997th_reference(geonames_full):
    """configs[2]'s haystack: 4 096 needles within every 97th reference (beyond the direct strategy's size: the mask
    serves both) and every 997th (served directly when forced), the strategies against each other and 256 needles against
    the truth"""
    hay, off = geonames_full.hay, geonames_full.off
    n = len(off) - 1
    m = RawMap()
    m.put_many_packed(hay, off, np.arange(1, n + 1, dtype=np.uint32))
    m.sync_device()
    q, qo = W.queries(hay, off, 4096, seed=5)
    needles = W.unpack(q, qo)
    buf = np.frombuffer(q, dtype=np.uint8) if not isinstance(q, np.ndarray) else q
    for step in (97, 997):
        scope_refs = np.arange(1, n + 1, step, dtype=np.uint32)
        t = Truth()
        for r in scope_refs.tolist():
            t.entries[r] = (bytes(hay[int(off[r - 1]):int(off[r])]), int(off[r] - off[r - 1]))
        mem = t.members(scope_refs)
        with m.scope(scope_refs) as sc:
            got = {}
            for strategy in (1, 2):
                m.set_option("scope_strategy", strategy)
                got[strategy] = m.find_batch_in(sc, buf, qo, 10)
                assert ("scope_find_kernel" in m.last_kernels()) == (strategy == 2 and step == 997)
            assert np.array_equal(got[1][1], got[2][1]) and np.array_equal(_live(*got[1]), _live(*got[2]))
            rows, counts = got[1]
            for i in range(256):
                assert rows[i, :counts[i]].tolist() == Truth.rows(mem, needles[i], 10), (step, i)
    m.set_option("scope_strategy", 0)
    m.close()
