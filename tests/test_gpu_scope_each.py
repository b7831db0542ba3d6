"""A scope per needle on the GPU (scope.hip: each_plan / each_run, kernels/scope.inc: scope_each_kernel):
blurrily_storage_find_batch_each_in[_device] and _find_references_each_in return, for needle i, exactly what find_in
in scopes[which[i]] -- or find, for BLURRILY_NO_SCOPE -- returns for that needle alone.  Checked against a numpy
restatement anchored on the oracle, against find_in and find_batch, with each strategy forced and auto, across a family
of scopes, limits and needles at the find path's class boundaries; every directly served needle in one launch; by
reference and the blocked self-join; under mutations; the device form; the unscoped path left as it was; configs[2]."""
import ctypes as C

import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, RawMap, _native
from blurrily_amd.map import _pack
from helpers import Oracle

pytestmark = pytest.mark.gpu
NUM_CODES = 28 * 28 * 28
NO = None                             # which[i]: the whole map
STRATEGIES = (0, 1, 2)                # auto, mask, direct
EXACT = (16, 64, 65, 127, 128)        # distinct trigram counts at the find path's class boundaries


def _exact(rng, letters, t):
    while True:
        s = bytes(rng.choice(letters, size=t - 1).tolist())
        if len(Oracle.tokenise(s)) == t:
            return s


class Truth:
    """The map's contents (reference -> (string, weight)) and the scoped find restated in numpy: a member's matches are
    the needle's distinct codes among its own; rows by (matches desc, weight asc, reference asc), matches >= 1."""

    def __init__(self):
        self.entries = {}
        self._mem = {}

    def put(self, s, ref, weight):
        if ref not in self.entries:
            self.entries[ref] = (s, weight if weight else len(s))
            self._mem.clear()

    def delete(self, ref):
        if self.entries.pop(ref, None) is not None:
            self._mem.clear()

    def members(self, scope):
        key = None if scope is None else tuple(sorted({int(r) for r in scope}))
        if key in self._mem:
            return self._mem[key]
        refs = sorted(self.entries) if key is None else [r for r in key if r in self.entries]
        codes = [Oracle.tokenise(self.entries[r][0]) for r in refs]
        lens = np.array([len(c) for c in codes], dtype=np.int64)
        flat = np.array([c for cs in codes for c in cs], dtype=np.int64)
        starts = np.zeros(len(refs), dtype=np.int64)
        if len(refs):
            starts[1:] = np.cumsum(lens)[:-1]
        self._mem[key] = (np.array(refs, dtype=np.int64), np.array([self.entries[r][1] for r in refs], dtype=np.int64),
                          flat, starts)
        return self._mem[key]

    @staticmethod
    def rows(mem, needle, limit, codes=None):
        refs, weights, flat, starts = mem
        if len(refs) == 0 or limit == 0:
            return []
        mask = np.zeros(NUM_CODES, dtype=bool)
        mask[Oracle.tokenise(needle) if codes is None else codes] = True
        matches = np.add.reduceat(mask[flat].astype(np.int64), starts)
        keep = np.nonzero(matches >= 1)[0]
        order = keep[np.lexsort((refs[keep], weights[keep], -matches[keep]))][:limit]
        return [[int(refs[i]), int(matches[i]), int(weights[i])] for i in order]


def _put(m, t, strings, refs, weights):
    packed, offsets = _pack(strings)
    m.put_many_packed(packed, offsets, np.asarray(refs, dtype=np.uint32), np.asarray(weights, dtype=np.uint32))
    for s, r, w in zip(strings, refs, weights):
        t.put(s, int(r), int(w))


@pytest.fixture(scope="module")
def geo():
    """(restated from tests/test_gpu_scope.py) ~300 k strings over five windows, weights at random, references sparse
    and shuffled, needles-to-be of exactly 16 .. 128 distinct trigrams -- and here one string of more than 255"""
    hay, off = W.geonames(300000, 50000, 91)
    strings = W.unpack(hay, off)
    rng = np.random.default_rng(92)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    strings += [_exact(rng, letters, t) for t in EXACT for _ in range(2)] + [b"", b"1234 !!", b"a"]
    strings += [_exact(rng, letters, 300)]
    n = len(strings)
    refs = rng.permutation(np.arange(1, 3 * n, 3, dtype=np.uint32))[:n]
    weights = rng.integers(1, 400, size=n).astype(np.uint32)
    m, t = RawMap(), Truth()
    _put(m, t, strings, refs, weights)
    m.sync_device()
    assert m.device_info()["n_windows"] >= 5
    return m, t, strings, refs


def _needles(strings, rng, n):
    """n needles: the exact-trigram strings, an empty needle, one without letters, then stored strings and prefixes"""
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    fixed = [_exact(rng, letters, t) for t in EXACT] + [b"", b"1234 !!"]
    picks = rng.choice(len(strings), size=max(n - len(fixed), 0))
    out = [strings[i][: max(3, len(strings[i]) - int(rng.integers(0, 4)))] for i in picks.tolist()]
    return (fixed + out)[:n]


def _family(refs, rng):
    """the scope family the issue names, as reference lists (the last one is the same handle twice, see _handles)"""
    n = len(refs)
    absent = np.arange(2, 3 * n, 3, dtype=np.uint32)[:300]          # never put (references are 1 mod 3)
    thousand = rng.choice(refs, 1000, replace=False)
    wide = np.concatenate([refs[-1:], rng.choice(refs, 200, replace=False)])   # refs[-1]: the 300-trigram string
    return [
        np.zeros(0, dtype=np.uint32),                               # 0 empty
        absent,                                                     # 1 no held member
        refs[:1],                                                   # 2 one member
        rng.choice(refs, 100, replace=False),                       # 3 ~10^2
        thousand,                                                   # 4 ~10^3
        rng.choice(refs, 16000, replace=False),                     # 5 above scope_direct_max's codes
        wide,                                                       # 6 a member of > 255 trigrams: no direct form
        np.concatenate([thousand[:600], rng.choice(refs, 400, replace=False)]),   # 7 overlaps 4
    ]


def _handles(m, family):
    scopes = [m.scope(f) for f in family]
    return scopes + [scopes[4]]                                     # 8: the same handle as 4


def _live(rows, counts):
    keep = np.arange(rows.shape[1])[None, :] < counts[:, None].astype(np.int64)
    return np.where(keep[:, :, None], rows, 0)


def _as_lists(rows, counts):
    return [rows[i, :counts[i]].tolist() for i in range(len(counts))]


def _expect(t, family_refs, which, needles, limit):
    out = []
    for nd, w in zip(needles, which):
        out.append(Truth.rows(t.members(None if w is None else family_refs[w]), nd, limit))
    return out


def test_the_truth_is_the_oracle_for_the_whole_map():
    rng = np.random.default_rng(1)
    hay, off = W.geonames(3000, 500, 5)
    strings = W.unpack(hay, off)
    t, o = Truth(), Oracle()
    for r, s in enumerate(strings, 1):
        t.put(s, r, 0)
        o.put(s, r, 0)
    mem = t.members(None)
    for nd in _needles(strings, rng, 30):
        for limit in (10, 300):
            assert Truth.rows(mem, nd, limit) == o.find(nd, limit), nd


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_rows_equal_the_truth_find_in_and_find_batch(geo, strategy):
    m, t, strings, refs = geo
    rng = np.random.default_rng(10 + strategy)
    family = _family(refs, rng)
    fam = family + [family[4]]
    scopes = _handles(m, family)
    needles = _needles(strings, rng, 90)
    which = [NO if k % 10 == 9 else int(k % len(scopes)) for k in range(len(needles))]
    rng.shuffle(which)
    full = _expect(t, fam, which, needles, 1000)
    packed, offsets = _pack(needles)
    buf = np.frombuffer(packed, dtype=np.uint8)
    m.set_option("scope_strategy", strategy)
    try:
        for limit in (1, 10, 256, 257, 1000):
            rows, counts = m.find_batch_each_in(scopes, which, buf, offsets, limit)
            got = _as_lists(rows, counts)
            for i in range(len(needles)):
                assert got[i] == full[i][:limit], (strategy, limit, i, which[i])
            # each needle alone: find_in for a scoped one, find_batch for the whole map's
            for i in range(0, len(needles), 7):
                if which[i] is None:
                    continue
                assert m.find_in(scopes[which[i]], needles[i], limit) == got[i], (strategy, limit, i)
            lone = [i for i in range(len(needles)) if which[i] is None]
            p1, o1 = _pack([needles[i] for i in lone])
            r1, c1 = m.find_batch_packed(np.frombuffer(p1, dtype=np.uint8), o1, limit)
            assert _as_lists(r1, c1) == [got[i] for i in lone], (strategy, limit)
    finally:
        m.set_option("scope_strategy", 0)
        for sc in scopes[:-1]:
            sc.close()


def test_every_direct_needle_is_one_launch(geo):
    m, t, strings, refs = geo
    rng = np.random.default_rng(20)
    blocks = [rng.choice(refs[:-1], int(rng.integers(1, 400)), replace=False) for _ in range(80)]   # (no 300-trigram member)
    scopes = [m.scope(b) for b in blocks]
    try:
        for n_q in (24, 600):                                   # the pinned page's path, then the copies'
            needles = _needles(strings, rng, n_q)
            which = rng.integers(0, len(scopes), size=n_q).astype(np.uint32)
            packed, offsets = _pack(needles)
            rows, counts = m.find_batch_each_in(scopes, which, np.frombuffer(packed, dtype=np.uint8), offsets, 10)
            assert m.last_kernels() == ["scope_each_kernel"], n_q
            want = _expect(t, blocks, which.tolist(), needles, 10)
            assert _as_lists(rows, counts) == want, n_q
    finally:
        for sc in scopes:
            sc.close()


def test_by_reference_equals_the_strings_and_the_blocked_self_join(geo):
    m, t, strings, refs = geo
    rng = np.random.default_rng(30)
    family = _family(refs, rng)
    fam = family + [family[4]]
    scopes = _handles(m, family)
    try:
        asked = np.concatenate([rng.choice(refs, 150, replace=False), np.array([2, 5, 3 * len(refs) + 7], np.uint32)])
        which = [NO if k % 9 == 0 else int(rng.integers(0, len(scopes))) for k in range(len(asked))]
        for strategy in STRATEGIES:
            m.set_option("scope_strategy", strategy)
            for limit in (10, 300):
                rows, counts, ntri = m.find_batch_by_reference_each_in(scopes, which, asked, limit)
                held = [int(r) in t.entries for r in asked.tolist()]
                assert [int(x) for x in ntri] == [len(Oracle.tokenise(t.entries[int(r)][0])) if h else 0
                                                  for r, h in zip(asked.tolist(), held)]
                s_needles = [t.entries[int(r)][0] if h else b"" for r, h in zip(asked.tolist(), held)]
                s_rows, s_counts = m.find_batch_each_in(scopes, which, np.frombuffer(_pack(s_needles)[0], np.uint8),
                                                        _pack(s_needles)[1], limit)
                got = _as_lists(rows, counts)
                want = _as_lists(s_rows, s_counts)
                for i, h in enumerate(held):
                    assert got[i] == (want[i] if h else []), (strategy, limit, i)
                    if h and i % 5 == 0:
                        codes = Oracle.tokenise(t.entries[int(asked[i])][0])
                        w = which[i]
                        assert got[i] == Truth.rows(t.members(None if w is None else fam[w]), b"", limit, codes)
        m.set_option("scope_strategy", 0)
        blocks = [rng.choice(refs, 300, replace=False) for _ in range(6)] + [family[1], family[6]]
        got_refs, got_which, got_rows = m.join_within(blocks, 10)
        k = 0
        for j, b in enumerate(blocks):
            mem = t.members(b)
            for r in mem[0].tolist():
                assert int(got_refs[k]) == r and int(got_which[k]) == j
                assert got_rows[k] == Truth.rows(mem, t.entries[r][0], 10), (j, r)
                k += 1
        assert k == len(got_refs)
    finally:
        m.set_option("scope_strategy", 0)
        for sc in scopes[:-1]:
            sc.close()


def test_mutations_between_calls_prepare_stale_scopes_again():
    rng = np.random.default_rng(40)
    hay, off = W.geonames(30000, 5000, 17)
    strings = W.unpack(hay, off)
    n = len(strings)
    refs = np.arange(1, n + 1, dtype=np.uint32)
    weights = rng.integers(1, 50, size=n).astype(np.uint32)
    m, t = RawMap(), Truth()
    _put(m, t, strings, refs, weights)
    m.sync_device()
    family = [np.concatenate([rng.choice(refs, 500, replace=False), np.array([n + 10 + j], np.uint32)])
              for j in range(12)]
    scopes = [m.scope(f) for f in family]
    needles = _needles(strings, rng, 60)
    which = [NO if k % 6 == 5 else k % len(scopes) for k in range(len(needles))]
    packed, offsets = _pack(needles)
    buf = np.frombuffer(packed, dtype=np.uint8)

    def check(what):
        want = _expect(t, family, which, needles, 20)
        for strategy in (1, 2):
            m.set_option("scope_strategy", strategy)
            assert _as_lists(*m.find_batch_each_in(scopes, which, buf, offsets, 20)) == want, (what, strategy)

    check("fresh")
    victims = [int(r) for f in family[:4] for r in f[:5]]
    for r in victims:                                          # deleting members
        m.delete(r)
        t.delete(r)
    check("deleted")
    for j in range(3):                                         # members put after the scopes were made (pending)
        s = strings[j][::-1] + b" new"
        m.put(s, n + 10 + j, 3)
        t.put(s, n + 10 + j, 3)
    check("put")
    for r in victims[:6]:                                      # deleted and put again, with another string
        s = strings[r % 100] + b" again"
        m.put(s, r, 1)
        t.put(s, r, 1)
    check("re-put")
    bulk = [strings[i] + b" bulk" for i in range(6000)]       # past the log's budget: the log is folded
    before = m.device_info()["base_builds"]
    _put(m, t, bulk, list(range(n + 100, n + 100 + len(bulk))), [2] * len(bulk))
    check("folded")
    assert m.device_info()["base_builds"] > before
    m.set_option("scope_strategy", 0)
    for sc in scopes:
        sc.close()
    m.close()


def test_a_small_plan_with_pending_puts_by_strings_and_by_reference_in_every_shape():
    """ the each-in's plan upload and needle carrier with the delta masks live: 300 references and
    five pending puts, a scope of three members, one holding a member of 256 trigrams (it declines direct), one of unheld
    references, an unscoped needle -- as a plan of both kinds with the empty scope and NO_SCOPE in the call, of swept
    groups only (the mask forced) and of direct needles only (24 needles at limit 256: past the pinned page)."""
    rng = np.random.default_rng(71)
    strings = W.unpack(*W.geonames(300, 60, 19)) + [_exact(rng, np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8), 256)]
    n = len(strings)
    m, t = RawMap(), Truth()
    _put(m, t, strings, np.arange(1, n + 1, dtype=np.uint32), rng.integers(1, 50, size=n).astype(np.uint32))
    m.sync_device()
    family = [np.array([3, 4, n + 1], np.uint32), np.array([n, 10, 11, 12, n + 2], np.uint32),
              np.arange(10 ** 6, 10 ** 6 + 4, dtype=np.uint32)]    # three members; the 256-trigram member; unheld
    scopes = [m.scope(f) for f in family]
    for k in range(5):                                     # pending: n + 1 in `three`, n + 2 in `wide`, three in neither
        m.put(strings[k] + b" late", n + 1 + k, 2)
        t.put(strings[k] + b" late", n + 1 + k, 2)
    needles = [strings[0], strings[1], strings[2], strings[2], strings[3], strings[9], strings[n - 1], strings[2]] * 3
    by = [3, n + 1, n, 10, n + 3, n + 3, 10 ** 6, 4] * 3
    both, direct_only = [0, 1, 0, 1, NO, 1, 2, NO] * 3, [0] * 24
    # (a pending put outside both scopes matches needles asked within them: only the delta mask keeps it out)
    assert n + 3 in [r[0] for r in Truth.rows(t.members(None), strings[2], 256)]
    packed, offsets = _pack(needles)
    buf = np.frombuffer(packed, dtype=np.uint8)
    try:
        for strategy, which, each in ((0, both, True), (1, both, False), (0, direct_only, True)):
            m.set_option("scope_strategy", strategy)
            for limit in (10, 256):
                got = _as_lists(*m.find_batch_each_in(scopes, which, buf, offsets, limit))
                names = m.last_kernels()
                assert names == ["scope_each_kernel"] if which is direct_only else \
                    ("scope_each_kernel" in names) == each and len(names) > each, (strategy, names)
                assert got == _expect(t, family, which, needles, limit), (strategy, limit)
                rows, counts, ntri = m.find_batch_by_reference_each_in(scopes, which, by, limit)
                codes = [Oracle.tokenise(t.entries[r][0]) if r in t.entries else None for r in by]
                assert ntri.tolist() == [len(c) if c is not None else 0 for c in codes]
                assert _as_lists(rows, counts) == [
                    [] if c is None else Truth.rows(t.members(None if w is None else family[w]), b"", limit, c)
                    for c, w in zip(codes, which)], (strategy, limit)
    finally:
        m.set_option("scope_strategy", 0)
        for sc in scopes:
            sc.close()
        m.close()


def test_the_device_form_equals_the_host_form_on_another_stream(geo):
    import torch
    m, t, strings, refs = geo
    rng = np.random.default_rng(50)
    family = _family(refs, rng)
    scopes = _handles(m, family)
    lib = _native.lib()
    try:
        needles = _needles(strings, rng, 300)
        which = np.array([_native.NO_SCOPE if k % 8 == 0 else k % len(scopes) for k in range(len(needles))], np.uint32)
        packed, offsets = _pack(needles)
        limit = 12
        host = m.find_batch_each_in(scopes, which, np.frombuffer(packed, dtype=np.uint8), offsets, limit)
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            d_packed = torch.from_numpy(np.frombuffer(packed + b"\0", dtype=np.uint8).copy()).to(dev)
            d_off = torch.from_numpy(offsets.astype(np.int64)).to(dev)
            d_which = torch.from_numpy(which.view(np.int32).copy()).to(dev)
            d_rows = torch.zeros((len(needles), limit, 3), dtype=torch.int32, device=dev)
            d_counts = torch.zeros((len(needles),), dtype=torch.int32, device=dev)
            hs = (C.c_void_p * len(scopes))(*[sc._h.value for sc in scopes])
            rc = lib.blurrily_storage_find_batch_each_in_device(m.handle, hs, len(scopes), d_which.data_ptr(),
                                                                d_packed.data_ptr(), len(packed), d_off.data_ptr(),
                                                                len(needles), limit, d_rows.data_ptr(),
                                                                d_counts.data_ptr(), side.cuda_stream)
            assert rc == 0, C.get_errno()
        side.synchronize()
        got = (d_rows.cpu().numpy().view(np.uint32), d_counts.cpu().numpy().view(np.uint32))
        assert np.array_equal(got[1], host[1]) and np.array_equal(_live(*got), _live(*host))
    finally:
        for sc in scopes[:-1]:
            sc.close()


def test_each_in_calls_leave_the_unscoped_path_as_it_was(geo):
    m, t, strings, refs = geo
    rng = np.random.default_rng(60)
    packed, offsets = _pack(_needles(strings, rng, 20000))
    buf = np.frombuffer(packed, dtype=np.uint8)
    for _ in range(2):                                         # (the first batch of a class may measure every sweep)
        rows0, counts0 = m.find_batch_packed(buf, offsets, 10)
    kernels0 = m.last_kernels()
    choice0, tuned0 = m.get_option("ws_choice"), m.get_option("tuned_class")
    family = _family(refs, rng)
    scopes = _handles(m, family)
    which = rng.integers(0, len(scopes), size=len(offsets) - 1).astype(np.uint32)
    try:
        for strategy in STRATEGIES:
            m.set_option("scope_strategy", strategy)
            for limit in (10, 64):
                m.find_batch_each_in(scopes, which, buf, offsets, limit)
    finally:
        m.set_option("scope_strategy", 0)
        for sc in scopes[:-1]:
            sc.close()
    assert m.get_option("ws_choice") == choice0 and m.get_option("tuned_class") == tuned0
    rows1, counts1 = m.find_batch_packed(buf, offsets, 10)
    assert m.last_kernels() == kernels0
    assert np.array_equal(counts0, counts1) and np.array_equal(_live(rows0, counts0), _live(rows1, counts1))


def test_map_surface_normalises_and_joins_within_blocks():
    mp = Map()
    mp.put("Saint-Étienne du Rouvray", 10)
    mp.put("saint etienne", 11)
    mp.put("saint malo", 12)
    mp.put("saint etienne", 13)
    with mp.scope([10, 12]) as a:
        got = mp.find_batch_each_in([a, {11, 13}], [0, 1, None], ["SAINT Etienne", "Saint", "saint malo"])
        assert got == [mp.find_in([10, 12], "SAINT Etienne"), mp.find_in([11, 13], "Saint"), mp.find("saint malo")]
        with pytest.raises(ValueError):
            mp.find_batch_each_in([a], [0, 0], ["saint"])               # which of the wrong length
        refs, which, rows = mp.join_within([a, [11, 13, 99]])
        assert refs.tolist() == [10, 12, 11, 13] and which.tolist() == [0, 0, 1, 1]
        within = [(10, {10, 12}), (12, {10, 12}), (11, {11, 13}), (13, {11, 13})]     # find_by_reference in the block
        assert rows == [[r for r in mp.find_by_reference(ref, 100) if r[0] in block][:10] for ref, block in within]
    mp.close()


def test_an_each_in_batch_with_empty_needles_equals_the_single_finds():
    """An empty needle is a valid find (no rows); a batch of nothing but empty needles has no bytes to point to."""
    mp = Map()
    for ref, s in ((1, "san jose"), (2, "san jose california"), (3, "santa cruz")):
        mp.put(s, ref)
    with mp.scope([1, 3]) as held:
        for scope in (held, [1, 3]):
            for needles in (["", "san jose", ""], [""], ["", "", ""], ["  ", "!"]):
                n = len(needles)
                assert mp.find_batch_each_in([scope], [0] * n, needles) == [mp.find_in(scope, s) for s in needles]
                which = [None if i % 2 else 1 for i in range(n)]
                assert mp.find_batch_each_in([[2], scope], which, needles) == \
                    [mp.find(s) if w is None else mp.find_in(scope, s) for s, w in zip(needles, which)], needles
        assert mp.find_batch_each_in([held], [0, 0, 0], ["", "san jose", ""])[1] != []
        rows, counts = RawMap.find_batch_each_in(mp, [held], [0], b"", np.zeros(2, dtype=np.uint64), 10)
        assert rows.shape == (1, 10, 3) and counts.tolist() == [0]
    mp.close()


def test_configs2_scale_100k_needles_over_1000_blocks(geonames_full):
    """configs[2]'s haystack: every 8th reference in 1 000 blocks, 100 000 needles each in a block at random (a tenth
    with no scope); 200 needles from 20 blocks against the restatement"""
    hay, off = geonames_full.hay, geonames_full.off
    n = len(off) - 1
    m = RawMap()
    m.put_many_packed(hay, off, np.arange(1, n + 1, dtype=np.uint32))
    m.sync_device()
    rng = np.random.default_rng(70)
    blocks = np.array_split(np.arange(1, n + 1, 8, dtype=np.uint32), 1000)
    q, qo = W.queries(hay, off, 100000, seed=71)
    needles = W.unpack(q, qo)
    which = rng.integers(0, len(blocks), size=len(needles)).astype(np.uint32)
    which[rng.random(len(needles)) < 0.1] = _native.NO_SCOPE
    buf = np.frombuffer(q, dtype=np.uint8) if not isinstance(q, np.ndarray) else q
    scopes = [m.scope(b) for b in blocks]
    try:
        rows, counts = m.find_batch_each_in(scopes, which, buf, qo, 10)
        for b in rng.choice(len(blocks), 20, replace=False).tolist():
            t = Truth()
            for r in blocks[b].tolist():
                t.entries[r] = (bytes(hay[int(off[r - 1]):int(off[r])]), int(off[r] - off[r - 1]))
            mem = t.members(blocks[b])
            for i in np.nonzero(which == b)[0][:10].tolist():
                assert rows[i, :counts[i]].tolist() == Truth.rows(mem, needles[i], 10), (b, i)
        lone = np.nonzero(which == _native.NO_SCOPE)[0][:64]
        p1, o1 = _pack([needles[i] for i in lone.tolist()])
        r1, c1 = m.find_batch_packed(np.frombuffer(p1, dtype=np.uint8), o1, 10)
        assert _as_lists(r1, c1) == [rows[i, :counts[i]].tolist() for i in lone.tolist()]
    finally:
        for sc in scopes:
            sc.close()
        m.close()
