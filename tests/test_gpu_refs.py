"""By reference on the GPU (refs.hip: refs_extract, kernels/refs.inc): blurrily_storage_get gives a stored reference's
weight and exactly the tokeniser's codes of the string it was put with, and blurrily_storage_find_references gives, for
every reference, exactly the oracle's find of that string -- across batch sizes that cross every find path, limits of
one pass and of several, needles of 1 to more than 127 trigrams, duplicates and absent references, weights that bear no
relation to string lengths, and a map under pending puts, deletes, re-puts and a save / load round trip."""
import ctypes as C

import numpy as np
import pytest

import workloads as W
from blurrily_amd import Map, RawMap, _native
from blurrily_amd.map import _pack
from helpers import Oracle

pytestmark = pytest.mark.gpu
WINDOW = 65520                        # ranks per window (device_index.h: kWindowRanks)


def _ranks(refs, weights):
    """rank of every reference: (weight, reference) ascending (device_index.h)"""
    order = np.lexsort((refs, weights))
    rank = np.empty(len(refs), dtype=np.int64)
    rank[order] = np.arange(len(refs))
    return rank


EXACT = (16, 64, 65, 127, 128)       # distinct trigram counts at the find path's class boundaries (_extra_strings)


def _exact(rng, letters, t):
    """a string of exactly `t` distinct trigrams: t - 1 letters whose trigrams do not repeat"""
    while True:
        s = bytes(rng.choice(letters, size=t - 1).tolist())
        if len(Oracle.tokenise(s)) == t:
            return s


def _extra_strings(rng):
    """strings of exactly EXACT distinct trigrams, long ones (more than 64, more than 127 distinct trigrams), an empty
    one (one trigram), one without letters"""
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    out = [_exact(rng, letters, t) for t in EXACT for _ in range(3)]
    for n_words in (14, 22, 30, 45, 60):
        words = [bytes(rng.choice(letters, size=int(rng.integers(3, 9))).tolist()) for _ in range(n_words)]
        out.append(b" ".join(words))
    return out + [b"", b"1234 !!", b"a", b"ab"]


@pytest.fixture(scope="module")
def geo():
    """~300 k strings over five windows, weights at random (unrelated to lengths), references sparse and shuffled"""
    hay, off = W.geonames(300000, 50000, 81)
    strings = W.unpack(hay, off)
    rng = np.random.default_rng(82)
    strings += _extra_strings(rng)
    n = len(strings)
    refs = rng.permutation(np.arange(1, 3 * n, 3, dtype=np.uint32))[:n]
    weights = rng.integers(1, 400, size=n).astype(np.uint32)
    m, o = RawMap(), Oracle()
    packed, offsets = _pack(strings)
    m.put_many_packed(packed, offsets, refs, weights)
    for s, r, w in zip(strings, refs.tolist(), weights.tolist()):
        o.put(s, r, w)
    m.sync_device()
    assert m.device_info()["n_windows"] == 5
    return m, o, strings, refs, weights


def _check_get(m, strings, refs, weights, idx):
    w, offs, codes = m.get_batch(refs[idx])
    for k, i in enumerate(idx.tolist()):
        want = Oracle.tokenise(strings[i])
        got = codes[int(offs[k]):int(offs[k + 1])].tolist()
        assert got == want and w[k] == weights[i], (i, strings[i], got, want, int(w[k]), int(weights[i]))


def test_get_parity_two_windows_random_and_window_edges(geo):
    m, o, strings, refs, weights = geo
    rank = _ranks(refs, weights)
    rng = np.random.default_rng(83)
    two = np.nonzero((rank // WINDOW == 1) | (rank // WINDOW == 4))[0]
    _check_get(m, strings, refs, weights, two)
    _check_get(m, strings, refs, weights, rng.choice(len(refs), 10000, replace=False))
    edges = []
    for w in range(5):
        in_w = np.nonzero(rank // WINDOW == w)[0]
        edges += [in_w[np.argmin(rank[in_w])], in_w[np.argmax(rank[in_w])]]
    edges = np.array(edges)
    _check_get(m, strings, refs, weights, edges)
    # the single call, at the edges and for the short / empty strings at the end
    for i in edges.tolist() + list(range(len(strings) - 9, len(strings))):
        got = m.get(int(refs[i]))
        assert got == (int(weights[i]), Oracle.tokenise(strings[i])), (i, strings[i])
    # absent references (the map's are 1 mod 3), mixed with present ones and duplicates
    absent = np.array([2, 3, 5, 0, 0xFFFFFFFF], dtype=np.uint32)
    mixed = np.concatenate([absent, refs[edges[:3]], refs[edges[:3]]])
    w, offs, codes = m.get_batch(mixed)
    lens = np.diff(offs.astype(np.int64))
    assert (lens[:5] == 0).all() and (w[:5] == 0).all()
    for k in range(3):
        want = Oracle.tokenise(strings[edges[k]])
        for at in (5 + k, 8 + k):
            assert codes[int(offs[at]):int(offs[at + 1])].tolist() == want
    for r in absent.tolist():
        assert m.get(r) is None
    # a caller's buffer too small: ERANGE, the size needed in code_offsets[n]
    lib = _native.lib()
    q = np.ascontiguousarray(refs[:100])
    ww = np.zeros(100, dtype=np.uint32)
    oo = np.zeros(101, dtype=np.uint64)
    cc = np.zeros(10, dtype=np.uint16)
    assert lib.blurrily_storage_get_batch(m.handle, q.ctypes.data, 100, ww.ctypes.data, oo.ctypes.data, cc.ctypes.data, 10) == -1
    assert C.get_errno() == 34
    assert int(oo[100]) == sum(len(Oracle.tokenise(strings[i])) for i in range(100))


def test_get_on_one_window_with_dense_slices():
    """dense_min lowered: many slices exist as bitmaps, and the extraction reads them (not their postings)"""
    hay, off = W.words(40000, 84)
    strings = W.unpack(hay, off)
    m = RawMap()
    m.set_option("dense_min", 64)
    refs = np.arange(1, len(strings) + 1, dtype=np.uint32)
    m.put_many_packed(hay, off, refs)
    m.sync_device()
    info = m.device_info()
    assert info["n_windows"] == 1 and info["n_bitmaps"] > 50, info
    _check_get(m, strings, refs, np.array([len(s) for s in strings], dtype=np.uint32), np.arange(len(strings)))


def _compare(m, o, strings, refs, idx, limit, expect=None):
    """find_references(refs[idx]) against the oracle finding each reference's string; idx -1: an absent reference"""
    q = np.array([refs[i] if i >= 0 else 2 for i in idx], dtype=np.uint32)
    rows, counts, ntri = m.find_batch_by_reference(q, limit)
    needles = [strings[i] if i >= 0 else None for i in idx]
    present = [k for k, nd in enumerate(needles) if nd is not None]
    packed, offsets = _pack([needles[k] for k in present])
    want = o.batch(np.frombuffer(packed, dtype=np.uint8), offsets, limit=limit, ntri=True)
    for j, k in enumerate(present):
        c = int(want["counts"][j])
        assert int(counts[k]) == c and int(ntri[k]) == int(want["ntri"][j]), (k, needles[k], int(counts[k]), c)
        assert np.array_equal(rows[k, :c], want["rows"][j, :c]), (k, needles[k], rows[k, :c].tolist(), want["rows"][j, :c].tolist())
    for k, nd in enumerate(needles):
        if nd is None:
            assert counts[k] == 0 and ntri[k] == 0
    return rows, counts


@pytest.mark.parametrize("n_q", [1, 24, 25, 128, 129, 20000])
def test_find_references_parity_across_batch_sizes(geo, n_q):
    m, o, strings, refs, weights = geo
    rng = np.random.default_rng(85 + n_q)
    idx = rng.choice(len(refs), n_q, replace=False).tolist()
    if n_q >= 24:                      # long needles, duplicates and absent references inside the batch
        long_ones = list(range(len(strings) - 9, len(strings) - 4))
        idx[:len(long_ones)] = long_ones
        idx[-3:] = [idx[0], -1, idx[1]]
    _compare(m, o, strings, refs, idx, 10)


@pytest.mark.parametrize("limit", [1, 10, 100, 121, 300])
def test_find_references_parity_across_limits(geo, limit):
    m, o, strings, refs, weights = geo
    rng = np.random.default_rng(90 + limit)
    idx = rng.choice(len(refs), 600, replace=False).tolist() + list(range(len(strings) - 9, len(strings))) + [-1, 7, 7]
    rows, counts = _compare(m, o, strings, refs, idx, limit)
    # the reference itself is among its rows (its own matches are all of its trigrams)
    for k, i in enumerate(idx[:50]):
        assert int(refs[i]) in rows[k, :counts[k], 0].tolist() or counts[k] == limit


def test_trigram_counts_cover_every_class(geo):
    m, o, strings, refs, weights = geo
    _, offs, _ = m.get_batch(refs)
    nt = np.diff(offs.astype(np.int64))
    # each class -- one trigram, the 16 / 64 / 65 / 127 / 128 boundaries (4-bit counters, short list, mid list, big
    # list), more than 128 -- is present, and found alone, together, and at a limit of several passes
    picked = []
    for lo, hi in ((1, 1),) + tuple((t, t) for t in EXACT) + ((129, 10**6),):
        hits = np.nonzero((nt >= lo) & (nt <= hi))[0]
        assert len(hits) > 0, (lo, hi)
        _compare(m, o, strings, refs, hits[:20].tolist(), 10)
        picked += hits[:3].tolist()
    _compare(m, o, strings, refs, picked, 300)


def test_configs2_scale_one_full_window_against_the_string_path(geonames_full):
    """configs[2]'s haystack: every reference of one full window at limit 10, row for row against find_batch_device over
    the same references' strings, and the first hundred against the oracle"""
    import torch
    hay, off = geonames_full.hay, geonames_full.off
    n = len(off) - 1
    refs = np.arange(1, n + 1, dtype=np.uint32)
    m = RawMap()
    m.put_many_packed(hay, off, refs)
    m.sync_device()
    lens = np.diff(off.astype(np.int64))                     # (weight 0: the string's length)
    idx = np.nonzero(_ranks(refs, lens) // WINDOW == 64)[0]
    assert len(idx) == WINDOW
    limit = 10
    rows, counts, ntri = m.find_batch_by_reference(refs[idx], limit)
    q_off = np.zeros(len(idx) + 1, dtype=np.uint64)
    q_off[1:] = np.cumsum(lens[idx])
    packed = np.concatenate([hay[int(off[i]):int(off[i + 1])] for i in idx.tolist()])
    dev = torch.device("cuda", 0)
    d_packed = torch.from_numpy(packed).to(dev)
    d_off = torch.from_numpy(q_off.astype(np.int64)).to(dev)
    d_rows = torch.zeros((len(idx), limit, 3), dtype=torch.int32, device=dev)
    d_counts = torch.zeros((len(idx),), dtype=torch.int32, device=dev)
    rc = _native.lib().blurrily_storage_find_batch_device(m.handle, d_packed.data_ptr(), int(q_off[-1]), d_off.data_ptr(),
                                                          len(idx), limit, d_rows.data_ptr(), d_counts.data_ptr(), None,
                                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0, C.get_errno()
    torch.cuda.synchronize()
    c_s = d_counts.cpu().numpy().view(np.uint32)
    r_s = d_rows.cpu().numpy().view(np.uint32)
    assert np.array_equal(counts, c_s) and (counts > 0).all()
    live = np.arange(limit)[None, :] < counts[:, None].astype(np.int64)
    assert np.array_equal(np.where(live[:, :, None], rows, 0), np.where(live[:, :, None], r_s, 0))
    want = geonames_full.oracle.batch(packed, q_off, idx=np.arange(100, dtype=np.uint32), limit=limit, ntri=True)
    assert np.array_equal(counts[:100], want["counts"]) and np.array_equal(ntri[:100], want["ntri"])
    for k in range(100):
        assert np.array_equal(rows[k, :counts[k]], want["rows"][k, :counts[k]]), k
    m.close()


def test_rows_do_not_depend_on_the_start_window():
    """q_start comes from the weight (not a length): the same references under weights 1 and 300 -- a window apart --
    give the oracle's rows both ways"""
    hay, off = W.geonames(200000, 40000, 95)
    strings = W.unpack(hay, off)
    n = len(strings)
    refs = np.arange(1, n + 1, dtype=np.uint32)
    rng = np.random.default_rng(96)
    for weights in (np.ones(n, dtype=np.uint32), rng.integers(200, 300, n).astype(np.uint32)):
        m, o = RawMap(), Oracle()
        m.put_many_packed(hay, off, refs, weights)
        for s, r, w in zip(strings, refs.tolist(), weights.tolist()):
            o.put(s, r, w)
        _compare(m, o, strings, refs, rng.choice(n, 20000, replace=False).tolist(), 10)
        m.close()


def test_mutations_pending_puts_deletes_reputs_and_save_load(tmp_path):
    hay, off = W.words(150000, 97)
    strings = W.unpack(hay, off)
    n = len(strings)
    m, o = Map(), Oracle()
    refs = np.arange(1, n + 1, dtype=np.uint32)
    RawMap.put_many_packed(m, hay, off, refs)
    o.put_many(hay, off)
    m.sync_device()
    builds = m.device_info()["base_builds"]
    cur = dict(zip(refs.tolist(), strings))
    # pending puts (new references), deletes, a delete then a put of a different string under the same reference
    for k in range(40):
        s = strings[(k * 977) % n] + b" x" + bytes([97 + k % 26])
        RawMap.put(m, s, n + 1 + k, 0)
        o.put(s, n + 1 + k, 0)
        cur[n + 1 + k] = s
    for r in (5, 17, 1000, 2000):
        m.delete(r)
        o.delete(r)
        del cur[r]
    for r, s in ((17, b"zebra crossing"), (3000, b"totally different")):
        m.delete(r)
        o.delete(r)
        RawMap.put(m, s, r, 0)
        o.put(s, r, 0)
        cur[r] = s
    info = m.device_info()
    asked = [5, 17, 1000, 3000, 1, 2, n + 1, n + 40, 2000, 77, 78]
    for r in asked:
        got = m.get(r)
        if r in cur:
            assert got == (len(cur[r]), Oracle.tokenise(cur[r])), r
        else:
            assert got is None, r
    def check(mm):
        for limit in (10, 121):
            rows, counts, ntri = RawMap.find_batch_by_reference(mm, np.array(asked, dtype=np.uint32), limit)
            for k, r in enumerate(asked):
                want = o.find(cur[r], limit) if r in cur else []
                assert rows[k, :counts[k]].tolist() == want, (r, limit)
                assert ntri[k] == (len(Oracle.tokenise(cur[r])) if r in cur else 0)
    check(m)
    info = m.device_info()
    assert info["base_builds"] == builds and info["n_pending"] > 0 and info["n_tombstones"] > 0, info
    assert m.find_by_reference(17) == o.find(b"zebra crossing", 10)
    path = str(tmp_path / "m.trigrams")
    m.save(path)
    m2 = Map.load(path)
    check(m2)
    m2.close()


def test_device_entry_and_devices_two_give_the_host_rows(geo):
    import torch
    m, o, strings, refs, weights = geo
    rng = np.random.default_rng(99)
    q = np.concatenate([refs[rng.choice(len(refs), 3000, replace=False)], np.array([2, 2], dtype=np.uint32)])
    n, limit = len(q), 10
    rows_h, counts_h, ntri_h = m.find_batch_by_reference(q, limit)
    dev = torch.device("cuda", 0)
    d_refs = torch.from_numpy(q.view(np.int32)).to(dev)
    lib = _native.lib()
    for devices in (1, 2):
        m.set_option("devices", devices)
        rows = torch.zeros((n, limit, 3), dtype=torch.int32, device=dev)
        counts = torch.zeros((n,), dtype=torch.int32, device=dev)
        nt = torch.zeros((n,), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.blurrily_storage_find_references_device(m.handle, d_refs.data_ptr(), n, limit, rows.data_ptr(),
                                                         counts.data_ptr(), nt.data_ptr(), stream)
        assert rc == 0, C.get_errno()
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(np.uint32)
        r = rows.cpu().numpy().view(np.uint32)
        assert np.array_equal(c, counts_h) and np.array_equal(nt.cpu().numpy().view(np.uint32), ntri_h)
        live = np.arange(limit)[None, :] < c[:, None].astype(np.int64)
        assert np.array_equal(np.where(live[:, :, None], r, 0), np.where(live[:, :, None], rows_h, 0))
        rows_b, counts_b, _ = m.find_batch_by_reference(q, limit)
        assert np.array_equal(counts_b, counts_h)
    m.set_option("devices", 1)


def test_string_finds_launch_what_they_did_and_the_reference_path_adds_one_kernel(geo):
    m, o, strings, refs, weights = geo
    packed, offsets = _pack(strings[:5000])
    for _ in range(2):                 # (the first batch of a class may measure every sweep)
        m.find_batch_packed(np.frombuffer(packed, dtype=np.uint8), offsets, 10)
    before = m.last_kernels()
    assert before and "ref_needles_kernel" not in before
    m.find_batch_by_reference(refs[:5000], 10)
    by_ref = m.last_kernels()
    # (references may be long: the launches for needles of 65 trigrams and more follow, as on the device entry)
    assert by_ref[0] == "ref_needles_kernel" and set(before) <= set(by_ref[1:]), (by_ref, before)
    m.find_batch_packed(np.frombuffer(packed, dtype=np.uint8), offsets, 10)
    assert m.last_kernels() == before
