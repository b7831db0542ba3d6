"""The scoped find's mask strategy under EVERY sweep.  The mask strategy hands run_find the scope's
bitmap in the tombstone bitmap's place, and every sweep has code that turns once `A.tomb` is set (no cold start, the
window-major task's pass test, the pending list of a leaving sweep, the floor key of later passes).  That code was
written for a handful of deleted rows; a scope is a tombstone bitmap with nearly every bit SET: the rows that give the
unscoped find its thresholds are excluded, whole windows hold no member, a needle's own window may hold none, and fewer
members than the limit may exist.

On the maps of tests/boundary_case.py and the scopes of tests/scope_boundary_case.py, every route is forced through the
map's options with "scope_strategy" 1 and ASSERTED TAKEN ("last_sweep", last_kernels()) exactly as
tests/test_gpu_find_boundaries.py asserts it for the unscoped find; every copy's rows and counts equal the numpy truth
(tests/scope_truth.py, anchored on the oracle by tests/test_scope_boundary_case.py), the counted build's rows equal the
timed build's, the structural path flags equal the unscoped tables -- the dispatch depends on T, not on the mask -- and
after every case one unscoped find of the same batch still equals the oracle: the mask does not leak into the map."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import boundary_case as B
import scope_boundary_case as S
from scope_truth import Truth
from blurrily_amd import _native
from boundary_built import COPIES, LEAVE, PLAIN, SMALL, STRUCT, WINDOW_MAJOR, Built, F, counters_of, passes_of

pytestmark = pytest.mark.gpu

SINGLE_RANKS = tuple(f"rank_{r}" for r in S.EDGE_RANKS)
EDGE = SINGLE_RANKS + ("edge_ranks",)                           # "edge_ranks" of the routes: the four one-member scopes and all four


class Scoped:
    """A built map, the truth over it, and its scopes (made at first use, closed with the map)."""

    def __init__(self, which):
        self.b = Built(which)
        self.which, self.case, self.m = which, self.b.case, self.b.m
        self.truth = S.ScopedTruth(self.case, which)
        self._scopes, self._refs = {}, {}

    def refs(self, name):
        if name not in self._refs:
            self._refs[name] = S.scope(self.case, self.which, name)
        return self._refs[name]

    def scope(self, name):
        if name not in self._scopes:
            self._scopes[name] = self.m.scope(self.refs(name))
        return self._scopes[name]

    def close(self):
        for sc in self._scopes.values():
            sc.close()
        self.m.close()

    def avail(self, name):
        """rows there are within the scope, up to the largest limit."""
        return self.truth.batch(name, self.refs(name), 65535)[1].astype(np.int64)

    def compare(self, name, limit, rows, counts, copies, want=None):
        want_rows, want_counts = want if want is not None else self.truth.batch(name, self.refs(name), limit)
        n = len(want_counts)
        live = np.arange(limit)[None, :] < want_counts[:, None].astype(np.int64)
        for k in range(copies):
            sl = slice(k * n, (k + 1) * n)
            assert np.array_equal(counts[sl], want_counts), (self.which, name, limit, k, counts[sl].tolist(), want_counts.tolist())
            bad = np.nonzero((np.where(live[:, :, None], rows[sl], 0) != want_rows).any(axis=(1, 2)))[0]
            if len(bad):
                q = int(bad[0])
                col = int(np.nonzero((np.where(live[q, :, None], rows[sl][q], 0) != want_rows[q]).any(axis=1))[0][0])
                raise AssertionError((self.which, name, limit, k, "T", int(self.b.T[q]), "row", col,
                                      rows[sl][q, col].tolist(), want_rows[q, col].tolist()))
        return np.tile(live, (copies, 1))

    def check(self, name, batch, limit, copies, want=None):
        """One counted and one timed scoped call through the mask: rows against the truth, copy by copy, and against
        each other; the measured choices untouched.  Returns the first copy's flags, the sweep and the kernels of the
        counted call."""
        m, n = self.m, len(self.b.T)
        sc = self.scope(name)
        m.set_option("scope_strategy", 1)
        held = (m.get_option("ws_choice"), m.get_option("tuned_class"))
        try:
            m.set_stats(True)
            rows, counts = m.find_batch_in(sc, *batch, limit)
            flags = m.find_path_flags(n * copies)
            sweep, kernels = m.get_option("last_sweep"), m.last_kernels()
            m.set_stats(False)
            assert "scope_find_kernel" not in kernels, kernels
            live_all = self.compare(name, limit, rows, counts, copies, want)
            for k in range(copies):
                assert np.array_equal(flags[k * n:(k + 1) * n] & STRUCT, flags[:n] & STRUCT), (name, limit, k)
            rows_t, counts_t = m.find_batch_in(sc, *batch, limit)
            assert np.array_equal(counts_t, counts), (name, limit)
            assert np.array_equal(np.where(live_all[:, :, None], rows_t, 0), np.where(live_all[:, :, None], rows, 0)), (name, limit)
            assert (m.get_option("ws_choice"), m.get_option("tuned_class")) == held
        finally:
            m.set_stats(False)
            m.set_option("scope_strategy", 0)
        return flags[:n], sweep, kernels

    def classes(self, flags, flag):
        return {t for i, t in enumerate(self.b.T.tolist()) if flags[i] & F[flag]}


@pytest.fixture(scope="module")
def maps():
    made = {}

    def get(which):
        if which not in made:
            made[which] = Scoped(which)
        return made[which]
    yield get
    for s in made.values():
        s.close()


def on(which_scopes, limits, *more):
    """[(map, scope, limit, ...)] with ids."""
    out = []
    for which, scopes in which_scopes:
        for name in scopes:
            for limit in limits:
                for extra in (more[0] if more else [()]):
                    out.append(pytest.param(which, name, limit, *extra,
                                            id="-".join([which, name, str(limit)] + [str(e) for e in extra])))
    return out


# ---- 1. the plain needle-major sweep -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which,name,limit", on([("a", S.SCOPES_A), ("b", EDGE + ("no_twins",))], [1, 10, 64, 65, 1024]))
def test_plain_needle_major_sweep_under_a_scope(maps, which, name, limit):
    """No cold start once `A.tomb` is set (needle_major.inc, counters.inc): the threshold comes from the candidates the
    mask lets through alone.  Under no_twins every class needle's twin passes whatever threshold there is -- it has
    every match -- and is dropped for its bit: "tombstone"."""
    s = maps(which)
    b = s.b
    b.options(PLAIN)
    flags, sweep, kernels = s.check(name, b.many, limit, COPIES)
    assert sweep == 1 and kernels[0] == "find_kernel<uint8_t,1024,false,true>", (sweep, kernels)
    assert "find_kernel<uint16_t,1024,false,false>" in kernels and "find_kernel<uint8_t,1024,false,false>" in kernels
    within = SimpleNamespace(avail=s.avail(name))
    b.assert_flags(flags, lambda i, t: counters_of(t, which) | passes_of(within, i, t, limit), ("plain", name, limit))
    if name == "no_twins":
        assert set(B.CLASSES) <= s.classes(flags, "tombstone"), sorted(s.classes(flags, "tombstone"))
    b.check(b.many, limit, COPIES)


# ---- 2. its later passes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,name,limit", on([("a", ("no_twins", "alternate", "specials"))], [1025, 65535]))
def test_later_passes_under_a_scope(maps, which, name, limit):
    """The floor key of a later pass together with the mask (counters.inc): a pass starts behind the last SCOPED row of
    the one before.  "multi_pass" where the scoped rows fill a pass; `specials` has fewer members than a pass."""
    s = maps(which)
    b = s.b
    b.options(PLAIN)
    flags, sweep, kernels = s.check(name, b.once, limit, 1)
    assert sweep == 1
    within = SimpleNamespace(avail=s.avail(name))
    b.assert_flags(flags, lambda i, t: counters_of(t, which) | passes_of(within, i, t, limit), ("passes", name, limit))
    multi = s.classes(flags, "multi_pass")
    if name == "specials":
        assert not multi and int(within.avail.max()) < 149, multi
    else:
        assert {15, 16, 64, 65, 127, 128, 1200} <= multi, multi
    b.check(b.once, limit, 1)


# ---- 3. the needle-major sweep that leaves dense slices out ------------------------------------------------------------
@pytest.mark.parametrize("which,name,limit,cmin", on([("a", ("hot", "hot_w1", "no_twins", "no_prefix15", "specials", "window0_all")),
                                                      ("b", ("hot", "hot_w1", "no_twins", "no_prefix15", "specials", "window0_all"))],
                                                     [10, 149, 150], [(1,), (3,)]))
def test_slices_left_out_under_a_scope(maps, which, name, limit, cmin):
    """A candidate whose matches lie in left-out dense slices goes to the pending list only if its bit is clear
    (counters.inc).  Every member of `hot` holds the hot word's four codes, which are what a 16 .. 64 needle's step
    leaves out: the bitmaps are the only way to those matches.  `no_prefix15` takes away a reference of windows 0 and
    1 that enters a 16 .. 64 needle's first rows BY the left-out slices: a non-member that went pending would be settled
    into the pool, where nobody looks at the mask again (on map C `no_late` does the same in window 4)."""
    s = maps(which)
    b = s.b
    b.options(dict(LEAVE, nm_cmin=cmin))
    flags, sweep, kernels = s.check(name, b.many, limit, COPIES)
    b.assert_flags(flags, lambda i, t: counters_of(t, which), ("leave", name, limit, cmin))
    left = s.classes(flags, "nm_left_out")
    print("leave", which, name, limit, cmin, sweep, sorted(left))
    if limit == 150:
        assert sweep == 1 and not left, (sweep, left)
    else:
        assert sweep == 3
        assert left <= {t for t in b.T.tolist() if 15 < t <= 64}, left
        if name == "hot":
            assert left, "no needle of 16 .. 64 trigrams settled a member of `hot` through the bitmaps"
    b.check(b.many, limit, COPIES)


@pytest.mark.parametrize("which,name,limit,cmin", on([("c", S.SCOPES_C)], [10, 149], [(1,), (3,)]))
def test_slices_left_out_of_a_4_bit_sweep_under_a_scope(maps, which, name, limit, cmin):
    """Map C: five windows, three 4-bit steps; `late_only` leaves the second twins of window 4 alone in the scope, `no_late`
    takes exactly them away."""
    s = maps(which)
    b = s.b
    b.options(dict(LEAVE, nm_cmin=cmin))
    flags, sweep, kernels = s.check(name, b.many, limit, COPIES)
    assert sweep == 3
    b.assert_flags(flags, lambda i, t: counters_of(t, "a"), ("leave, five windows", name, limit, cmin))
    left = s.classes(flags, "nm_left_out")
    print("leave c", name, limit, cmin, sorted(left))
    assert left <= {t for t in b.T.tolist() if cmin < t <= 64}, left
    b.check(b.many, limit, COPIES)


# ---- 4. the window-major sweep -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,name,limit", on([("a", ("window0_all", "hot_w1", "no_twins") + EDGE),
                                                 ("b", ("window0_all", "hot_w1", "no_twins") + EDGE)], [10, 128, 129]))
def test_window_major_sweep_under_a_scope(maps, which, name, limit):
    """The task's pass test and cold start (window_major.inc).  Phase 1 sweeps the needle's own window -- window 2 for
    every needle of two bytes and more -- where `window0_all` and `hot_w1` have no member: it seeds no threshold, the
    tasks of windows 0 and 1 start without one."""
    s = maps(which)
    b, c = s.b, s.case
    b.options(WINDOW_MAJOR)
    flags, sweep, kernels = s.check(name, b.many, limit, COPIES)
    if limit == 129:
        assert sweep == 1 and "wsweep_kernel" not in "+".join(kernels), (sweep, kernels)
        b.assert_flags(flags, lambda i, t: counters_of(t, which), ("not window-major", name, limit))
    else:
        assert sweep == 2 and any(k.startswith("wsweep_kernel") for k in kernels), (sweep, kernels)

        def expect(i, t):
            if t > 64:
                return counters_of(t, which)
            return F["own_only"] | F["ws_task"] | counters_of(t, which, own_window_only=len(c.needles[i]) >= 2)
        b.assert_flags(flags, expect, ("window-major", name, limit))
    b.check(b.many, limit, COPIES)


# ---- 5. the small-haystack sweep ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,name,limit", on([("a", ("no_twins", "specials", "window0_all"))], [64, 65]))
def test_small_haystack_sweep_under_a_scope(maps, which, name, limit):
    """No cold start once `A.tomb` is set (small.inc)."""
    s = maps(which)
    b = s.b
    b.options(SMALL)
    flags, sweep, kernels = s.check(name, b.many, limit, COPIES)
    if limit == 65:
        assert sweep == 1 and not any(flags & F["small"]), sweep
        b.assert_flags(flags, lambda i, t: counters_of(t, which), ("not small", name, limit))
    else:
        assert sweep == 4 and kernels[0].startswith("find_small_kernel"), (sweep, kernels)
        b.assert_flags(flags, lambda i, t: counters_of(t, which) | (F["small"] if t <= 15 else 0), ("small", name, limit))
    b.check(b.many, limit, COPIES)


# ---- 6. latency mode on the device entry -------------------------------------------------------------------------------
def _device_find_in(m, sc, packed, off, limit):
    import torch
    dev = torch.device("cuda", 0)
    n = len(off) - 1
    d_packed = torch.from_numpy(np.concatenate([packed, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_rows = torch.zeros((n, limit, 3), dtype=torch.int32, device=dev)
    d_counts = torch.full((n,), -1, dtype=torch.int32, device=dev)
    res = _native.lib().blurrily_storage_find_batch_in_device(m.handle, sc._h, d_packed.data_ptr(), int(off[-1]),
                                                              d_off.data_ptr(), n, limit, d_rows.data_ptr(),
                                                              d_counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert res == 0, C.get_errno()
    torch.cuda.synchronize()
    return d_rows.cpu().numpy().view(np.uint32), d_counts.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("which,name,limit", on([("a", ("window0_all", "hot_w1", "specials") + EDGE)], [10, 64, 65]))
def test_latency_mode_on_the_device_entry_under_a_scope(maps, which, name, limit):
    """The needle list once, device-resident: two ranges, windows (0, 1) and window (2).  `window0_all`, `hot_w1` and the
    one-member scopes leave at least one range of every needle without a member -- it hands the merge nothing, and where
    that range holds the needle's own window, the other learnt no threshold there."""
    s = maps(which)
    b, m, n = s.b, s.m, len(s.b.T)
    b.options(PLAIN)
    if name in ("window0_all", "hot_w1") + SINGLE_RANKS:
        win = set((s.truth.v.rank[s.truth.v.index(s.refs(name))] // B.WINDOW_RANKS).tolist())
        assert not ({0, 1} & win) or 2 not in win, win
    sc = s.scope(name)
    m.set_option("scope_strategy", 1)
    try:
        m.set_stats(True)
        rows, counts = _device_find_in(m, sc, *b.once, limit)
        flags, kernels = m.find_path_flags(n), m.last_kernels()
        m.set_stats(False)
        live = s.compare(name, limit, rows, counts, 1)
        rows_t, counts_t = _device_find_in(m, sc, *b.once, limit)
        assert np.array_equal(counts_t, counts)
        assert np.array_equal(np.where(live[:, :, None], rows_t, 0), np.where(live[:, :, None], rows, 0))
    finally:
        m.set_stats(False)
        m.set_option("scope_strategy", 0)
    assert kernels[0] == "find_kernel<uint8_t,1024,true,true>", kernels
    b.assert_flags(flags, lambda i, t: counters_of(t, which) | (F["ranged"] if t <= 64 else 0), ("latency", name, limit))
    b.check(b.once, limit, 1)


# ---- 7. the delta image (last: it changes map A) -----------------------------------------------------------------------
def test_a_scope_made_before_the_puts_finds_the_second_twins_in_the_delta_image(maps):
    """A scope names references the map does not hold yet and leaves the first twins out.  Then every needle's twin is
    put again under those references (the delta image), and every other first twin is deleted (a tombstone under the
    mask): the next scoped find has the new rows -- through the delta image's mask, `sm->delta` -- under the plain and
    the leaving sweep, within a pass and beyond one."""
    s = maps("a")
    b, m, o, c, v = s.b, s.m, s.b.o, s.case, s.truth.v
    n = len(c.needles)
    twins = [c.ref_at(i, 0) for i in range(n)]
    new = [900000 + i for i in range(n)]
    scope_refs = np.concatenate([v.refs[~np.isin(v.refs, twins)], new]).astype(np.uint32)
    sc = m.scope(scope_refs)
    try:
        s._scopes["delta"] = sc
        assert sc.members() == len(scope_refs) - n
        w = c.weights("a")
        for i in range(n):
            wt = int(w[c._at[twins[i]]])
            assert m.put(c.needles[i], new[i], wt) == o.put(c.needles[i], new[i], wt)
            if i % 2 == 0:
                assert m.delete(twins[i]) == o.delete(twins[i]) > 0
        b._want.clear()
        assert sc.members() == len(scope_refs)
        # the truth: a new twin matches every needle as the first twin of its string does
        at = v.index(twins)
        refs = np.concatenate([v.refs, new])
        weights = np.concatenate([v.weights, v.weights[at]])
        keep = np.concatenate([~np.isin(v.refs, twins), np.ones(n, dtype=bool)])
        for opts, limit, sweep_want in ((PLAIN, 10, 1), (PLAIN, 1025, 1), (dict(LEAVE, nm_cmin=1), 10, 3),
                                        (dict(LEAVE, nm_cmin=1), 1025, 1)):
            rows, counts = np.zeros((n, limit, 3), dtype=np.uint32), np.zeros(n, dtype=np.uint32)
            for j in range(n):
                mj = np.concatenate([s.truth.matches[j], s.truth.matches[j][at]])
                r = Truth.ranked_array(refs[keep], weights[keep], mj[keep], limit)
                counts[j] = len(r)
                rows[j, :len(r)] = r
                assert [new[j], c.T[j], int(weights[len(v.refs) + j])] in r[:10].tolist(), (j, r[:3])
                assert twins[j] not in r[:, 0]
            b.options(opts)
            copies = COPIES if limit == 10 else 1
            flags, sweep, kernels = s.check("delta", b.many if limit == 10 else b.once, limit, copies, want=(rows, counts))
            assert sweep == sweep_want, (opts, limit, sweep)
            b.check(b.many if limit == 10 else b.once, limit, copies)
        info = m.device_info()
        assert info["base_builds"] == 1 and info["n_pending"] == n and info["n_tombstones"] == (n + 1) // 2, info
    finally:
        c._oracles.pop("a", None)                                 # the oracle was changed with the map: the next user builds its own
