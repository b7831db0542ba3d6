"""The scoped find's direct strategy on the edges of its own select (kernels/scope.inc: scope_score_rows,
scope_map_string; scope.hip: the pinned page, the scope-per-needle plan).  "scope_strategy" 2 is
forced; `last_kernels() == ["scope_find_kernel"]` (or the each kernel) is asserted wherever the direct form is expected
and its ABSENCE wherever it must decline -- a member of 256 trigrams, 57 345 members, limit 257 -- where the mask's
kernels are named and the rows still equal the truth.  Every direct case also runs through the mask and must give the
same bytes in the live rows.  Inputs: tests/scope_boundary_case.py (proven by tests/test_scope_boundary_case.py)."""
import numpy as np
import pytest

import scope_boundary_case as S
from blurrily_amd import RawMap
from blurrily_amd.map import _pack
from boundary_built import COPIES, LEAVE, PLAIN, Built
from scope_truth import Truth

pytestmark = pytest.mark.gpu


def _live(rows, counts):
    keep = np.arange(rows.shape[1])[None, :] < counts[:, None].astype(np.int64)
    return np.where(keep[:, :, None], rows, 0)


def _lists(rows, counts):
    return [rows[i, :counts[i]].tolist() for i in range(len(counts))]


def _is_direct(kernels):
    return kernels == ["scope_find_kernel"]


def both(m, sc, needles, limit, direct):
    """The batch with the direct strategy forced -- taken, or declined for the mask's kernels, as `direct` says -- and
    through the mask: the same counts and the same bytes in the live rows.  Returns the forced call's rows as lists."""
    packed, offsets = _pack(needles)
    buf = np.frombuffer(packed, dtype=np.uint8)
    try:
        m.set_option("scope_strategy", 2)
        rows2, counts2 = m.find_batch_in(sc, buf, offsets, limit)
        kernels = m.last_kernels()
        if direct:
            assert _is_direct(kernels), kernels
        else:
            assert "scope_find_kernel" not in kernels and any(k.startswith("find_") for k in kernels), kernels
        m.set_option("scope_strategy", 1)
        rows1, counts1 = m.find_batch_in(sc, buf, offsets, limit)
        assert "scope_find_kernel" not in m.last_kernels()
    finally:
        m.set_option("scope_strategy", 0)
    assert np.array_equal(counts1, counts2), (counts1.tolist(), counts2.tolist())
    assert np.array_equal(_live(rows1, counts1), _live(rows2, counts2))
    return _lists(rows2, counts2)


# ---- the small map -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    d = S.direct_case()
    m = RawMap()
    packed, offsets = _pack(d.strings)
    m.put_many_packed(packed, offsets, d.refs, d.weights)
    m.sync_device()
    assert m.device_info()["n_windows"] == 1
    yield m, d
    m.close()


def check_small(m, d, scope_refs, needles, limit, direct=True):
    mem = d.members(scope_refs)
    with m.scope(np.asarray(scope_refs, dtype=np.uint32)) as sc:
        got = both(m, sc, needles, limit, direct)
    want = [d.rows(mem, nd, limit) for nd in needles]
    assert got == want, next((i, g[:3], w[:3]) for i, (g, w) in enumerate(zip(got, want)) if g != w)
    return got


def test_the_255_ceiling_of_a_members_matches(small):
    """A member's matches are kept in a byte and counted in a histogram of 256 bins; `tid == 255` is a special case of the
    threshold pick.  A member of exactly 255 trigrams under its own string, and under its superstring, has 255."""
    m, d = small
    some = d.fill_refs[:40].tolist()
    for nd in (d.m255, d.super255):
        got = check_small(m, d, [S.REF_255A] + some, [nd], 10)
        assert got[0][0] == [S.REF_255A, 255, 7]
        got = check_small(m, d, [S.REF_255A, S.REF_255B] + some, [nd], 1)
        assert got[0] == [[S.REF_255A, 255, 7]]                 # the lighter one
        got = check_small(m, d, [S.REF_255A, S.REF_255B] + some, [nd], 2)
        assert got[0] == [[S.REF_255A, 255, 7], [S.REF_255B, 255, 9]]
        # ... and only 255-members: every passing member sits in the last bin
        got = check_small(m, d, [S.REF_255A, S.REF_255B], [nd], 256)
        assert got[0] == [[S.REF_255A, 255, 7], [S.REF_255B, 255, 9]]
        # a member of 256 trigrams in the scope: no direct form
        check_small(m, d, [S.REF_255A, S.REF_255B, S.REF_256] + some, [nd], 2, direct=False)


@pytest.mark.parametrize("n_members", [1, 255, 256, 257, 513])
def test_scope_sizes_around_a_chunk_of_256_members(small, n_members):
    m, d = small
    for limit in (1, 10, 256):
        check_small(m, d, d.fill_refs[:n_members], d.select_needles + d.needles, limit)


def test_limits_on_either_side_of_the_select_boundary(small):
    """`passing`: the members with one match or more.  Limits passing - 1, passing, passing + 1; and the same three around
    the count of members at the highest and at the two highest values of matches, where the threshold value steps: one
    more row then comes from the ties at the next value (need 1), one fewer leaves none above (above 0)."""
    m, d = small
    scope_refs = d.fill_refs[:S.SELECT_MEMBERS]
    mem = d.members(scope_refs)
    for nd in d.select_needles:
        matches = Truth.matches(mem, nd)
        values = np.unique(matches[matches >= 1])[::-1]
        edges = {int((matches >= 1).sum()), int((matches >= values[0]).sum())}
        if len(values) > 1:
            edges.add(int((matches >= values[1]).sum()))
        limits = sorted({e + k for e in edges for k in (-1, 0, 1) if 1 <= e + k <= S.MAX_KEEP})
        assert len(limits) >= 3, (nd, edges)
        for limit in limits:
            check_small(m, d, scope_refs, [nd], limit)


@pytest.mark.parametrize("limit", [1, 2, 128, 129, 255, 256])
def test_ties_at_the_threshold_across_ballot_chunks(small, limit):
    """1 200 members, the copies of one string at every other member index: the members at the threshold are taken in
    member order by ballots over five chunks of 256 members.  The rows are the first `limit` copies in weight order;
    under a prefix of the copied string three other members rank above the tie."""
    m, d = small
    got = check_small(m, d, d.ties, [S.COPIED], limit)
    assert [r[0] for r in got[0]] == list(range(S.COPY_REF0, S.COPY_REF0 + limit))
    got = check_small(m, d, d.ties_plus, [S.COPIED_PREFIX, S.COPIED], limit)
    first = [S.PREFIX_REF0 + k for k in range(3)] + list(range(S.COPY_REF0, S.COPY_REF0 + limit))
    assert [r[0] for r in got[0]] == first[:limit]
    assert [r[0] for r in got[1]] == list(range(S.COPY_REF0, S.COPY_REF0 + limit))


def test_needles_empty_long_repeated_and_cut_at_an_embedded_nul(small):
    """scope_map_string finds the needle's NUL with an atomicMin over a 256-thread stride; the truth tokenises the
    needle's C-string prefix.  Every NUL needle has a second NUL 256 bytes behind the first: the same thread meets both."""
    m, d = small
    scope_refs = d.refs[d.refs != S.REF_256]
    for limit in (1, 10, 256):
        got = check_small(m, d, scope_refs, d.needles, limit)
        assert got[0] == [] and got[3] == []                       # the empty needle; the needle cut at byte 0
        assert got[1] and got[2] and got[4] and got[5]


def test_batches_on_both_sides_of_the_pinned_page(small):
    """scope.hip: a direct batch goes through a 64 KiB pinned page when needles and rows fit (BatchBlocks: the offsets
    padded to 256 bytes in front of the packed bytes; the counts padded to 256 in front of the rows), through device
    buffers otherwise.  At limit 256 the rows of 21 needles fit (256 + 21 x 3 072 = 64 768) and those of 22 do not;
    65 280 packed bytes fit beside up to 31 offsets (256 + 65 280 = 65 536) and 65 281 do not."""
    m, d = small
    scope_refs = d.fill_refs[:700]
    pool = d.select_needles + d.needles[1:] + [d.m255, S.COPIED, d.strings[50], d.strings[2000]] * 3
    few = check_small(m, d, scope_refs, pool[:21], 256)
    more = check_small(m, d, scope_refs, pool[:22], 256)
    assert more[:21] == few
    text = (b"san jose de la " + d.strings[3000] + b" " + d.strings[3001] + b" ") * 200
    fits = [text[k:k + 2176] for k in range(30)]
    assert sum(len(s) for s in fits) == 65280
    over = fits[:-1] + [fits[-1] + b"z"]
    a = check_small(m, d, scope_refs, fits, 10)
    b = check_small(m, d, scope_refs, over, 10)
    assert a[:29] == b[:29]


# ---- map A -------------------------------------------------------------------------------------------------------------
class OnA:
    def __init__(self):
        self.b = Built("a")
        self.m, self.case = self.b.m, self.b.case
        self.truth = S.ScopedTruth(self.case, "a")
        self._scopes = {}

    def refs(self, name):
        return S.scope(self.case, "a", name)

    def scope(self, name):
        if name not in self._scopes:
            self._scopes[name] = self.m.scope(self.refs(name))
        return self._scopes[name]

    def want(self, name, limit):
        return _lists(*self.truth.batch(name, self.refs(name), limit))


@pytest.fixture(scope="module")
def on_a():
    a = OnA()
    yield a
    for sc in a._scopes.values():
        sc.close()
    a.m.close()


@pytest.mark.parametrize("limit", [1, 10, 255, 256])
@pytest.mark.parametrize("name", ["hot_255", "specials_255", "window0"])
def test_scopes_of_map_a_up_to_the_caps_of_the_direct_form(on_a, name, limit):
    """Every needle of tests/boundary_case.py -- 1 .. 1 200 trigrams -- within `hot_255` (8 664 members), `specials_255`
    (every member of at most 255 trigrams) and `window0` (kScopeMaxMembers = 57 344 members exactly)."""
    a = on_a
    a.b.options(PLAIN)
    assert both(a.m, a.scope(name), a.case.needles, limit, True) == a.want(name, limit)


@pytest.mark.parametrize("name,limit", [("window0_plus", 10), ("window0_plus", 256), ("specials", 10), ("specials", 256),
                                        ("hot", 10), ("hot", 256), ("hot_255", 257), ("specials_255", 257), ("window0", 257)])
def test_what_the_direct_form_declines_on_map_a(on_a, name, limit):
    """57 345 members, a member of 256 trigrams or more (`specials`; `hot`, which holds the twins of the long class needles),
    limit 257: the mask serves the call, with the same rows."""
    a = on_a
    a.b.options(PLAIN)
    assert both(a.m, a.scope(name), a.case.needles, limit, False) == a.want(name, limit)


# ---- a scope per needle --------------------------------------------------------------------------------------------------
def test_one_launch_for_scopes_of_57344_members_of_one_and_of_a_few_dozen(on_a):
    """scope_each_kernel's dynamic LDS is a byte per member of the LARGEST scope of the launch."""
    a = on_a
    a.b.options(PLAIN)
    m, c = a.m, a.case
    names = ["window0", "rank_65519", "specials_255"]
    needles = c.needles * 3
    which = [(i + i // len(c.needles)) % 3 for i in range(len(needles))]
    packed, offsets = _pack(needles)
    try:
        m.set_option("scope_strategy", 2)
        rows, counts = m.find_batch_each_in([a.scope(n) for n in names], which, np.frombuffer(packed, dtype=np.uint8),
                                            offsets, 10)
        assert m.last_kernels() == ["scope_each_kernel"], m.last_kernels()
    finally:
        m.set_option("scope_strategy", 0)
    got = _lists(rows, counts)
    want = {n: a.want(n, 10) for n in names}
    for i, w in enumerate(which):
        assert got[i] == want[names[w]][i % len(c.needles)], (i, names[w])


DEAL = ["no_twins", "hot_255", "specials", None]                    # mask (too many members), direct, mask (a 256-member), no scope


@pytest.mark.parametrize("opts", [PLAIN, dict(LEAVE, nm_cmin=1)], ids=["plain", "leave"])
@pytest.mark.parametrize("by_reference", [False, True], ids=["strings", "references"])
def test_a_mixed_batch_deals_every_class_to_the_mask_the_direct_form_and_no_scope(on_a, opts, by_reference):
    """Every needle of the case under every one of four scopes in ONE call: the direct ones in one launch of
    scope_each_kernel, each masked scope's needles compacted (scope_gather_strings_kernel / scope_gather_refs_kernel,
    whose offset arithmetic meets needles of 1 .. 1 200 trigrams side by side), swept and put back
    (scope_scatter_kernel), the unscoped ones the same way.  Rows element for element the single-scope calls' and the
    truth's; the twins of every class are the references."""
    a = on_a
    a.b.options(opts)
    m, c, n = a.m, a.case, len(a.case.needles)
    limit = 10
    reps = 4 * COPIES                                            # 1 120 needles a group: whole needles per workgroup, no ranges
    which = [(i + i // n) % 4 for i in range(reps * n)]
    scopes = [a.scope(name) for name in DEAL[:3]]
    which_arg = [None if w == 3 else w for w in which]
    try:
        m.set_option("scope_strategy", 2)
        if by_reference:
            twins = [c.ref_at(i, 0) for i in range(n)]
            rows, counts, ntri = m.find_batch_by_reference_each_in(scopes, which_arg, np.array(twins * reps, dtype=np.uint32), limit)
            assert ntri.tolist() == c.T * reps
        else:
            packed, offsets = _pack(c.needles * reps)
            rows, counts = m.find_batch_each_in(scopes, which_arg, np.frombuffer(packed, dtype=np.uint8), offsets, limit)
        kernels = m.last_kernels()
        # (distinct names in launch order: the direct launch first, then the groups' sweeps -- whole needles per workgroup)
        assert kernels[0] == "scope_each_kernel" and "find_kernel<uint8_t,1024,false,true>" in kernels, kernels
        assert "find_kernel<uint8_t,1024,true,true>" not in kernels and "scope_find_kernel" not in kernels, kernels
        single = {}
        for k, name in enumerate(DEAL[:3]):                       # the single-scope calls
            packed1, offsets1 = _pack(c.needles)
            single[k] = _lists(*m.find_batch_in(scopes[k], np.frombuffer(packed1, dtype=np.uint8), offsets1, limit))
            assert _is_direct(m.last_kernels()) == (name == "hot_255"), (name, m.last_kernels())
    finally:
        m.set_option("scope_strategy", 0)
    got = _lists(rows, counts)
    plain = a.b.want(limit)
    unscoped = _lists(plain["rows"], plain["counts"])
    for i, w in enumerate(which):
        want = unscoped[i % n] if w == 3 else a.want(DEAL[w], limit)[i % n]
        assert got[i] == want, (i, DEAL[w], c.T[i % n], got[i][:2], want[:2])
        if w < 3:
            assert got[i] == single[w][i % n], (i, DEAL[w])
