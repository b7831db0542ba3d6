"""What tests/test_gpu_find_boundaries.py and tests/test_gpu_scope_sweeps.py share: a map of tests/boundary_case.py
built on the GPU beside its oracle (`Built`), the option sets that force each sweep, and the tables of the kernels'
dispatch rules keyed by a needle's distinct-trigram count (DESIGN.md sections 23 and 26)."""
import numpy as np

import boundary_case as B
from blurrily_amd import RawMap

F = {name: 1 << i for i, name in enumerate(RawMap.PATH_FLAGS)}
# what the dispatch decides (the table's columns); "ring_overflow" is reserved -- set by no kernel -- and asserted clear
STRUCT = (F["nibble"] | F["byte"] | F["ring_overflow"] | F["pipelined"] | F["wide"] | F["chunked"] | F["ranged"] |
          F["multi_pass"] | F["own_only"] | F["ws_task"] | F["small"])
COPIES = 56                                                     # 20 needles x 56 = 1 120: whole needles per workgroup, no ranges
PLAIN = dict(ws_autotune=0, wsweep=0, nm_min_windows=1 << 20, small_sweep=0)
LEAVE = dict(ws_autotune=0, wsweep=0, nm_min_windows=0, small_sweep=0, nm_dense=64)
WINDOW_MAJOR = dict(ws_autotune=0, wsweep=1, ws_min_windows=0, ws_min_needles=0, ws_min_slice=0, ws_static_slice=0,
                    nm_min_windows=1 << 20, small_sweep=0)
SMALL = dict(ws_autotune=0, wsweep=0, nm_min_windows=1 << 20, small_sweep=1, small_min_needles=0)


def names(flags):
    return "|".join(n for n, b in F.items() if flags & b) or "-"


class Built:
    """One of the two maps, the oracle over the same strings, and the needles packed once per shape."""

    def __init__(self, which):
        self.which, self.case = which, B.case()
        c = self.case
        self.m = RawMap()
        self.m.set_option("dense_min", B.DENSE_MIN)             # before the first put: changing it later forces a rebuild
        src = c.long() if which == "c" else c
        self.m.put_many_packed(src.packed, src.offsets, src.refs, src.weights(which))
        self.m.sync_device()
        info = self.m.device_info()
        assert info["n_windows"] == (5 if which == "c" else 3) and info["n_bitmaps"] >= 8, info
        self.o = c.oracle(which)
        self.once = c.pack(c.needles)
        self.many = c.pack(c.needles * COPIES)
        self.T = np.array(c.T)
        self.avail = self.o.batch(*self.once, limit=65535)["counts"].astype(np.int64)   # rows there are, up to the largest limit
        self._want = {}

    def options(self, opts):
        for k, v in opts.items():
            self.m.set_option(k, v)

    def want(self, limit):
        """the oracle's rows of the needle list at `limit` (once per limit; left unchanged)."""
        if limit not in self._want:
            self._want[limit] = self.o.batch(*self.once, limit=limit)
        return self._want[limit]

    def check(self, batch, limit, copies):
        """One counted and one timed call: rows against the oracle's, copy by copy, and against each other.  Returns the
        first copy's flags, the sweep and the kernels of the counted call."""
        m, n = self.m, len(self.T)
        m.set_stats(True)
        rows, counts = m.find_batch_packed(*batch, limit)
        flags = m.find_path_flags(n * copies)
        sweep, kernels = m.get_option("last_sweep"), m.last_kernels()
        m.set_stats(False)
        want = self.want(limit)
        live = np.arange(limit)[None, :] < want["counts"][:, None].astype(np.int64)
        want_rows = np.where(live[:, :, None], want["rows"], 0)
        for k in range(copies):
            sl = slice(k * n, (k + 1) * n)
            assert np.array_equal(counts[sl], want["counts"]), (k, counts[sl].tolist(), want["counts"].tolist())
            bad = np.nonzero((np.where(live[:, :, None], rows[sl], 0) != want_rows).any(axis=(1, 2)))[0]
            if len(bad):
                q = int(bad[0])
                col = int(np.nonzero((np.where(live[q, :, None], rows[sl][q], 0) != want_rows[q]).any(axis=1))[0][0])
                raise AssertionError((self.which, limit, k, "T", int(self.T[q]), "row", col, rows[sl][q, col].tolist(),
                                      want_rows[q, col].tolist()))
            assert np.array_equal(flags[sl] & STRUCT, flags[:n] & STRUCT), k
        rows_t, counts_t = m.find_batch_packed(*batch, limit)
        live_all = np.tile(live, (copies, 1))
        assert np.array_equal(counts_t, counts)
        assert np.array_equal(np.where(live_all[:, :, None], rows_t, 0), np.where(live_all[:, :, None], rows, 0))
        return flags[:n], sweep, kernels

    def assert_flags(self, flags, expect, what):
        for i, t in enumerate(self.T.tolist()):
            want = expect(i, t)
            assert int(flags[i]) & STRUCT == want, (self.which, what, "T", t, "bytes", len(self.case.needles[i]),
                                                    names(int(flags[i])), "expected", names(want))


def counters_of(t, which, own_window_only=False):
    """The counters a needle of t distinct trigrams is swept with by the needle-major kernels.
    needle_major.inc (BLURRILY_SWEEP): T <= 15: 4-bit counters in every window; T <= 64: 4-bit in the windows below
    "nib_windows" (2 of 3 on map A, 0 on map B), byte counters in the rest; tokenise.inc: 65 .. 127 the mid list
    (sweep_pipelined, byte counters), from 128 on the big list (16-bit counters; sweep_pipelined up to kCodeChunk =
    128, sweep_chunked beyond).  own_window_only: the sweep covers window 2 alone."""
    if t <= 15:
        return F["nibble"]
    if t <= 64:
        return F["byte"] if which == "b" or own_window_only else F["nibble"] | F["byte"]
    if t <= 127:
        return F["pipelined"]
    return F["wide"] | (F["pipelined"] if t == 128 else F["chunked"])


def passes_of(b, i, t, limit):
    """"multi_pass": a pass keeps 1 024 rows of a needle of up to 127 trigrams, 256 of a longer one; a later pass runs
    when the needle filled the ones before (find_run.hip: run_nm and the long-needle loop; needle_major.inc: `have <
    pass_base`)."""
    rows = 1024 if t <= 127 else 256
    return F["multi_pass"] if limit > rows and b.avail[i] >= rows else 0
