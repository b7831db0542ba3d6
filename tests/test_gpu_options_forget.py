"""Which options forget the sweep's measured choice (options.hip: a row's `forgets`).  Setting one of the fourteen
tunables the choice depends on has every class of batch measured again by its next batch; setting any of the other
eighteen -- to the very value it has -- leaves the choice and the last measurement where they were.  The map is the
smallest on which a batch of 129 needles at limit 10 is measured at all (class 6): one window (more than two, and
latency mode cuts so few needles' windows into ranges instead), slices dense enough for bitmaps at "dense_min" 64,
"nm_cmin" at its default 3 -- so leaving slices out is a sweep the class can take, and there is a choice to measure."""
import numpy as np
import pytest

import workloads as W
from blurrily_amd import RawMap
from helpers import Oracle

pytestmark = pytest.mark.gpu

FORGETS = ["wsweep", "ws_cmin", "ws_min_windows", "ws_min_needles", "ws_min_slice", "dense_min", "ws_autotune",
           "ws_static_slice", "ws_choice", "nm_cmin", "nm_dense", "nm_min_windows", "small_sweep", "small_min_needles"]
KEEPS = ["host_chunk", "last_sweep", "devices", "tuned_class", "tuned_nm_us", "tuned_ws_us", "tuned_leave_us",
         "one_launch", "one_taken", "one_windows_per_wg", "retunes", "tune_inject", "mid_workgroups", "few_max",
         "mid_max", "latency_tasks", "scope_strategy", "scope_direct_max"]
READ_ONLY = {"ws_choice", "last_sweep", "tuned_class", "tuned_nm_us", "tuned_ws_us", "tuned_leave_us", "one_taken", "retunes"}


def test_fourteen_options_forget_the_choice_and_eighteen_do_not():
    assert len(FORGETS) == 14 and len(KEEPS) == 18 and not set(FORGETS) & set(KEEPS)
    hay, off = W.geonames(6000, 2000, 81)
    n = len(off) - 1
    m, o = RawMap(), Oracle()
    m.set_option("dense_min", 64)
    m.set_option("nm_dense", 64)
    m.put_many_packed(hay, off, np.arange(1, n + 1, dtype=np.uint32))
    o.put_many(hay, off)
    q, qo = W.queries(hay, off, 129, 82)
    assert m.get_option("ws_choice") == 0 and m.get_option("tuned_class") == -1
    rows, counts = m.find_batch_packed(q, qo, 10)
    info = m.device_info()
    assert info["n_windows"] <= 2 and info["n_bitmaps"] > 0, info
    assert m.get_option("ws_choice") != 0 and m.get_option("tuned_class") == 6     # the precondition: class 6 was measured
    assert m.get_option("ws_choice") >> 12 in (1, 3)

    def same_value(key):
        m.set_option(key, 0 if key in READ_ONLY else m.get_option(key))

    for key in KEEPS:
        before = m.get_option("ws_choice"), m.get_option("tuned_class"), m.get_option("tuned_nm_us"), m.get_option("retunes")
        same_value(key)
        after = m.get_option("ws_choice"), m.get_option("tuned_class"), m.get_option("tuned_nm_us"), m.get_option("retunes")
        assert after == before and after[0] != 0, key
    for key in FORGETS:
        assert m.get_option("ws_choice") != 0, key
        same_value(key)
        assert m.get_option("ws_choice") == 0, key
        assert m.get_option("tuned_class") == 6, key                               # (the last measurement's figures stay)
        rows, counts = m.find_batch_packed(q, qo, 10)                              # ... and the next batch measures again
        assert m.get_option("ws_choice") >> 12 in (1, 3) and m.get_option("last_sweep") == 1, key
    assert m.get_option("retunes") == 0
    want = o.batch(q, qo, limit=10)
    live = np.arange(10)[None, :] < want["counts"][:, None].astype(np.int64)
    assert np.array_equal(counts, want["counts"])
    assert np.array_equal(np.where(live[:, :, None], rows, 0), np.where(live[:, :, None], want["rows"], 0))
    m.close()
