"""The line bench.py prints is what the driver parses: short, numbers and tokens only, every contract key present.
(Round 5's line was 24 kB with prose in it and the driver recorded `parsed: null`.)"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline")


@pytest.fixture(scope="module")
def bench():
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        import bench as B
    finally:
        sys.argv = argv
    return B


@pytest.fixture(scope="module")
def canned():
    # a full record of a real run (round 5, the driver's flags): the input the compact line is built from
    with open(os.path.join(ROOT, "profiles", "r05_bench_driver_flags.json")) as fh:
        return json.load(fh)


def test_line_is_short_and_round_trips(bench, canned):
    line = bench.compact_line(canned)
    assert "\n" not in line
    assert len(line) <= 6000, len(line)
    back = json.loads(line)
    for k in CONTRACT:
        assert k in back, k
    assert back["value"] == pytest.approx(canned["value"], rel=1e-3)
    assert back["ms_per_step"] == pytest.approx(canned["ms_per_step"], rel=1e-3)
    assert back["config"]["workload"].startswith("configs[2]")
    rf = back["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "pmc", "kernel", "algorithmic_ratio"):
        assert k in rf, k
    assert rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"], rel=1e-3)
    cb = back["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample", "parity_checked", "parity_mismatches"):
        assert k in cb, k
    assert set(back["extra_configs"]) == set(canned["extra_configs"])
    for name in ("words", "skewed", "geonames_x4", "geonames_miss"):
        x = back["extra_configs"][name]
        assert x["value"] == pytest.approx(canned["extra_configs"][name]["value"], rel=1e-3)
        assert x["parity_mismatches"] == 0


def test_line_holds_no_prose(bench, canned):
    back = json.loads(bench.compact_line(canned))

    def strings(o):
        if isinstance(o, dict):
            for v in o.values():
                yield from strings(v)
        elif isinstance(o, list):
            for v in o:
                yield from strings(v)
        elif isinstance(o, str):
            yield o
    longest = max(strings(back), key=len)
    assert len(longest) <= 120, longest


def test_a_failed_leg_stays_visible_and_short(bench, canned):
    full = json.loads(json.dumps(canned))
    full["cpu_baseline"] = {"error": "RuntimeError('" + "x" * 5000 + "')"}
    full["extra_configs"]["skewed"] = {"error": "boom " * 2000}
    back = json.loads(bench.compact_line(full))
    assert "error" in back["cpu_baseline"] and len(back["cpu_baseline"]["error"]) <= 120
    assert "error" in back["extra_configs"]["skewed"]


def test_a_plain_line_carries_no_leg_of_full(bench, canned):
    """Without --full the record holds no roofline, CPU baseline, latency probes or extra configs: the line names none
    of them, and keeps every headline key."""
    plain = {k: v for k, v in canned.items() if k not in ("roofline", "cpu_baseline", "extra_configs", "mid_batch",
                                                            "p50_query_us", "p99_query_us", "latency_probes",
                                                            "host_buffer_queries_per_sec", "unpinned", "parity_checked")}
    back = json.loads(bench.compact_line(plain))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in back, k
    for k in ("roofline", "cpu_baseline", "extra_configs", "p50_query_us", "host_buffer_queries_per_sec"):
        assert k not in back, k
    assert back["value"] == pytest.approx(canned["value"], rel=1e-3)


def test_a_line_that_outgrows_the_limit_is_refused(bench, canned):
    full = json.loads(json.dumps(canned))
    full["config"]["workload"] = "w" * 7000
    with pytest.raises(RuntimeError):
        bench.compact_line(full)


def test_multi_rank_line_names_the_collective(bench, canned):
    full = json.loads(json.dumps(canned))
    full.pop("extra_configs"); full.pop("cpu_baseline")
    full.update(n_gpus=8, replicas=8, collective={"backend": "nccl", "world": 8, "rccl_version": "2.22.3", "distinct_devices": 8,
                                                  "op": "gather to rank 0 " * 10, "device_names": ["AMD Instinct MI355X"]},
                per_rank={"kernel_ms": [430.0] * 8, "gather_ms": [1.0] * 8}, gather_ms=1.0, gather_bytes_per_rank=124000000,
                gather_checked=2)
    back = json.loads(bench.compact_line(full))
    assert back["collective"] == {"backend": "nccl", "world": 8, "rccl_version": "2.22.3", "distinct_devices": 8}
    assert len(back["per_rank_kernel_ms"]) == 8


def test_dumped_outputs_are_the_rows_within_the_budget(bench, tmp_path, monkeypatch):
    """--dump-outputs: float64 rows (slots past the count zeroed) and counts; a batch over the budget is a fixed,
    seeded, sorted sample of its needles, the same every time."""
    import numpy as np
    rng = np.random.default_rng(1)
    n, limit = 1000, 4
    rows = rng.integers(1, 2**32, size=(n, limit, 3), dtype=np.uint64).astype(np.uint32)
    counts = rng.integers(0, limit + 1, size=n).astype(np.uint32)
    bench.dump_outputs(str(tmp_path / "all"), rows, counts, limit)
    got = {k: np.load(tmp_path / "all" / f"{k}.npy") for k in ("rows", "counts", "needle_index")}
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["needle_index"], np.arange(n)) and np.array_equal(got["counts"], counts)
    live = np.arange(limit)[None, :] < counts[:, None]
    assert np.array_equal(got["rows"], np.where(live[:, :, None], rows, 0))       # u32 values exact in float64
    monkeypatch.setattr(bench, "DUMP_BYTES", 100 * 8 * (3 * limit + 2) + 3 * 1024)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), rows, counts, limit)
    idx = np.load(tmp_path / "a" / "needle_index.npy")
    assert len(idx) == 100 and np.all(np.diff(idx) > 0)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BYTES
    for k in ("rows", "counts", "needle_index"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "rows.npy"), got["rows"][idx.astype(np.int64)])
