"""bench.py's ONE stdout line stays small and strictly parseable (the 23-KB line of round 5 came back
`parsed: null` from the driver).  The canned record is round 5's own full line (profiles/r05_bench_driver_flags.json)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (imports nothing that needs a GPU at module level)

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline")


def canned():
    text = open(os.path.join(ROOT, "profiles", "r05_bench_driver_flags.json")).read()
    rec = json.loads([l for l in text.splitlines() if l.lstrip().startswith("{")][-1])
    assert len(json.dumps(rec)) > 20000  # the record that did not parse
    return rec


def strict(text):
    def refuse(c):
        raise ValueError(c)
    return json.loads(text, parse_constant=refuse)  # NaN / Infinity are not JSON


def test_line_is_small_strict_json_with_every_contract_key():
    rec = canned()
    line = bench.compact_line(rec, "gpurun_out/bench_detail.json")
    assert "\n" not in line and len(line) < 6000, len(line)
    got = strict(line)
    for k in CONTRACT:
        assert k in got, k
    assert got["value"] == float(f"{rec['value']:.6g}") and got["unit"] == "edges/s" and got["dtype"] == "f32"
    rl = got["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rl, k
    assert abs(rl["frac"] - rl["achieved"] / rl["peak"]) < 1e-4
    cb = got["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert set(got["config"]) <= {"workload", "graphs_per_step_per_gpu", "edges_per_step_per_gpu", "parallelism"}
    assert len(got["config"]["workload"]) <= 200
    # one number per side block
    assert got["sweep_whole"]["seconds"] > 0 and got["train"]["SGC-1"] > 0 and got["secondary"]["ms_per_step"] > 0
    assert all(len(v) == 2 for v in got["configs"].values())


def test_nan_and_oversized_blocks_cannot_break_the_line():
    rec = canned()
    rec["ms_per_step"] = float("nan")
    rec["configs"] = {f"config {i} " + "x" * 80: {"us": 1.0, "roofline": {"frac": 0.5}} for i in range(200)}
    line = bench.compact_line(rec)
    got = strict(line)
    assert len(line) < 6000 and got["ms_per_step"] is None and "configs" not in got
    for k in CONTRACT:
        assert k in got, k


def test_multi_gpu_record_keeps_the_measured_strong_speedup():
    rec = {k: v for k, v in canned().items() if k in CONTRACT and k != "cpu_baseline"}
    rec.update(n_gpus=8, sweep_whole={"jobs": 1680, "n_gpus": 8, "scaling": "strong", "seconds": 0.05, "one_gpu_s": 0.3,
                                      "strong_speedup_vs_1gpu": 6.0, "rows_equal_one_gpu": True, "per_rank_s": [0.05] * 8,
                                      "workload": "w" * 900})
    got = strict(bench.compact_line(rec))
    assert got["sweep_whole"]["strong_speedup_vs_1gpu"] == 6.0 and got["sweep_whole"]["rows_equal_one_gpu"] is True
    assert "workload" not in got["sweep_whole"] and "cpu_baseline" not in got


def test_plain_run_line_keeps_the_headline_keys_without_the_full_blocks():
    """a run without --full measures no roofline, no CPU baseline and no side block: the line still carries the headline's keys
    and no empty `roofline`"""
    rec = {k: v for k, v in canned().items() if k in CONTRACT and k not in ("roofline", "cpu_baseline")}
    got = strict(bench.compact_line(rec))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert k in got, k
    assert got["ms_per_step"] > 0 and "roofline" not in got and "cpu_baseline" not in got and "detail" not in got


def test_dump_outputs_are_float32_npy_files_under_the_size_limit(tmp_path):
    import numpy as np
    import pytest
    outs = {"results": np.arange(12, dtype=np.float64).reshape(4, 3), "logits": np.ones((2, 5, 5), np.float32)}
    bench.write_outputs(outs, str(tmp_path / "d"))
    for name, a in outs.items():
        got = np.load(tmp_path / "d" / f"{name}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32))
    with pytest.raises(SystemExit):
        bench.write_outputs({"y_sample": np.zeros(bench.DUMP_LIMIT // 4 + 1, np.float32)}, str(tmp_path / "big"))
    assert not (tmp_path / "big").exists()


def test_help_lists_full_and_dump_outputs():
    import subprocess
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "--full" in res.stdout and "--dump-outputs" in res.stdout
