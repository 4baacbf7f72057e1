"""The sweep driver is four modules (sweep_jobs <- sweep_batch <- kr_plan <- sweep); `wdg_amd.sweep` still serves every name it had as
one file, the moved ones as the SAME objects as in their home modules, and the job-list module needs neither the library nor ops."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# dir() of the one-file sweep module, minus what it imported from the standard library, numpy and torch
SWEEP_NAMES = (
    "BaseSweep", "JOB_ROW_COST", "Job", "KrPlan", "METRIC_NAMES", "PAIR_COST_PER_ENTRY_US", "PAIR_COST_US", "SAMPLE_COST_US",
    "STEP_METRICS", "SYNTH_TAG", "SweepBatch", "TrainBatch", "WdgError", "_GramPair", "_InFlight", "_PAIRS_MEMO", "_PIPE_STREAMS",
    "_PrelaunchedGram", "_SHARD_MEMO", "_SIDE_STREAMS", "_check_generate", "_generated_labels", "_mix64", "_pipe_streams",
    "_queue_graphs", "_route_propagates", "_shard_owner", "_side_stream", "_take_graphs", "_upload_features", "_upload_features_of",
    "_visit_order", "broadcast_jobs", "decode_jobs", "encode_jobs", "exchange_rows", "gather_results", "job_cost", "make_jobs",
    "pairs_of_rank", "propagates", "run_bases", "run_shards", "shard_jobs", "shard_pairs", "synth", "synth_seed", "synth_specs",
    "welch_p_values", "whole_sweep_rank")

# where the classes, functions and tables that left sweep.py live now
HOME = {
    "sweep_jobs": ("JOB_ROW_COST", "Job", "METRIC_NAMES", "PAIR_COST_PER_ENTRY_US", "PAIR_COST_US", "SAMPLE_COST_US", "STEP_METRICS",
                   "SYNTH_TAG", "_PAIRS_MEMO", "_SHARD_MEMO", "_check_generate", "_generated_labels", "_mix64", "_shard_owner",
                   "broadcast_jobs", "decode_jobs", "encode_jobs", "exchange_rows", "gather_results", "job_cost", "make_jobs",
                   "shard_jobs", "shard_pairs", "synth_seed", "synth_specs"),
    "sweep_batch": ("BaseSweep", "SweepBatch", "_SIDE_STREAMS", "_side_stream", "_upload_features", "_upload_features_of"),
    "kr_plan": ("KrPlan", "_GramPair", "_PrelaunchedGram", "_route_propagates", "propagates", "welch_p_values"),
    "train_batch": ("TrainBatch",),
}
STAYED = ("_InFlight", "_PIPE_STREAMS", "_pipe_streams", "_queue_graphs", "_take_graphs", "_visit_order", "pairs_of_rank", "run_bases",
          "run_shards", "whole_sweep_rank")


def test_sweep_serves_every_name_it_had():
    from wdg_amd import sweep
    missing = [n for n in SWEEP_NAMES if not hasattr(sweep, n)]
    assert not missing, missing


def test_moved_names_are_their_home_modules_objects():
    import importlib

    from wdg_amd import sweep
    for module, names in HOME.items():
        home = importlib.import_module("wdg_amd." + module)
        for n in names:
            assert getattr(sweep, n) is getattr(home, n), (module, n)
    for n in STAYED:
        assert getattr(getattr(sweep, n), "__module__", sweep.__name__) == sweep.__name__, n  # (a table has no __module__)
    # every listed name is accounted for: moved, kept, or an import of the one-file module that was not its own (synth, WdgError)
    homed = {n for names in HOME.values() for n in names}
    assert homed | set(STAYED) | {"synth", "WdgError"} == set(SWEEP_NAMES)


def test_job_list_module_imports_without_library_or_ops():
    code = ("import sys; sys.path.insert(0, %r); import wdg_amd.sweep_jobs as m; "
            "bad = sorted(n for n in sys.modules if n in ('wdg_amd.ops', 'wdg_amd._lib', 'wdg_amd.sweep', 'wdg_amd.sweep_batch')); "
            "assert not bad, bad; assert m.shard_jobs(m.make_jobs([0.1, 0.5], [0, 1]), 2, 0); print('ok')" % ROOT)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stderr[-2000:]
