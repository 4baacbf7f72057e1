"""The bytes of the training job tables are pinned: scripts/describe_job_tables.py builds the ten tables of train.py and SparseDenseBatch
at small shapes and describes every record, every owned buffer (as built, and after reset()), every per-job view and state_tensors();
tests/golden/job_table_layout.json is that description at the commit BEFORE the tables moved onto job_table.JobTable.  The tables a
sweep shard builds and the generators' (kernel_regression.py, stats.py, gemm.py, graphs.py, synth.py, csbmh.py, SparseDenseBatch) are pinned
the same way by tests/golden/job_table_layout_sweep.json (describe_sweep(), written at the commit before THEY moved)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what the base gives the tables that had no reset() / state_tensors() of their own when the fixture was written (so the fixture is silent
# about them): reset() puts back what the constructor left, and a run rewinds XentEvalBatch.best and AdamBatch.moments - what
# SplitTrainBatch.capture() listed by hand
NEW_STATE = {"XentEvalBatch": ["best"], "AdamBatch": ["moments"]}


@pytest.fixture(scope="module")
def describer():
    spec = importlib.util.spec_from_file_location("describe_job_tables", os.path.join(ROOT, "scripts", "describe_job_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def described(describer):
    return json.loads(json.dumps(describer.describe_all()))  # (through JSON: tuples and lists compare alike)


@pytest.mark.gpu
def test_every_table_is_laid_out_as_in_the_fixture(described):
    with open(os.path.join(ROOT, "tests", "golden", "job_table_layout.json")) as f:
        want = json.load(f)
    assert sorted(described) == sorted(want)
    for label, got in described.items():
        kind = label.split(" ")[0]
        if "buffers_after_reset" not in want[label] and "buffers_after_reset" in got:
            assert got.pop("buffers_after_reset") == got["buffers"], label
        if "state_tensors" not in want[label] and "state_tensors" in got:
            assert got.pop("state_tensors") == NEW_STATE.get(kind, []), label
        assert got == want[label], label


@pytest.mark.gpu
def test_every_sweep_table_is_laid_out_as_in_the_fixture(describer):
    with open(os.path.join(ROOT, "tests", "golden", "job_table_layout_sweep.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(describer.describe_sweep()))
    assert sorted(got) == sorted(want)
    for label in want:
        if "buffers_after_reset" not in want[label] and "buffers_after_reset" in got[label]:  # (SparseDenseBatch: what the base gives, as above)
            assert got[label].pop("buffers_after_reset") == got[label]["buffers"], label
            assert got[label].pop("state_tensors") == [], label
    for label in want:
        assert got[label] == want[label], label
