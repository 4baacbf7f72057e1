"""The step runner of scripts/_timing.py, driven by a throw-away script whose steps are plain Python: what it assembles when every
step succeeds, and that NOTHING more is started after a step that fails, runs into its limit, or fails after writing its part."""
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")

SCRIPT = '''
import argparse, json, os, sys, time
sys.path.insert(0, %r)
from _timing import Step, flags, run_step, run_steps, write


def step_ok(a):
    return {"value": a.value, "argv": sys.argv[1:], "path0": sys.path[0]}


def step_exit3(a):
    sys.exit(3)


def step_sleep(a):
    time.sleep(30)
    return {}


def step_write_then_fail(a):
    with open(a.part, "w") as f:
        json.dump({"value": "stale"}, f)
    sys.exit(5)


def step_marker(a):
    open(a.marker, "w").close()
    return {"ran": True}


STEP_FNS = {"ok": step_ok, "exit3": step_exit3, "sleep": step_sleep, "write_then_fail": step_write_then_fail, "marker": step_marker}

ap = argparse.ArgumentParser()
ap.add_argument("--value", type=int, default=7)
ap.add_argument("--marker")
ap.add_argument("--echo")
ap.add_argument("--plan", help="JSON: [[key, step, limit, [argv], tree or null]]")
ap.add_argument("--step")
ap.add_argument("--tree", default=%r)
ap.add_argument("--part")
ap.add_argument("--out")
a = ap.parse_args()
if a.step:
    run_step(a, STEP_FNS, a.tree, device=False)
else:
    steps = [Step(k, s, limit, tuple(argv), tree) for k, s, limit, argv, tree in json.loads(a.plan)]
    write(a.out, dict(run_steps(__file__, steps, flags(a, "value", "marker"), a.out)))
''' % (SCRIPTS, ROOT)


def _run(tmp_path, plan):
    script, out, marker = tmp_path / "throwaway.py", tmp_path / "doc" / "out.json", tmp_path / "marker"
    script.write_text(SCRIPT)
    p = subprocess.run([sys.executable, str(script), "--plan", json.dumps(plan), "--marker", str(marker), "--out", str(out)], capture_output=True, text=True)
    doc = json.loads(out.read_text()) if out.exists() else None
    return p, doc, marker.exists(), glob.glob(str(tmp_path / "doc" / "*.part"))


def test_all_steps_succeed(tmp_path):
    p, doc, marker, parts = _run(tmp_path, [["first", "ok", 20, [], None], ["second", "marker", 20, [], None], ["third", "ok", 20, [], None]])
    assert p.returncode == 0, p.stderr
    assert list(doc) == ["first", "second", "third"]
    assert doc["first"]["value"] == 7 and doc["second"] == {"ran": True} and doc["third"]["value"] == 7
    assert marker and parts == []


def _stopped_at_second(tmp_path, step, limit, status):
    p, doc, marker, parts = _run(tmp_path, [["first", "ok", 20, [], None], ["second", step, limit, [], None], ["third", "marker", 20, [], None]])
    assert p.returncode != 0
    assert f"step 'second' ended with status {status}: stopping" in p.stderr
    assert list(doc) == ["first", "second"]
    assert doc["first"]["value"] == 7
    assert doc["second"] == f"not measured: the step ended with status {status}"
    assert not marker  # the third step was never started
    assert parts == []


def test_a_failing_step_ends_the_run(tmp_path):
    _stopped_at_second(tmp_path, "exit3", 20, 3)


def test_a_step_past_its_limit_ends_the_run(tmp_path):
    _stopped_at_second(tmp_path, "sleep", 1, 124)


def test_a_part_written_before_the_failure_is_removed_and_not_used(tmp_path):
    _stopped_at_second(tmp_path, "write_then_fail", 20, 5)


def test_extra_argv_and_tree_reach_the_child(tmp_path):
    other = tmp_path / "checkout"
    other.mkdir()
    p, doc, _, parts = _run(tmp_path, [["here", "ok", 20, [], None], ["there", "ok", 20, ["--echo", "x y"], str(other)]])
    assert p.returncode == 0, p.stderr
    assert doc["here"]["path0"] == ROOT and "--tree" not in doc["here"]["argv"]
    assert doc["there"]["path0"] == str(other)
    argv = doc["there"]["argv"]
    assert argv[:2] == ["--step", "ok"] and argv[2] == "--part"
    assert argv[argv.index("--echo") + 1] == "x y" and argv[argv.index("--tree") + 1] == str(other)
    assert argv[argv.index("--value") + 1] == "7"  # (the pass-through arguments)
    assert parts == []
