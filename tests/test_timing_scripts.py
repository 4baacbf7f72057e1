"""Every scripts/time_*.py imports without a device and without the built library, and the child processes that the ported scripts
would start - (key, step, time limit in seconds, extra argv), in order - are the ones their main() bodies started before the runner
moved to scripts/_timing.py."""
import glob
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
ALL = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(SCRIPTS, "time_*.py")))


def _plain(*steps):
    return [(s, s, limit, ()) for s, limit in steps]


G = lambda group: ("--group", group)  # noqa: E731
SPARSE, DENSE = ("--arm", "sparse"), ("--arm", "dense")

# with the scripts' default arguments
EXPECTED = {
    "time_acm": [("shard acm 1", "shard", 300, G("acm")), ("shard base 1", "shard", 300, G("base")), ("shard acm 2", "shard", 300, G("acm")),
                 ("shard base 2", "shard", 300, G("base")), ("kernel", "kernel", 240, ())],
    "time_acm_split_train": _plain(("kernel", 180), ("epoch", 420)),
    "time_auc": _plain(("kernel", 300), ("switch", 240), ("default", 240), ("default", 240), ("default", 240), ("default", 240)),
    "time_drop_edge": _plain(("kernels", 240), ("epochs", 240), ("accuracy", 420)),
    "time_dropout": [("shard new 1", "shard", 420, ()), ("kernel", "kernel", 300, ())],
    "time_gat": _plain(("layers", 300), ("epoch", 240), ("accuracy", 420)),
    "time_gat_split": _plain(("scores", 200), ("epoch", 360)),
    "time_gcnii": _plain(("errors", 120), ("layers", 240), ("epochs", 240), ("accuracy", 300)),
    "time_grid_train": _plain(("grid", 420), ("stages", 180), ("adam", 180)),
    "time_head_train": _plain(("shard", 600), ("table", 600)),
    "time_keep_best": _plain(("kernel", 240), ("default", 300), ("default", 300), ("optin", 600)),
    "time_knn": _plain(("select", 300), ("graphs", 420), ("behaviour", 420)),
    "time_neighbor_max": _plain(("kernels", 300), ("split", 120), ("epochs", 240), ("accuracy", 420)),
    "time_neighbor_sample": _plain(("kernels", 240), ("aggregation", 120), ("epochs", 240), ("accuracy", 420)),
    "time_poly_filter": _plain(("filters", 300), ("accuracy", 300)),
    "time_signed_att": _plain(("layers", 300), ("accuracy", 480)),
    "time_sparse_first_layer": [("products", "products", 300, SPARSE), ("tail", "tail", 180, SPARSE)] + [("epoch", "epoch", 240, DENSE), ("epoch", "epoch", 240, SPARSE)] * 4,
    "time_split_train": _plain(("epoch", 420), ("kernel", 180)),
    "time_two_hop": _plain(("build", 420), ("accuracy", 420), ("torch", 240)),
    "time_xent_curve": _plain(("kernel", 240), ("default", 300), ("default", 300), ("default", 300), ("default", 300), ("optin", 600)),
}
NO_RUNNER = ["time_csbmh", "time_feature_upload", "time_job_tables", "time_kr_classes", "time_kr_large", "time_svm", "time_synth_device"]


def _module(name):
    if SCRIPTS not in sys.path:
        sys.path.insert(0, SCRIPTS)
    return importlib.import_module(name)


def _steps(name, argv=()):
    m = _module(name)
    return m.invocations(m.parse(list(argv)))


def test_the_tables_cover_every_script():
    assert ALL == sorted(list(EXPECTED) + NO_RUNNER)


@pytest.mark.parametrize("name", ALL)
def test_imports_without_a_device(name):
    _module(name)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_invocations_with_default_arguments(name):
    m = _module(name)
    steps = _steps(name)
    assert [(s.key, s.step, s.limit, tuple(s.argv)) for s in steps] == EXPECTED[name]
    assert all(s.tree in (None, ROOT) for s in steps)
    assert {s.step for s in steps} <= set(m.STEP_FNS)


def test_head_train_keeps_its_table():
    assert _module("time_head_train").STEPS == (("shard", 600), ("table", 600))


def test_steps_selects_and_orders():
    assert [(s.key, s.limit) for s in _steps("time_neighbor_max", ["--steps", "epochs,kernels"])] == [("epochs", 240), ("kernels", 300)]


def test_dropout_with_a_parent(tmp_path):
    parent = str(tmp_path)
    steps = _steps("time_dropout", ["--parent-root", parent])
    assert [(s.key, s.step, s.limit) for s in steps] == [("shard new 1", "shard", 420), ("shard parent 1", "shard", 420), ("shard new 2", "shard", 420),
                                                         ("shard parent 2", "shard", 420), ("kernel", "kernel", 300)]
    for s in steps:
        in_parent = "parent" in s.key
        assert s.tree == (parent if in_parent else ROOT)
        assert tuple(s.argv) == (("--parent",) if in_parent else ())


@pytest.mark.parametrize("name,first,last", [("time_keep_best", 1, 5), ("time_xent_curve", 1, 9), ("time_auc", 2, 10)])
def test_default_path_with_a_parent(tmp_path, name, first, last):
    parent = str(tmp_path)
    steps = _steps(name, ["--parent", parent])
    assert len(steps) == (last if name == "time_auc" else last + 1)
    for i, s in enumerate(steps):
        if first <= i < last:  # parent, new, parent, new, ...
            assert s.step == "default" and s.tree == (parent if (i - first) % 2 == 0 else ROOT)
        else:
            assert s.step != "default" and s.tree == ROOT


def test_sparse_first_layer_with_a_parent(tmp_path):
    parent = str(tmp_path)
    steps = _steps("time_sparse_first_layer", ["--parent", parent, "--processes", "2"])
    assert [(s.step, tuple(s.argv), s.tree) for s in steps] == [("products", SPARSE, ROOT), ("tail", SPARSE, ROOT)] + [("epoch", DENSE, parent), ("epoch", SPARSE, ROOT)] * 2


def test_only_the_shared_module_starts_processes():
    for name in ALL:
        with open(os.path.join(SCRIPTS, name + ".py")) as f:
            assert "subprocess" not in f.read(), name
