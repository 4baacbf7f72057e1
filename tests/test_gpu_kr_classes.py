"""Class windows on the device: kernel regressions of 9 .. 16 classes as two window jobs of 8 class columns each over the solvers'
window instantiations (csrc/kernel_reg.hip, csrc/kernel_reg_large_windows.hip) and the combine pass (csrc/kr_combine.hip), through
KrBatch(class_windows=True).  The probe oracle (tests/_kr_probe.py, cases: tests/_kr_classes_cases.py) makes every check an exact
integer: the hit problem counts its probes, the control problem 0, the flags word is the configuration's."""
import numpy as np
import pytest
import torch

import _kr_probe as kp
import _kr_classes_cases as kc
from test_gpu_kr_solver import Built

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from wdg_amd import ops as o
    return o


def _table(kb):
    from wdg_amd.kernel_regression import _KR_JOB_DTYPE
    return kb.table.cpu().numpy().view(_KR_JOB_DTYPE).copy()


def _launch(ops, problems, classes, route="auto", patch=None):
    """one windowed table (n_classes patched per window job: C is per job in wdg_kr_job) -> (correct, flags, table object)"""
    kb = ops.KrBatch(problems, 16, route=route, class_windows=True)
    assert kb.windowed and kb.n_table_jobs == 2 * len(problems) and kb.n_jobs == len(problems)
    tab = _table(kb)
    tab["n_classes"] = np.repeat(np.asarray(classes), 2)
    if patch is not None:
        patch(tab)
    kb.table.copy_(torch.from_numpy(tab.view(np.uint8)))
    kb.flags.fill_(-1)
    kb.correct.fill_(-7)
    kb.launch()
    torch.cuda.synchronize()
    return kb.correct[:kb.n_jobs].cpu().numpy(), kb.flags[:kb.n_jobs].cpu().numpy(), kb


def _check(ops, built, route="auto", label=""):
    problems, classes, want, want_flags = [], [], [], []
    for b in built:
        problems += b.problems()
        classes += [b.case.c] * 2
        want += b.want()
        want_flags += [b.case.flags] * 2
    got, flags, kb = _launch(ops, problems, classes, route)
    print(f"[kr classes] {label}: " + ", ".join(f"{b.case.name}: {got[2 * i]}/{b.case.n_probes} hit, {got[2 * i + 1]} control, flags "
                                                 f"{flags[2 * i]}" for i, b in enumerate(built)))
    assert got.tolist() == want and flags.tolist() == want_flags, (label, got.tolist(), want, flags.tolist(), want_flags)
    assert np.array_equal(kb.ridged().cpu().numpy(), (flags & 1) != 0) and np.array_equal(kb.deflated().cpu().numpy(), (flags & 2) != 0)
    assert np.array_equal(kb.dropped().cpu().numpy(), (flags & 4) != 0)
    return kb


# ------------------------------------------------------------------------------------------------ 1: register solver, plain entry
def test_register_solver_plain_entry(ops):
    """nt 1, 33, 97, 320 x C 9, 12, 16 (absent classes included): exact counts, flags 0"""
    rng = np.random.default_rng(500)
    cases = kc.window_cases([1, 33, 97, 320], (9, 12, 16), seed=401)
    assert sum(kc.cross_window_pairs(c) for c in cases) >= 50
    kb = _check(ops, [Built(c, rng) for c in cases], label="registers, plain")
    assert not kb.large and kb.ws is None


# ------------------------------------------------------------------------------------------------ 2: deflating entry
def test_register_solver_deflating_entry(ops):
    """labels mixed across the windows (a duplicate class labelled {2, 11}: mixed in both), a pure class in the second window, zero
    rows, and an all-zero block whose class 0 wins by the first maximum across the windows: counts and flags exact"""
    rng = np.random.default_rng(501)
    cases = [kc.mixed_window_case()] + kc.relabelled_deflation_cases()
    kb = _check(ops, [Built(c, rng) for c in cases], label="registers, deflating")
    assert not kb.large and kb.ws is not None


# ------------------------------------------------------------------------------------------------ 3: large solver
@pytest.fixture(scope="module")
def large_cases():
    return kc.window_cases([321, 609, 1024], (9, 16), seed=402)


def test_large_solver(ops, large_cases):
    """nt 321, 609, 1024 x C 9, 16 through route "large", and the mixed-window deflation case pushed through it"""
    rng = np.random.default_rng(502)
    kb = _check(ops, [Built(c, rng) for c in large_cases], route="large", label="large, plain")
    assert kb.large
    _check(ops, [Built(kc.mixed_window_case(), rng)], route="large", label="large, deflating")


# ------------------------------------------------------------------------------------------------ 4: window invariance
@pytest.mark.parametrize("route", ["registers", "large"])
def test_one_problem_three_ways(ops, route):
    """a problem whose train labels lie in 0 .. 7: the default table (8 classes), the windowed table of 16 classes with unchanged
    labels (the second window holds zero columns) and the one with every label + 8 (the first window does): equal counts and flags"""
    rng = np.random.default_rng(503)
    built = [Built(kc.low_window_case(nt, 60 + nt), rng) for nt in (33, 97)]
    problems = [p for b in built for p in b.problems()]
    want = [w for b in built for w in b.want()]
    kb = ops.KrBatch(problems, 8, route=route)
    kb.launch()
    plain = (kb.correct[:kb.n_jobs].cpu().numpy().tolist(), kb.flags[:kb.n_jobs].cpu().numpy().tolist())
    same = _launch(ops, problems, [16] * len(problems), route)
    moved = _launch(ops, [(k, tr, va, lab + 8) for k, tr, va, lab in problems], [16] * len(problems), route)
    assert plain[0] == want
    assert (same[0].tolist(), same[1].tolist()) == plain and (moved[0].tolist(), moved[1].tolist()) == plain
    # with 8 or fewer classes the argument changes nothing: one row per problem, the plain entries
    kb8 = ops.KrBatch(problems, 8, route=route, class_windows=True)
    assert not kb8.windowed and kb8.n_table_jobs == kb8.n_jobs and kb8.combine_table is None
    assert not _table(kb8)["class_base"].any() and not _table(kb8)["rows_out"].any()


@pytest.mark.parametrize("route", ["registers", "large"])
def test_relaunch_and_table_position_change_nothing(ops, route):
    """a windowed table relaunched: bit-identical window rows, counts and flags; and a problem answers the same alone and inside a
    table of 200 problems (several problems per workgroup: the register solver makes a problem's predictions, and stores its window
    rows, inside the next problem's factorisation)"""
    rng = np.random.default_rng(504)
    cases = kc.window_cases([33, 97], (12, 16), seed=403)
    built = [Built(c, rng) for c in cases]
    distinct = [p for b in built for p in b.problems()]
    classes = [b.case.c for b in built for _ in range(2)]
    want = [w for b in built for w in b.want()]
    alone = [_launch(ops, [p], [c], route) for p, c in zip(distinct, classes)]
    assert [int(a[0][0]) for a in alone] == want
    m = len(distinct)
    order = [(7 * i) % m if i % 3 else i % m for i in range(200)]
    got, flags, kb = _launch(ops, [distinct[i] for i in order], [classes[i] for i in order], route)
    assert got.tolist() == [want[i] for i in order] and not flags.any()
    for j, i in enumerate(order[:2 * m]):  # the window rows of a problem: those of the problem alone, bit for bit
        nv = distinct[i][2].shape[0]
        assert torch.equal(kb.rows[2 * j:2 * j + 2, :nv], alone[i][2].rows[:, :nv]), (j, i)
    first = (kb.rows.clone(), kb.win_correct.clone(), kb.win_flags.clone())
    kb.rows.fill_(-1), kb.correct.fill_(-7), kb.flags.fill_(-1)
    kb.launch()
    torch.cuda.synchronize()
    # (rows_out beyond a problem's n_val is never written: compared where the first launch wrote)
    for j, i in enumerate(order):
        nv = distinct[i][2].shape[0]
        assert torch.equal(kb.rows[2 * j:2 * j + 2, :nv], first[0][2 * j:2 * j + 2, :nv]), j
    assert torch.equal(kb.win_correct, first[1]) and torch.equal(kb.win_flags, first[2])
    assert kb.correct[:kb.n_jobs].cpu().numpy().tolist() == got.tolist() and not kb.flags[:kb.n_jobs].any()


def test_window_rows_against_the_restated_rule(ops):
    """the window jobs' rows_out and the combine pass against the numpy restatement (tests/_kr_classes_cases.py): per validation
    row the window that holds the designed arg-max reports it (the probes' margin protects that class alone; the other window's
    leader is not designed), every class lies inside its window, and the problem's count is the restated combine of the DEVICE's rows"""
    rng = np.random.default_rng(505)
    case = kc.window_cases([97], (12,), seed=404)[0]
    b = Built(case, rng)
    got, _flags, kb = _launch(ops, b.problems(), [12, 12])
    rows = kb.rows.cpu().numpy()
    values, classes = rows[..., 0].view(np.float32), rows[..., 1]
    for w in range(4):  # window jobs (problem 0, window 0), (0, 1), (1, 0), (1, 1)
        cb, cls = 8 * (w % 2), classes[w, :case.n_probes]
        assert ((cls >= cb) & (cls < min(cb + 8, 12))).all(), w
        mine = case.a // 8 == w % 2
        assert mine.any() and np.array_equal(cls[mine], case.a[mine]), w
    for j, lab in enumerate((case.a, case.b_)):
        assert kc.combine_restated(values[2 * j:2 * j + 2, :case.n_probes], classes[2 * j:2 * j + 2, :case.n_probes],
                                   kb.win_correct[2 * j:2 * j + 2].cpu().numpy(), kb.win_flags[2 * j:2 * j + 2].cpu().numpy(), lab)[0] == got[j]


# ------------------------------------------------------------------------------------------------ 5: refusals
def _refusals():
    def classes_17(tab):
        tab["n_classes"][2:4] = 17          # both window jobs of problem 1: more classes than two windows hold

    def base_4(tab):
        tab["class_base"][3] = 4            # not a multiple of 8

    def base_16(tab):
        tab["class_base"][3] = 16           # a multiple of 8, but >= n_classes

    def no_rows(tab):
        tab["rows_out"][2] = 0              # more than 8 classes without the per-row output
    return [classes_17, base_4, base_16, no_rows]


@pytest.mark.parametrize("route", ["registers", "large"])
def test_refusals(ops, route):
    """a malformed window job: its problem answers -1 with flags 0, the table's other problems are exact"""
    rng = np.random.default_rng(506)
    built = [Built(c, rng) for c in kc.window_cases([33], (12, 16), seed=405)]
    problems = [p for b in built for p in b.problems()]
    classes = [b.case.c for b in built for _ in range(2)]
    want = [w for b in built for w in b.want()]
    assert want[1] == 0 and want[0] > 0
    for patch in _refusals():
        got, flags, kb = _launch(ops, problems, classes, route, patch=patch)
        assert got[1] == -1 and flags[1] == 0, (patch.__name__, got.tolist(), flags.tolist())
        assert [got[0], got[2], got[3]] == [want[0], want[2], want[3]] and not flags[[0, 2, 3]].any(), (patch.__name__, got.tolist())
        with pytest.raises(RuntimeError):
            kb.accuracy()
    with pytest.raises(ValueError):
        ops.KrBatch(problems, 17, route=route, class_windows=True)
    with pytest.raises(ValueError):
        ops.KrBatch(problems, 12, route=route)


# ------------------------------------------------------------------------------------------------ 6: the API
def _synthetic_graph():
    """N = 480, 12 balanced classes, F = 160 continuous features (no duplicate rows; full rank at the ~120 train rows of
    sample_max = 200), a sparse directed adjacency in which every node has an edge in either direction: no aggregated row is all
    zero.  (A zero row makes a train block exactly singular: there the reference's fp32 pinv and the device's deflation part ways
    by design - DESIGN.md 4.8, measured on texas -, which is not what the class windows are about.)"""
    rng = np.random.default_rng(12)
    n, f, c = 480, 160, 12
    lab = torch.from_numpy(np.arange(n) % c)
    x = torch.from_numpy((rng.standard_normal((n, f)) + 2.0 * np.eye(c, f)[lab.numpy()]).astype(np.float32))
    ring = np.arange(n)
    src = np.concatenate([rng.integers(0, n, 2400), ring, (ring + c) % n])
    dst = np.concatenate([(src[:2400] + c * rng.integers(1, 6, 2400)) % n, (ring + c) % n, ring])  # (mostly the same class: the aggregated features carry signal too)
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.stack([src, dst])), torch.ones(src.shape[0]), (n, n)).coalesce()
    return x, adj, lab


def _api_call(clf, solver, class_windows, epochs=6):
    from wdg_amd.utils import homophily_metrics as hm
    x, adj, lab = _synthetic_graph()
    torch.manual_seed(21)
    accs = []
    orig = hm.accuracy
    hm.accuracy = lambda l_, o_, _o=orig, _a=accs: (_a.append(float(_o(l_, o_))), _o(l_, o_))[1]
    hm.LAST_KR_ACCURACIES = None
    try:
        p, _ = hm.classifier_based_performance_metric(x, adj, lab, 200.0, base_classifier=clf, epochs=epochs, solver=solver,
                                                      class_windows=class_windows)
    finally:
        hm.accuracy = orig
    return float(p), accs, hm.LAST_KR_ACCURACIES


@pytest.mark.parametrize("clf", ["kernel_reg1", "kernel_reg0"])
def test_api_metric_with_twelve_classes(clf):
    """classifier_based_performance_metric(class_windows=True) on a 12-class graph stays on the device; per-epoch accuracies within 2
    validation rows of solver="host" on the same generator state (the margin tests/test_gpu_api.py and tests/test_gpu_kr_large.py
    give the device over the host route), p within what that implies.  Without the switch the call takes the host path.
    Measured on the MI355X with this graph's first version (random edges only: one node without out-edges, two without in-edges,
    so that some graph-aware train blocks were exactly singular): kernel_reg1 7 of 84 validation rows from the host route in the
    worst epoch, no block ridged, the features-only column equal to an fp64 solve of the same blocks in every epoch.  The graph then
    got its ring of edges (no zero and no duplicate aggregated rows); that version has not been run on a device yet."""
    from _golden import p_tolerance
    from wdg_amd.utils import homophily_metrics as hm
    p_host, accs, last = _api_call(clf, "host", True)
    assert last is None and len(accs) == 12
    host = np.asarray(accs, np.float64).reshape(-1, 2)
    p_dev, _accs, last = _api_call(clf, "device", True)
    assert last is not None
    dev = last.numpy().astype(np.float64)
    from wdg_amd.utils.util_funcs import kernel_regression_epoch_indices
    x, adj, lab = _synthetic_graph()
    torch.manual_seed(21)
    sets = kernel_regression_epoch_indices(lab, 200.0, 6)
    n_val = float(sets[0][1].shape[0])
    assert all(va.shape[0] == n_val and 100 <= tr.shape[0] <= 140 for tr, va in sets), [(tr.shape[0], va.shape[0]) for tr, va in sets]
    rows = np.abs(dev - host).max() * n_val
    print(f"[kr classes] api {clf}: device within {rows:.2f} rows of the host route; p {p_dev:.6f} vs {p_host:.6f}; ridged {hm.LAST_KR_RIDGED}")
    assert rows <= 2 + 0.01, (clf, dev, host)
    assert abs(p_dev - p_host) <= p_tolerance(host[:, 0], host[:, 1], n_val, 2), (p_dev, p_host)
    # without the switch: the host path, no device regression
    p_off, accs_off, last = _api_call(clf, "device", None)
    assert last is None and len(accs_off) == 12 and p_off == p_host
    assert hm._kernel_regression_on_device(x, adj, lab, 200.0, clf, 2) is None


def test_cli_flag(tmp_path, monkeypatch):
    """homophily_tests.py --kr_class_windows reaches the metric: the 12-class graph runs on the device"""
    from wdg_amd import homophily_tests as ht
    from wdg_amd.utils import homophily_metrics as hm
    x, adj, lab = _synthetic_graph()
    idx = adj.indices().numpy()
    path = str(tmp_path / "twelve.npz")
    np.savez(path, adj_row=idx[0], adj_col=idx[1], labels=lab.numpy(), features=x.numpy())
    seen = {}
    orig = hm.classifier_based_performance_metric

    def spy(*a, **k):
        seen["class_windows"] = k.get("class_windows")
        k["epochs"] = 2
        return orig(*a, **k)
    monkeypatch.setattr(hm, "classifier_based_performance_metric", spy)
    monkeypatch.delenv("WDG_KR_CLASS_WINDOWS", raising=False)
    for argv, want_device in ((["--kr_class_windows"], True), ([], False)):
        hm.LAST_KR_ACCURACIES = None
        torch.manual_seed(5)
        lvl = ht.main(["--dataset_name", path, "--homophily_metric", "kernel_reg1_based_homo", "--sample_max", "200"] + argv)
        assert 0.0 <= float(lvl) <= 1.0
        assert seen["class_windows"] is (True if want_device else None)
        assert (hm.LAST_KR_ACCURACIES is not None) == want_device
