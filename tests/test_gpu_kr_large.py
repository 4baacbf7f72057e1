"""The kernel-regression solver of up to 1024 train rows (csrc/kernel_reg_large.hip: kr_large_solve_kernel, kr_large_deflate_kernel)
through KrBatch, probe by probe (tests/_kr_probe.py, tests/_kr_probe_large.py) as tests/test_gpu_kr_solver.py asks the 320-row
solver: every problem twice - validation rows labelled with their designed arg-max (hit count = n_val exactly) and with their
runner-up (hit count = 0 exactly) - and the flags word the configuration predicts; then a mixed table longer than the device has
CUs, and the fp64 pseudo-inverse on arc-cosine kernels."""
import numpy as np
import pytest
import torch

import _kr_probe as kp
import _kr_probe_large as kl
from test_gpu_kr_solver import Built, _dev, _identity_rep

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from wdg_amd import ops as o
    return o


def _launch(ops, problems, classes, route="auto"):
    """one table (n_classes patched per job) -> (correct, flags) host arrays, the batch"""
    from wdg_amd.kernel_regression import _KR_JOB_DTYPE
    kb = ops.KrBatch(problems, 8, route=route)
    tab = kb.table.cpu().numpy().view(_KR_JOB_DTYPE).copy()
    tab["n_classes"] = classes
    kb.table.copy_(torch.from_numpy(tab.view(np.uint8)))
    kb.flags.fill_(-1)
    kb.correct.fill_(12345)
    kb.launch()
    torch.cuda.synchronize()
    return kb.correct[:kb.n_jobs].cpu().numpy(), kb.flags[:kb.n_jobs].cpu().numpy(), kb


def _check(ops, built, with_rep=None, label="", route="auto", large=True):
    """one table of every case's hit and control problem: exact counts and flags (each figure printed before it is asserted)"""
    with_rep = [True] * len(built) if with_rep is None else with_rep
    problems, classes, want, want_flags = [], [], [], []
    for b, wr in zip(built, with_rep):
        problems += b.problems(wr)
        classes += [b.case.c] * 2
        want += b.want()
        want_flags += [b.case.flags if wr else 0] * 2
    got, flags, kb = _launch(ops, problems, classes, route)
    assert kb.large == large
    assert np.array_equal(kb.dropped().cpu().numpy(), (flags & 4) != 0)
    for i, b in enumerate(built):
        print(f"[kr large] {label}: {b.case.name} (rho {b.case.rho:g}): counts {got[2 * i:2 * i + 2].tolist()} want {want[2 * i:2 * i + 2]} "
              f"flags {flags[2 * i:2 * i + 2].tolist()} want {want_flags[2 * i]}")
    bad = [(b.case.name, got[2 * i:2 * i + 2].tolist(), want[2 * i:2 * i + 2], flags[2 * i:2 * i + 2].tolist(), want_flags[2 * i])
           for i, b in enumerate(built)
           if got[2 * i:2 * i + 2].tolist() != want[2 * i:2 * i + 2] or flags[2 * i:2 * i + 2].tolist() != [want_flags[2 * i]] * 2]
    assert not bad, (label, bad)
    return got, flags


# ------------------------------------------------------------------------------------------------ 3: the new cases, route "auto"
@pytest.mark.parametrize("family", ["spd", "spread", "deflate", "ridge"])
def test_blocks_of_321_to_1024_rows_through_krbatch(ops, family):
    """every case of tests/_kr_probe_large.py as a hit and a control problem: exact counts (n_probes, 0) and the designed flags word;
    a table whose largest block has more than 320 rows goes, whole, through the large entry"""
    rng = np.random.default_rng(200)
    cases = dict(kl.asserted_cases())[family]
    assert all(c.nt > ops.KrBatch.MAX_TRAIN for c in cases)
    _check(ops, [Built(c, rng) for c in cases], label=family)
    if family == "spread":  # every node its own representative: the pre-pass drops no row the solver can factor
        _check(ops, [Built(c, rng, rep=_identity_rep) for c in cases], label="spread deflating")


def test_more_than_1024_rows_and_unknown_routes_are_refused(ops):
    k = torch.eye(1100, device="cuda")
    lab = (torch.arange(1100, device="cuda") % 3).to(torch.int32)
    tr, va = torch.arange(1025, device="cuda", dtype=torch.int32), torch.arange(1025, 1100, device="cuda", dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.KrBatch([(k, tr, va, lab)], 3)
    with pytest.raises(ValueError):
        ops.KrBatch([(k, tr[:321], va, lab)], 3, route="registers")
    with pytest.raises(ValueError):
        ops.KrBatch([(k, tr[:100], va, lab)], 3, route="memory")
    with pytest.raises(ValueError):
        ops.KrBatch([(k, tr[:100], va, lab)], 9, route="large")
    kb = ops.KrBatch([(k, tr[:1024], va, lab)], 3)
    kb.launch()
    # (K = I: a validation row sees no train row, every prediction is 0 -> class 0 by the first maximum)
    assert kb.large and kb.correct[:1].cpu().tolist() == [int((lab[va.long()] == 0).sum())] and kb.flags[:1].cpu().tolist() == [0]


# ------------------------------------------------------------------------------------------------ 4: the existing families, route "large"
@pytest.fixture(scope="module")
def spd():
    return kp.spd_cases()


def test_existing_spd_blocks_through_the_large_route(ops, spd):
    rng = np.random.default_rng(100)
    _check(ops, [Built(c, rng) for c in spd], label="spd", route="large")


def test_existing_validation_counts_through_the_large_route(ops):
    rng = np.random.default_rng(101)
    case = kp.n_val_case()
    _check(ops, [Built(case.take(nv), rng) for nv in kp.N_VAL_EDGES], label="n_val", route="large")


def test_existing_unsorted_train_ids_through_the_large_route(ops, spd):
    rng = np.random.default_rng(102)
    _check(ops, [Built(c, rng, sort_train=False) for c in spd[1::3]], label="unsorted", route="large")


def test_existing_diagonal_spreads_through_the_large_route(ops):
    rng = np.random.default_rng(103)
    cases = kp.spread_cases()
    _check(ops, [Built(c, rng) for c in cases], label="spread plain", route="large")
    _check(ops, [Built(c, rng, rep=_identity_rep) for c in cases], label="spread deflating", route="large")


def test_existing_deflation_cases_through_the_large_route(ops):
    rng = np.random.default_rng(104)
    _check(ops, [Built(c, rng) for c in kp.deflation_cases()], label="deflate", route="large")


def test_existing_ridge_cases_through_the_large_route(ops):
    rng = np.random.default_rng(108)
    cases = kp.ridge_cases()
    assert [c.rho for c in cases] == [1e-3, 1e-1] and all(c.flags == kp.FLAG_RIDGE for c in cases)
    _check(ops, [Built(c, rng) for c in cases], label="ridge", route="large")


def test_existing_layouts_and_refusal_through_the_large_route(ops):
    """ldk = n + 13 and ldk = 65 535; ldk = 65 536 patched into a table: that problem answers -1 with flags 0"""
    from wdg_amd.kernel_regression import _KR_JOB_DTYPE
    rng = np.random.default_rng(106)
    built = []
    for c in kp.layout_cases()[:2]:
        n = c.nt + c.n_probes + 5
        built += [Built(c, rng, ld_extra=13), Built(c, rng, ld_extra=65535 - n)]
    _check(ops, built, label="layout", route="large")
    problems, classes = [], []
    for b in built:
        problems += b.problems()
        classes += [b.case.c] * 2
    kb = ops.KrBatch(problems, 8, route="large")
    tab = kb.table.cpu().numpy().view(_KR_JOB_DTYPE).copy()
    tab["n_classes"] = classes
    tab["ldk"][3] = 65536
    kb.table.copy_(torch.from_numpy(tab.view(np.uint8)))
    kb.flags.fill_(12345)
    kb.correct.fill_(12345)
    kb.launch()
    torch.cuda.synchronize()
    got, flags = kb.correct[:len(problems)].cpu().numpy(), kb.flags[:len(problems)].cpu().numpy()
    want = np.array(sum((b.want() for b in built), []))
    want[3] = -1
    assert got.tolist() == want.tolist() and flags.tolist() == [0] * len(problems)


# ------------------------------------------------------------------------------------------------ 5: one mixed table
def test_mixed_table_longer_than_the_device_equals_one_problem_launches(ops):
    """at least 600 problems (more than CUs) with 97, 320, 321, 600 and 1024 train rows mixed, plain and deflating: each answers what
    its own one-problem launch answers; a relaunch is bit-identical; every 7th problem patched to n_train 0 or 1025 in the device
    table answers -1 and disturbs no neighbour"""
    from wdg_amd.kernel_regression import _KR_JOB_DTYPE
    rng = np.random.default_rng(205)
    cus = int(ops.lib.wdg_device_cus())
    pool = []
    for i, nt in enumerate((97, 320, 321, 600, 1024)):
        c = kp.C_ROTATION[(i + 1) % len(kp.C_ROTATION)]
        case = kp.Case(f"mixed nt={nt}", kp.spd_block(rng, nt, 10.0), kp._labels(rng, nt, c, set()), c, rng, per_window=1)
        pool.append(Built(case, rng, ld_extra=3 * i))
    pool.append(Built(kl.deflation_large_cases()[0], rng, ld_extra=5))
    pool.append(Built(kp.deflation_cases()[2], rng))
    items = []
    for b in pool:
        for p in b.problems(with_rep=True):
            items.append((p, b.case.c))
    n_items = max(600, cus + 17)
    reps = -(-n_items // len(items))
    items = items * reps
    items = [items[i] for i in rng.permutation(len(items))]
    assert len(items) >= 600 and len(items) > cus
    one = {}
    for p, c in items:
        key = tuple(int(t.data_ptr()) if t is not None else 0 for t in p)
        if key not in one:
            g1, f1, _ = _launch(ops, [p], [c], route="large")
            one[key] = (int(g1[0]), int(f1[0]))
    want = np.array([one[tuple(int(t.data_ptr()) if t is not None else 0 for t in p)] for p, _ in items])
    got, flags, kb = _launch(ops, [p for p, _ in items], [c for _, c in items])
    assert kb.large and kb.ws is not None
    assert np.array_equal(got, want[:, 0]) and np.array_equal(flags, want[:, 1])
    kb.launch()  # relaunch: bit-identical
    torch.cuda.synchronize()
    assert np.array_equal(kb.correct[:kb.n_jobs].cpu().numpy(), got) and np.array_equal(kb.flags[:kb.n_jobs].cpu().numpy(), flags)
    tab = kb.table.cpu().numpy().view(_KR_JOB_DTYPE).copy()
    bad = np.arange(3, len(items), 7)
    tab["n_train"][bad] = np.where(np.arange(len(bad)) % 2 == 0, 0, 1025)
    kb.table.copy_(torch.from_numpy(tab.view(np.uint8)))
    kb.correct.fill_(12345)
    kb.flags.fill_(12345)
    kb.launch()
    torch.cuda.synchronize()
    got2, flags2 = kb.correct[:kb.n_jobs].cpu().numpy(), kb.flags[:kb.n_jobs].cpu().numpy()
    ok = np.ones(len(items), bool)
    ok[bad] = False
    assert (got2[bad] == -1).all() and (flags2[bad] == 0).all()
    assert np.array_equal(got2[ok], got[ok]) and np.array_equal(flags2[ok], flags[ok])


# ------------------------------------------------------------------------------------------------ 6: against LAPACK
ROWS_PD = 2  # tests/test_gpu_kr_epochs.py: blocks the device solver factors as they are, against the host pseudo-inverse


@pytest.mark.parametrize("n,nt,nv,c", [(700, 321, 300, 2), (1100, 600, 400, 5), (1500, 960, 500, 7), (1700, 1024, 600, 8)])
def test_large_solver_against_lapack(ops, n, nt, nv, c):
    """the recipe of test_kernel_regression_solver_against_lapack (arc-cosine kernel of 40 random features plus class signal, six
    problems each): per problem within 2 rows of the fp64 pinv count (on these inputs fp32 Cholesky and fp32 pinv on the host are
    0 rows from fp64; the blocks have condition 3e3 .. 2e4)"""
    rng = np.random.default_rng(n + nt)
    problems, want = [], []
    for p in range(6):
        h = rng.standard_normal((n, 40)).astype(np.float32)
        lab = rng.integers(0, c, n).astype(np.int32)
        h += np.eye(c, 40, dtype=np.float32)[lab] * 2.0
        gb = ops.GramBatch([torch.from_numpy(h).cuda()], linear=False)
        gb.launch()
        k = gb.k_arccos[0]
        kk = k.cpu().numpy().astype(np.float64)
        perm = rng.permutation(n)
        tr, va = np.sort(perm[:nt]).astype(np.int32), np.sort(perm[nt:nt + nv]).astype(np.int32)
        alpha = np.linalg.pinv(kk[np.ix_(tr, tr)]) @ np.eye(c)[lab[tr]]
        want.append(int(((kk[np.ix_(va, tr)] @ alpha).argmax(1) == lab[va]).sum()))
        problems.append((k, _dev(tr), _dev(va), _dev(lab)))
    kb = ops.KrBatch(problems, c)
    kb.launch()
    torch.cuda.synchronize()
    got = kb.correct[:len(problems)].cpu().numpy()
    print(f"[kr large] lapack nt={nt}: device {got.tolist()} fp64 pinv {want} flags {kb.flags[:6].cpu().tolist()}")
    assert kb.large and (np.abs(got - np.asarray(want)) <= ROWS_PD).all(), (got, want)
    kb.launch()
    torch.cuda.synchronize()
    assert np.array_equal(kb.correct[:len(problems)].cpu().numpy(), got)
    assert ((got >= 0) & (got <= nv)).all() and np.mean(np.asarray(want)) > nv / c


# ------------------------------------------------------------------------------------------------ 7: the API against the real reference
def load_kr_large(tag):
    """per-epoch golden of tests/golden/kr_epochs_large.npz (make_golden_kr_large.py), shaped like _golden.load_kr"""
    import os
    from _golden import GOLDEN_DIR
    z = np.load(os.path.join(GOLDEN_DIR, "kr_epochs_large.npz"))
    out = {"epochs": int(z["epochs"]), "seed": int(z[f"{tag}/seed"]), "sample_max": float(z[f"{tag}/sample_max"])}
    for clf in ("kernel_reg0", "kernel_reg1"):
        tr, va = z[f"{tag}/train_{clf}"], z[f"{tag}/val_{clf}"]
        out[clf] = dict(node_sets=[(t[t >= 0].astype(np.int64), v[v >= 0].astype(np.int64)) for t, v in zip(tr, va)],
                        g_results=z[f"{tag}/g_results_{clf}"], x_results=z[f"{tag}/x_results_{clf}"], p=float(z[f"{tag}/p_{clf}"]))
    return out


def api_rows_off(tag, clf, solver):
    """the API call the fixture recorded (cora, raw adjacency, raw features, seed 11, 8 epochs) on route `solver` -> (largest
    per-epoch deviation from the reference's accuracies in validation rows, p, the record, n_val)"""
    from _golden import load
    from test_gpu_api import _raw
    from wdg_amd.utils import homophily_metrics as hm
    rec = load_kr_large(tag)
    adj_raw, features, labels = _raw(load("real_cora"))
    torch.manual_seed(rec["seed"])
    accs = []
    orig = hm.accuracy
    hm.accuracy = lambda lab, out, _o=orig, _a=accs: (_a.append(float(_o(lab, out))), _o(lab, out))[1]
    hm.LAST_KR_ACCURACIES = None
    try:
        p, _secs = hm.classifier_based_performance_metric(features, adj_raw, labels, rec["sample_max"], base_classifier=clf,
                                                          epochs=rec["epochs"], solver=solver)
    finally:
        hm.accuracy = orig
    if solver == "device":
        assert hm.LAST_KR_ACCURACIES is not None
        acc = hm.LAST_KR_ACCURACIES.numpy().astype(np.float64)
    else:
        assert hm.LAST_KR_ACCURACIES is None and len(accs) == 2 * rec["epochs"]
        acc = np.asarray(accs, np.float64).reshape(-1, 2)
    r = rec[clf]
    n_val = float(len(r["node_sets"][0][1]))
    off = max(np.abs(acc[:, 0] - r["g_results"]).max(), np.abs(acc[:, 1] - r["x_results"]).max()) * n_val
    return float(off), float(p), r, n_val


# R per (fixture, classifier) = the HOST route's largest per-epoch deviation from the recorded reference (solver="host": the
# reference's own arithmetic on this machine's kernels) + 2 rows, the margin tests/test_gpu_api.py gives the device over the host
# route on cora / texas.  Measured on the MI355X (rows; host route, device route):
API_ROWS_MEASURED = {
    ("real_cora_s1000", "kernel_reg0"): (1, 1),   # (5 of its 16 blocks are rank deficient and solved again with pinv on the host)
    ("real_cora_s1000", "kernel_reg1"): (0, 0),
    ("real_cora_s1600", "kernel_reg0"): (2, 2),   # (8 of 16 solved again on the host)
    ("real_cora_s1600", "kernel_reg1"): (0, 1),
}


@pytest.mark.parametrize("tag", ["real_cora_s1000", "real_cora_s1600"])
@pytest.mark.parametrize("clf", ["kernel_reg0", "kernel_reg1"])
def test_api_metric_above_320_train_rows_against_the_reference(tag, clf):
    """classifier_based_performance_metric at sample_max 1000 (602 train rows) and 1600 (924) stays on the device and lands within
    R rows per epoch of what the reference computed in those epochs, p within what that implies"""
    from _golden import load, p_tolerance
    from test_gpu_api import _raw
    from wdg_amd.utils import homophily_metrics as hm
    rec = load_kr_large(tag)
    adj_raw, features, labels = _raw(load("real_cora"))
    state = torch.get_rng_state()
    torch.manual_seed(rec["seed"])
    assert hm._kernel_regression_on_device(features, adj_raw, labels, rec["sample_max"], clf, rec["epochs"]) is not None
    torch.set_rng_state(state)
    off, p, r, n_val = api_rows_off(tag, clf, "device")
    host_rows = API_ROWS_MEASURED[tag, clf][0]
    R = int(round(host_rows)) + 2
    print(f"[kr large] api {tag} {clf}: device route {off:.0f} rows off the reference, host route {host_rows} (measured), R = {R}; p {p:.6f} vs {r['p']:.6f}")
    assert off <= R + 0.01, (tag, clf, off, R)
    assert abs(p - r["p"]) <= p_tolerance(r["g_results"], r["x_results"], n_val, R), (p, r["p"])


# ------------------------------------------------------------------------------------------------ 8: host route against device route
@pytest.mark.parametrize("clf", ["kernel_reg1", "kernel_reg0"])
def test_whole_graph_epochs_of_720_train_rows_host_against_device(clf):
    """Texas-style inputs (nnodes <= sample_max: every epoch takes the whole graph) built so that an epoch has 321 .. 1024 train
    rows: 1200 nodes, 5 classes, sample_max 1200 -> 720 train rows.  Same node sets on both routes (same torch CPU generator);
    per-epoch accuracies within 2 validation rows, as test_classifier_metric_device_solver asks on texas."""
    from _golden import p_tolerance
    from wdg_amd.utils import homophily_metrics as hm
    rng = np.random.default_rng(31)
    n, c, f, e = 1200, 5, 1500, 5000
    lab = rng.integers(0, c, n)
    x = ((rng.random((n, f)) < 0.04) | (np.arange(f)[None, :] % 50 == lab[:, None])).astype(np.float32)  # bag of words + class words
    src = rng.integers(0, n, e)
    same = rng.random(e) < 0.7
    by_class = [np.flatnonzero(lab == k) for k in range(c)]
    dst = np.where(same, np.array([by_class[lab[u]][rng.integers(0, len(by_class[lab[u]]))] for u in src]), rng.integers(0, n, e))
    key = np.unique(np.concatenate([src * n + dst, dst * n + src]))
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.stack([key // n, key % n])), torch.ones(len(key)), (n, n)).coalesce()
    features, labels = torch.from_numpy(x), torch.from_numpy(lab)
    seen = {}
    for solver in ("host", "device"):
        torch.manual_seed(11)
        accs = []
        orig = hm.accuracy
        hm.accuracy = lambda l_, o_, _o=orig, _a=accs: (_a.append(float(_o(l_, o_))), _o(l_, o_))[1]
        hm.LAST_KR_ACCURACIES = None
        try:
            p, secs = hm.classifier_based_performance_metric(features, adj, labels, 1200.0, base_classifier=clf, epochs=6, solver=solver)
        finally:
            hm.accuracy = orig
        if solver == "device":
            assert len(accs) == hm.LAST_KR_RIDGED and hm.LAST_KR_ACCURACIES is not None
            accs = hm.LAST_KR_ACCURACIES.reshape(-1).tolist()
        assert 0.0 <= p <= 1.0 and secs > 0 and len(accs) == 12
        seen[solver] = (p, np.array(accs))
    n_val = 480.0
    rows = np.abs(seen["host"][1] - seen["device"][1]) * n_val
    print(f"[kr large] whole-graph {clf}: rows host vs device per (epoch, kernel) {np.round(rows).astype(int).tolist()}, ridged {hm.LAST_KR_RIDGED}; "
          f"p host {seen['host'][0]:.6f} device {seen['device'][0]:.6f}")
    assert rows.max() <= 2.01
    h = seen["host"][1].reshape(-1, 2)
    assert abs(seen["host"][0] - seen["device"][0]) <= p_tolerance(h[:, 0], h[:, 1], n_val, 2)


# ------------------------------------------------------------------------------------------------ 9: the CLI
def test_cli_sample_max_1000_equals_the_api_call():
    """homophily_tests.py --sample_max 1000 on cora: the metric stays on the device (no new flag) and gives the API call's p-value"""
    from _golden import GOLDEN_DIR, load
    from test_gpu_api import _raw
    from wdg_amd import homophily_tests as cli
    from wdg_amd.utils import homophily_metrics as hm
    hm.LAST_KR_ACCURACIES = None
    torch.manual_seed(11)
    got = float(cli.main(["--dataset_name", "cora", "--data_dir", GOLDEN_DIR, "--homophily_metric", "kernel_reg1_based_homo",
                          "--sample_max", "1000"]))
    assert hm.LAST_KR_ACCURACIES is not None and tuple(hm.LAST_KR_ACCURACIES.shape) == (100, 2)
    acc_cli = hm.LAST_KR_ACCURACIES.clone()
    adj_raw, features, labels = _raw(load("real_cora"))
    torch.manual_seed(11)
    want, _ = hm.classifier_based_performance_metric(features, adj_raw, labels, 1000.0, base_classifier="kernel_reg1", epochs=100)
    assert torch.equal(acc_cli, hm.LAST_KR_ACCURACIES)
    assert got == pytest.approx(float(want), rel=1e-12, abs=1e-15) and 0.0 <= got <= 1.0


# ------------------------------------------------------------------------------------------------ 10: the sweep
def _sweep_rows_off(n_feat=None, ridge=None):
    """one small shard - 4 graphs of 2000 nodes, prepare_full(epochs=3, sample_max=1000): 600 train rows per regression -> rows by
    which each regression's accuracy (full_metrics(ridge)) differs from the reference's own per-epoch computation on the host
    (KrPlan.pinv_accuracies(kernels="host")), the mask of the regularised blocks, n_val, the batch.
    n_feat None: SweepBatch's own default width (500)"""
    from wdg_amd import sweep
    jobs = [sweep.Job(h, 7, 2, 2000, 5) for h in (0.1, 0.3, 0.6, 0.9)]
    sb = sweep.SweepBatch(jobs, gcn_hidden=0, **({} if n_feat is None else {"n_feat": n_feat}))
    sb.prepare_full(epochs=3, sample_max=1000, base_seed=9)
    assert sb.kr.large and int(sb.plan._n_tr.max()) == 600
    sb.step()
    sb.launch_full()
    torch.cuda.synchronize()
    rows9 = (sb.full_metrics() if ridge is None else sb.full_metrics(ridge=ridge)).numpy()
    assert rows9.shape == (4, 9) and np.isfinite(rows9[:, 7:9]).all() and ((rows9[:, 7:9] >= 0) & (rows9[:, 7:9] <= 1)).all()
    acc_dev = sb.kr_acc.copy().reshape(-1)
    ridged = sb.plan.kr_ridged_mask().cpu().numpy().reshape(-1)
    assert acc_dev.size == 4 * 2 * 3 * 2 and sb.kr_total == acc_dev.size and sb.kr_ridged == int(ridged.sum())
    n_val = float(sb.kr_val.shape[2])
    host = sb.plan.pinv_accuracies(np.arange(acc_dev.size), kernels="host")
    return np.abs(acc_dev.astype(np.float64) - host) * n_val, ridged, n_val, sb


def _assert_sweep_bounds(d, ridged):
    from test_gpu_kr_epochs import RIDGED_MAX, RIDGED_SHARE_WITHIN_2, ROWS_PD as ROWS_PD_SWEEP
    assert d[~ridged].max(initial=0) <= ROWS_PD_SWEEP + 0.01
    if ridged.any():
        assert (d[ridged] <= 2.01).mean() >= RIDGED_SHARE_WITHIN_2 and d[ridged].max() <= RIDGED_MAX + 0.01


def test_sweep_plan_at_sample_max_1000(ops, monkeypatch):
    """The shard as a sweep runs it - SweepBatch's default width (500 features), full_metrics() with no argument - with 600 train
    rows per regression against the host pinv, within the bounds tests/test_gpu_kr_epochs.py states: blocks factored as they are
    and deflated ones <= 2 rows; regularised ones >= 98 % within 2 rows, none beyond 4.
    500 features are fewer than the 600 train rows: EVERY linear-kernel block is rank deficient by at least 100 dimensions and
    flagged.  A plan on the large solver solves flagged blocks again the reference's way by default (full_metrics: ridge "pinv"),
    which is what keeps them inside the bound; the arc-cosine blocks of the shard are factored as they are."""
    monkeypatch.delenv("WDG_SWEEP_KR_RIDGE", raising=False)
    d, ridged, n_val, sb = _sweep_rows_off()
    print(f"[kr large] sweep F=500, default ridge: rows off the host pinv: not regularised {np.round(d[~ridged]).astype(int).tolist()}, "
          f"regularised {np.round(d[ridged]).astype(int).tolist()} (n_val {n_val:.0f}), pinv {sb.kr_pinv_seconds:.2f} s")
    assert ridged.reshape(4, 2, 3, 2)[:, 0].all()  # (every linear-kernel block of rank <= 500 < 600 is flagged)
    assert sb.kr_pinv_seconds > 0                  # (... and was solved again on the host without being asked to)
    _assert_sweep_bounds(d, ridged)


def test_sweep_plan_at_sample_max_1000_device_ridge_on_full_rank_width(ops):
    """ridge="device" at feature width 932, the narrowest of the reference's feature bases (synthetic_plot.py:64-65): the linear
    kernel of 600 train rows then has full rank, as every kernel has that the bounds of tests/test_gpu_kr_epochs.py were measured
    on (500 features over 300 train rows) - the large solver's own ridge answers hold those bounds"""
    d, ridged, n_val, _ = _sweep_rows_off(932, "device")
    print(f"[kr large] sweep F=932, ridge=device: rows off the host pinv: not regularised {np.round(d[~ridged]).astype(int).tolist()}, "
          f"regularised {np.round(d[ridged]).astype(int).tolist()} (n_val {n_val:.0f})")
    _assert_sweep_bounds(d, ridged)


def test_sweep_plan_device_ridge_below_full_rank_says_how_far_it_is(ops, monkeypatch):
    """ridge="device" asked for by name at 500 features over 600 train rows keeps the ridge answers of the flagged linear-kernel
    blocks - measured 0 .. 89 of 400 validation rows from the reference's pinv, 3 of 24 within 2 - and the warning says so instead
    of the 2 - 4 rows that hold for tables of up to 320 train rows; the blocks that are not flagged hold their bound either way"""
    from test_gpu_kr_epochs import ROWS_PD as ROWS_PD_SWEEP
    monkeypatch.setenv("WDG_KR_QUIET", "0")
    with pytest.warns(UserWarning, match="NOT close to the reference"):
        d, ridged, _, sb = _sweep_rows_off(None, "device")
    print(f"[kr large] sweep F=500, ridge=device: not regularised {np.round(d[~ridged]).astype(int).tolist()}, regularised "
          f"{np.round(d[ridged]).astype(int).tolist()}")
    assert sb.kr_pinv_seconds == 0 and ridged.reshape(4, 2, 3, 2)[:, 0].all()
    assert d[~ridged].max(initial=0) <= ROWS_PD_SWEEP + 0.01
