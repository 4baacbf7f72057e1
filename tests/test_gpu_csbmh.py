"""The CSBM-H device entries against the numpy restatement of their definitions (tests/_csbmh_ref.py): the class-structured generator
bit for bit (and against the regular generator where the two meet), the Gaussian features within the bound derived from the number
formats, the Bayes rule's error counts for equality, and csbmh.empirical end to end against the closed-form curve."""
import numpy as np
import pytest
import torch

import _csbmh_ref as ref
import _synth_ref

pytestmark = pytest.mark.gpu

SEED = 0xC5B0000012345678


def _check_graphs(specs, graphs, loops):
    for (sizes, k, d, seed), (g, lab) in zip(specs, graphs):
        rowptr, col, labels = ref.class_graph(sizes, k, d, seed, _synth_ref.SELF_LOOPS * loops)
        assert g.n_rows == g.n_cols == sum(sizes)
        assert g.rowptr.dtype == torch.int32 and np.array_equal(g.rowptr.cpu().numpy(), rowptr), (sizes, k, d)
        got = g.col.cpu().numpy()
        assert got.shape == col.shape and np.array_equal(got, col), (sizes, k, d, np.flatnonzero(got != col)[:5])
        assert g.val.dtype == torch.float32 and g.val.shape == g.col.shape and bool((g.val == 1).all())
        assert lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), labels)


@pytest.mark.parametrize("loops", [0, 1])
def test_every_class_shape_in_one_launch_equals_the_restatement(loops):
    from wdg_amd import synth
    specs = [(s, k, d, SEED + 17 * i) for i, (s, k, d) in enumerate(ref.CLASS_SHAPES)]
    batch = synth.ClassGraphBatch(specs, self_loops=bool(loops))
    graphs = batch.launch()
    _check_graphs(specs, graphs, loops)
    before = batch.pool.clone()
    batch.launch()  # counter-based: the same bits into the same arrays
    assert torch.equal(batch.pool, before)
    other = synth.class_graphs_device([(s, k, d, seed + 1) for s, k, d, seed in specs], self_loops=bool(loops))
    assert not torch.equal(other[3][0].col, graphs[3][0].col) and torch.equal(other[2][0].col, graphs[2][0].col)  # (shape 2 takes every candidate)


@pytest.mark.parametrize("loops", [0, 1])
def test_equal_classes_give_the_regular_generators_bits(loops):
    from wdg_amd import ops, synth
    shapes = [(10, 5, 1, 9), (2000, 5, 2, 40)]
    reg = ops.GraphBatch.generated([(n, C, k, d, SEED + i) for i, (n, C, k, d) in enumerate(shapes)], ops.COO_ADD_SELF_LOOPS if loops else 0, quad=False)
    got = synth.class_graphs_device([((n // C,) * C, (k,) * C, (d,) * C, SEED + i) for i, (n, C, k, d) in enumerate(shapes)], self_loops=bool(loops))
    for (g, lab), r, rl in zip(got, reg.graphs, reg.labels):
        assert torch.equal(g.rowptr, r.rowptr) and torch.equal(g.col, r.col) and torch.equal(g.val, r.val) and torch.equal(lab, rl)


def test_gaussian_features_equal_the_restatement_within_the_formats_bound():
    """F in {1, 2, 5, 16} x n in {1, 257} in one launch.  sd = 0 gives the mean exactly; with mean 0 and sd 1 the fp32 Box-Muller is
    within 4e-6 of the fp64 one from the same Philox words: |z| <= sqrt(48 ln 2) = 5.77, the library functions within 2 ulp, about
    4 ulp of relative error in total - 5.77 x 4 x 2^-23 = 2.8e-6, with margin.  (measured maximum: see DESIGN 4.24)"""
    from wdg_amd import synth
    rng = np.random.default_rng(5)
    shapes = [(n, F) for F in (1, 2, 5, 16) for n in (1, 257)]
    worst = 0.0
    for F in (1, 2, 5, 16):
        jobs = [(n, f) for n, f in shapes if f == F]
        labels_h = [rng.integers(0, 3, n).astype(np.int32) for n, _f in jobs]
        labels = [torch.from_numpy(lab).cuda() for lab in labels_h]
        seeds = [SEED + 1000 * F + i for i in range(len(jobs))]
        mean = rng.standard_normal((3, F)).astype(np.float32)
        exact = synth.gauss_features_device(labels, mean, np.zeros(3, np.float32), seeds, ld=F + 3)
        for x, lab in zip(exact, labels_h):
            assert x.shape == (len(lab), F) and x.stride(0) == F + 3 and np.array_equal(x.cpu().numpy(), mean[lab])
        draw = synth.GaussFeatureBatch(labels, np.zeros((3, F), np.float32), np.ones(3, np.float32), seeds)
        xs = draw.launch()
        for x, (n, _f), seed in zip(xs, jobs, seeds):
            got, want = x.cpu().numpy().astype(np.float64), ref.standard_normals(n, F, seed)
            assert got.shape == want.shape and np.isfinite(got).all()
            worst = max(worst, float(np.abs(got - want).max()))
        scaled = synth.gauss_features_device(labels, mean, np.array([0.5, 2.0, 3.0], np.float32), seeds)
        for x, z, lab in zip(scaled, xs, labels_h):  # x = fmaf(sd, z, mean): within an ulp of the fp64 product-sum of the device's own z
            want = mean[lab].astype(np.float64) + np.array([0.5, 2.0, 3.0])[lab][:, None] * z.cpu().numpy().astype(np.float64)
            assert np.array_equal(x.cpu().numpy(), want.astype(np.float32))
        bad = synth.gauss_features_device([torch.tensor([0, 7, -1, 2], dtype=torch.int32).cuda()], mean, np.ones(3, np.float32), [1])[0].cpu().numpy()
        assert np.isfinite(bad[[0, 3]]).all() and np.isnan(bad[[1, 2]]).all()  # a label outside the classes: NaN
    print("largest |x - fp64 restatement|", worst)
    assert worst <= 4e-6, worst
    big = synth.gauss_features_device([torch.zeros(200000, dtype=torch.int32).cuda()], np.zeros((1, 2), np.float32), np.ones(1, np.float32), [SEED])[0]
    m, v = float(big.mean()), float(big.var())
    assert abs(m) < 5 / np.sqrt(400000) and abs(v - 1) < 5 * np.sqrt(2 / 400000)  # a standard normal sample


def _qda_job(rng, n, F):
    x = rng.standard_normal((n, F)).astype(np.float32)
    h = (0.5 * rng.standard_normal((n, F))).astype(np.float32)
    labels = rng.integers(0, 2, n).astype(np.int32)
    mean = rng.standard_normal((3, 2, F))
    inv2v, bias = rng.uniform(0.2, 2.0, (3, 2)), rng.standard_normal((3, 2))
    # set 0: mirrored centres, the same variance and prior - a row with x_0 = 0 has g_0 == g_1 EXACTLY and predicts 1
    mean[0, 1] = mean[0, 0]
    mean[0, 0, 0], mean[0, 1, 0] = -1.0, 1.0
    inv2v[0, 1], bias[0, 1] = inv2v[0, 0], bias[0, 0]
    x[::3, 0] = 0.0
    if n > 10:
        x[7, F - 1] = np.nan  # one NaN row: every set that reads x predicts 1
        labels[11] = 2        # a label outside the two classes is not counted
    return x, h, labels, (mean, inv2v, bias)


def test_error_counts_equal_the_fp64_rule_on_the_devices_rows():
    from wdg_amd import csbmh
    rng = np.random.default_rng(11)
    host = [_qda_job(rng, n, F) for n in (1, 1000) for F in (1, 2, 16)]
    jobs = []
    for x, h, labels, consts in host:
        F = x.shape[1]
        xd = torch.zeros((x.shape[0], F + 2), dtype=torch.float32).cuda()  # (a leading dimension of its own)
        xd[:, :F] = torch.from_numpy(x).cuda()
        jobs.append((xd[:, :F], torch.from_numpy(h).cuda(), torch.from_numpy(labels).cuda(), consts))
    batch = csbmh.QdaBatch(jobs)
    counts = batch.launch().cpu().numpy()
    ties = 0
    for got, (x, h, labels, (mean, inv2v, bias)) in zip(counts, host):
        want = ref.qda_counts(x, h, labels, mean, inv2v, bias)
        assert np.array_equal(got, want), (x.shape, got, want)
        assert got.sum() == 3 * int(np.sum(labels < 2))
        tie = (x[:, 0] == 0) & ~np.isnan(x).any(1) & (labels < 2)
        ties += int(tie.sum())
        assert got[0, :, 1].sum() >= tie.sum()
    assert ties > 300
    n_tie_pred0 = ref.qda_counts(host[4][0][::3], host[4][1][::3], host[4][2][::3], *host[4][3])[0, :, 0].sum()
    assert n_tie_pred0 == 0  # every tie row predicts 1
    batch.counts.fill_(-5)
    assert np.array_equal(batch.launch().cpu().numpy(), counts)  # plain stores: nothing to clear, the same bits


E2E = dict(n0=3000, n1=2000, mu0=[-1, 0], mu1=[1, 0], sigma0=1, sigma1=5, d0=5, d1=10)


@pytest.fixture(scope="module")
def end_to_end():
    from wdg_amd import csbmh
    return csbmh.empirical(**E2E, levels=[0, .2, .4, .6, .8, 1], graphs=32, seed=3), csbmh.empirical(**E2E, levels=[0, .2, .4, .6, .8, 1], graphs=32, seed=3)


def test_measured_error_rates_follow_the_closed_form_curve(end_to_end):
    """sizes (3000, 2000), d (5, 10), mu (-+1, 0), sigma (1, 5), six levels, 32 graphs each.  Per level, set and class, with N_c =
    graphs n_c: |count / N_c - pbe_class| <= 5 sqrt((3 + max(d0, d1)) p (1 - p) / N_c) + 1 / N_c.  The factor 3 + d is derived: nodes
    that share neighbours have correlated features, the indicators' correlation is at most the features' canonical correlation, and
    a row's correlations sum to about d + 2, whatever n."""
    from wdg_amd import csbmh
    out, _ = end_to_end
    N = np.array([32 * 3000, 32 * 2000], np.float64)
    assert np.array_equal(out["levels"], [0, .2, .4, .6, .8, 1]) and out["counts"].shape == (6, 3, 2, 2)
    assert np.array_equal(out["counts"].sum(-1), np.broadcast_to(N.astype(np.int64), (6, 3, 2)))
    want = csbmh.curves(**E2E, levels=out["levels"])
    assert np.array_equal(out["pbe_class"], want["pbe_class"]) and np.array_equal(out["pbe"], want["pbe"])
    p = want["pbe_class"]
    bound = 5 * np.sqrt((3 + 10) * p * (1 - p) / N) + 1 / N
    assert np.array_equal(out["bound"], bound)
    rate_class = np.stack([out["counts"][:, :, 0, 1], out["counts"][:, :, 1, 0]], -1) / N
    assert np.array_equal(out["rate_class"], rate_class)
    dev = np.abs(rate_class - p)
    print("rate_class\n", rate_class, "\npbe_class\n", p, "\n|difference| / bound\n", dev / bound, "\nseconds", out["seconds"])
    assert np.all(dev <= bound), (dev / bound).max()
    assert np.allclose(out["rate"], (rate_class * N).sum(-1) / N.sum(), rtol=0, atol=1e-15)
    assert np.abs(np.diff(p[:, 1, :], axis=0)).max() > 0.1 > 2 * bound.max()  # a generator that ignored h or a class's degree would fail


def test_two_runs_give_identical_counts(end_to_end):
    a, b = end_to_end
    assert np.array_equal(a["counts"], b["counts"])


def test_empirical_takes_other_widths_and_default_levels():
    """F = 3 (padded rows on the narrow aggregation) and F = 9 (the CSR family), the default levels: the counts are those of the fp64
    rule on the batch's own x and h, and h is the neighbour mean"""
    from wdg_amd import csbmh
    for F in (3, 9):
        mu0, mu1 = np.linspace(-1, 0, F), np.linspace(1, 0, F)
        batch = csbmh.EmpiricalBatch(40, 25, mu0, mu1, 1.5, 0.5, 4, 5, graphs=2, seed=9)
        assert np.array_equal(batch.levels, [0, 1])
        counts = batch.run().cpu().numpy()
        for j, ((g, lab), x, h) in enumerate(zip(batch.gen.graphs, batch.draw.x, batch.h)):
            xh, hh, labels = x.cpu().numpy(), h.cpu().numpy(), lab.cpu().numpy()
            rowptr, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
            mean_nb = np.stack([xh[col[rowptr[i]:rowptr[i + 1]]].astype(np.float64).mean(0) for i in range(65)])
            assert np.abs(hh - mean_nb).max() < 1e-5
            same = np.array([np.sum(labels[col[rowptr[i]:rowptr[i + 1]]] == labels[i]) for i in range(65)])
            level = batch.levels[j // 2]
            assert np.array_equal(same, np.where(labels == 0, level * 4, level * 5))
            want = ref.qda_counts(xh, hh, labels, *csbmh.rule_constants(40, 25, mu0, mu1, 1.5, 0.5, 4, 5, float(level)))
            assert np.array_equal(counts[j // 2, j % 2], want), (F, j)
