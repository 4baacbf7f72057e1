"""GPU tests of csrc/neighbor_moments.hip against tests/_neighbor_moments_ref.py, for EQUALITY of the seven outputs and of D (a NaN
for a NaN: include/wdg.h leaves the payload of a NaN that arithmetic made open; the extremes copy bits and are compared as bits): the
patterns, widths and layouts of tests/test_gpu_neighbor_max.py - one table of nine jobs per width over the 16 x 300 pattern with rows of
0 .. 129 entries and a hub row of 1 950, unsorted, with duplicates, a -1 and an n_cols per longer row, a kept_len below, at and above the
extent, n = 1, 3, 4, 5 rows, rows outside [0, nnz], contiguous, pitched and 4-byte-misaligned views - with values that tie, both zeros,
infinities, NaNs and a column shifted by 100, every combination of NULL outputs that changes what the kernel does, the four statistics
as column slices of one matrix; the extremes against NeighborMaxBatch; every job alone; a column slice; sentinels outside the blocks;
then two draws of a DropEdgeBatch and a NeighborSampleBatch through tables built once."""
import numpy as np
import pytest
import torch

import _neighbor_moments_ref as R
from test_gpu_neighbor_max import LAYOUTS, N_COLS, WIDTHS, _bits, _Case, _dev, _filled, _values, _view, cases  # noqa: F401  (cases: the fixture)

pytestmark = pytest.mark.gpu

F_SENTINEL, I_SENTINEL, EPS = -3.0, -7, 1e-5
FLOATS, ARGS = ("mean", "std", "max", "min"), ("arg_max", "arg_min")
REF_KEY = {"mean": "mean", "std": "std", "max": "mx", "min": "mn", "arg_max": "arg_max", "arg_min": "arg_min"}
# which outputs a job asks for: everything; evaluation (no args); each statistic alone - std without mean, an extreme without its arg,
# an arg without its extreme -; the sums alone; the extremes alone
WANTED = [FLOATS + ARGS, FLOATS + ARGS, FLOATS, ("mean",), ("std",), ("max", "arg_max"), ("min",), ("mean", "std"), ("arg_max", "max", "min", "arg_min")]


def _shifted(rng, rows, cols):
    x = _values(rng, rows, cols)
    with np.errstate(invalid="ignore"):
        x[:, cols // 2] = x[:, cols // 2] + np.float32(100)  # a column whose mean is large against its spread
    return x


def _forward_entries(cases, width, seed=0, sliced=True):
    """the table's entries over sentinel-filled outputs -> (entries, [(case, x, {key: (buffer, view)}, cnt)])"""
    rng = np.random.default_rng(300 + width + seed)
    entries, wants, xs = [], [], {}
    for k, c in enumerate(cases):
        x = xs.setdefault(c.n_cols, _shifted(rng, c.n_cols, width))
        outs = {}
        if k == 0 and sliced:  # the four statistics as column slices of one [n, 4 w] matrix
            base = torch.full((c.n_rows, 4 * width), F_SENTINEL, dtype=torch.float32, device="cuda")
            outs = {key: (None, base[:, q * width:(q + 1) * width]) for q, key in enumerate(FLOATS)}
        for q, key in enumerate(WANTED[k % len(WANTED)]):
            if key not in outs:
                outs[key] = _view(c.n_rows, width, LAYOUTS[(k + q + 1) % 3], torch.int32 if key in ARGS else torch.float32, I_SENTINEL if key in ARGS else F_SENTINEL)
        cnt = torch.full((c.n_rows,), I_SENTINEL, dtype=torch.int32, device="cuda")
        entries.append(dict(pattern=c.pattern, x=_filled(LAYOUTS[k % 3], x, torch.float32), cnt=cnt, eps=EPS, **{key: v[1] for key, v in outs.items()}))
        wants.append((c, x, outs, cnt))
    return entries, wants


def _assert_forward(wants):
    for k, (c, x, outs, cnt) in enumerate(wants):
        shape = (c.n_rows, x.shape[1])
        keep = {key: np.full(shape, F_SENTINEL, np.float32) for key in ("mean", "std", "mx", "mn")}
        keep.update(arg_max=np.full(shape, I_SENTINEL, np.int32), arg_min=np.full(shape, I_SENTINEL, np.int32), cnt=np.full(c.n_rows, I_SENTINEL, np.int32))
        want = R.neighbor_moments(c.rowptr, c.col, c.kept_len, x, c.n_rows, EPS, keep=keep)
        assert np.array_equal(cnt.cpu().numpy(), want["cnt"]), (k, "cnt")
        for key, (buf, view) in outs.items():
            got = np.ascontiguousarray(view.cpu().numpy())
            if key in ("max", "min"):  # bits, copied: a NaN keeps its payload
                assert np.array_equal(got.view(np.uint32), want[REF_KEY[key]].view(np.uint32)), (k, key)
            else:
                assert R.same(got, want[REF_KEY[key]]), (k, key)
            if buf is not None:  # nothing outside the block is written
                fill = I_SENTINEL if key in ARGS else F_SENTINEL
                saved = view.clone()
                view.fill_(fill)
                assert bool((buf == fill).all()), (k, key, "outside the block")
                view.copy_(saved)


@pytest.mark.parametrize("width", WIDTHS)
def test_the_forward_pass_equals_the_restatement_in_a_table_and_alone(cases, width):
    from wdg_amd import ops
    entries, wants = _forward_entries(cases, width)
    ops.NeighborMomentsBatch(entries).launch()
    torch.cuda.synchronize()
    _assert_forward(wants)
    hub = wants[0]
    assert int(hub[3][0]) == 0 and int(hub[3][15]) > 1900 and np.isnan(hub[2]["mean"][1].cpu().numpy()[15]).any()  # an empty row; the hub row meets the NaN sources
    # the extremes are NeighborMaxBatch's on the same jobs, bit for bit
    for k, (c, x, outs, _) in enumerate(wants):
        for key, arg, minimum in (("max", "arg_max", False), ("min", "arg_min", True)):
            if key in outs and arg in outs:
                y, a = ops.neighbor_max(c.pattern, entries[k]["x"], minimum=minimum, return_arg=True)
                untouched = (outs[arg][1] == I_SENTINEL)  # (rows outside [0, nnz])
                assert np.array_equal(_bits(torch.where(untouched, y, outs[key][1])), _bits(y)) and torch.equal(torch.where(untouched, a, outs[arg][1]), a), (k, key)
    alone_entries, alone_wants = _forward_entries(cases, width)
    for e in alone_entries:  # every job alone gives the table's bytes
        ops.NeighborMomentsBatch([e]).launch()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(alone_wants, wants)):
        assert torch.equal(a[3], b[3]), k
        for key in a[2]:
            assert np.array_equal(_bits(a[2][key][1]), _bits(b[2][key][1])), (k, key)


def test_a_column_slice_gives_the_wide_jobs_bits_and_the_shifted_column_keeps_its_spread(cases):
    from wdg_amd import ops
    c = cases[0]
    x_host = _shifted(np.random.default_rng(3), N_COLS, 260)
    x = _filled("contiguous", x_host, torch.float32)
    agg, cnt, amax, amin = ops.neighbor_moments(c.pattern, x, eps=EPS, return_args=True)
    wide = agg.view(c.n_rows, 4, 260)
    for lo, hi in ((0, 7), (3, 67), (4, 260), (250, 260), (1, 257), (128, 144)):
        part, pc, pmax, pmin = ops.neighbor_moments(c.pattern, x[:, lo:hi], eps=EPS, return_args=True)
        assert np.array_equal(_bits(part.view(c.n_rows, 4, hi - lo)), _bits(wide[:, :, lo:hi])) and torch.equal(pc, cnt), (lo, hi)
        assert torch.equal(pmax, amax[:, lo:hi]) and torch.equal(pmin, amin[:, lo:hi]), (lo, hi)
    # the column shifted by 100: the centred deviation lies within 2^-18 of the fp64 one (relative to the largest) - the one-pass form is off by some 2^-8 there
    want64 = R.neighbor_moments(c.rowptr, c.col, None, x_host.astype(np.float64), c.n_rows, EPS)["std"][:, 130]
    got = wide[:, 1, 130].cpu().numpy().astype(np.float64)
    fine = np.isfinite(want64)
    assert fine.sum() >= 4 and np.abs(got[fine] - want64[fine]).max() <= 2.0 ** -18 * np.abs(want64[fine]).max()


def _backward_entries(cases, width, rng):
    """every case's pattern taken as a TRANSPOSED pattern: n_src = its n_cols sources, args pointing at its rows (and at none)"""
    entries, wants = [], []
    for k, c in enumerate(cases):
        n_src, shape = c.n_cols, (c.n_cols, width)
        scale = lambda: (rng.standard_normal(shape) * 2.0 ** rng.integers(-6, 6, (n_src, 1))).astype(np.float32)  # noqa: E731
        host = dict(x=rng.standard_normal((c.n_rows, width)).astype(np.float32), g_mean=scale(), g_std=scale(), g_max=scale(), g_min=scale(), mean=scale(),
                    std=(np.abs(scale()) + np.float32(2.0 ** -8)), cnt=rng.integers(0, 6, n_src).astype(np.int32))
        for key in ("arg_max", "arg_min"):
            arg = rng.integers(-1, c.n_rows + 1, shape).astype(np.int32)
            arg[rng.random(shape) < 0.5] = c.n_rows - 1  # (many winners on the last row: the hub's chains are long)
            host[key] = arg
        drop = [(), (), ("g_std",), ("g_max", "arg_max"), ("g_mean", "g_std", "g_max"), ("g_min",), ("g_mean", "g_std", "g_max", "g_min"), ("g_mean",), ()][k % 9]
        db, d = _view(c.n_rows, width, LAYOUTS[(k + 1) % 3], torch.float32, F_SENTINEL)
        e = dict(pattern=c.pattern, d=d, cnt=_dev(host["cnt"], np.int32))
        for q, key in enumerate(("x", "g_mean", "g_std", "g_max", "g_min", "mean", "std", "arg_max", "arg_min")):
            if key not in drop:
                e[key] = _filled(LAYOUTS[(k + q) % 3], host[key], torch.int32 if key.startswith("arg") else torch.float32)
        entries.append(e)
        wants.append((c, host, drop, db, d))
    return entries, wants


@pytest.mark.parametrize("width", WIDTHS)
def test_the_backward_pass_equals_the_restatement_in_a_table_and_alone(cases, width):
    from wdg_amd import ops
    rng = np.random.default_rng(400 + width)
    state = rng.bit_generator.state
    entries, wants = _backward_entries(cases, width, rng)
    ops.NeighborMomentsBackwardBatch(entries).launch()
    torch.cuda.synchronize()
    for k, (c, h, drop, db, d) in enumerate(wants):
        g = {name: h[key] for name, key in (("mean", "g_mean"), ("std", "g_std"), ("mx", "g_max"), ("mn", "g_min")) if key not in drop}
        want = R.neighbor_moments_backward(c.rowptr, c.col, c.kept_len, h["x"], g, h, c.n_rows, d=np.full((c.n_rows, width), F_SENTINEL, np.float32))
        assert R.same(d.cpu().numpy(), want), k
        saved = d.clone()
        d.fill_(F_SENTINEL)
        assert bool((db == F_SENTINEL).all()), (k, "outside the block")
        d.copy_(saved)
    assert np.abs(wants[0][4].cpu().numpy()[15]).max() > 0
    rng.bit_generator.state = state  # the same operands again, every job alone
    alone, alone_wants = _backward_entries(cases, width, rng)
    for e in alone:
        ops.NeighborMomentsBackwardBatch([e]).launch()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(alone_wants, wants)):
        assert np.array_equal(_bits(a[4]), _bits(b[4])), k


@pytest.mark.parametrize("kind", ["drop_edge", "neighbor_sample"])
def test_two_draws_through_tables_built_once_equal_the_restatement_on_the_kept_graph(kind):
    from wdg_amd import ops
    rng = np.random.default_rng(17)
    n, width = 203, 7
    dense = rng.random((n, n)) < 0.06
    dense[:, 3] = True  # a hub row of the transposed pattern
    dense[9] = False    # a node without neighbours
    src, dst = np.nonzero(dense)
    g = ops.CsrGraph.from_coo(src, dst, n)
    batch = (ops.DropEdgeBatch([dict(graph=g)], 0.5, 7) if kind == "drop_edge" else ops.NeighborSampleBatch([dict(graph=g)], 5, 7))
    x_host = (np.round(rng.standard_normal((n, width)) * 4) / 2).astype(np.float32)
    x = _dev(x_host, np.float32)
    gy_host = rng.standard_normal((n, 4 * width)).astype(np.float32)
    gy = _dev(gy_host, np.float32)
    agg = torch.empty(n, 4 * width, device="cuda")
    part = lambda t, q: t[:, q * width:(q + 1) * width]  # noqa: E731
    amax, amin = (torch.empty(n, width, dtype=torch.int32, device="cuda") for _ in range(2))
    cnt, d = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, width, device="cuda")
    fwd = ops.NeighborMomentsBatch([dict(pattern=batch.thinned(0), x=x, cnt=cnt, mean=part(agg, 0), std=part(agg, 1), max=part(agg, 2), min=part(agg, 3),
                                         arg_max=amax, arg_min=amin, eps=EPS)])  # built ONCE: the jobs hold the blocks' addresses
    bwd = ops.NeighborMomentsBackwardBatch([dict(pattern=batch.thinned_t(0), x=x, d=d, cnt=cnt, g_mean=part(gy, 0), g_std=part(gy, 1), g_max=part(gy, 2),
                                                 g_min=part(gy, 3), mean=part(agg, 0), std=part(agg, 1), arg_max=amax, arg_min=amin)])
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    seen = []
    for _ in range(2):  # a later thinning launch changes what they reduce over; nothing is rebuilt
        batch.launch(step)
        step.add_(1)
        fwd.launch()
        bwd.launch()
        torch.cuda.synchronize()
        kept = batch.kept_graph(0)
        want = R.neighbor_moments(kept.rowptr.cpu().numpy(), kept.col.cpu().numpy(), None, x_host, n, EPS)
        got = agg.cpu().numpy()
        for q, key in enumerate(("mean", "std", "mx", "mn")):
            assert R.same(got[:, q * width:(q + 1) * width], want[key]), key
        assert np.array_equal(amax.cpu().numpy(), want["arg_max"]) and np.array_equal(amin.cpu().numpy(), want["arg_min"])
        assert np.array_equal(cnt.cpu().numpy(), want["cnt"]) and want["cnt"][9] == 0 and (want["std"][9] == 0).all()
        t = batch.thinned_t(0)
        gs = {key: gy_host[:, q * width:(q + 1) * width] for q, key in enumerate(("mean", "std", "mx", "mn"))}
        wd = R.neighbor_moments_backward(t.rowptr.cpu().numpy(), t.kept_col.cpu().numpy(), t.kept_len.cpu().numpy(), x_host, gs, want, n)
        assert R.same(d.cpu().numpy(), wd)
        seen.append(want["cnt"])
    assert kind == "neighbor_sample" or not np.array_equal(seen[0], seen[1])
