"""GPU tests of wdg_adam_batched_f32 (csrc/adam.hip, ops.AdamBatch) against the float32 restatement of tests/_adam_ref.py, BIT FOR BIT:
every operation of the step is one correctly rounded fp32 operation (the unit is compiled with contraction off), the two bias
corrections are formed in double and rounded once, and numpy does the same - so the bound is equality, derived and not measured."""
import numpy as np
import pytest
import torch

import _adam_ref as ref

pytestmark = pytest.mark.gpu

ROWS = (0, 1, 3, 64, 65, 130)
COLS = (1, 4, 5, 63, 64, 65, 129, 260)
SEG_COLS = (1, 4, 5, 8, 64, "cols")
SEG_ROWS = (1, 16, "rows")
LAYOUTS = ("plain", "padded", "slices")
STEPS = (1, 2, 1000, 100000)
BETAS, EPS = (0.9, 0.999), 1e-8


def _cases():
    """every (rows, cols) in all three layouts; the segment shapes cycle so that every seg_rows meets every seg_cols and the ragged
    last segments occur (65 rows in segments of 16, 63 / 65 / 129 / 260 columns in segments of 4, 5, 8, 64)"""
    out, k = [], 0
    for rows in ROWS:
        for cols in COLS:
            for layout in LAYOUTS:
                sc, sr = SEG_COLS[k % len(SEG_COLS)], SEG_ROWS[(k // len(SEG_COLS)) % len(SEG_ROWS)]
                out.append((rows, cols, max(rows, 1) if sr == "rows" else sr, max(cols, 1) if sc == "cols" else sc, layout))
                k += 1
    return out


CASES = _cases()


def _pair(rows, cols, layout):
    """-> (p, g): two [rows, cols] device views with one leading dimension.  "plain": contiguous; "padded": a pitch of cols + 3 floats
    and a start one float in (never 16-byte rows: the scalar path); "slices": column slices of one wider matrix whose pitch and
    slice starts are multiples of 16 bytes (the 16-byte path wherever a whole group of four columns lies inside the job)"""
    dev = "cuda"
    if layout == "plain":
        return torch.zeros((rows, cols), device=dev), torch.zeros((rows, cols), device=dev)
    if layout == "padded":
        return torch.zeros((rows, cols + 3), device=dev)[:, 1:1 + cols], torch.zeros((rows, cols + 3), device=dev)[:, 1:1 + cols]
    w = -(-cols // 4) * 4
    wide = torch.zeros((rows, 2 * w), device=dev)
    return wide[:, :cols], wide[:, w:w + cols]


def _host_inputs(case, seed):
    rows, cols, seg_rows, seg_cols, _ = case
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    shape = (rows, cols)
    # |g| is 0 or at least 1e-12, and v is 0 or at least 1e-20: v stays in the normal range
    g = f32(rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-12, 2, shape))
    g[rng.random(shape) < 0.1] = 0.0
    v = f32(10.0 ** rng.uniform(-20, 2, shape))
    v[rng.random(shape) < 0.1] = 0.0
    m = f32(rng.standard_normal(shape) * 10.0 ** rng.uniform(-6, 1, shape))
    p = f32(rng.standard_normal(shape))
    segs = ref.n_segments(rows, cols, seg_rows, seg_cols)
    hyper = f32(np.stack([10.0 ** rng.uniform(-4, -1, segs), np.where(rng.random(segs) < 0.3, 0.0, 10.0 ** rng.uniform(-5, -2, segs))], 1)).reshape(segs, 2)
    return dict(p=p, g=g, m=m, v=v, hyper=hyper)


def _load(batch, entries, hosts, only=None):
    for i, (e, h) in enumerate(zip(entries, hosts)):
        if only is not None and i != only:
            continue
        e[0].copy_(torch.from_numpy(h["p"]))
        e[1].copy_(torch.from_numpy(h["g"]))
        j = 0 if only is not None else i
        batch.m[j].copy_(torch.from_numpy(h["m"]))
        batch.v[j].copy_(torch.from_numpy(h["v"]))


def _read(batch, entries):
    return [(e[0].cpu().numpy().copy(), m.cpu().numpy().copy(), v.cpu().numpy().copy()) for e, m, v in zip(entries, batch.m, batch.v)]


def _step_word(t):
    return torch.tensor([t - 1], dtype=torch.int32, device="cuda")


def _same_bits(a, b):
    """the same 32 bits everywhere, except that a NaN matches a NaN (IEEE 754 leaves a NaN's sign and payload open)"""
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def table():
    """the ragged table, launched once per step of STEPS from the same inputs: (entries, hosts, batch, {t: results})"""
    from wdg_amd import ops
    hosts = [_host_inputs(case, 100 + i) for i, case in enumerate(CASES)]
    entries = []
    for case, h in zip(CASES, hosts):
        p, g = _pair(case[0], case[1], case[4])
        entries.append((p, g, case[2], case[3], h["hyper"]))
    batch = ops.AdamBatch(entries, betas=BETAS, eps=EPS)
    got = {}
    for t in STEPS:
        _load(batch, entries, hosts)
        batch.launch(_step_word(t))
        torch.cuda.synchronize()
        got[t] = _read(batch, entries)
    return entries, hosts, batch, got


@pytest.fixture(scope="module")
def expected():
    hosts = [_host_inputs(case, 100 + i) for i, case in enumerate(CASES)]
    return {t: [ref.adam_step(h["p"], h["g"], h["m"], h["v"], h["hyper"], case[2], case[3], t, BETAS[0], BETAS[1], EPS)
                for case, h in zip(CASES, hosts)] for t in STEPS}


@pytest.mark.parametrize("t", STEPS)
def test_the_kernel_equals_the_float32_restatement_bit_for_bit(table, expected, t):
    got, misses = table[3][t], []
    for i, (case, g, w) in enumerate(zip(CASES, got, expected[t])):
        for name, a, b in zip(("p", "m", "v"), g, w):
            assert a.dtype == b.dtype == np.float32
            if not _same_bits(a, b):
                bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
                r, c = bad[0]
                misses.append(f"job {i} {case} {name}: {len(bad)} of {a.size} elements differ, first at ({r}, {c}): {a[r, c]!r} against {b[r, c]!r}")
    assert not misses, "\n".join(misses[:20])
    assert sum(g[0].size for g in got) > 100000


def _vector_path(t):
    """the kernel's rule (csrc/adam.hip: ad_operand / ad_load4): 16-byte accesses for an operand whose pointer and pitch are multiples
    of 16 bytes, for the groups of four columns that lie inside the job"""
    return t.shape[0] > 0 and t.shape[1] >= 4 and t.data_ptr() % 16 == 0 and (max(t.stride(0), t.shape[1]) * 4) % 16 == 0


def test_the_table_covers_both_access_paths(table):
    """the table really holds jobs whose four operands all take the 16-byte path (contiguous and sliced), jobs whose parameter and
    gradient take the scalar path while the moments take the 16-byte one, jobs that are scalar throughout, and ragged right edges
    beside 16-byte groups"""
    entries, _, batch, _ = table
    vec = {(case[1], case[4]) for case, e, m in zip(CASES, entries, batch.m) if case[0] and _vector_path(e[0]) and _vector_path(e[1]) and _vector_path(m)}
    scalar = {(case[1], case[4]) for case, e, m in zip(CASES, entries, batch.m) if case[0] and not _vector_path(e[0]) and not _vector_path(e[1])}
    mixed = {(case[1], case[4]) for case, e, m in zip(CASES, entries, batch.m) if case[0] and not _vector_path(e[0]) and _vector_path(m)}
    assert {(4, "plain"), (64, "plain"), (260, "plain"), (4, "slices"), (64, "slices"), (260, "slices")} <= vec, vec
    assert {(c, "padded") for c in COLS} | {(1, "plain"), (5, "plain"), (63, "plain"), (65, "plain"), (129, "plain")} <= scalar, scalar
    assert {(64, "padded"), (260, "padded"), (4, "padded")} <= mixed, mixed
    # slices of 5, 63, 65, 129 columns: 16-byte groups with a ragged scalar edge for p and g, scalar moments (an odd pitch)
    assert all(_vector_path(e[0]) and not _vector_path(m) for case, e, m in zip(CASES, entries, batch.m) if case[0] and case[4] == "slices" and case[1] in (5, 63, 65, 129))
    assert {case[2] for case in CASES} >= {1, 16, 130} and {case[3] for case in CASES} >= {1, 4, 5, 8, 64, 260}


def test_a_job_alone_equals_the_job_in_the_table(table):
    from wdg_amd import ops
    entries, hosts, _, got = table
    t = 1000
    for i, (case, e, h) in enumerate(zip(CASES, entries, hosts)):
        alone = ops.AdamBatch([e], betas=BETAS, eps=EPS)
        _load(alone, entries, hosts, only=i)
        alone.launch(_step_word(t))
        res = _read(alone, [e])[0]
        assert all(_same_bits(a, b) for a, b in zip(res, got[t][i])), (i, case)


def test_a_second_launch_repeats_the_bits(table):
    entries, hosts, batch, got = table
    _load(batch, entries, hosts)
    batch.launch(_step_word(2))
    torch.cuda.synchronize()
    for i, (res, first) in enumerate(zip(_read(batch, entries), got[2])):
        assert all(_same_bits(a, b) for a, b in zip(res, first)), i


def test_padding_zero_lr_and_one_nan():
    """w [F, R cs] with cs = 8, C = 5: the padding columns (p = 0, g = 0) stay +0.0f in p, m and v; the replica with lr = 0 keeps its
    weights while its moments move; one NaN gradient poisons its own element alone"""
    from wdg_amd import ops
    rng = np.random.default_rng(5)
    F, R, cs, C = 70, 3, 8, 5
    p = rng.standard_normal((F, R * cs)).astype(np.float32)
    g = rng.standard_normal((F, R * cs)).astype(np.float32)
    pad = (np.arange(R * cs) % cs) >= C
    p[:, pad], g[:, pad] = 0.0, 0.0
    g[11, 2] = np.nan  # (in the first replica)
    hyper = np.array([[0.01, 5e-4], [0.0, 5e-4], [0.05, 0.0]], np.float32)
    pt, gt = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    batch = ops.AdamBatch([(pt, gt, F, cs, hyper)])
    step = _step_word(1)
    for _ in range(3):
        batch.launch(step)
        step.add_(1)
    torch.cuda.synchronize()
    outs = [pt.cpu().numpy(), batch.m[0].cpu().numpy(), batch.v[0].cpu().numpy()]
    for a in outs:
        assert not a.view(np.uint32)[:, pad].any()                            # +0.0f: not even a sign bit
        assert np.isnan(a[11, 2]) and int(np.isnan(a).sum()) == 1
    assert np.array_equal(outs[0][:, cs:cs + C], p[:, cs:cs + C]) and outs[1][:, cs:cs + C].all() and outs[2][:, cs:cs + C].all()
    moved = np.abs(outs[0] - p)
    assert float(np.nanmin(moved[:, :C])) > 0 and float(np.nanmin(moved[:, 2 * cs:2 * cs + C])) > float(np.nanmax(moved[:, :C]))
    want = (p, np.zeros_like(p), np.zeros_like(p))
    for t in (1, 2, 3):
        want = ref.adam_step(want[0], g, want[1], want[2], hyper, F, cs, t)
    assert all(_same_bits(a, b) for a, b in zip(outs, want))


def test_set_hyper_rewrites_the_device_table_in_place():
    from wdg_amd import ops
    rng = np.random.default_rng(6)
    p0, g = rng.standard_normal((8, 12)).astype(np.float32), rng.standard_normal((8, 12)).astype(np.float32)
    pt, gt = torch.from_numpy(p0).cuda(), torch.from_numpy(g).cuda()
    batch = ops.AdamBatch([(pt, gt, 8, 4, np.full((3, 2), 0.01, np.float32))])
    where = batch.hyper.data_ptr()
    batch.set_hyper([0.1, 0.0, 0.001], 0.0)
    assert batch.hyper.data_ptr() == where and batch.hyper_of[0].cpu().tolist() == [[np.float32(0.1), 0.0], [0.0, 0.0], [np.float32(0.001), 0.0]]
    batch.launch(_step_word(1))
    want = ref.adam_step(p0, g, np.zeros_like(p0), np.zeros_like(p0), np.array([[0.1, 0], [0, 0], [0.001, 0]], np.float32), 8, 4, 1)
    assert _same_bits(pt.cpu().numpy(), want[0])
    with pytest.raises(ValueError):
        batch.set_hyper([0.1, 0.2], 0.0)
    batch.reset()
    assert not batch.moments.any()


def test_three_captured_replays_equal_three_eager_steps():
    from wdg_amd import ops
    rng = np.random.default_rng(8)
    shapes = [(70, 96, 70, 32), (96, 8, 32, 8)]  # w0 [F, R hidden] and w1 [R hidden, cs] of three replicas
    hosts = [(rng.standard_normal((r, c)).astype(np.float32), rng.standard_normal((r, c)).astype(np.float32)) for r, c, _, _ in shapes]
    hyper = np.array([[0.01, 5e-4], [0.05, 0.0], [0.002, 5e-3]], np.float32)
    runs = []
    for captured in (False, True):
        tensors = [(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()) for p, g in hosts]
        batch = ops.AdamBatch([(p, g, sr, sc, hyper) for (p, g), (_, _, sr, sc) in zip(tensors, shapes)])
        step = torch.zeros(1, dtype=torch.int32, device="cuda")

        def one():
            batch.launch(step)
            step.add_(1)

        if captured:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                one()
            for _ in range(3):
                graph.replay()
        else:
            for _ in range(3):
                one()
        torch.cuda.synchronize()
        assert int(step) == 3
        runs.append([p.cpu().numpy() for p, _ in tensors] + [m.cpu().numpy() for m in batch.m] + [v.cpu().numpy() for v in batch.v])
    assert all(_same_bits(a, b) for a, b in zip(*runs))
    want = [(p, np.zeros_like(p), np.zeros_like(p)) for p, _ in hosts]
    for t in (1, 2, 3):
        want = [ref.adam_step(w[0], g, w[1], w[2], hyper, sr, sc, t) for w, (_, g), (_, _, sr, sc) in zip(want, hosts, shapes)]
    assert all(_same_bits(a, w[0]) for a, w in zip(runs[0][:2], want))


def test_refusals():
    import ctypes
    from wdg_amd import ops
    from wdg_amd._lib import lib
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    h1 = np.zeros((1, 2), np.float32)
    ok = (z(4, 8), z(4, 8), 4, 8, h1)
    ops.AdamBatch([ok])
    ops.AdamBatch([])  # an empty table launches nothing
    ops.AdamBatch([]).launch(_step_word(1))
    bad = [(z(4, 8), z(4, 8), 0, 8, h1), (z(4, 8), z(4, 8), 4, 0, h1), (z(4, 8), z(4, 8), 4, -1, h1),      # segments below 1 x 1
           (z(4, 8), z(4, 8), 4, 4, h1),                                                               # two segments, one row of hyper
           (z(4, 8), z(4, 9)[:, :8], 4, 8, h1),                                                        # two leading dimensions
           (z(4, 8), z(4, 7), 4, 8, h1), (z(4, 8).double(), z(4, 8).double(), 4, 8, h1),               # shapes, dtypes
           (z(8, 4).t(), z(8, 4).t(), 4, 8, h1), (z(4, 8).cpu(), z(4, 8).cpu(), 4, 8, h1), (z(32), z(32), 4, 8, h1)]
    for e in bad:
        with pytest.raises(ValueError):
            ops.AdamBatch([e])
    wide = z(4, 16)
    with pytest.raises(ValueError):
        ops.AdamBatch([(wide[:, :8], wide[:, 4:12], 4, 8, h1)])   # the parameter and its gradient overlap
    ops.AdamBatch([(wide[:, :8], wide[:, 8:], 4, 8, h1)])         # (disjoint column slices of one matrix are fine)
    for kw in (dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=float("nan"))):
        with pytest.raises(ValueError):
            ops.AdamBatch([ok], **kw)
    batch = ops.AdamBatch([ok])
    for step in (None, 3, torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32)):
        with pytest.raises(ValueError):
            batch.launch(step)
    # the entry itself, with a device present: refused before any launch
    tab, step = ctypes.c_void_p(batch.table.data_ptr()), ctypes.c_void_p(_step_word(1).data_ptr())
    assert lib.wdg_adam_batched_f32(None, 1, 4, 8, 0.9, 0.999, 1e-8, step, None) == -1
    assert lib.wdg_adam_batched_f32(tab, 1, 4, 8, 0.9, 0.999, 1e-8, None, None) == -1
    assert lib.wdg_adam_batched_f32(tab, 1, 4, 8, 1.0, 0.999, 1e-8, step, None) == -1
    assert lib.wdg_adam_batched_f32(tab, 1, 4, 8, 0.9, 0.999, float("nan"), step, None) == -1
    assert lib.wdg_adam_batched_f32(tab, 65536, 4, 8, 0.9, 0.999, 1e-8, step, None) == -1
    assert lib.wdg_adam_batched_f32(tab, -1, 4, 8, 0.9, 0.999, 1e-8, step, None) == -1
    torch.cuda.synchronize()
    assert not ok[0].any() and not batch.moments.any()  # nothing ran
