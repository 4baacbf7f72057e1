"""GPU tests of the signed-attention kernels (csrc/signed_att.hip: wdg_signed_att_forward_batched_f32, wdg_signed_att_backward_batched_f32)
against the fp64 restatement of tests/_signed_att_ref.py with a DERIVED bound: for every element |got - ref| <= K 2^-24 companion, K per
output from _signed_att_ref.bound_factors (its docstring has the derivation: roundings on the way to the element, plus T, the error of the
device's tanhf in ulps).  T is MEASURED here, not assumed: job T_JOB has no scales, so its alpha IS tanhf(pre), and pre is one fp32 add
the test reproduces exactly; the bound uses the measured maximum + 1 ulp.  T and the largest ratio error / bound per output are printed;
DESIGN 4.27 records them.  And the exact properties the header states.

One property is stated otherwise than the issue that asked for these tests words it: at S = 0 the weights alpha and d_H are +0 and out is
fmaf(eps, res, +0) bit for bit, but d_pre and d_S are NOT zero - u = 1 - tanh(0)^2 = 1 there, so d_pre = dalpha coef, the largest score
gradient the layer has (the header's formulas, and torch's autograd on the dense restatement, agree)."""
import numpy as np
import pytest
import torch

import _signed_att_ref as ref

pytestmark = pytest.mark.gpu

CANARY = 777.0
U = 2.0 ** -24
EPS = 0.3


def _rows_to_csr(rows):
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rowptr, (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)


def _p140():
    """a directed 140-node pattern: rows of 1, 63, 64, 65 and 130 entries (rows 0 .. 4: the chunk boundary of 64 and the batch tails 8, 4,
    2, 1 of gt_chains), 1 .. 12 entries elsewhere, row 139 empty; column 7 is stored by rows 0 .. 130, so its transposed row crosses two
    chunk boundaries as well"""
    rng = np.random.default_rng(140)
    n, rows = 140, []
    lengths = {0: 1, 1: 63, 2: 64, 3: 65, 4: 130, 139: 0}
    others = np.setdiff1d(np.arange(n), [7])
    for i in range(n):
        k = lengths.get(i, int(rng.integers(1, 13)))
        if i <= 130:
            rows.append(np.sort(np.concatenate([rng.choice(others, k - 1, replace=False), [7]])))
        else:
            rows.append(np.sort(rng.choice(others, k, replace=False)))
    return _rows_to_csr(rows)


def _p65():
    """65 rows - a seventeenth workgroup with one live wave -, 0 .. 9 entries each, directed"""
    rng = np.random.default_rng(65)
    return _rows_to_csr([np.sort(rng.choice(65, int(rng.integers(0, 10)), replace=False)) for _ in range(65)])


def _p0():
    return np.array([0], np.int32), np.zeros(0, np.int32)


def _p1():
    return np.array([0, 1], np.int32), np.array([0], np.int32)


def _p3():
    """row 0 empty, row 1 with one entry that is not itself, column 1 stored by nobody"""
    return np.array([0, 0, 1, 3], np.int32), np.array([2, 0, 2], np.int32)


PATTERNS = {"p0": _p0, "p1": _p1, "p3": _p3, "p65": _p65, "p140": _p140}
# (pattern, heads, w, layout, scales, residual, largest |S|): layout "plain" = contiguous matrices, "slices" = every operand a column
# slice, one float in, of a wider matrix with an ODD leading dimension (scalar accesses), "wide16" = slices that keep the 16-byte
# alignment (the vector path on a slice); scales "both" / "row" / "none"; |S| <= 10: pre reaches +-20
CASES = [("p0", 1, 4, "plain", "both", True, 4), ("p1", 2, 4, "plain", "row", True, 4), ("p3", 1, 5, "slices", "both", True, 4),
         ("p3", 8, 8, "plain", "none", False, 4), ("p65", 3, 5, "slices", "both", True, 4), ("p65", 2, 4, "wide16", "row", False, 4),
         ("p140", 1, 1, "plain", "both", True, 4), ("p140", 1, 7, "plain", "row", False, 4), ("p140", 2, 4, "wide16", "both", True, 4),
         ("p140", 3, 5, "slices", "both", True, 4), ("p140", 8, 8, "plain", "none", False, 10), ("p140", 8, 32, "plain", "both", True, 4),
         ("p140", 1, 256, "wide16", "both", False, 4)]
T_JOB = 10  # no scales, |pre| up to 20: alpha is tanhf(pre) itself
OUTPUTS = ("out", "alpha", "d_h", "d_s")
MATS = ("h", "out", "d_out", "d_h")


@pytest.fixture(scope="module")
def graphs():
    """{name: (the CsrGraph, its transpose, t_pos, the host pattern, the host transposed pattern)}"""
    from wdg_amd import ops
    out = {}
    for name, make in PATTERNS.items():
        rowptr, col = make()
        n = len(rowptr) - 1
        if n == 0:  # (nothing to build: the pattern of no rows, its transpose and no positions)
            i32 = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
            g, gt, t_pos = ops.CsrGraph(i32(rowptr), i32(col), None, 0, 0), ops.CsrGraph(i32(rowptr.copy()), i32(col.copy()), None, 0, 0), i32(col.copy())
        else:
            g = ops.CsrGraph.from_coo(ref.entry_rows(rowptr), col, n)
            assert np.array_equal(g.rowptr.cpu().numpy(), rowptr) and np.array_equal(g.col.cpu().numpy(), col)
            gt = g.transpose()
            t_pos = g.transpose_positions(gt)
        out[name] = (g, gt, t_pos, (rowptr, col), ref.transposed(rowptr, col))
    assert not np.array_equal(out["p140"][2].cpu().numpy(), np.arange(out["p140"][0].nnz))  # directed: the transpose differs
    return out


def _view(rows, cols, layout, fill=None):
    """-> (view [rows, cols], the buffer around it): a canary row above and below and, in the sliced layouts, canary columns left and
    right of the view"""
    left, right = {"plain": (0, 0), "slices": (1, 1 if cols % 2 else 2), "wide16": (4, 4 + (-cols) % 4)}[layout]  # (slices: an odd pitch)
    full = torch.full((rows + 2, left + cols + right), CANARY, device="cuda")
    v = full[1:rows + 1, left:left + cols]
    if fill is not None:
        v.copy_(torch.from_numpy(fill))
    return v, full


def _canaries_intact(full, view):
    mask = torch.ones_like(full, dtype=torch.bool)
    mask[1:1 + view.shape[0], view.storage_offset() % full.stride(0):view.storage_offset() % full.stride(0) + view.shape[1]] = False
    return bool((full[mask] == CANARY).all())


def _scores(rng, n, heads, smax):
    s = rng.uniform(-smax, smax, (n, 2 * heads))
    if smax > 4:  # a quarter of the rows sit at the ends of the range: pairs of them reach |pre| = 19 .. 20
        far = rng.random(n) < 0.25
        s[far] = np.sign(s[far]) * rng.uniform(smax - 0.5, smax, (int(far.sum()), 2 * heads))
    return s


def _entry(case, seed, graphs):
    """-> (the entry of ops.SignedAttBatch, its fp32 host inputs, the buffers around its outputs)"""
    name, heads, w, layout, scales, residual, smax = case
    g, gt, t_pos, _, _ = graphs[name]
    n, rng = g.n_rows, np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    host = dict(h=f32(rng.standard_normal((n, heads * w))), s=f32(_scores(rng, n, heads, smax)), d_out=f32(rng.standard_normal((n, heads * w))),
                res=f32(rng.standard_normal((n, heads * w))) if residual else None,
                row_scale=f32(rng.uniform(0.2, 1.0, n)) if scales in ("both", "row") else None, col_scale=f32(rng.uniform(0.2, 1.0, n)) if scales == "both" else None)
    e, around = dict(graph=g, graph_t=gt, t_pos=t_pos, heads=heads), {}
    for k, cols in (("h", heads * w), ("s", 2 * heads), ("d_out", heads * w), ("res", heads * w)):
        if host[k] is not None:
            e[k], _ = _view(n, cols, layout, host[k])
    for k in ("row_scale", "col_scale"):
        if host[k] is not None:
            e[k] = torch.from_numpy(host[k]).cuda()
    for k, cols in (("out", heads * w), ("d_h", heads * w), ("d_s", 2 * heads)):
        e[k], around[k] = _view(n, cols, layout)
    return e, host, around


def _restated(case, host, graphs):
    name, heads = case[:2]
    rowptr, col = graphs[name][3]
    x = {k: None if v is None else v.astype(np.float64) for k, v in host.items()}
    res = ref.forward(rowptr, col, x["h"], x["s"], heads, x["row_scale"], x["col_scale"], x["res"], EPS)
    res.update(ref.backward(rowptr, col, x["h"], x["s"], heads, x["d_out"], x["row_scale"], x["col_scale"]))
    return res


def _results(entries, batch):
    got = [{k: e[k].cpu().numpy().copy() for k in ("out", "d_h", "d_s")} for e in entries]
    for g_, alpha in zip(got, batch.alpha_of):
        g_["alpha"] = alpha.cpu().numpy().copy()
    return got


def _launch(entries, eps=EPS, backward=True):
    from wdg_amd import ops
    batch = ops.SignedAttBatch(entries, eps)
    batch.launch()
    if backward:
        batch.launch_backward()
    torch.cuda.synchronize()
    return batch


@pytest.fixture(scope="module")
def table(graphs):
    """the ragged table - jobs of 0, 1, 3, 65 and 140 rows share a launch -, run forward and backward once:
    (entries, host inputs, the batch, its results on the host, the buffers around the outputs, the fp64 restatement, d_pre on the host)"""
    built = [_entry(case, 40 + i, graphs) for i, case in enumerate(CASES)]
    entries, hosts, around = [b[0] for b in built], [b[1] for b in built], [b[2] for b in built]
    batch = _launch(entries)
    restated = [_restated(case, host, graphs) for case, host in zip(CASES, hosts)]  # (computed once, shared, never changed)
    offs = np.concatenate([[0], np.cumsum([graphs[c[0]][0].nnz * c[1] for c in CASES])])
    flat = batch.d_pre.cpu().numpy()
    d_pre = [flat[offs[i]:offs[i + 1]].reshape(-1, c[1]).copy() for i, c in enumerate(CASES)]
    return entries, hosts, batch, _results(entries, batch), around, restated, d_pre


@pytest.fixture(scope="module")
def tanh_ulps(table):
    """T: the largest error of the device's tanhf over the entries of T_JOB, in ulps of the correctly rounded result, + 1 ulp"""
    hosts, got, case = table[1], table[3], CASES[T_JOB]
    assert case[4] == "none" and case[6] >= 10
    rowptr, col = PATTERNS[case[0]]()
    rows, heads, s = ref.entry_rows(rowptr), case[1], hosts[T_JOB]["s"]
    pre = s[rows, :heads] + s[col.astype(np.int64), heads:]     # fp32 + fp32: the kernel's one add, bit for bit
    assert pre.dtype == np.float32 and pre.size >= 3000 and pre.min() < -19 and pre.max() > 19
    assert min(np.histogram(pre, bins=8, range=(-20, 20))[0]) >= 50  # spread over +-20
    measured = ref.tanh_ulps(got[T_JOB]["alpha"], pre)
    print(f"tanhf on the device: largest error {measured:.3f} ulps over {pre.size} arguments in [{pre.min():.2f}, {pre.max():.2f}]; T = {measured + 1:.3f}")
    return measured + 1.0, pre


def test_kernels_match_the_fp64_restatement_within_the_derived_bound(table, graphs, tanh_ulps):
    entries, hosts, batch, got, around, restated, d_pre = table
    misses, worst = [], {}
    for i, (case, g_, r) in enumerate(zip(CASES, got, restated)):
        rowptr, t_rowptr = graphs[case[0]][3][0], graphs[case[0]][4][0]
        ks = ref.bound_factors(tanh_ulps[0], rowptr, t_rowptr, case[2])
        for k in OUTPUTS + ("d_pre",):
            have = d_pre[i] if k == "d_pre" else g_[k]
            if r[k].size == 0:
                assert have.size == 0
                continue
            bound = ks[k] * U * r[k + "_abs"]
            err = np.abs(have.astype(np.float64) - r[k])
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = float(np.nanmax(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))))
            worst[k] = max(worst.get(k, 0.0), ratio)
            print(f"job {i} {case} {k}: K {ks[k]:.0f} largest error / bound {ratio:.4f}")
            if not (err <= bound).all():
                misses.append(f"job {i} {case} {k}: error / bound {ratio:.3e}")
    print("largest error / bound per output:", {k: round(v, 4) for k, v in worst.items()})
    assert not misses, "\n".join(misses)


def test_saturated_scores_give_weights_of_one_and_no_score_gradient(table, tanh_ulps):
    """|pre| >= 15: t = +-1 and u = fmaf(-t, t, 1) = 0 exactly, so d_pre is +-0; and the job holds weights of both signs"""
    got, d_pre, pre = table[3], table[6], tanh_ulps[1]
    far = np.abs(pre) >= 15
    assert far.sum() >= 100
    assert np.array_equal(got[T_JOB]["alpha"][far], np.sign(pre[far])) and not d_pre[T_JOB][far].any()
    assert (got[T_JOB]["alpha"] < 0).any() and (got[T_JOB]["alpha"] > 0).any() and d_pre[T_JOB][~far].any()


def test_rows_beyond_a_job_and_columns_beside_it_are_untouched(table):
    entries, _, _, _, around, _, _ = table
    for case, e, bufs in zip(CASES, entries, around):
        for k, full in bufs.items():
            assert _canaries_intact(full, e[k]), (case, k)


def test_the_table_covers_both_access_paths(table):
    """jobs whose rows take the 16-byte path (plain and sliced) and jobs that take the scalar path, 256 columns and 15 with an odd
    leading dimension among them; the residual follows its job's layout"""
    entries = table[0]
    vec = lambda t: t.shape[1] >= 4 and t.shape[1] % 4 == 0 and t.data_ptr() % 16 == 0 and (t.stride(0) * 4) % 16 == 0  # noqa: E731
    mats = lambda e: [e[k] for k in MATS + ("res",) if k in e]  # noqa: E731
    live = [(c, e) for c, e in zip(CASES, entries) if c[0] not in ("p0", "p1")]
    on_vec = {(c[1] * c[2], c[3]) for c, e in live if all(vec(t) for t in mats(e))}
    scalar = {(c[1] * c[2], c[3]) for c, e in live if not any(vec(t) for t in mats(e))}
    assert on_vec == {(256, "plain"), (256, "wide16"), (64, "plain"), (8, "wide16")}, on_vec
    assert scalar == {(15, "slices"), (5, "slices"), (1, "plain"), (7, "plain")}, scalar
    assert len(on_vec) + len(scalar) == len({(c[1] * c[2], c[3]) for c, _ in live})  # no job mixes the paths
    assert entries[9]["h"].stride(0) % 2 == 1 and "res" in entries[9]  # (3, 5) in slices: an odd leading dimension, residual included


def test_a_second_launch_repeats_every_bit(table):
    entries, _, batch, got, _, _, d_pre = table
    before = batch.d_pre.clone()
    for e in entries:  # (what the launches write is cleared first: a stale value would not pass for a repeated one)
        for k in ("out", "d_h", "d_s"):
            e[k].fill_(5.0)
    batch.alpha.fill_(5.0)
    batch.d_pre.fill_(5.0)
    batch.launch()
    batch.launch_backward()
    torch.cuda.synchronize()
    for case, a, b in zip(CASES, got, _results(entries, batch)):
        for k in a:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (case, k)
    assert torch.equal(before.view(torch.int32), batch.d_pre.view(torch.int32))


def test_a_job_alone_answers_what_it_answers_in_the_table(table, graphs):
    got = table[3]
    for i, case in enumerate(CASES):
        e, _, _ = _entry(case, 40 + i, graphs)
        res = _results([e], _launch([e]))[0]
        for k in got[i]:
            assert np.array_equal(got[i][k].view(np.uint32), res[k].view(np.uint32)), (case, k)


def test_a_head_has_the_bits_of_a_one_head_job_on_its_slices(table):
    """H, d_out, the residual and the outputs' columns of head h are passed IN PLACE (slices with the job's leading dimension); the
    head's two score columns are copied side by side"""
    entries, _, _, got, _, _, _ = table
    seen = 0
    for i, case in enumerate(CASES):
        heads, w = case[1], case[2]
        if heads == 1 or case[0] == "p0":
            continue
        e = entries[i]
        for h in {0, heads - 1, heads // 2}:
            sl = slice(h * w, (h + 1) * w)
            s1 = torch.stack([e["s"][:, h], e["s"][:, heads + h]], 1).contiguous()
            one = dict(graph=e["graph"], graph_t=e["graph_t"], t_pos=e["t_pos"], heads=1, h=e["h"][:, sl], s=s1, d_out=e["d_out"][:, sl],
                       out=torch.zeros_like(e["out"][:, sl]), d_h=torch.zeros_like(e["d_h"][:, sl]), d_s=torch.zeros_like(s1))
            one.update({k: e[k] for k in ("row_scale", "col_scale") if k in e})
            if "res" in e:
                one["res"] = e["res"][:, sl]
            res = _results([one], _launch([one]))[0]
            bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
            assert np.array_equal(bits(res["out"]), bits(got[i]["out"][:, sl])), (case, h)
            assert np.array_equal(bits(res["alpha"][:, 0]), bits(got[i]["alpha"][:, h])), (case, h)
            assert np.array_equal(bits(res["d_h"]), bits(got[i]["d_h"][:, sl])), (case, h)
            assert np.array_equal(bits(res["d_s"]), bits(got[i]["d_s"][:, [h, heads + h]])), (case, h)
            seen += 1
    assert seen >= 15


def test_zero_scores_give_the_residual_alone_bit_for_bit(graphs):
    """S = 0: t = tanhf(+0) = +0, so alpha and d_H are +0 in every bit and out = fmaf(eps, res, +0); u = 1 there, so d_pre = dalpha coef
    and d_S do NOT vanish (the module's docstring) - they stay within the derived bound of the restatement, which the table's test
    asserts for every job"""
    g, gt, t_pos, (rowptr, col), _ = graphs["p140"]
    n, heads, w = g.n_rows, 3, 5
    rng = np.random.default_rng(5)
    dev = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()  # noqa: E731
    z = lambda *shape: torch.full(shape, 5.0, device="cuda")  # noqa: E731
    res = rng.standard_normal((n, heads * w)).astype(np.float32)
    e = dict(graph=g, graph_t=gt, t_pos=t_pos, heads=heads, h=dev(rng.standard_normal((n, heads * w))), s=torch.zeros(n, 2 * heads, device="cuda"),
             d_out=dev(rng.standard_normal((n, heads * w))), res=torch.from_numpy(res).cuda(), row_scale=dev(rng.uniform(0.2, 1, n)),
             col_scale=dev(rng.uniform(0.2, 1, n)), out=z(n, heads * w), d_h=z(n, heads * w), d_s=z(n, 2 * heads))
    batch = _launch([e])
    want = np.float32(EPS) * res + np.float32(0.0)   # fmaf(eps, res, +0): one rounding of the product, and -0 + +0 = +0
    assert np.array_equal(e["out"].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert not batch.alpha_of[0].cpu().numpy().view(np.uint32).any() and not e["d_h"].cpu().numpy().view(np.uint32).any()
    assert batch.d_pre.cpu().numpy().any() and e["d_s"].cpu().numpy()[:139].any()
    e2 = dict(e, out=z(n, heads * w), d_h=z(n, heads * w), d_s=z(n, 2 * heads))
    del e2["res"]
    _launch([e2])
    assert not e2["out"].cpu().numpy().view(np.uint32).any()  # no residual: +0


def test_the_empty_row_and_the_unstored_column_give_plus_zero(table):
    """p3: row 0 stores nothing, column 1 is stored by nobody"""
    hosts, got = table[1], table[3]
    seen = 0
    for case, host, g_ in zip(CASES, hosts, got):
        if case[0] != "p3":
            continue
        heads = case[1]
        for a in (g_["d_s"][0, :heads], g_["d_h"][1], g_["d_s"][1, heads:]):
            assert not a.view(np.uint32).any(), case  # every bit zero: +0
        want = np.float32(EPS) * host["res"][0] + np.float32(0.0) if case[5] else np.zeros(heads * case[2], np.float32)
        assert np.array_equal(g_["out"][0].view(np.uint32), want.view(np.uint32)), case
        seen += 1
    assert seen == 2


def test_a_nan_reaches_exactly_the_rows_that_store_it(graphs):
    """forward: a NaN in row j of H -> out[i, :] of exactly the rows i that store j; backward: a NaN in d_out[i, :] -> d_H[j, :] of
    exactly the columns j that row i stores"""
    case = ("p140", 2, 4, "plain", "both", True, 4)
    rowptr, col = graphs["p140"][3]
    rows = ref.entry_rows(rowptr)
    e, _, _ = _entry(case, 91, graphs)
    j = 33
    e["h"][j, 3] = float("nan")
    _launch([e])
    bad = torch.isnan(e["out"]).any(1).cpu().numpy()
    assert np.array_equal(np.flatnonzero(bad), np.unique(rows[col == j])) and bad.any() and not bad.all()
    assert not torch.isnan(e["out"][:, 4:]).any()  # (the other head's columns hold no NaN)
    e, _, _ = _entry(case, 92, graphs)
    i = 3
    e["d_out"][i, 6] = float("nan")
    _launch([e])
    bad = torch.isnan(e["d_h"]).any(1).cpu().numpy()
    assert np.array_equal(np.flatnonzero(bad), col[rowptr[i]:rowptr[i + 1]]) and not bad.all()
    assert not torch.isnan(e["out"]).any() and not torch.isnan(e["d_h"][:, :4]).any()


def test_binding_refuses_on_the_device_what_the_kernel_does_not_take(graphs):
    from wdg_amd import ops
    e, _, _ = _entry(("p3", 2, 4, "plain", "both", True, 4), 1, graphs)
    with pytest.raises(ValueError, match="contiguous"):
        ops.SignedAttBatch([dict(e, h=torch.zeros((8, 3), device="cuda").t())])
    with pytest.raises(ValueError, match="overlap"):
        ops.SignedAttBatch([dict(e, d_h=e["res"])])
    with pytest.raises(ValueError, match="device"):
        ops.SignedAttBatch([dict(e, row_scale=torch.ones(3))])
    with pytest.raises(ValueError, match="t_pos"):
        ops.SignedAttBatch([dict(e, t_pos=e["t_pos"][:-1])])
    forward_only = {k: v for k, v in e.items() if k not in ("graph_t", "t_pos", "d_out", "d_h", "d_s")}
    batch = _launch([forward_only], backward=False)
    with pytest.raises(ValueError, match="SignedAttBatch.launch_backward: the table was built without gradient"):
        batch.launch_backward()
    empty = ops.SignedAttBatch([])
    empty.launch()
    empty.launch_backward()
