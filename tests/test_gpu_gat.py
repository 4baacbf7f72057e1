"""GPU tests of the attention kernels (csrc/gat.hip: wdg_gat_forward_batched_f32, wdg_gat_backward_batched_f32,
wdg_csr_transpose_positions) against the fp64 restatement of tests/_gat_ref.py with a DERIVED bound: for every element
|got - ref| <= K 2^-24 companion, K = 10 E + 4 d + 2 w + 32 (E the largest |pre| of the job, d the longest row of the pattern or of its
transpose; the companion is the formula with every product and summed term replaced by its absolute value) - the rounding of pre,
e - m and exp ((5 E + 4) units of roundoff per q, twice for alpha), sums of d terms for Z, c and the chains, a sum of w terms for dalpha.
The largest ratio error / bound is printed; DESIGN 4.25 records it.  And the exact properties the header states."""
import numpy as np
import pytest
import torch

import _gat_ref as ref

pytestmark = pytest.mark.gpu

CANARY = 777.0
U = 2.0 ** -24


def _p140():
    """a directed 140-node pattern: rows of 1, 63, 64, 65, 128, 129 entries (rows 0 .. 5), 0 .. 12 entries elsewhere (row 139 empty),
    and column 7 stored by rows 0 .. 128"""
    rng = np.random.default_rng(140)
    n, rows = 140, []
    lengths = {0: 1, 1: 63, 2: 64, 3: 65, 4: 128, 5: 129, 139: 0}
    for i in range(n):
        k = lengths.get(i, int(rng.integers(1, 13)))
        others = np.setdiff1d(np.arange(n), [7])
        cols = rng.choice(others, max(k - 1, 0), replace=False) if i < 129 else rng.choice(others, k, replace=False)
        if i < 129:
            cols = np.concatenate([cols, [7]])
        rows.append(np.sort(cols))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rowptr, np.concatenate(rows).astype(np.int32)


def _p1():
    return np.array([0, 1], np.int32), np.array([0], np.int32)


def _p3():
    """row 0 empty, row 1 with one entry that is not itself, column 1 stored by nobody"""
    return np.array([0, 0, 1, 3], np.int32), np.array([2, 0, 2], np.int32)


PATTERNS = {"p1": _p1, "p3": _p3, "p140": _p140}
# (pattern, heads, w, slope, layout, largest |S|): layout "plain" = contiguous matrices, "slices" = every operand a column slice, one
# float in, of a wider matrix with an ODD leading dimension (scalar accesses; (3, 33): 99 columns), "wide16" = slices that keep the
# 16-byte alignment (the vector path on a slice)
CASES = [("p1", 2, 8, 0.2, "plain", 4), ("p3", 1, 5, 0.0, "slices", 4), ("p3", 8, 8, 1.0, "plain", 4),
         ("p140", 1, 1, 0.2, "plain", 4), ("p140", 1, 5, 0.0, "slices", 4), ("p140", 1, 7, 1.0, "plain", 4), ("p140", 2, 8, 0.2, "wide16", 4),
         ("p140", 8, 8, 0.2, "plain", 4), ("p140", 3, 33, 0.2, "slices", 4), ("p140", 4, 64, 0.0, "plain", 4), ("p140", 2, 8, 0.2, "plain", 60),
         ("p140", 4, 64, 1.0, "wide16", 4)]
OUTPUTS = ("out", "alpha", "d_h", "d_s")


@pytest.fixture(scope="module")
def graphs():
    """{name: (the CsrGraph, its transpose, t_pos, the host pattern, the host transposed pattern)}"""
    from wdg_amd import ops
    out = {}
    for name, make in PATTERNS.items():
        rowptr, col = make()
        n = len(rowptr) - 1
        g = ops.CsrGraph.from_coo(ref.entry_rows(rowptr), col, n)
        assert np.array_equal(g.rowptr.cpu().numpy(), rowptr) and np.array_equal(g.col.cpu().numpy(), col)
        gt = g.transpose()
        out[name] = (g, gt, g.transpose_positions(gt), (rowptr, col), ref.transposed(rowptr, col))
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
    r0 = (view.data_ptr() - full.data_ptr()) // 4 // full.stride(0)
    c0 = (view.data_ptr() - full.data_ptr()) // 4 % full.stride(0)
    mask[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = False
    return bool((full[mask] == CANARY).all())


def _entry(case, seed, graphs):
    """-> (the entry of ops.GatBatch, its fp32 host inputs, the buffers around its outputs)"""
    name, heads, w, slope, layout, smax = case
    g, gt, t_pos, (rowptr, col), _ = graphs[name]
    n, rng = g.n_rows, np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    # |S| <= 4: uniform in +-4.  |S| <= 60: uniform in [30, 60] - pre reaches 120, where exp(pre) overflows unless the maximum is
    # subtracted, while e - m stays above -60: a bound RELATIVE to alpha can only hold while exp(e - m) is a normal fp32 number
    # (e - m > -87); scores of both signs up to 60 would put e - m at -144, where fp32 has no number at all
    s = rng.uniform(-smax, smax, (n, 2 * heads)) if smax <= 4 else rng.uniform(smax / 2, smax, (n, 2 * heads))
    host = dict(h=f32(rng.standard_normal((n, heads * w))), s=f32(s), d_out=f32(rng.standard_normal((n, heads * w))))
    e, around = dict(graph=g, graph_t=gt, t_pos=t_pos, heads=heads), {}
    for k, cols in (("h", heads * w), ("s", 2 * heads), ("d_out", heads * w)):
        e[k], _ = _view(n, cols, layout, host[k])
    for k, cols in (("out", heads * w), ("d_h", heads * w), ("d_s", 2 * heads)):
        e[k], around[k] = _view(n, cols, layout)
    return e, host, around


def _restated(case, host, graphs):
    name, heads, w, slope = case[:4]
    rowptr, col = graphs[name][3]
    h64 = {k: v.astype(np.float64) for k, v in host.items()}
    res = ref.forward(rowptr, col, h64["h"], h64["s"], heads, slope)
    res.update(ref.backward(rowptr, col, h64["h"], h64["s"], heads, slope, h64["d_out"]))
    return res


def _results(entries, batch):
    got = [{k: e[k].cpu().numpy().copy() for k in ("out", "d_h", "d_s")} for e in entries]
    for g_, alpha in zip(got, batch.alpha_of):
        g_["alpha"] = alpha.cpu().numpy().copy()
    return got


def _launch(entries, slopes):
    from wdg_amd import ops
    batch = ops.GatBatch(entries, slopes)
    batch.launch()
    batch.launch_backward()
    torch.cuda.synchronize()
    return batch


@pytest.fixture(scope="module")
def table(graphs):
    """the ragged table - jobs of 1, 3 and 140 rows share a launch -, run forward and backward once:
    (entries, host inputs, the batch, its results on the host, the buffers around the outputs, the fp64 restatement)"""
    built = [_entry(case, 20 + i, graphs) for i, case in enumerate(CASES)]
    entries, hosts, around = [b[0] for b in built], [b[1] for b in built], [b[2] for b in built]
    batch = _launch(entries, [case[3] for case in CASES])
    restated = [_restated(case, host, graphs) for case, host in zip(CASES, hosts)]  # (computed once, shared, never changed)
    return entries, hosts, batch, _results(entries, batch), around, restated


def test_kernels_match_the_fp64_restatement_within_the_derived_bound(table, graphs):
    entries, hosts, batch, got, around, restated = table
    misses, worst = [], {}
    for i, (case, g_, r) in enumerate(zip(CASES, got, restated)):
        rowptr, t_rowptr = graphs[case[0]][3][0], graphs[case[0]][4][0]
        k_factor = ref.bound_factor(r["pre"], rowptr, t_rowptr, case[2])
        for k in OUTPUTS:
            if r[k].size == 0:
                continue
            bound = k_factor * U * r[k + "_abs"]
            err = np.abs(g_[k].astype(np.float64) - r[k])
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = float(np.nanmax(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))))
            worst[k] = max(worst.get(k, 0.0), ratio)
            print(f"job {i} {case} {k}: K {k_factor:.0f} largest error / bound {ratio:.4f}")
            if not (err <= bound).all():
                misses.append(f"job {i} {case} {k}: error / bound {ratio:.3e}")
    print("largest error / bound per output:", {k: round(v, 4) for k, v in worst.items()})
    assert not misses, "\n".join(misses)


def test_rows_beyond_a_job_and_columns_beside_it_are_untouched(table):
    entries, _, _, _, around, _ = table
    for case, e, bufs in zip(CASES, entries, around):
        for k, full in bufs.items():
            assert _canaries_intact(full, e[k]), (case, k)


def test_the_table_covers_both_access_paths(table):
    """jobs whose rows take the 16-byte path (plain and sliced) and jobs that take the scalar path, 256 columns and 99 with an odd
    leading dimension among them"""
    entries = table[0]
    vec = lambda t: t.shape[1] >= 4 and t.data_ptr() % 16 == 0 and (t.stride(0) * 4) % 16 == 0  # noqa: E731
    on_vec = {(c[1] * c[2], c[4]) for c, e in zip(CASES, entries) if all(vec(e[k]) for k in ("h", "out", "d_out", "d_h"))}
    scalar = {(c[1] * c[2], c[4]) for c, e in zip(CASES, entries) if not any(vec(e[k]) for k in ("h", "out", "d_out", "d_h"))}
    assert {(256, "plain"), (256, "wide16"), (64, "plain"), (16, "wide16")} <= on_vec, on_vec
    assert {(99, "slices"), (5, "slices"), (1, "plain"), (7, "plain")} <= scalar, scalar
    assert entries[8]["h"].stride(0) % 2 == 1  # (3, 33): an odd leading dimension


def test_a_second_launch_repeats_every_bit(table):
    entries, _, batch, got, _, _ = table
    for e in entries:  # (what the launches write is cleared first: a stale value would not pass for a repeated one)
        for k in ("out", "d_h", "d_s"):
            e[k].fill_(5.0)
    batch.alpha.fill_(5.0)
    batch.launch()
    batch.launch_backward()
    torch.cuda.synchronize()
    for case, a, b in zip(CASES, got, _results(entries, batch)):
        for k in a:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (case, k)


def test_a_job_alone_answers_what_it_answers_in_the_table(table, graphs):
    got = table[3]
    for i, case in enumerate(CASES):
        e, _, _ = _entry(case, 20 + i, graphs)
        res = _results([e], _launch([e], case[3]))[0]
        for k in got[i]:
            assert np.array_equal(got[i][k].view(np.uint32), res[k].view(np.uint32)), (case, k)


def test_a_head_has_the_bits_of_a_one_head_job_on_its_slices(table):
    """H, d_out and the outputs' columns of head h are passed IN PLACE (slices with the job's leading dimension); the head's two
    score columns are copied side by side"""
    entries, _, _, got, _, _ = table
    seen = 0
    for i, case in enumerate(CASES):
        heads, w = case[1], case[2]
        if heads == 1 or case[5] != 4:
            continue
        e = entries[i]
        for h in {0, heads - 1, heads // 2}:
            sl = slice(h * w, (h + 1) * w)
            s1 = torch.stack([e["s"][:, h], e["s"][:, heads + h]], 1).contiguous()
            one = dict(graph=e["graph"], graph_t=e["graph_t"], t_pos=e["t_pos"], heads=1, h=e["h"][:, sl], s=s1, d_out=e["d_out"][:, sl],
                       out=torch.zeros_like(e["out"][:, sl]), d_h=torch.zeros_like(e["d_h"][:, sl]), d_s=torch.zeros_like(s1))
            res = _results([one], _launch([one], case[3]))[0]
            bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
            assert np.array_equal(bits(res["out"]), bits(got[i]["out"][:, sl])), (case, h)
            assert np.array_equal(bits(res["alpha"][:, 0]), bits(got[i]["alpha"][:, h])), (case, h)
            assert np.array_equal(bits(res["d_h"]), bits(got[i]["d_h"][:, sl])), (case, h)
            assert np.array_equal(bits(res["d_s"]), bits(got[i]["d_s"][:, [h, heads + h]])), (case, h)
            seen += 1
    assert seen >= 10


def test_alpha_is_a_distribution_over_every_row(table, graphs):
    got = table[3]
    for case, g_ in zip(CASES, got):
        rowptr = graphs[case[0]][3][0]
        rows, deg = ref.entry_rows(rowptr), np.diff(rowptr)
        assert (g_["alpha"] >= 0).all(), case
        sums = np.zeros((len(deg), case[1]))
        np.add.at(sums, rows, g_["alpha"].astype(np.float64))
        d = int(deg.max(initial=0))
        assert (np.abs(sums[deg > 0] - 1.0) <= (d + 2) * U).all(), (case, np.abs(sums[deg > 0] - 1.0).max())
        assert not sums[deg == 0].any()


def test_zero_scores_give_one_over_the_degree_bit_for_bit(graphs):
    g, gt, t_pos, (rowptr, col), _ = graphs["p140"]
    n, heads, w = g.n_rows, 3, 5
    z = lambda *shape: torch.zeros(shape, device="cuda")  # noqa: E731
    e = dict(graph=g, heads=heads, h=torch.randn(n, heads * w, device="cuda"), s=z(n, 2 * heads), out=z(n, heads * w))
    batch = _launch_forward([e], 0.2)
    deg = np.diff(rowptr)
    want = (np.float32(1.0) / deg[ref.entry_rows(rowptr)].astype(np.float32)).astype(np.float32)
    alpha = batch.alpha_of[0].cpu().numpy()
    for h in range(heads):
        assert np.array_equal(alpha[:, h].view(np.uint32), want.view(np.uint32))


def _launch_forward(entries, slope):
    from wdg_amd import ops
    batch = ops.GatBatch(entries, slope)
    batch.launch()
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="without gradient"):
        batch.launch_backward()
    return batch


def test_the_empty_row_and_the_unstored_column_give_plus_zero(table):
    """p3: row 0 stores nothing, column 1 is stored by nobody"""
    got = table[3]
    for case, g_ in zip(CASES, got):
        if case[0] != "p3":
            continue
        heads = case[1]
        for a in (g_["out"][0], g_["d_s"][0, :heads], g_["d_h"][1], g_["d_s"][1, heads:]):
            assert not a.view(np.uint32).any(), case  # every bit zero: +0


def test_a_nan_reaches_exactly_the_rows_that_store_it(graphs):
    """forward: a NaN in row j of H -> out[i, :] of exactly the rows i that store j; backward: a NaN in d_out[i, :] -> d_H[j, :] of
    exactly the columns j that row i stores"""
    case = ("p140", 2, 8, 0.2, "plain", 4)
    rowptr, col = graphs["p140"][3]
    rows = ref.entry_rows(rowptr)
    e, _, _ = _entry(case, 91, graphs)
    j = 33
    e["h"][j, 3] = float("nan")
    _launch([e], 0.2)
    bad = torch.isnan(e["out"]).any(1).cpu().numpy()
    assert np.array_equal(np.flatnonzero(bad), np.unique(rows[col == j])) and bad.any() and not bad.all()
    assert not torch.isnan(e["out"][:, 8:]).any()  # (the other head's columns hold no NaN)
    e, _, _ = _entry(case, 92, graphs)
    i = 3
    e["d_out"][i, 12] = float("nan")
    _launch([e], 0.2)
    bad = torch.isnan(e["d_h"]).any(1).cpu().numpy()
    assert np.array_equal(np.flatnonzero(bad), col[rowptr[i]:rowptr[i + 1]]) and not bad.all()
    assert not torch.isnan(e["out"]).any()


def test_transpose_positions_equal_the_host_restatement(graphs):
    for name, (g, gt, t_pos, _, (t_rowptr, t_col, want)) in graphs.items():
        assert np.array_equal(gt.rowptr.cpu().numpy(), t_rowptr) and np.array_equal(gt.col.cpu().numpy(), t_col), name
        assert np.array_equal(t_pos.cpu().numpy(), want), name
    assert not np.array_equal(graphs["p140"][2].cpu().numpy(), np.arange(graphs["p140"][0].nnz))  # directed: not the identity


def test_transpose_positions_refuse_a_repeated_entry():
    from wdg_amd import ops
    src, dst = np.array([0, 0, 1, 2, 2]), np.array([1, 1, 2, 0, 1])  # (0, 1) twice
    g = ops.CsrGraph.from_coo(src, dst, 3, None, ops.COO_KEEP_DUPLICATES)
    assert g.nnz == 5
    gt = ops.CsrGraph.from_coo(dst, src, 3, None, ops.COO_KEEP_DUPLICATES)
    with pytest.raises(ValueError, match="strictly ascending"):
        g.transpose_positions(gt)
    with pytest.raises(ValueError):
        g.transpose_positions(g.transpose())  # (the coalesced transpose has fewer entries)


def test_binding_refuses_on_the_device_what_the_kernel_does_not_take(graphs):
    from wdg_amd import ops
    e, _, _ = _entry(("p3", 2, 4, 0.2, "plain", 4), 1, graphs)
    with pytest.raises(ValueError, match="contiguous"):
        ops.GatBatch([dict(e, h=torch.zeros((8, 3), device="cuda").t())])
    with pytest.raises(ValueError, match="overlap"):
        ops.GatBatch([dict(e, d_h=e["d_out"])])
    with pytest.raises(ValueError, match="device"):
        ops.GatBatch([dict(e, s=torch.zeros(3, 4))])
    with pytest.raises(ValueError, match="t_pos"):
        ops.GatBatch([dict(e, t_pos=e["t_pos"][:-1])])
    empty = ops.GatBatch([])
    empty.launch()
    empty.launch_backward()
