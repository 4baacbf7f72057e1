"""tests/_poly_filter_ref.py against itself, without a device: the fp64 restatement of the polynomial graph filter equals the dense fp64
matrix polynomial; the BACKWARD FORMULATION the models use - the same filter on the transposed pattern with the two scales swapped,
v = d_out and u = H0: out is d_H0, dots are d_gamma - equals torch autograd on the dense fp64 model, on a DIRECTED pattern with both
scales; the exact-order dot products agree with the plain ones; the bound factors count what the docstring states; and
models.ppr_coefficients sums to 1."""
import numpy as np
import pytest
import torch

import _poly_filter_ref as ref
from test_gat_ref import _pattern


def _inputs(n, cols, n_seg, order, seed):
    rng = np.random.default_rng(seed)
    gamma = rng.standard_normal((order + 1, n_seg))
    gamma[order // 2] = 0.0                                           # mixed signs, a zero among them
    return dict(v=rng.standard_normal((n, cols)), u=rng.standard_normal((n, cols)), gamma=gamma, r=rng.uniform(0.2, 1.0, n), c=rng.uniform(0.2, 1.0, n))


close = lambda a, b: np.abs(a - b).max(initial=0.0) <= 1e-10 * max(np.abs(b).max(initial=0.0), 1e-300)  # noqa: E731


@pytest.mark.parametrize("cols,seg_cols,order,scales", [(7, 7, 10, "both"), (12, 4, 3, "row"), (10, 5, 2, "none"), (8, 1, 1, "both"), (5, 5, 0, "both"),
                                                        (7, 7, 4, "both+val"), (6, 3, 3, "val")])
def test_restatement_equals_the_dense_matrix_polynomial(cols, seg_cols, order, scales):
    n = 40
    rowptr, col = _pattern(n)
    x = _inputs(n, cols, cols // seg_cols, order, 100 * cols + order)
    r = x["r"] if scales in ("both", "row", "both+val") else None
    c = x["c"] if scales in ("both", "both+val") else None
    val = np.random.default_rng(9).uniform(0.5, 2.0, len(col)) if "val" in scales else None
    got = ref.forward(rowptr, col, x["v"], x["gamma"], seg_cols, r, c, x["u"], val)
    a = ref.dense(rowptr, col, r, c, val)
    assert not np.array_equal(a, a.T)                                 # directed
    per_col = np.repeat(x["gamma"], seg_cols, axis=1)
    want, want_dots, power = np.zeros((n, cols)), [], np.eye(n)
    for k in range(order + 1):
        want += per_col[k] * (power @ x["v"])
        want_dots.append(((power @ x["v"]) * x["u"]).sum(0).reshape(-1, seg_cols).sum(1))
        power = a @ power
    assert close(got["out"], want) and close(got["dots"], np.stack(want_dots))
    assert (got["out_abs"] >= np.abs(got["out"]) * (1 - 1e-12)).all() and (got["dots_abs"] >= np.abs(got["dots"]) * (1 - 1e-12)).all()
    if order == 0:
        assert np.array_equal(got["out"], per_col[0] * x["v"])


def test_backward_formulation_equals_dense_autograd_on_a_directed_pattern():
    n, cols, order = 40, 7, 6
    rowptr, col = _pattern(n)
    t_rowptr, t_col, _ = ref.transposed(rowptr, col)
    x = _inputs(n, cols, 1, order, 5)
    g = np.random.default_rng(6).standard_normal((n, cols))
    a = torch.from_numpy(ref.dense(rowptr, col, x["r"], x["c"]))
    h0, gamma = torch.from_numpy(x["v"]).requires_grad_(), torch.from_numpy(x["gamma"][:, 0]).requires_grad_()
    t, out = h0, gamma[0] * h0
    for k in range(1, order + 1):
        t = a @ t
        out = out + gamma[k] * t
    out.backward(torch.from_numpy(g))
    # (R A C)^T = C A^T R: the transposed pattern, row_scale = c, col_scale = r; v = d_out, u = H0
    bwd = ref.forward(t_rowptr, t_col, g, x["gamma"], cols, x["c"], x["r"], x["v"])
    assert close(bwd["out"], h0.grad.numpy()) and close(bwd["dots"][:, 0], gamma.grad.numpy())
    fwd = ref.forward(rowptr, col, x["v"], x["gamma"], cols, x["r"], x["c"])
    assert close(fwd["out"], out.detach().numpy())


def test_exact_order_dots_agree_with_the_plain_ones_and_are_fp32():
    n, cols, seg_cols, order = 70, 10, 5, 3                           # 70 rows: two whole blocks of 32 and one of 6
    rowptr, col = _pattern(40)
    rng = np.random.default_rng(3)
    t = [rng.standard_normal((n, cols)).astype(np.float32) for _ in range(order + 1)]
    u = rng.standard_normal((n, cols)).astype(np.float32)
    got = ref.dots_bits(t, u, seg_cols)
    assert got.dtype == np.float32 and got.shape == (order + 1, 2)
    want = np.stack([(tk.astype(np.float64) * u).sum(0).reshape(2, seg_cols).sum(1) for tk in t])
    assert np.abs(got - want).max() <= 2.0 ** -23 * np.abs(want).max()
    assert np.array_equal(ref.dots_bits([np.zeros((n, cols), np.float32)], u, seg_cols).view(np.uint32), np.zeros((1, 2), np.uint32))  # +0


def test_the_bound_factors_count_what_the_docstring_states():
    assert [ref.row_roundings(d) for d in (0, 1, 8, 9, 128, 129, 1900)] == [3, 4, 5, 6, 35, 10, 37]
    rowptr = np.array([0, 1, 10, 10, 139])                            # rows of 1, 9, 0 and 129 entries
    ks = ref.bound_factors(rowptr, 10)
    assert ks["r"] == 10 and ks["out"] == 102.0 and ks["dots"].tolist() == [10.0 * k + 2 for k in range(11)]
    assert ref.bound_factors(rowptr, 10, weighted=True)["r"] == 11 and ref.bound_factors(np.array([0]), 3)["r"] == 1 and (ref.TEAM, ref.LONG_ROW, ref.DOT_ROWS) == (4, 128, 32)


@pytest.mark.parametrize("K,alpha", [(0, 0.1), (1, 0.5), (10, 0.1), (10, 0.9), (64, 0.05), (5, 0.0), (5, 1.0)])
def test_ppr_coefficients_sum_to_one(K, alpha):
    from wdg_amd import models
    g = models.ppr_coefficients(K, alpha)
    assert g.dtype == torch.float32 and tuple(g.shape) == (K + 1,)
    assert abs(float(g.double().sum()) - 1.0) <= (K + 1) * 2.0 ** -24
    want = [alpha * (1 - alpha) ** k for k in range(K)] + [(1 - alpha) ** K]
    assert np.allclose(g.numpy(), want, rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        models.ppr_coefficients(-1, 0.1)
    with pytest.raises(ValueError):
        models.ppr_coefficients(3, 1.5)
