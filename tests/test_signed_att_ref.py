"""tests/_signed_att_ref.py against itself, without a device: the fp64 restatement of the signed-attention layer equals a dense
composition in torch fp64 - its backward pass equals that composition's autograd - on a directed 40-node pattern with an empty row, with
both scales, one and none, with a residual and without; and its fp32 form (the same numpy code on fp32 inputs) lies within the derived
bound of its fp64 form, T measured for numpy's fp32 tanh the way the GPU test measures the device's."""
import numpy as np
import pytest
import torch

import _signed_att_ref as ref
from test_gat_ref import _pattern

U = 2.0 ** -24


def _inputs(n, heads, w, seed, smax=4.0):
    rng = np.random.default_rng(seed)
    return dict(h=rng.standard_normal((n, heads * w)), s=rng.uniform(-smax, smax, (n, 2 * heads)), g=rng.standard_normal((n, heads * w)),
                res=rng.standard_normal((n, heads * w)), r=rng.uniform(0.2, 1.0, n), c=rng.uniform(0.2, 1.0, n))


@pytest.mark.parametrize("heads,w,scales,residual", [(1, 7, "both", True), (2, 8, "row", False), (3, 5, "none", True), (8, 4, "both", False)])
def test_restatement_equals_dense_autograd(heads, w, scales, residual):
    n, eps = 40, 0.3
    rowptr, col = _pattern(n)
    x = _inputs(n, heads, w, heads * 100 + w)
    r = x["r"] if scales in ("both", "row") else None
    c = x["c"] if scales == "both" else None
    res = x["res"] if residual else None
    fwd = ref.forward(rowptr, col, x["h"], x["s"], heads, r, c, res, eps)
    bwd = ref.backward(rowptr, col, x["h"], x["s"], heads, x["g"], r, c)
    mask = torch.zeros((n, n), dtype=torch.bool)
    mask[torch.from_numpy(ref.entry_rows(rowptr)), torch.from_numpy(col.astype(np.int64))] = True
    ht, st = torch.from_numpy(x["h"]).requires_grad_(), torch.from_numpy(x["s"]).requires_grad_()
    tt = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    out, alpha = ref.torch_layer(mask, ht, st, heads, tt(r), tt(c), tt(res), eps)
    out.backward(torch.from_numpy(x["g"]))
    close = lambda a, b: np.abs(a - b).max() <= 1e-10 * max(np.abs(b).max(), 1e-300)  # noqa: E731
    assert close(fwd["out"], out.detach().numpy())
    assert close(fwd["alpha"], alpha.detach().numpy()[ref.entry_rows(rowptr), col])
    assert close(bwd["d_h"], ht.grad.numpy()) and close(bwd["d_s"], st.grad.numpy())
    assert (fwd["alpha"] < 0).any() and (fwd["alpha"] > 0).any()                 # signed weights
    want_empty = eps * res[5] if residual else np.zeros(heads * w)
    assert np.array_equal(fwd["out"][5], want_empty) and not bwd["d_s"][5, :heads].any()   # the empty row
    assert (fwd["out_abs"] >= np.abs(fwd["out"])).all() and (bwd["d_h_abs"] >= np.abs(bwd["d_h"])).all()
    assert (bwd["d_pre_abs"] >= np.abs(bwd["d_pre"])).all() and (bwd["d_s_abs"] >= np.abs(bwd["d_s"]) * (1 - 1e-12)).all()


def test_saturated_scores_have_no_score_gradient():
    """|pre| near 20: tanh is +-1 in fp64 as well (1 - tanh(20) = 8.5e-18 lies below half an ulp of 1), so 1 - t^2 is 0 exactly"""
    n, heads, w = 40, 2, 4
    rowptr, col = _pattern(n)
    x = _inputs(n, heads, w, 9)
    s = np.where(x["s"] > 0, 10.0, -10.0) + x["s"] * 0.01
    s[:, heads:] = np.abs(s[:, heads:]) * np.sign(s[:, :heads])                   # both scores of a row carry its sign ...
    fwd = ref.forward(rowptr, col, x["h"], s, heads)
    same = np.abs(fwd["pre"]) > 19
    assert same.any() and (np.abs(fwd["t"][same]) == 1.0).all()                   # ... so rows of one sign meet at |pre| = 20
    bwd = ref.backward(rowptr, col, x["h"], s, heads, x["g"])
    assert not bwd["d_pre"][same].any() and bwd["d_pre_abs"][same].all()


@pytest.mark.parametrize("heads,w,smax", [(1, 7, 4.0), (2, 8, 4.0), (8, 4, 10.0)])
def test_fp32_form_lies_within_the_derived_bound_of_the_fp64_form(heads, w, smax):
    n, eps = 40, 0.3
    rowptr, col = _pattern(n)
    t_rowptr = ref.transposed(rowptr, col)[0]
    x32 = {k: v.astype(np.float32) for k, v in _inputs(n, heads, w, 7 * heads + w, smax).items()}
    x64 = {k: v.astype(np.float64) for k, v in x32.items()}
    got = ref.forward(rowptr, col, x32["h"], x32["s"], heads, x32["r"], x32["c"], x32["res"], eps)
    got.update(ref.backward(rowptr, col, x32["h"], x32["s"], heads, x32["g"], x32["r"], x32["c"]))
    want = ref.forward(rowptr, col, x64["h"], x64["s"], heads, x64["r"], x64["c"], x64["res"], eps)
    want.update(ref.backward(rowptr, col, x64["h"], x64["s"], heads, x64["g"], x64["r"], x64["c"]))
    assert got["out"].dtype == np.float32 and got["d_s"].dtype == np.float32
    t_ulps = ref.tanh_ulps(got["t"], got["pre"]) + 1.0                            # numpy's fp32 tanh, measured as the device's is
    assert t_ulps <= 5.0, t_ulps
    ks = ref.bound_factors(t_ulps, rowptr, t_rowptr, w, unfused=True)
    for k in ("alpha", "out", "d_h", "d_pre", "d_s"):
        err, bound = np.abs(got[k].astype(np.float64) - want[k]), ks[k] * U * want[k + "_abs"]
        assert (err <= bound).all(), (k, float((err / np.maximum(bound, 1e-300)).max()))
        assert err.max() > 0 or k == "alpha"                                       # (the comparison is not vacuous)


def test_the_bound_factors_count_what_the_docstring_states():
    rowptr, col = _pattern(40)
    t_rowptr = ref.transposed(rowptr, col)[0]
    d_row, d_col = int(np.diff(rowptr).max()), int(np.diff(t_rowptr).max())
    ks = ref.bound_factors(2.0, rowptr, t_rowptr, 7)
    assert ks == dict(alpha=8.0, out=9.0 + d_row, d_h=8.0 + d_col, d_pre=7 + 16.0, d_s=7 + 16.0 + max(d_row, d_col))
    assert ref.tanh_ulps(np.float32([0.5]), np.float32([0.0])) > 1e6 and ref.tanh_ulps(np.tanh(np.float32([0.3, -2.0])), np.float32([0.3, -2.0])) <= 2.0
