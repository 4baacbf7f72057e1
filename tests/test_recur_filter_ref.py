"""tests/_recur_filter_ref.py and models.recurrence_table without a device: the basis tables against scipy.special; the fp32 restatement
(forward32: the header's arithmetic, operation by operation) against the fp64 one under the DERIVED bound on the pattern that has both
routes of a row - a team of 4 lanes and a wave - at orders 10 and 24; the monomial table in fp64 against _poly_filter_ref.forward; the
backward formulation the models use against torch autograd on a dense fp64 model; and ChebNetII's interpolation map."""
import numpy as np
import pytest
import torch

import _poly_filter_ref as pref
import _recur_filter_ref as ref
from test_gat_ref import _pattern
from test_gpu_poly_filter import _plong

U = 2.0 ** -24
X33 = np.linspace(-1.0, 1.0, 33)


def _polynomials(table, x):
    """[p_0(x) .. p_K(x)] of a recurrence table in the scalar variable the table's `A_hat` stands for"""
    p = [np.ones_like(x)]
    for k, (a, b, c) in enumerate(table):
        p.append(a * x * p[k] + b * p[k] + (c * p[k - 1] if k else 0.0))
    return p


@pytest.mark.parametrize("alpha,beta", [(1.0, 1.0), (0.5, -0.3), (0.0, 0.0)])
def test_jacobi_and_legendre_tables_against_scipy(alpha, beta):
    from scipy import special
    from wdg_amd import models
    K = 12
    tab = models.recurrence_table("jacobi", K, alpha, beta)
    assert tab.dtype == np.float64 and tab.shape == (K, 3) and tab[0, 2] == 0.0
    for k, p in enumerate(_polynomials(tab, X33)):
        assert np.abs(p - special.eval_jacobi(k, alpha, beta, X33)).max() <= 1e-12 * max(1.0, np.abs(p).max()), k
    if alpha == beta == 0.0:
        assert np.array_equal(tab, models.recurrence_table("legendre", K, 7.0, 7.0))     # (the arguments are not read)
        for k, p in enumerate(_polynomials(tab, X33)):
            assert np.abs(p - special.eval_legendre(k, X33)).max() <= 1e-12, k


def test_chebyshev_and_monomial_tables():
    from scipy import special
    from wdg_amd import models
    K = 12
    tab = models.recurrence_table("chebyshev", K)
    assert tab[0].tolist() == [-1.0, 0.0, 0.0] and all(row.tolist() == [-2.0, 0.0, -1.0] for row in tab[1:])
    for k, p in enumerate(_polynomials(tab, -X33)):                   # the table's variable is A_hat = -x
        assert np.abs(p - special.eval_chebyt(k, X33)).max() <= 1e-12, k
    assert np.array_equal(models.recurrence_table("monomial", 3), [[1.0, 0.0, 0.0]] * 3)
    assert models.recurrence_table("chebyshev", 0).shape == (0, 3) and models.recurrence_table("jacobi", 1).shape == (1, 3)
    for bad in (("bernstein", 3), ("jacobi", -1), ("jacobi", 3, -1.0, 0.0), ("jacobi", 3, 0.0, -1.5)):
        with pytest.raises(ValueError):
            models.recurrence_table(*bad)


def _ratio(err, bound):
    """the largest error / bound; where the bound is 0 - a companion of 0: an element no term reaches - the error must be 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)), initial=0.0))


def _tables(order, rng):
    from wdg_amd import models
    return {"chebyshev": models.recurrence_table("chebyshev", order), "jacobi11": models.recurrence_table("jacobi", order, 1.0, 1.0),
            "random": ref.random_sign_table(rng, order)}


@pytest.mark.parametrize("order", [10, 24])
def test_forward32_matches_forward64_within_the_derived_bound(order):
    """both routes of a row (127 / 128 entries: a team; 129 / 300: a wave), both scales, stored values"""
    rowptr, col = _plong()
    n, cols, seg_cols = len(rowptr) - 1, 6, 3
    rng = np.random.default_rng(order)
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    x = dict(v=f32(rng.standard_normal((n, cols))), rs=f32(rng.uniform(0.5, 1.5, n) / np.maximum(np.diff(rowptr), 1)), cs=f32(rng.uniform(0.5, 1.5, n)),
             val=f32(rng.uniform(0.5, 2.0, len(col))), u=f32(rng.standard_normal((n, cols))))
    gamma = f32(rng.uniform(0.3, 1.0, (order + 1, 2)) * rng.choice([-1.0, 1.0], (order + 1, 2)))
    ks = ref.bound_factors(rowptr, order, weighted=True)
    assert ks["r"] == pref.row_roundings(128) + 1 == 36 and ks["m"] == 37 and ks["out"] == order * 37 + 2.0
    d = lambda a: a.astype(np.float64)  # noqa: E731
    for name, table in _tables(order, rng).items():
        recur = f32(table)
        got = ref.forward32(rowptr, col, x["v"], gamma, recur, seg_cols, x["rs"], x["cs"], x["val"])
        want = ref.forward64(rowptr, col, d(x["v"]), d(gamma), d(recur), seg_cols, d(x["rs"]), d(x["cs"]), d(x["u"]), d(x["val"]))
        worst_t = max(_ratio(np.abs(d(got["t"][k]) - want["t"][k]), ks["t"][k] * U * want["t_abs"][k]) for k in range(order + 1))
        worst_out = _ratio(np.abs(d(got["out"]) - want["out"]), ks["out"] * U * want["out_abs"])
        dots = ref.dots_bits(got["t"], x["u"], seg_cols)
        worst_dots = _ratio(np.abs(d(dots) - want["dots"]), ks["dots"][:, None] * U * want["dots_abs"])
        print(f"order {order} {name}: largest error / bound T_k {worst_t:.4f} out {worst_out:.4f} dots {worst_dots:.4f}")
        assert 0 < worst_t <= 1.0 and 0 < worst_out <= 1.0 and worst_dots <= 1.0, name
        assert np.array_equal(got["t"][0], x["v"]) and (want["out_abs"] >= np.abs(want["out"]) * (1 - 1e-12)).all()


def test_the_monomial_table_in_fp64_is_the_polynomial_filter():
    from wdg_amd import models
    n, cols, seg_cols, order = 40, 6, 3, 7
    rowptr, col = _pattern(n)
    rng = np.random.default_rng(2)
    v, u, gamma = rng.standard_normal((n, cols)), rng.standard_normal((n, cols)), rng.standard_normal((order + 1, 2))
    rs, cs, val = rng.uniform(0.2, 1.0, n), rng.uniform(0.2, 1.0, n), rng.uniform(0.5, 2.0, len(col))
    got = ref.forward64(rowptr, col, v, gamma, models.recurrence_table("monomial", order), seg_cols, rs, cs, u, val)
    want = pref.forward(rowptr, col, v, gamma, seg_cols, rs, cs, u, val)
    for k in ("out", "out_abs", "dots", "dots_abs"):
        assert np.array_equal(got[k], want[k]), k
    assert all(np.array_equal(a, b) for a, b in zip(got["t"] + got["t_abs"], want["t"] + want["t_abs"]))


def test_the_fp32_restatement_of_the_monomial_table_equals_the_plain_hops_where_sums_are_exact():
    """small integers: every sum is exact in fp32, so forward32 with (1, 0, 0) must give the integer A^k v - the chains, the butterfly
    and the recurrence lose no entry and count none twice (rows of 0 .. 300 entries)"""
    from wdg_amd import models
    rowptr, col = _plong()
    n = len(rowptr) - 1
    v = np.random.default_rng(4).integers(-3, 4, (n, 2)).astype(np.float32)
    gamma = np.array([[1.0], [2.0], [-1.0]], np.float32)
    got = ref.forward32(rowptr, col, v, gamma, models.recurrence_table("monomial", 2).astype(np.float32))
    want = pref.forward(rowptr, col, v.astype(np.float64), gamma.astype(np.float64))
    assert np.array_equal(got["out"].astype(np.float64), want["out"]) and np.abs(want["out"]).max() < 2 ** 24


@pytest.mark.parametrize("basis,per_channel", [("chebyshev", False), ("jacobi", True), ("jacobi", False)])
def test_backward_formulation_equals_dense_autograd_on_a_directed_pattern(basis, per_channel):
    """T_k = p_k(A_hat) v, so d_v = sum_k gamma_k p_k(A_hat^T) d_out and d_gamma_k = <p_k(A_hat^T) d_out, v>: the same filter with the
    same table on the transposed pattern with the scales swapped, v = d_out, u = H0"""
    from wdg_amd import models
    n, cols, order = 40, 6, 6
    rowptr, col = _pattern(n)
    t_rowptr, t_col, _ = pref.transposed(rowptr, col)
    rng = np.random.default_rng(5)
    table = models.recurrence_table(basis, order, 0.5, -0.3)
    n_seg = cols if per_channel else 1
    v, g, gam, rs, cs = rng.standard_normal((n, cols)), rng.standard_normal((n, cols)), rng.standard_normal((order + 1, n_seg)), rng.uniform(0.2, 1.0, n), rng.uniform(0.2, 1.0, n)
    a = torch.from_numpy(pref.dense(rowptr, col, rs, cs))
    assert not torch.equal(a != 0, (a != 0).t())
    h0, gamma = torch.from_numpy(v).requires_grad_(), torch.from_numpy(gam).requires_grad_()
    t, out = [h0], gamma[0] * h0
    for k, (ca, cb, cc) in enumerate(table):
        t.append(ca * (a @ t[k]) + cb * t[k] + (cc * t[k - 1] if k else 0.0))
        out = out + gamma[k + 1] * t[k + 1]
    out.backward(torch.from_numpy(g))
    close = lambda x, y: np.abs(x - y).max() <= 1e-10 * np.abs(y).max()  # noqa: E731
    fwd = ref.forward64(rowptr, col, v, gam, table, cols // n_seg, rs, cs)
    bwd = ref.forward64(t_rowptr, t_col, g, gam, table, cols // n_seg, cs, rs, v)   # (R A C)^T = C A^T R
    assert close(fwd["out"], out.detach().numpy()) and close(bwd["out"], h0.grad.numpy()) and close(bwd["dots"], gamma.grad.numpy())


def test_chebnet2_interpolation_map_recovers_a_polynomial_filter():
    """theta_j = h(x_j) for a non-negative polynomial h of degree <= K: filter_response IS h (Chebyshev interpolation is exact there);
    theta = 1, the start, is the identity filter; a negative theta_j is clipped by the ReLU"""
    from wdg_amd import models
    K = 10
    nodes = models.chebyshev_nodes(K)
    m = models.chebyshev_interpolation_map(K)
    assert m.dtype == np.float64 and m.shape == (K + 1, K + 1)
    assert np.abs(np.polynomial.chebyshev.chebval(nodes, m @ np.arange(1.0, K + 2)) - np.arange(1.0, K + 2)).max() <= 1e-12   # it interpolates
    model = models.ChebNetII2(5, 3, nhid=4, order=K).double()
    assert list(dict(model.named_parameters())) == ["w0", "w1", "theta"] and torch.equal(model.theta, torch.ones(K + 1, dtype=torch.float64))
    start = model.filter_coefficients()
    assert start.shape == (K + 1,) and abs(start[0] - 1.0) <= 1e-6 and np.abs(start[1:]).max() <= 1e-6       # gamma = e_0
    assert np.abs(model.filter_response(X33) - 1.0).max() <= 1e-12
    coeffs = np.random.default_rng(7).standard_normal(K + 1)
    h = lambda x: np.polynomial.polynomial.polyval(x, coeffs[:K // 2 + 1]) ** 2 + 0.25  # noqa: E731
    assert (h(nodes) > 0).all()                                       # a square plus a constant: degree 2 (K / 2) <= K, non-negative
    with torch.no_grad():
        model.theta.copy_(torch.from_numpy(h(nodes)))
    assert np.abs(model.filter_response(X33) - h(X33)).max() <= 1e-12 * max(1.0, np.abs(h(X33)).max())
    with torch.no_grad():
        model.theta[3] = -2.0
    clipped = h(nodes)
    clipped[3] = 0.0
    assert np.abs(model.filter_response(nodes) - clipped).max() <= 1e-12 * max(1.0, clipped.max())
    # (the coefficients the forward pass uses go through the map as an fp32 buffer: K + 1 terms, each entry rounded to fp32 once)
    assert np.abs(model.filter_coefficients() - m @ clipped).max() <= (K + 1) * U * np.abs(m).max() * clipped.max()


def test_model_shapes_and_parameter_order():
    from wdg_amd import models
    torch.manual_seed(3)
    a = models.JacobiConv1(5, 3, order=4)
    torch.manual_seed(3)
    assert torch.equal(a.weight, models._xavier(5, 3))
    assert [k for k, _ in a.named_parameters()] == ["weight", "gamma"] and tuple(a.gamma.shape) == (5, 3)
    assert all(torch.equal(a.gamma[:, c], models.ppr_coefficients(4, 0.1)) for c in range(3))
    b = models.JacobiConv2(5, 3, nhid=4, order=4, per_channel=False, ppr_alpha=0.3)
    assert [k for k, _ in b.named_parameters()] == ["w0", "w1", "gamma"] and torch.equal(b.gamma[:, 0], models.ppr_coefficients(4, 0.3))
    assert b.filter_coefficients().shape == (5, 1) and a.filter_coefficients().shape == (5, 3)
    assert [k for k, _ in models.ChebNetII1(5, 3).named_parameters()] == ["weight", "theta"]
    assert np.array_equal(a._filter.recur, models.recurrence_table("jacobi", 4, 1.0, 1.0)) and a._filter.per_channel and not b._filter.per_channel
    with pytest.raises(ValueError, match="order 65"):
        models.ChebNetII1(5, 3, order=65)
    assert a._filter.is_fused(20448) and not a._filter.is_fused(20449) and not models.JacobiConv1(5, 3, fused=False)._filter.is_fused(10)
