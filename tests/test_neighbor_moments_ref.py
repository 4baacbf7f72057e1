"""CPU-only checks of tests/_neighbor_moments_ref.py, the numpy restatement the GPU tests compare csrc/neighbor_moments.hip with: in
fp64 against torch autograd of the mean / sqrt(mean((x - m)^2) + eps) / amax / amin composition on tie-free data, forward and backward;
its extremes against tests/_neighbor_max_ref.py; that the four chains by position are NOT one chain; what the centred second pass buys
over E[x^2] - E[x]^2; skipped entries, duplicates and the duplicate rule of the routed terms."""
import numpy as np
import torch

import _neighbor_max_ref as M
import _neighbor_moments_ref as R

EPS = 1e-5
KEYS = ("mean", "std", "mx", "mn")


def _ragged(rng, lens, n_cols):
    """rowptr, col without duplicates inside a row"""
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    return rowptr, np.concatenate([rng.permutation(n_cols)[:k] for k in lens]).astype(np.int64)


def _transpose(rowptr, col, n_cols):
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    order = np.lexsort((rows, col))
    return np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n_cols))]), rows[order]


def test_the_restatement_equals_torch_autograd_in_fp64():
    rng = np.random.default_rng(0)
    n, m, f = 9, 11, 3
    lens = [0, 1, 2, 3, 5, 7, 4, 9, 6]  # ragged, with an empty row
    rowptr, col = _ragged(rng, lens, m)
    x = rng.standard_normal((m, f))
    out = R.neighbor_moments(rowptr, col, None, x, n, EPS)
    xt = torch.tensor(x, requires_grad=True)
    rows = []
    for i in range(n):
        js = col[rowptr[i]:rowptr[i + 1]]
        if len(js) == 0:
            rows.append(torch.zeros(4 * f, dtype=torch.float64))
            continue
        v = xt[js]
        mu = v.mean(0)
        rows.append(torch.cat([mu, torch.sqrt(((v - mu) ** 2).mean(0) + EPS), v.amax(0), v.amin(0)]))
    agg = torch.stack(rows)
    mine = np.concatenate([out[k] for k in KEYS], 1)
    assert np.abs(agg.detach().numpy() - mine).max() <= 4 * 2.0 ** -52 * np.abs(mine).max()
    assert list(out["cnt"]) == lens and (out["arg_max"][0] == -1).all() and (mine[0] == 0).all()
    g = rng.standard_normal((n, 4 * f))
    (agg * torch.tensor(g)).sum().backward()
    rowptr_t, col_t = _transpose(rowptr, col, m)
    d = R.neighbor_moments_backward(rowptr_t, col_t, None, x, {k: g[:, q * f:(q + 1) * f] for q, k in enumerate(KEYS)}, out, m)
    want = xt.grad.numpy()
    # (a row of one entry has std = sqrt(eps): its gradient carries 1 / sqrt(eps) of a difference that is 0 up to rounding)
    assert np.abs(d - want).max() <= 2.0 ** -40 * np.abs(want).max() and np.abs(want).max() > 0.1


def test_the_extremes_are_the_neighbour_maximums():
    rng = np.random.default_rng(1)
    lens = [0, 1, 4, 5, 17, 9]
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    col = rng.integers(-1, 9, rowptr[-1])  # duplicates, -1 and an index past the 8 columns
    kept = np.asarray([0, 1, 2, 9, 16, 3])
    x = (np.round(rng.standard_normal((8, 5)) * 2) / 2).astype(np.float32)  # ties
    x[2, 1], x[3, 2], x[4, 3], x[5, 3] = np.nan, np.inf, 0.0, -0.0
    for kl in (None, kept):
        out = R.neighbor_moments(rowptr, col, kl, x, 6, EPS)
        for key, arg, minimum in (("mx", "arg_max", False), ("mn", "arg_min", True)):
            y, a = M.neighbor_max(rowptr, col, kl, x, 6, minimum)
            assert np.array_equal(out[key].view(np.uint32), y.view(np.uint32)) and np.array_equal(out[arg], a)
        js = col[rowptr[4]:rowptr[4] + (17 if kl is None else 16)]
        assert out["cnt"][4] == ((js >= 0) & (js < 8)).sum() > len(np.unique(js[(js >= 0) & (js < 8)]))  # copies count per occurrence


def test_four_chains_by_position_are_not_one_chain():
    """the sense of test_neighbor_max_ref.py's non-associativity example: the definition's tree is part of the result"""
    vals = np.asarray([[1.0], [2.0 ** 24], [1.0], [-(2.0 ** 24)]], np.float32)
    four, one = R.chain_sum(vals, np.ones((4, 1), bool)), R.one_chain_sum(vals, np.ones((4, 1), bool))
    assert four[0] == np.float32(1.0) and one[0] == np.float32(0.0)  # (1 + 2^24) + (1 - 2^24) = 2^24 + (1 - 2^24) = 1 against ((1 + 2^24) + 1) - 2^24 = 0
    # a skipped position keeps its place: the chains are by POSITION, not by count
    big = 2.0 ** 24
    skipped = R.chain_sum(np.asarray([[big], [5.0], [1.0], [1.0]], np.float32), np.asarray([[True], [False], [True], [True]]))
    compact = R.chain_sum(np.asarray([[big], [1.0], [1.0]], np.float32), np.ones((3, 1), bool))
    assert skipped[0] == np.float32(big + 2) and compact[0] == np.float32(big)  # big + (1 + 1) against (big + 1) + 1


def test_the_centred_second_pass_keeps_what_the_one_pass_form_loses():
    """the recorded fact of DESIGN 4.37: data shifted by 100 - E[x^2] - E[x]^2 in fp32 is off by some 1e-3, the centred form by some 1e-7"""
    rng = np.random.default_rng(2)
    lens = [3, 5, 8, 13, 21, 34]
    rowptr, col = _ragged(rng, lens, 40)
    x = (rng.standard_normal((40, 4)) + 100.0).astype(np.float32)
    want = R.neighbor_moments(rowptr, col, None, x.astype(np.float64), 6, EPS)["std"]
    two = R.neighbor_moments(rowptr, col, None, x, 6, EPS)["std"]
    one = np.zeros_like(two)
    for i in range(6):
        v = x[col[rowptr[i]:rowptr[i + 1]]]
        ok = np.ones((len(v), 1), bool)
        c = np.float32(len(v))
        ex, ex2 = R.chain_sum(v, ok) / c, R.chain_sum(v * v, ok) / c
        one[i] = np.sqrt(np.maximum(ex2 - ex * ex, np.float32(0)) + np.float32(EPS))
    err_one, err_two = np.abs(one - want).max(), np.abs(two - want).max()
    print("one-pass fp32 std error", err_one, "centred two-pass", err_two)
    assert err_two <= 2.0 ** -20 and err_one >= 2.0 ** -12


def test_the_backward_pass_skips_and_routes_as_stated():
    """entries out of range are skipped in every chain; a repeated entry adds A and B again but routes an extreme's gradient once"""
    x = np.asarray([[2.0], [3.0]], np.float32)
    fwd = dict(mean=np.asarray([[1.0], [4.0], [0.0]], np.float32), std=np.asarray([[2.0], [1.0], [1.0]], np.float32), cnt=np.asarray([2, 1, 0], np.int32),
               arg_max=np.asarray([[0], [0], [-1]], np.int32), arg_min=np.asarray([[1], [0], [-1]], np.int32))
    g = dict(mean=np.asarray([[4.0], [8.0], [5.0]], np.float32), std=np.asarray([[1.0], [2.0], [7.0]], np.float32), mx=np.asarray([[16.0], [32.0], [9.0]], np.float32),
             mn=np.asarray([[64.0], [128.0], [9.0]], np.float32))
    a, b = R.prepare(g["mean"], g["std"], fwd["mean"], fwd["std"], fwd["cnt"])
    assert a.tolist() == [[2.0 - 0.25], [8.0 - 8.0], [0.0]] and b.tolist() == [[0.25], [2.0], [0.0]]  # B = g_std / (c std), A = g_mean / c - B mean; c == 0: +0
    rowptr_t, col_t = np.asarray([0, 6, 8]), np.asarray([0, 0, -1, 3, 1, 2, 0, 1])  # row 0: source 0 twice, -1, 3 (out of range), 1, 2
    d = R.neighbor_moments_backward(rowptr_t, col_t, None, x, g, fwd, 2)
    sa, sb = 1.75 + 1.75 + 0.0 + 0.0, 0.25 + 0.25 + 2.0 + 0.0
    assert d[0, 0] == np.float32(2.0 * sb + (sa + (16.0 + 32.0)) + 128.0)   # arg_max == 0 at sources 0 (once) and 1; arg_min == 0 at source 1
    assert d[1, 0] == np.float32(3.0 * (0.25 + 2.0) + (1.75 + 0.0) + 64.0)  # arg_min == 1 at source 0
    none = R.neighbor_moments_backward(rowptr_t, col_t, None, x, {}, fwd, 2)
    assert not none.any() and not np.signbit(none).any()
