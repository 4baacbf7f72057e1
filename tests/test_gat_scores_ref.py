"""The numpy restatement of the attention scores (tests/_gat_scores_ref.py) checked on the CPU: its fp64 form against H @ blockdiag and
torch's fp64 autograd, its fp32 form - the bits the GPU test demands of csrc/gat_scores.hip - against the fp64 form within a derived bound.

The bound of an fp32 element against its fp64 value: (k + 2) 2^-24 * the companion sum of the absolute values of its terms, k the number
of roundings on the way to the element in the order include/wdg.h states (a chain of k operations with one rounding each is within
gamma_k = k u / (1 - k u) of the exact sum's companion; the + 2 covers 1 / (1 - k u) for every k used here and the fp64 side's own error):
    S[i, dst(g) | src(g)]   k = w                       one fma per column of the group
    d_H[i, c]               k = 2                       two fmas
    d_att[p, g, k]          k = min(n, 32) + ceil(n / 32)   the fma chain of a block of 32 rows, then one addition per block"""
import numpy as np
import pytest
import torch

import _gat_scores_ref as ref

SHAPES = [(1, 1, 1, 1), (3, 3, 1, 5), (65, 10, 8, 8), (65, 16, 8, 7), (40, 6, 2, 33), (70, 4, 4, 64), (33, 3, 8, 256)]  # (n, G, heads, w)


def _inputs(n, G, w, seed=0):
    rng = np.random.default_rng(seed + 1000 * n + 10 * G + w)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    return f(n, G * w), f(2, G, w), f(n, 2 * G), f(n, G * w)


def test_score_columns_are_the_blocks_a_gat_job_reads():
    dst, src = ref.score_columns(10, 8)  # the ragged last block: 8 + 2 groups
    assert dst.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 16, 17] and src.tolist() == [8, 9, 10, 11, 12, 13, 14, 15, 18, 19]
    dst, src = ref.score_columns(6, 2)
    assert dst.tolist() == [0, 1, 4, 5, 8, 9] and src.tolist() == [2, 3, 6, 7, 10, 11]
    for G, heads in ((10, 8), (16, 8), (3, 1), (7, 3)):
        dst, src = ref.score_columns(G, heads)
        assert sorted(dst.tolist() + src.tolist()) == list(range(2 * G))  # a permutation of the 2 G columns


@pytest.mark.parametrize("n,G,heads,w", SHAPES)
def test_fp64_restatement_is_the_dense_product_and_its_autograd(n, G, heads, w):
    h, att, d_s, d_h = _inputs(n, G, w)
    s, _ = ref.forward64(h, att, heads)
    dense = h.astype(np.float64) @ ref.operand(att.astype(np.float64), heads)
    assert np.abs(s - dense).max() <= 1e-10
    ht, at = torch.tensor(h, dtype=torch.float64, requires_grad=True), torch.tensor(att, dtype=torch.float64, requires_grad=True)
    dst, src = ref.score_columns(G, heads)
    rows = torch.arange(G * w).repeat(2)
    cols = torch.cat([torch.as_tensor(dst).repeat_interleave(w), torch.as_tensor(src).repeat_interleave(w)])
    op = torch.zeros((G * w, 2 * G), dtype=torch.float64).index_put((rows, cols), at.reshape(-1))
    assert np.abs(op.detach().numpy() - ref.operand(att.astype(np.float64), heads)).max() == 0
    (ht @ op).backward(torch.tensor(d_s, dtype=torch.float64))
    g_h, g_att, _, _ = ref.backward64(h, att, heads, d_s, d_h)
    assert np.abs(g_h - (d_h.astype(np.float64) + ht.grad.numpy())).max() <= 1e-10
    assert np.abs(g_att - at.grad.numpy()).max() <= 1e-10


@pytest.mark.parametrize("n,G,heads,w", SHAPES)
def test_fp32_restatement_stays_within_the_derived_bound(n, G, heads, w):
    h, att, d_s, d_h = _inputs(n, G, w)
    k_s, k_h, k_att = ref.roundings(n, w)
    s64, s_abs = ref.forward64(h, att, heads)
    g_h64, g_att64, g_h_abs, g_att_abs = ref.backward64(h, att, heads, d_s, d_h)
    s32 = ref.forward32(h, att, heads)
    g_h32, g_att32, partial = ref.backward32(h, att, heads, d_s, d_h)
    assert s32.dtype == g_h32.dtype == g_att32.dtype == np.float32 and partial.shape == (-(-n // ref.ROW_BLOCK), 2, G, w)
    assert (np.abs(s32 - s64) <= (k_s + 2) * ref.U * s_abs).all()
    assert (np.abs(g_h32 - g_h64) <= (k_h + 2) * ref.U * g_h_abs).all()
    assert (np.abs(g_att32 - g_att64) <= (k_att + 2) * ref.U * g_att_abs).all()


def test_fp32_restatement_special_cases():
    h, att, d_s, d_h = _inputs(5, 3, 4)
    unit = np.zeros_like(att)
    unit[0, :, 2] = 1.0  # a_dst = e_2: the dst score IS column 2 of the group
    dst, _ = ref.score_columns(3, 2)
    assert (ref.forward32(h, unit, 2)[:, dst] == h.reshape(5, 3, 4)[:, :, 2]).all()
    g_h, g_att, _ = ref.backward32(h, np.zeros_like(att), 2, d_s, d_h)
    assert (g_h == d_h).all()  # att = 0: d_h passes through
    e = np.zeros((0, 12), np.float32)
    g_h, g_att, partial = ref.backward32(e, att, 2, np.zeros((0, 6), np.float32), e)
    assert g_h.shape == (0, 12) and partial.shape[0] == 0 and (g_att == 0).all()
