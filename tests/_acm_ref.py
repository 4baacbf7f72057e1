"""The ACM channel mix of include/wdg.h (wdg_acm_mix_batched_f32 and its backward pass) and the two models built on it
(models.ACMSGC1 / ACMGCN2), restated in numpy.  Everything is evaluated in the dtype of the inputs: fp64 arrays give
the reference the kernels are measured against, fp32 arrays the error a fp32 evaluation in another order has (the tolerance of
tests/test_gpu_acm.py is taken from the difference of the two).  tests/test_acm_ref.py pins it against torch autograd in fp64."""
import numpy as np

T = 3


def _act(p, relu):
    return np.where(p <= 0, np.zeros((), p.dtype), p) if relu else p  # (a NaN fails the comparison and stays)


def channels(low, high, high_agg, ident, relu):
    """-> (P [3, rows, cols], H [3, rows, cols])"""
    p = np.stack([low, high if high_agg is None else high - high_agg, ident])
    return p, _act(p, relu)


def mix_forward(low, high, high_agg, ident, att, wmix, relu):
    """-> out [rows, cols], aux [rows, 8] = alpha_L alpha_H alpha_I s_L s_H s_I 0 0"""
    dt = low.dtype
    _, h = channels(low, high, high_agg, ident, relu)
    u = np.einsum("crk,ck->rc", h, att.astype(dt))
    s = (1 / (1 + np.exp(-u))).astype(dt)
    z = (s / dt.type(T)) @ wmix.astype(dt)
    e = np.exp(z - z.max(1, keepdims=True))
    alpha = (e / e.sum(1, keepdims=True)).astype(dt)
    out = dt.type(3) * np.einsum("rc,crk->rk", alpha, h)
    aux = np.zeros((low.shape[0], 8), dt)
    aux[:, :3], aux[:, 3:6] = alpha, s
    return out.astype(dt), aux


def mix_backward(low, high, high_agg, ident, att, wmix, relu, d_out):
    """-> dict(d_low, d_high, d_ident [rows, cols], d_att [3, cols], d_wmix [3, 3]); d(high_agg) = -d_high"""
    dt = low.dtype
    p, h = channels(low, high, high_agg, ident, relu)
    _, aux = mix_forward(low, high, high_agg, ident, att, wmix, relu)
    alpha, s = aux[:, :3], aux[:, 3:6]
    wmix, att = wmix.astype(dt), att.astype(dt)
    dalpha = dt.type(3) * np.einsum("rk,crk->rc", d_out, h)
    dz = alpha * (dalpha - (alpha * dalpha).sum(1, keepdims=True))
    ds = (dz @ wmix.T) / dt.type(T)
    d_wmix = (s / dt.type(T)).T @ dz
    du = ds * s * (1 - s)
    dh = dt.type(3) * alpha.T[:, :, None] * d_out[None] + du.T[:, :, None] * att[:, None, :]
    d_att = np.einsum("rc,crk->ck", du, h)
    dp = np.where(p > 0, dh, np.zeros((), dt)) if relu else dh
    return dict(d_low=dp[0].astype(dt), d_high=dp[1].astype(dt), d_ident=dp[2].astype(dt), d_att=d_att.astype(dt), d_wmix=d_wmix.astype(dt))


# ---------------------------------------------------------------------------------------------------------------- the models
def layer_forward(a_hat, m, w, att, wmix, relu):
    """one ACM layer on a dense A_hat; w = [W_L | W_H | W_I] ([Fin, 3 width]) -> (out, the operands of the mix)"""
    width = w.shape[1] // 3
    mw = m @ w
    ops = dict(low=a_hat @ mw[:, :width], high=mw[:, width:2 * width], high_agg=a_hat @ mw[:, width:2 * width], ident=mw[:, 2 * width:])
    out, _ = mix_forward(ops["low"], ops["high"], ops["high_agg"], ops["ident"], att, wmix, relu)
    return out, ops


def layer_backward(a_hat, m, w, att, wmix, relu, ops, d_out):
    """-> (d_m, d_w, d_att, d_wmix)"""
    g = mix_backward(ops["low"], ops["high"], ops["high_agg"], ops["ident"], att, wmix, relu, d_out)
    d_mw = np.concatenate([a_hat.T @ g["d_low"], g["d_high"] - a_hat.T @ g["d_high"], g["d_ident"]], 1)
    return d_mw @ w.T, m.T @ d_mw, g["d_att"], g["d_wmix"]


def acm_sgc1_forward(a_hat, x, w, att, wmix):
    """ACM-SGC-1: one layer on M = X, width C, no activation -> logits"""
    return layer_forward(a_hat, x, w, att, wmix, False)[0]


def acm_sgc1_backward(a_hat, x, w, att, wmix, d_logits):
    """-> dict(w, att, wmix) of gradients"""
    _, ops = layer_forward(a_hat, x, w, att, wmix, False)
    _, d_w, d_att, d_wmix = layer_backward(a_hat, x, w, att, wmix, False, ops, d_logits)
    return dict(w=d_w, att=d_att, wmix=d_wmix)


def acm_gcn2_forward(a_hat, x, p, keep_scale=None):
    """ACM-GCN-2: layer 1 (activation on) -> relu -> * keep_scale (the dropout mask times 1 / (1 - p); None: evaluation) -> layer 2.
    p: dict(w0, att0, wmix0, w1, att1, wmix1) -> (logits, what the backward pass needs)"""
    o1, ops1 = layer_forward(a_hat, x, p["w0"], p["att0"], p["wmix0"], True)
    hid = _act(o1, True)
    if keep_scale is not None:
        hid = hid * keep_scale
    logits, ops2 = layer_forward(a_hat, hid, p["w1"], p["att1"], p["wmix1"], False)
    return logits, (o1, ops1, hid, ops2)


def acm_gcn2_backward(a_hat, x, p, d_logits, keep_scale=None):
    _, (o1, ops1, hid, ops2) = acm_gcn2_forward(a_hat, x, p, keep_scale)
    d_hid, d_w1, d_att1, d_wmix1 = layer_backward(a_hat, hid, p["w1"], p["att1"], p["wmix1"], False, ops2, d_logits)
    if keep_scale is not None:
        d_hid = d_hid * keep_scale
    d_o1 = np.where(o1 > 0, d_hid, np.zeros((), d_hid.dtype))
    _, d_w0, d_att0, d_wmix0 = layer_backward(a_hat, x, p["w0"], p["att0"], p["wmix0"], True, ops1, d_o1)
    return dict(w0=d_w0, att0=d_att0, wmix0=d_wmix0, w1=d_w1, att1=d_att1, wmix1=d_wmix1)


# ------------------------------------------------------------------------------------- the same layer as torch operations
def torch_mix(low, high, high_agg, ident, att, wmix, relu):
    """the mix as a user would write it in torch (autograd supplies the backward pass): the yardstick of the restatement"""
    import torch
    h = torch.stack([low, high if high_agg is None else high - high_agg, ident])
    if relu:
        h = torch.relu(h)
    s = torch.sigmoid(torch.einsum("crk,ck->rc", h, att))
    alpha = torch.softmax((s / T) @ wmix, 1)
    return 3 * torch.einsum("rc,crk->rk", alpha, h)


def torch_layer(a_hat, m, w, att, wmix, relu):
    width = w.shape[1] // 3
    mw = m @ w
    return torch_mix(a_hat @ mw[:, :width], mw[:, width:2 * width], a_hat @ mw[:, width:2 * width], mw[:, 2 * width:], att, wmix, relu)
