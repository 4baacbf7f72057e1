"""The attention scores of include/wdg.h (wdg_gat_scores_forward_batched_f32 and its backward pass) restated in numpy: in fp32 with
fma32_exact of tests/_sparse_dense_ref.py, in the header's stated orders - the bits the kernel must give -, and in fp64 with the
ABSOLUTE-VALUE COMPANION of every output: the same formula with every term replaced by its absolute value, what a rounding-error bound
of the form K 2^-24 companion multiplies.  Also the dense operand blockdiag(a_dst, a_src) the per-graph model multiplies by."""
import numpy as np

from _sparse_dense_ref import fma32_exact

ROW_BLOCK = 32  # WDG_GAT_SCORES_ROW_BLOCK
U = 2.0 ** -24


def score_columns(G, heads):
    """-> (dst [G], src [G]): the column of S that holds group g's dst score and its src score.  The groups are cut into consecutive
    blocks of `heads` (the last may be shorter: hb groups); block b owns columns 2 heads b .. 2 heads b + 2 hb, dst scores first"""
    g = np.arange(G, dtype=np.int64)
    b = g // heads
    hb = np.minimum(heads, G - b * heads)
    dst = 2 * heads * b + (g - b * heads)
    return dst, dst + hb


def operand(att, heads):
    """blockdiag(a_dst, a_src) [G w, 2 G] of att [2, G, w] in the column layout above: S = H @ operand"""
    _, G, w = att.shape
    dst, src = score_columns(G, heads)
    m = np.zeros((G * w, 2 * G), att.dtype)
    for g in range(G):
        m[g * w:(g + 1) * w, dst[g]] = att[0, g]
        m[g * w:(g + 1) * w, src[g]] = att[1, g]
    return m


def _fma(a, b, c):
    a, b, c = np.broadcast_arrays(a, b, c)
    return fma32_exact(np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(c))


def forward32(h, att, heads):
    """fp32 h [n, G w], att [2, G, w] -> S fp32 [n, 2 G]: per (row, group) ONE fma chain from +0 over ascending k"""
    n, (_, G, w) = h.shape[0], att.shape
    dst, src = score_columns(G, heads)
    h3 = h.reshape(n, G, w)
    s = np.zeros((n, 2 * G), np.float32)
    for p, cols in ((0, dst), (1, src)):
        acc = np.zeros((n, G), np.float32)
        for k in range(w):
            acc = _fma(h3[:, :, k], att[p, :, k][None, :], acc)
        s[:, cols] = acc
    return s


def backward32(h, att, heads, d_s, d_h):
    """-> (d_h + the operand gradient [n, G w], d_att [2, G, w], partial [blocks, 2, G, w]), fp32, in the header's orders:
    d_h = fma(d_s_src, a_src, fma(d_s_dst, a_dst, d_h)); per block of ROW_BLOCK rows one chain fma(d_s, h, acc) from +0 over ascending
    rows; the blocks' sums added in ascending order from +0"""
    n, (_, G, w) = h.shape[0], att.shape
    dst, src = score_columns(G, heads)
    h3 = h.reshape(n, G, w)
    dsd, dss = d_s[:, dst][:, :, None], d_s[:, src][:, :, None]
    out = _fma(dss, att[1][None], _fma(dsd, att[0][None], d_h.reshape(n, G, w))).reshape(n, G * w)
    blocks = -(-n // ROW_BLOCK)
    partial = np.zeros((blocks, 2, G, w), np.float32)
    for t in range(min(ROW_BLOCK, n)):
        rows = np.arange(t, n, ROW_BLOCK)  # row t of every block that has one
        b = rows // ROW_BLOCK
        partial[b, 0] = _fma(dsd[rows], h3[rows], partial[b, 0])
        partial[b, 1] = _fma(dss[rows], h3[rows], partial[b, 1])
    d_att = np.zeros((2, G, w), np.float32)
    for b in range(blocks):
        d_att = d_att + partial[b]
    return out, d_att, partial


def forward64(h, att, heads):
    """-> (S, S_abs) in fp64"""
    h, att = h.astype(np.float64), att.astype(np.float64)
    n, (_, G, w) = h.shape[0], att.shape
    dst, src = score_columns(G, heads)
    h3 = h.reshape(n, G, w)
    s, s_abs = np.zeros((n, 2 * G)), np.zeros((n, 2 * G))
    for p, cols in ((0, dst), (1, src)):
        s[:, cols] = np.einsum("igk,gk->ig", h3, att[p])
        s_abs[:, cols] = np.einsum("igk,gk->ig", np.abs(h3), np.abs(att[p]))
    return s, s_abs


def backward64(h, att, heads, d_s, d_h):
    """-> (d_h, d_att, d_h_abs, d_att_abs) in fp64"""
    h, att, d_s, d_h = (a.astype(np.float64) for a in (h, att, d_s, d_h))
    n, (_, G, w) = h.shape[0], att.shape
    dst, src = score_columns(G, heads)
    h3 = h.reshape(n, G, w)
    dsd, dss = d_s[:, dst], d_s[:, src]
    out = d_h.reshape(n, G, w) + dsd[:, :, None] * att[0][None] + dss[:, :, None] * att[1][None]
    out_abs = np.abs(d_h.reshape(n, G, w)) + np.abs(dsd)[:, :, None] * np.abs(att[0])[None] + np.abs(dss)[:, :, None] * np.abs(att[1])[None]
    d_att = np.stack([np.einsum("ig,igk->gk", dsd, h3), np.einsum("ig,igk->gk", dss, h3)])
    d_att_abs = np.stack([np.einsum("ig,igk->gk", np.abs(dsd), np.abs(h3)), np.einsum("ig,igk->gk", np.abs(dss), np.abs(h3))])
    return out.reshape(n, G * w), d_att, out_abs.reshape(n, G * w), d_att_abs


def roundings(n, w):
    """the roundings on the way to one element in the stated orders -> (S, d_h, d_att): a chain of w fmas; two fmas; a chain of
    min(n, ROW_BLOCK) fmas and then one addition per block"""
    return w, 2, min(n, ROW_BLOCK) + -(-n // ROW_BLOCK)
