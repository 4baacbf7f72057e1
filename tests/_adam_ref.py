"""Numpy restatement of wdg_adam_batched_f32 (include/wdg.h, csrc/adam.hip) in the dtype of its inputs: the square-and-multiply power
behind the bias corrections, the segment rule, and the step with every multiply and add as an operation of its own.  In float32 it
is the kernel bit for bit (numpy rounds every float32 operation correctly and fuses nothing; the two bias corrections are formed in
float64 and rounded to float32 once, as on the device); in float64 it is torch.optim.Adam's rule (tests/test_adam_ref.py)."""
import numpy as np


def ipow(b, t):
    """b^t by square and multiply, in float64 (csrc/ipow.h)"""
    b, r, t = np.float64(b), np.float64(1.0), int(t)
    while t > 0:
        if t & 1:
            r = r * b
        b = b * b
        t >>= 1
    return r


def segment_index(rows, cols, seg_rows, seg_cols):
    """int64 [rows, cols]: the segment of every element, (r // seg_rows) * ceil(cols / seg_cols) + c // seg_cols"""
    per_row = -(-cols // seg_cols)
    return (np.arange(rows, dtype=np.int64)[:, None] // seg_rows) * per_row + np.arange(cols, dtype=np.int64)[None, :] // seg_cols


def n_segments(rows, cols, seg_rows, seg_cols):
    return (-(-rows // seg_rows)) * (-(-cols // seg_cols)) if rows and cols else 0


def adam_step(p, g, m, v, hyper, seg_rows, seg_cols, t, beta1=0.9, beta2=0.999, eps=1e-8):
    """one step t (1-based) -> (p, m, v), new arrays of p's dtype.  p, g, m, v: [rows, cols] of ONE dtype (float32 or float64);
    hyper: [segments, 2] (lr, weight_decay).  beta1, beta2 and eps are taken at p's precision, as the kernel takes them as floats."""
    dt = p.dtype.type
    assert g.dtype == m.dtype == v.dtype == p.dtype and p.ndim == 2
    rows, cols = p.shape
    hyper = np.asarray(hyper).astype(p.dtype).reshape(-1, 2)
    assert hyper.shape[0] == n_segments(rows, cols, seg_rows, seg_cols)
    if p.size == 0:
        return p.copy(), m.copy(), v.copy()
    seg = segment_index(rows, cols, seg_rows, seg_cols)
    b1, b2, e = dt(beta1), dt(beta2), dt(eps)
    # the bias corrections: in double from the (rounded) betas and lr, rounded to the working precision once
    bc1 = np.float64(1.0) - ipow(np.float64(b1), t)
    bc2_sqrt = dt(np.sqrt(np.float64(1.0) - ipow(np.float64(b2), t)))
    with np.errstate(all="ignore"):
        step_size = (hyper[:, 0].astype(np.float64) / bc1).astype(p.dtype)[seg]
        wd = hyper[:, 1][seg]
        one_b1, one_b2 = dt(1.0) - b1, dt(1.0) - b2
        g1 = g + wd * p
        m1 = b1 * m + one_b1 * g1
        v1 = b2 * v + (one_b2 * g1) * g1
        den = np.sqrt(v1) / bc2_sqrt + e
        p1 = p - step_size * (m1 / den)
    assert p1.dtype == m1.dtype == v1.dtype == p.dtype
    return p1, m1, v1
