"""The numpy restatement of the GCNII layer kernels (csrc/gcnii.hip) as include/wdg.h states them, operation by operation: the fp32 form
with an exact fma (the bits the GPU test demands), the fp64 form with the companion sums the derived bounds are taken against, the
epilogue's mask from tests/_dropout_ref.py, and the inputs the CPU and the GPU tests share.

The bound of an fp32 element against its fp64 value: (k + 2) 2^-24 * the companion sum of the absolute values of its terms, k the number
of roundings on the way to the element in the stated order (tests/test_gat_scores_ref.py derives the form); roundings() counts k."""
import numpy as np

import _dropout_ref
from _sparse_dense_ref import fma32_exact

U = 2.0 ** -24
ROW_BLOCK = 32  # WDG_GCNII_ROW_BLOCK
MAX_W = 128     # WDG_GCNII_MAX_W
F32 = np.float32


def _fma(a, b, c):
    shape = np.broadcast_shapes(np.shape(a), np.shape(b), np.shape(c))
    with np.errstate(invalid="ignore", over="ignore"):
        return fma32_exact(np.broadcast_to(np.asarray(a, F32), shape), np.broadcast_to(np.asarray(b, F32), shape),
                           np.broadcast_to(np.asarray(c, F32), shape))


def _mul(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, F32) * np.asarray(b, F32)).astype(F32)


def forward32(P, H0, W, alpha, beta):
    """-> (S, Z) fp32 [n, w]: S = fmaf(alpha, H0, a1 * P); T = one chain from +0 over ascending k of fmaf(S[:, k], W[k, :], acc);
    Z = fmaf(beta, T, b1 * S)"""
    alpha, beta = F32(alpha), F32(beta)
    a1, b1 = F32(1.0) - alpha, F32(1.0) - beta
    S = _fma(alpha, H0, _mul(a1, P))
    T = np.zeros_like(S)
    for k in range(W.shape[0]):
        T = _fma(S[:, k:k + 1], W[k][None, :], T)
    return S, _fma(beta, T, _mul(b1, S))


def relu_dropout32(Z, p, seed, stream, step):
    """what wdg_relu_dropout_batched_f32 makes of Z (tests/_dropout_ref.py)"""
    return _dropout_ref.relu_dropout(Z, p, seed, stream, step)


def d_z32(d_out, out, act, scale):
    if not act:
        return np.asarray(d_out, F32).copy()
    return np.where(out > 0, _mul(d_out, F32(scale)), F32(0.0)).astype(F32)


def backward32(d_out, out, S, W, alpha, beta, d_H0, act, scale):
    """-> (d_P, d_H0 after the launch, partial [blocks, w, w], d_W), all fp32, in the stated orders"""
    alpha, beta = F32(alpha), F32(beta)
    a1, b1 = F32(1.0) - alpha, F32(1.0) - beta
    n, w = S.shape
    dZ = d_z32(d_out, out, act, scale)
    Uc = np.zeros((n, w), F32)
    for c in range(w):
        Uc = _fma(dZ[:, c:c + 1], W[:, c][None, :], Uc)
    dS = _fma(beta, Uc, _mul(b1, dZ))
    d_P = _mul(a1, dS)
    d_H0_new = _fma(alpha, dS, d_H0)
    blocks = -(-n // ROW_BLOCK)
    partial = np.zeros((blocks, w, w), F32)
    for b in range(blocks):
        for i in range(b * ROW_BLOCK, min(n, (b + 1) * ROW_BLOCK)):
            partial[b] = _fma(S[i][:, None], dZ[i][None, :], partial[b])
    acc = np.zeros((w, w), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(blocks):
            acc = (acc + partial[b]).astype(F32)
    return d_P, d_H0_new, partial, _mul(beta, acc)


def forward64(P, H0, W, alpha, beta):
    """the fp64 value of the same expressions on the same fp32 inputs -> (S, S_abs, Z, Z_abs): values and companion sums"""
    alpha, beta = float(F32(alpha)), float(F32(beta))
    P, H0, W = (np.asarray(a, np.float64) for a in (P, H0, W))
    S = alpha * H0 + (1.0 - alpha) * P
    S_abs = abs(alpha) * np.abs(H0) + abs(1.0 - alpha) * np.abs(P)
    Z = beta * (S @ W) + (1.0 - beta) * S
    Z_abs = abs(beta) * (S_abs @ np.abs(W)) + abs(1.0 - beta) * S_abs
    return S, S_abs, Z, Z_abs


def backward64(d_out, out, S, W, alpha, beta, d_H0, act, scale):
    """the backward pass in fp64 on the kernel's own inputs (its fp32 S and out) -> dict name -> (value, companion) for d_P, d_H0, d_W"""
    alpha, beta, scale = float(F32(alpha)), float(F32(beta)), float(F32(scale))
    d_out, S, W, d_H0 = (np.asarray(a, np.float64) for a in (d_out, S, W, d_H0))
    dZ = np.where(np.asarray(out) > 0, d_out * scale, 0.0) if act else d_out
    dS = beta * (dZ @ W.T) + (1.0 - beta) * dZ
    dS_abs = abs(beta) * (np.abs(dZ) @ np.abs(W).T) + abs(1.0 - beta) * np.abs(dZ)
    return dict(d_P=((1.0 - alpha) * dS, abs(1.0 - alpha) * dS_abs),
                d_H0=(alpha * dS + d_H0, abs(alpha) * dS_abs + np.abs(d_H0)),
                d_W=(beta * (S.T @ dZ), abs(beta) * (np.abs(S).T @ np.abs(dZ))))


def roundings(n, w):
    """the roundings on the way to one element in the stated orders, counted from the statement in include/wdg.h:
    S       3: a1; a1 * P; the fma
    Z       max(w + 4, 6): a term of the chain carries S's 3, the chain's w fmas and the last fma; the other term b1, S's 3, b1 * S, the fma
    out     Z's + 1: the multiply by scale (the ReLU is 1-Lipschitz, the mask the same)
    dS      max(w + 2, 4): a term of the chain carries dZ's multiply by scale, w fmas and the last fma; the other b1, dZ's, b1 * dZ, the fma
    d_P     dS's + 2: a1; a1 * dS
    d_H0    dS's + 1: the fma
    d_W     min(n, ROW_BLOCK) + ceil(n / ROW_BLOCK) + 2: dZ's multiply; the block's chain; one addition per block; the multiply by beta"""
    z, ds = max(w + 4, 6), max(w + 2, 4)
    return dict(S=3, Z=z, out=z + 1, d_P=ds + 2, d_H0=ds + 1, d_W=min(n, ROW_BLOCK) + -(-n // ROW_BLOCK) + 2)


def within(name, got32, value64, companion, n, w):
    """the largest |got - value| / ((k + 2) U companion) over the elements whose companion is not zero (1.0 = the bound); elements
    with a zero companion must be exact"""
    k = roundings(n, w)[name]
    err = np.abs(np.asarray(got32, np.float64) - value64)
    bound = (k + 2) * U * companion
    assert (err[bound == 0] == 0).all(), name
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


# ------------------------------------------------------------------------------------------- the jobs the CPU and the GPU tests share
# (n, w, extra leading dimension, pointer offset in floats, (alpha, beta)): n at one below, at and one above ROW_BLOCK, at 1, three blocks
# and a ragged tail, no rows; every w at which the kernel takes another shape (the thread shapes change at 16, 32, 64; 16-byte accesses
# need w % 4 == 0); leading dimensions above w; one job on pointers 4 bytes off a 16-byte boundary
AB = ((0.1, 0.4), (0.0, 1.0), (1.0, 0.0))
JOBS = [(31, 1, 0, 0, AB[0]), (32, 3, 2, 0, AB[1]), (33, 4, 0, 0, AB[2]), (1, 5, 3, 0, AB[0]), (101, 17, 0, 0, AB[0]), (101, 64, 0, 0, AB[0]),
        (33, 65, 1, 0, AB[1]), (101, 128, 4, 0, AB[0]), (37, 64, 8, 1, AB[0]), (37, 64, 8, 0, AB[0]), (0, 8, 0, 0, AB[0]), (32, 32, 0, 0, AB[2]),
        (5, 16, 4, 0, AB[0]), (64, 128, 0, 0, AB[1])]
OFFSET_PAIR = (8, 9)  # the job on offset pointers and its aligned twin: the same numbers
SEED = 20260

_CACHE = {}


def job_inputs(index):
    """the fp32 inputs of JOBS[index] (read-only, computed once): P, H0, W, d_out, d_H0 - the offset job and its twin share theirs"""
    key = OFFSET_PAIR[1] if index == OFFSET_PAIR[0] else index
    if key not in _CACHE:
        n, w = JOBS[key][:2]
        rng = np.random.default_rng(1000 + key)
        out = dict(P=rng.standard_normal((n, w)), H0=np.abs(rng.standard_normal((n, w))), W=rng.standard_normal((w, w)) / np.sqrt(w),
                   d_out=rng.standard_normal((n, w)), d_H0=rng.standard_normal((n, w)))
        out = {k: v.astype(F32) for k, v in out.items()}
        for a in out.values():
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def job_reference(index, act, p=0.0, step=0):
    """the fp32 restatement of JOBS[index] (computed once per (job, act, p, step)): dict S, Z, out, d_P, d_H0, partial, d_W"""
    key = ("ref", OFFSET_PAIR[1] if index == OFFSET_PAIR[0] else index, bool(act), float(p), int(step))
    if key not in _CACHE:
        x = job_inputs(index)
        alpha, beta = JOBS[index][4]
        S, Z = forward32(x["P"], x["H0"], x["W"], alpha, beta)
        out = relu_dropout32(Z, p, SEED, stream_of(key[1]), step) if act else Z
        scale = _dropout_ref.constants(p)[1]
        d_P, d_H0, partial, d_W = backward32(x["d_out"], out, S, x["W"], alpha, beta, x["d_H0"], act, scale)
        _CACHE[key] = dict(S=S, Z=Z, out=out, d_P=d_P, d_H0=d_H0, partial=partial, d_W=d_W)
    return _CACHE[key]


def stream_of(index):
    """the generator stream of a job: the offset job draws its twin's"""
    return 7 + (OFFSET_PAIR[1] if index == OFFSET_PAIR[0] else index)
