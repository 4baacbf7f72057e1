"""Reference, data and case lists for the dense transforms C = act(A B + bias) and Z = act(A W0 + b0) W1 + b1
(tests/test_gpu_gemm_edges.py): plain numpy, no GPU.

The data is EXACT BY CONSTRUCTION in fp32, in any summation order, so a kernel on any route must return the fp64 reference bit
for bit.  Three families:
  ints       A, B and bias integers in [-8, 8], about a third of them zero: for K <= 4100 every partial sum of any order is an
             integer of magnitude <= 64 * 4100 + 8 < 2^24.  The two-layer transform takes integers in [-4, 4]: the hidden layer is
             bounded by 16 * 512 + 4 = 8196 and |Z| <= 64 * 8196 * 4 + 4 < 2^24.  Every entry is a bf16 (one piece of the split).
  selectors  A holds one 1.0 per row at column k_i and B[k][n] = 128 k + n, so C[i][n] = 128 k_i + n names the k and the n that
             were read; swapped, B holds one 1.0 per column at row k_n and A[i][k] = 128 k + i % 128.  < 2^24 for K <= 4100, N <= 100.
  full       one operand holds fp32 normals with all 24 significand bits in use (the last bit is set), the other one entry
             +-2^e, e in [-6, 6], per column (or per row) and zeros elsewhere: every output is +-2^e times ONE input element - on
             the fp32 chain and on the three-piece bf16 split alike, which must keep all three pieces of the full operand to get
             it.  A quarter of the columns have no entry and carry a full-mantissa bias instead (0 + b = b), the others no bias.
held by tests/test_gemm_ref.py."""
import numpy as np

EXACT_LIMIT = float(1 << 24)
WAYS = [(False, False), (True, False), (False, True), (True, True)]  # (bias, relu): the four ways every case runs
WAY_IDS = ["plain", "bias", "relu", "bias-relu"]
FAMILIES = ["ints", "selectors", "selectors-swapped", "full-a", "full-b"]
MLP2_FAMILIES = ["ints", "full-a", "full-w0"]


# ------------------------------------------------------------------------------------------- data
def ints(rng, shape, lim=8):
    """integers in [-lim, lim] as fp32, about a third of them zero"""
    v = rng.integers(-lim, lim + 1, shape)
    return np.where(rng.random(shape) < 0.3, 0, v).astype(np.float32)


def full(rng, shape):
    """fp32 normals +-(1.m) 2^e, e in [-8, 3], with the last significand bit set: all 24 bits (and all three bf16 pieces) in use"""
    bits = (rng.integers(0, 2, shape).astype(np.uint32) << 31) | (rng.integers(119, 131, shape).astype(np.uint32) << 23) | \
        rng.integers(0, 1 << 23, shape).astype(np.uint32) | np.uint32(1)
    return bits.astype(np.uint32).view(np.float32).reshape(shape)


def pow2(rng, n):
    """n values +-2^e, e in [-6, 6]"""
    return (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-6, 7, n)).astype(np.float32)


def _positions(rng, n, k):
    """n indices into [0, k): random, the first at k - 1 and the last at 0 (the edges of the K range are always read)"""
    p = rng.integers(0, k, n)
    if n > 0:
        p[0], p[-1] = k - 1, 0 if n > 1 else k - 1
    return p


def _no_entry(rng, n):
    """about a quarter of n columns (never all of them while n > 1): the columns of the full family that carry a bias instead"""
    none = rng.random(n) < 0.25
    if n > 1:
        none[0], none[-1] = False, True
    return none


def make_case(family, m, n, k, seed=0):
    """-> {"a" [m, k], "b" [k, n], "bias" [n]} fp32 (b is B itself: a transb launch stores its transpose)"""
    rng = np.random.default_rng([seed, m, n, k, FAMILIES.index(family)])
    a, b, bias = np.zeros((m, k), np.float32), np.zeros((k, n), np.float32), ints(rng, n)
    if family == "ints":
        a, b = ints(rng, (m, k)), ints(rng, (k, n))
    elif family == "selectors" and k > 0:
        a[np.arange(m), _positions(rng, m, k)] = 1.0
        b = (128.0 * np.arange(k)[:, None] + np.arange(n)[None, :]).astype(np.float32)
    elif family == "selectors-swapped" and k > 0:
        b[_positions(rng, n, k), np.arange(n)] = 1.0
        a = (128.0 * np.arange(k)[None, :] + (np.arange(m) % 128)[:, None]).astype(np.float32)
    elif family in ("full-a", "full-b"):
        none = _no_entry(rng, n) if k > 0 else np.ones(n, bool)
        bias = np.where(none, full(rng, n), 0).astype(np.float32)
        cols = np.flatnonzero(~none)
        if family == "full-a" and k > 0:
            a = full(rng, (m, k))
            b[_positions(rng, n, k)[cols], cols] = pow2(rng, cols.size)
        elif k > 0:
            b = full(rng, (k, n))
            b[:, none] = 0
            a[np.arange(m), _positions(rng, m, k)] = pow2(rng, m)
    return {"family": family, "m": m, "n": n, "k": k, "a": a, "b": b, "bias": bias}


def make_mlp2_case(family, m, k, h, c, seed=0):
    """-> {"a" [m, k], "w0" [k, h], "b0" [h], "w1" [h, c], "b1" [c]} fp32"""
    rng = np.random.default_rng([seed, m, k, h, c, MLP2_FAMILIES.index(family)])
    if family == "ints":
        a, w0, b0, w1, b1 = ints(rng, (m, k), 4), ints(rng, (k, h), 4), ints(rng, h, 4), ints(rng, (h, c), 4), ints(rng, c, 4)
    else:
        a, w0, w1 = np.zeros((m, k), np.float32), np.zeros((k, h), np.float32), np.zeros((h, c), np.float32)
        none0, none1 = _no_entry(rng, h), _no_entry(rng, c)
        b0, b1 = np.where(none0, full(rng, h), 0).astype(np.float32), np.where(none1, full(rng, c), 0).astype(np.float32)
        hid = np.flatnonzero(~none0)
        if family == "full-a":
            a = full(rng, (m, k))
            w0[_positions(rng, h, k)[hid], hid] = pow2(rng, hid.size)
        else:
            w0 = full(rng, (k, h))
            w0[:, none0] = 0
            a[np.arange(m), _positions(rng, m, k)] = pow2(rng, m)
        out = np.flatnonzero(~none1)
        w1[_positions(rng, c, h)[out], out] = pow2(rng, out.size)
    return {"family": family, "m": m, "k": k, "h": h, "c": c, "a": a, "w0": w0, "b0": b0, "w1": w1, "b1": b1}


# ------------------------------------------------------------------------------------------- references
def _f64(x):
    return np.asarray(x, np.float64)


def reference(case, way, a=None, b=None):
    """act(A B + bias) in fp64 -> [m, n]; a / b: operands to take instead of the case's (the non-finite cases: their products are
    formed one by one and summed, so that 0 x inf and 0 x NaN are NaN whatever the matrix library does with zeros); act = relu
    keeps a NaN"""
    use_bias, relu = way
    with np.errstate(all="ignore"):
        if a is None and b is None:
            c = _f64(case["a"]) @ _f64(case["b"])
        else:
            c = (_f64(case["a"] if a is None else a)[:, :, None] * _f64(case["b"] if b is None else b)[None, :, :]).sum(axis=1)
        if use_bias:
            c = c + _f64(case["bias"])[None, :]
        return np.where(c < 0, 0.0, c) if relu else c


def mlp2_reference(case, way):
    """act(A W0 + b0) W1 + b1 in fp64 -> [m, c]"""
    use_bias, relu = way
    hid = _f64(case["a"]) @ _f64(case["w0"])
    if use_bias:
        hid = hid + _f64(case["b0"])[None, :]
    z = (np.maximum(hid, 0.0) if relu else hid) @ _f64(case["w1"])
    return z + _f64(case["b1"])[None, :] if use_bias else z


def classes(y):
    """per element: 0 finite, 1 NaN, 2 +inf, 3 -inf"""
    y = np.asarray(y)
    return np.where(np.isnan(y), 1, np.where(np.isposinf(y), 2, np.where(np.isneginf(y), 3, 0))).astype(np.int8)


def magnitude(a, b, bias=None):
    """|A| |B| (+ |bias|) in fp64: what bounds every partial sum of every order"""
    s = np.abs(_f64(a)) @ np.abs(_f64(b))
    return s if bias is None else s + np.abs(_f64(bias))[None, :]


def terms_per_output(a, b):
    """how many of the K products of each output are non-zero"""
    return (np.asarray(a) != 0).astype(np.int64) @ (np.asarray(b) != 0).astype(np.int64)


# fp32 sums on the CPU in three orders (every add is numpy's own fp32 add: one rounding)
def _sum_forward(p):   # p [rows, k, cols] fp32 -> [rows, cols], k ascending
    acc = np.zeros((p.shape[0], p.shape[2]), np.float32)
    for j in range(p.shape[1]):
        acc = acc + p[:, j]
    return acc


def _sum_pairwise(p):
    if p.shape[1] == 0:
        return np.zeros((p.shape[0], p.shape[2]), np.float32)
    while p.shape[1] > 1:
        if p.shape[1] % 2:
            p = np.concatenate([p, np.zeros_like(p[:, :1])], axis=1)
        p = p[:, 0::2] + p[:, 1::2]
    return p[:, 0]


ORDERS = {"forward": _sum_forward, "reversed": lambda p: _sum_forward(p[:, ::-1]), "pairwise": _sum_pairwise}


def product_f32(a, b, order, rows=64):
    """A B with fp32 products and fp32 sums in the named order -> fp32 [m, n]"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    out = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for r in range(0, a.shape[0], rows):
        out[r:r + rows] = ORDERS[order](a[r:r + rows, :, None] * b[None, :, :])
    return out


def gemm_f32(case, way, order):
    use_bias, relu = way
    c = product_f32(case["a"], case["b"], order)
    if use_bias:
        c = c + case["bias"][None, :]
    return np.maximum(c, np.float32(0)) if relu else c


def mlp2_f32(case, way, order):
    use_bias, relu = way
    hid = product_f32(case["a"], case["w0"], order)
    if use_bias:
        hid = hid + case["b0"][None, :]
    z = product_f32(np.maximum(hid, np.float32(0)) if relu else hid, case["w1"], order)
    return z + case["b1"][None, :] if use_bias else z


def bf16_pieces(x):
    """the three bf16 pieces of csrc/split_bf16.h as fp32 arrays: x_h = bf16(x), x_m = bf16(x - x_h), x_l = bf16(x - x_h - x_m),
    round to nearest even each time"""
    def bf16(v):
        u = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(np.float32)
    x = np.ascontiguousarray(x, np.float32)
    h = bf16(x)
    m = bf16(x - h)
    return h, m, bf16(x - h - m)


# ------------------------------------------------------------------------------------------- case lists (the GPU file's shapes)
def pairwise_cover(*lists):
    """tuples over the lists such that every pair of values of two different lists occurs together: a Latin square over the two
    longest lists, the further lists indexed by (i + j) and (i + 2 j) modulo a prime >= the longest - fewer than the full product"""
    lists = [list(v) for v in lists]
    p = next(q for q in range(max(len(v) for v in lists), 100) if all(q % d for d in range(2, q)))
    out = []
    for i in range(p):
        for j in range(p):
            idx = [i, j] + [(i + (t + 1) * j) % p for t in range(len(lists) - 2)]
            if all(x < len(v) for x, v in zip(idx, lists)):
                out.append(tuple(v[x] for x, v in zip(idx, lists)))
    have = {(s, t, c[s], c[t]) for c in out for s in range(len(lists)) for t in range(s + 1, len(lists))}
    for s in range(len(lists)):  # (the index square is cut where p exceeds a list: add what the cut lost)
        for t in range(s + 1, len(lists)):
            for u in lists[s]:
                for v in lists[t]:
                    if (s, t, u, v) not in have:
                        c = [w[0] for w in lists]
                        c[s], c[t] = u, v
                        out.append(tuple(c))
                        have |= {(s2, t2, c[s2], c[t2]) for s2 in range(len(lists)) for t2 in range(s2 + 1, len(lists))}
    return out


TILE_M = [1, 31, 32, 33, 127, 128, 129, 257]
TILE_N = [1, 31, 32, 33, 63, 64, 65, 100]   # both column-tile widths, one and two column blocks, a ragged second tile
TILE_K = [0, 1, 15, 16, 17, 33, 300]        # the empty sum, below / at / above one K step of 16, odd, many steps
TILE_SHAPES = pairwise_cover(TILE_M, TILE_N, TILE_K)

BRES_K = [4, 28, 32, 36, 64, 68, 512]       # no whole group of 32, one group, odd and even group counts, a leftover, the LDS limit
BRES_K_REFUSED = [516, 6]                   # past the LDS limit; K % 4 != 0
BRES_M = [1, 33, 512, 513]                  # 513: the smallest M with two row parts on a device of >= 8 CUs
BRES_N = [1, 32, 33, 64]
BRES_SHAPES = pairwise_cover(BRES_M, BRES_N, BRES_K)

BATCH_JOBS = [(513, 64, 68), (0, 5, 4), (1, 1, 4), (33, 32, 512), (130, 33, 36)]  # (M, N, K); every second job has a bias

SPLITK_SHAPES = [(5, 3, 1040, 16),     # range length 80: ranges 13 .. 15 are empty
                 (129, 33, 1024, 16),  # exact ranges of 64
                 (130, 65, 1100, 7),   # ranges of 160, a ragged last one of 140, two column blocks
                 (5, 3, 100, 7)]       # K < 7 * 16: the single chain

SKINNY_K = [0, 1, 16, 17, 128, 129, 512, 513, 2049]
SKINNY_LANES = [1, 1, 1, 4, 4, 16, 16, 64, 64]
SKINNY_N = [1, 3, 7, 8]
SKINNY_M = [1, 4, 5, 63, 64, 65, 257]       # ragged row groups for 256 / 64 / 16 / 4 rows per workgroup
SKINNY_SHAPES = pairwise_cover(SKINNY_M, SKINNY_N, SKINNY_K)

MLP2_SHAPES = [(1, 4, 16, 1), (33, 68, 64, 1), (513, 260, 64, 5), (100, 28, 40, 8), (260, 512, 33, 8)]  # (M, K, H, C)

# non-finite inputs: (kernel, M, N, K), ragged for that kernel; the poison sits on the last row, the last k and the last column
NONFINITE_SHAPES = [("tile", 130, 33, 35), ("tile-transb", 130, 65, 35), ("resident", 545, 33, 36), ("splitk", 130, 33, 1100),
                    ("skinny", 65, 7, 1), ("skinny", 65, 7, 17), ("skinny", 65, 7, 129), ("skinny", 65, 7, 513)]
