"""numpy restatement of the CSBM-H device entries documented in include/wdg.h: wdg_synth_classes_batched (classes of any sizes,
a same-class count and a degree per class), wdg_gauss_features_batched_f32 (Box-Muller on Philox words) and the fp64 Bayes rule
of wdg_qda_errors_batched_i32; and the fp64 Monte Carlo the closed-form Bayes error is checked against."""
import functools

import numpy as np

from _synth_ref import SELF_LOOPS, keys_of_rows, philox4x32_10

# (class sizes, k, d) of the generator comparison: unequal classes; a one-node class and k = 0; every candidate taken; two blocks of rows
CLASS_SHAPES = [((5, 3), (2, 1), (3, 3)), ((4, 1, 3), (0, 0, 2), (2, 3, 2)), ((6, 4), (5, 3), (9, 9)), ((130, 70), (64, 3), (129, 40))]


def class_graph(sizes, k, d, seed, flags=0):
    """-> (rowptr int32 [n + 1], col int32 [nnz], labels int32 [n]); every stored value is 1"""
    n, loops = int(sum(sizes)), 1 if flags & SELF_LOOPS else 0
    starts = np.concatenate([[0], np.cumsum(sizes)])
    cols, lengths, labels = [], [], []
    for c, m in enumerate(sizes):
        cs, ce = int(starts[c]), int(starts[c + 1])
        assert 0 <= k[c] <= m - 1 and k[c] <= d[c] and d[c] - k[c] <= n - m
        rows = np.arange(cs, ce)
        key = keys_of_rows(rows, n, seed).astype(np.int64)
        same = key[:, cs:ce].copy()
        same[np.arange(m), np.arange(m)] = 1 << 40  # the row itself is no candidate
        parts = [np.argsort(same, axis=1, kind="stable")[:, :k[c]] + cs]  # stable: ties by column
        other_cols = np.concatenate([np.arange(0, cs), np.arange(ce, n)])
        parts.append(other_cols[np.argsort(key[:, other_cols], axis=1, kind="stable")[:, :d[c] - k[c]]])
        if loops:
            parts.append(rows[:, None])
        cols.append(np.sort(np.concatenate(parts, axis=1), axis=1).reshape(-1))
        lengths += [d[c] + loops] * m
        labels += [c] * m
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return rowptr, np.concatenate(cols).astype(np.int32), np.asarray(labels, np.int32)


def standard_normals(n, F, seed):
    """z(i, f) of wdg_gauss_features_batched_f32 from the same Philox words, in fp64 -> [n, F]"""
    Q = (F + 3) // 4
    w = philox4x32_10(np.arange(n)[:, None], np.arange(Q)[None, :], seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF).astype(np.uint64)  # [n, Q, 4]
    z = np.empty((n, Q, 4))
    for p in range(2):
        u1 = ((w[:, :, 2 * p] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
        u2 = (w[:, :, 2 * p + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        z[:, :, 2 * p], z[:, :, 2 * p + 1] = r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)
    return z.reshape(n, 4 * Q)[:, :F]


def qda_counts(x, h, labels, mean, inv2v, bias):
    """the rule of wdg_qda_errors_batched_i32 on fp32 x, h -> int64 [3, 2, 2] ([set][true][predicted]); every operation fp64 and
    rounded on its own, the high-pass row ONE fp32 subtraction"""
    x, h = np.asarray(x, np.float32), np.asarray(h, np.float32)
    n, F = x.shape
    sets = (x.astype(np.float64), h.astype(np.float64), (x - h).astype(np.float64))
    counts = np.zeros((3, 2, 2), np.int64)
    with np.errstate(invalid="ignore"):
        for t, z in enumerate(sets):
            g = []
            for c in range(2):
                s = np.zeros(n)
                for f in range(F):
                    e = z[:, f] - mean[t][c][f]
                    s = s + e * e
                g.append(bias[t][c] - inv2v[t][c] * s)
            pred = np.where(g[0] > g[1], 0, 1)  # (a NaN: 1)
            for y in range(2):
                for p in range(2):
                    counts[t, y, p] = int(np.sum((labels == y) & (pred == p)))
    return counts


MC_DRAWS = 1_000_000


@functools.lru_cache(maxsize=None)
def mc_normals():
    """the shared fp64 standard normals of the Monte Carlo: [2, MC_DRAWS, 3] (a class each), fixed seed, read-only"""
    w = np.random.default_rng(20240607).standard_normal((2, MC_DRAWS, 3))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _mc_square_norms(F):
    return (mc_normals()[:, :, :F] ** 2).sum(2)  # [2, MC_DRAWS]


def mc_errors(n0, n1, m0, m1, v0, v1):
    """-> (rate of class-0 draws predicted 1, rate of class-1 draws predicted 0) of the rule g_c = ln n_c - F/2 ln v_c -
    |z - m_c|^2 / (2 v_c), class 0 iff g_0 > g_1, on MC_DRAWS i.i.d. draws z = m + sqrt(v) w per class (|z - m_c|^2 expanded around
    the draw's own centre: |m - m_c|^2 + 2 sqrt(v) (m - m_c).w + v |w|^2)"""
    return _mc_errors(int(n0), int(n1), tuple(float(a) for a in m0), tuple(float(a) for a in m1), float(v0), float(v1))


@functools.lru_cache(maxsize=None)
def _mc_errors(n0, n1, m0, m1, v0, v1):
    m0, m1 = np.asarray(m0, np.float64), np.asarray(m1, np.float64)
    F = m0.shape[0]
    w, w2 = mc_normals(), _mc_square_norms(F)
    out = []
    for c, (m, v) in enumerate(((m0, v0), (m1, v1))):
        dist = [(m - mc) @ (m - mc) + 2 * np.sqrt(v) * (w[c][:, :F] @ (m - mc)) + v * w2[c] for mc in (m0, m1)]
        g0 = np.log(n0) - F / 2 * np.log(v0) - dist[0] / (2 * v0)
        g1 = np.log(n1) - F / 2 * np.log(v1) - dist[1] / (2 * v1)
        out.append(float(np.mean((g0 > g1) != (c == 0))))
    return tuple(out)
