"""numpy restatement of the device generators documented in include/wdg.h (wdg_synth_regular_batched, wdg_synth_feature_rows):
the synthetic regular graphs of the sweep and the per-class draw of base rows behind their features."""
import functools

import numpy as np

SELF_LOOPS = 1  # WDG_SYNTH_SELF_LOOPS
SYNTH_TAG = 0x53594E  # the tag of sweep.synth_seed

# the shapes (n, C, k, d) of the structure tests and of the device comparison
SHAPES = [(10, 5, 1, 1), (10, 5, 1, 9), (67, 1, 3, 3), (130, 2, 64, 129), (257, 1, 5, 5), (2000, 5, 10, 66), (2000, 5, 2, 40),
          (4100, 5, 2, 5)]


def philox4x32_10(c0, c1, k0, k1):
    """all four output words of Philox4x32-10, counter {c0, c1, 0, 0}, key {k0, k1} -> uint32 array [..., 4]"""
    c0 = np.asarray(c0, np.uint64)
    c1 = np.asarray(c1, np.uint64) + np.zeros_like(c0)
    c0 = c0 + np.zeros_like(c1)
    c2, c3 = np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = np.uint64(k0), np.uint64(k1)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n2 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & m32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & m32
        c1, c3, c0, c2 = p1 & m32, p0 & m32, n0, n2
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def keys_of_rows(rows, n, seed):
    """key(i, j) for the rows `rows` and every column j < n -> uint32 [len(rows), n]"""
    blocks = (n + 3) // 4
    w = philox4x32_10(np.asarray(rows)[:, None], np.arange(blocks)[None, :], seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return w.reshape(len(rows), 4 * blocks)[:, :n]


def regular_graph(n, n_classes, k, d, seed, flags=0):
    """-> (rowptr int32 [n + 1], col int32 [n D], labels int32 [n]); every stored value is 1"""
    assert n % n_classes == 0
    m = n // n_classes
    assert 1 <= k <= m - 1 and k <= d and d - k <= n - m
    loops = 1 if flags & SELF_LOOPS else 0
    D = d + loops
    col = np.empty((n, D), np.int64)
    for c in range(n_classes):
        rows = np.arange(c * m, (c + 1) * m)
        key = keys_of_rows(rows, n, seed).astype(np.int64)
        same = key[:, c * m:(c + 1) * m].copy()
        same[np.arange(m), np.arange(m)] = 1 << 40  # the row itself is no candidate
        parts = [np.argsort(same, axis=1, kind="stable")[:, :k] + c * m]  # stable: ties by column
        if d > k:
            other_cols = np.concatenate([np.arange(0, c * m), np.arange((c + 1) * m, n)])
            parts.append(other_cols[np.argsort(key[:, other_cols], axis=1, kind="stable")[:, :d - k]])
        if loops:
            parts.append(rows[:, None])
        col[rows] = np.sort(np.concatenate(parts, axis=1), axis=1)
    rowptr = (np.arange(n + 1) * D).astype(np.int32)
    return rowptr, col.reshape(-1).astype(np.int32), (np.arange(n) // m).astype(np.int32)


@functools.lru_cache(maxsize=None)
def cached_graph(n, n_classes, k, d, seed, flags=0):
    """regular_graph, computed once per process (the tests share the restated graphs and never write to them)"""
    out = regular_graph(n, n_classes, k, d, seed, flags)
    for a in out:
        a.setflags(write=False)
    return out


def coo_of(rowptr, col):
    """-> (src, dst) int64 host arrays of a CSR pattern"""
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)).astype(np.int64), col.astype(np.int64)


def mix64(*words):
    """sweep._mix64 (splitmix64 over a few integers), restated"""
    mask = 0xFFFFFFFFFFFFFFFF
    x = 0x9E3779B97F4A7C15
    for w in words:
        x = (x ^ (int(w) & mask)) & mask
        x = (x + 0x9E3779B97F4A7C15) & mask
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & mask
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & mask
        x ^= x >> 31
    return x


def job_seed(seed, h, n, k):
    """the per-graph seed of a sweep job: _mix64 over (job.seed, round(1000 h), n, k, a tag)"""
    return mix64(seed, int(round(1000 * h)), n, k, SYNTH_TAG)


def feature_rows(base_labels, n, n_classes, seed):
    """-> int32 [n]: node i of class c = i // (n // C) takes member (u |class c|) >> 32 of the ascending base rows labelled c,
    u = first word of Philox4x32-10(counter {i, 0, 0, 0}, key seed)"""
    base_labels = np.asarray(base_labels)
    m = n // n_classes
    u = philox4x32_10(np.arange(n), 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[:, 0].astype(np.uint64)
    out = np.empty(n, np.int32)
    for c in range(n_classes):
        members = np.flatnonzero(base_labels == c)
        if not len(members):
            raise ValueError(f"class {c} has no base rows")
        pick = (u[c * m:(c + 1) * m] * np.uint64(len(members))) >> np.uint64(32)
        out[c * m:(c + 1) * m] = members[pick.astype(np.int64)]
    return out


def column_chi2(cols_by_row, n, n_classes, k, d):
    """in-degree statistics of graphs of ONE shape: cols_by_row = list of [n, d] column arrays (no loops).  -> (same, other): the sum
    over columns of (count - expectation)^2 / variance, the variance being the sum of the rows' Bernoulli variances; other = None
    when d == k"""
    m = n // n_classes
    lab = np.arange(n) // m
    cnt_s, cnt_o = np.zeros(n), np.zeros(n)
    for col in cols_by_row:
        same = lab[col] == lab[:, None]
        cnt_s += np.bincount(col[same], minlength=n)
        cnt_o += np.bincount(col[~same], minlength=n)
    g = len(cols_by_row)
    ps, po = k / (m - 1), (d - k) / (n - m) if n > m else 0.0
    stat_s = float(((cnt_s - g * (m - 1) * ps) ** 2 / (g * (m - 1) * ps * (1 - ps))).sum()) if ps < 1 else 0.0
    stat_o = None
    if d > k and po < 1:
        stat_o = float(((cnt_o - g * (n - m) * po) ** 2 / (g * (n - m) * po * (1 - po))).sum())
    return stat_s, stat_o
