"""numpy restatement of the row representatives (include/wdg.h, wdg_row_rep_batched; csrc/row_rep.hip): rep[i] = the smallest row
whose CANONICAL bytes equal row i's - a dictionary over byte keys - and the inputs of tests/test_gpu_row_rep.py (numpy only, so that
tests/test_row_rep_ref.py can assert without a GPU what they hold).
Canonical: -0 becomes +0; a row that holds a NaN is unique; a CSR row's key is its entry count, its columns in stored order, its
values where they are used and its row scale where one is given."""
import numpy as np


def rep_numpy(keys):
    """keys: one hashable per row -> int32 [n], the first row with the same key"""
    first, rep = {}, []
    for i, k in enumerate(keys):
        rep.append(first.setdefault(k, i))
    return np.asarray(rep, np.int32)


def _canon(a):
    a = np.array(a, np.float32, copy=True)
    a[a == 0] = 0.0  # -0 -> +0
    return a


def dense_keys(x):
    x = _canon(x)
    return [r.tobytes() if not np.isnan(r).any() else (b"nan", i) for i, r in enumerate(x)]


def csr_keys(rowptr, col, val=None, scale=None):
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int32)
    val = None if val is None else _canon(val)
    scale = None if scale is None else _canon(scale)
    keys = []
    for i in range(len(rowptr) - 1):
        a, b = rowptr[i], rowptr[i + 1]
        key = np.int32(b - a).tobytes() + col[a:b].tobytes()
        nan = False
        if val is not None:
            key, nan = key + val[a:b].tobytes(), bool(np.isnan(val[a:b]).any())
        if scale is not None:
            key, nan = key + scale[i].tobytes(), nan or bool(np.isnan(scale[i]))
        keys.append((b"nan", i) if nan else key)
    return keys


def merged_share(rep):
    return float((rep != np.arange(len(rep))).mean()) if len(rep) else 0.0


# ----------------------------------------------------------------------------------------------------------------- inputs
DENSE_F = (1, 3, 4, 64, 260, 516)   # a tail only, a 16-byte group only, one / two / three trips of the 256-column vector loop
TILE_N = (1, 255, 256, 257, 513)    # around the 256-row tiles of the scan


def _dense_base(rng, n, f):
    """rows that are distinct unless planted: for F < 8 there are too few columns for random values to keep rows apart, so a row
    carries its own index in column 0"""
    x = rng.standard_normal((n, f)).astype(np.float32)
    x[rng.random((n, f)) < 0.4] = 0.0
    x[:, 0] = 1000.0 + np.arange(n)
    return x


def special_columns(f):
    """columns in which a planted pair differs: first, last, the last column of the 16-byte loop, the first tail column, column 256"""
    cols = {0, f - 1}
    if f >= 4:
        cols.add((f & ~3) - 1)
    if f % 4:
        cols.add(f & ~3)
    if f >= 260:
        cols.add(256)
    return sorted(cols)


def dense_case(f, n=600):
    """-> (x [n, f] fp32, pairs that must NOT merge [(a, b)], pairs that must merge)"""
    rng = np.random.default_rng(1000 + f)
    x = _dense_base(rng, n, f)
    for i in rng.choice(np.arange(100, n), 260, replace=False):  # duplicates and chains of duplicates
        x[i] = x[rng.integers(0, n)]
    apart, same, row = [], [], 2
    for c in special_columns(f):                                  # equal but for one column
        x[row + 1] = x[row]
        x[row + 1, c] = x[row, c] + 1.0
        apart.append((row, row + 1))
        row += 2
    if f >= 2:                                                    # the same values, two columns swapped
        x[row, 0], x[row, f - 1] = 1.5, 2.5
        x[row + 1] = x[row]
        x[row + 1, 0], x[row + 1, f - 1] = 2.5, 1.5
        apart.append((row, row + 1))
        row += 2
    x[row, f // 2] = 0.0                                          # +0 / -0
    x[row + 1] = x[row]
    x[row + 1, f // 2] = -0.0
    same.append((row, row + 1))
    x[row + 2], x[row + 3] = 0.0, -0.0                            # all-zero rows of both signs
    same.append((row + 2, row + 3))
    x[row + 4, f - 1] = np.nan                                    # NaN rows: equal bits, never merged
    x[row + 5] = x[row + 4]
    apart.append((row + 4, row + 5))
    assert row + 5 < 60
    # a copy of the SECOND row of every pair that must stay apart: were the hash blind to what tells the pair apart, the copy's
    # candidate would be the pair's first row, the verify pass would reject it, and the copy would find no representative at all -
    # a hash that misses a column shows in `rep`, although the verify pass keeps it from merging different rows
    for k, (_a, b) in enumerate(apart[:-1]):
        x[60 + k] = x[b]
        same.append((b, 60 + k))
    return x, apart, same


def tile_edge_case(n, f=5):
    """duplicates across the edges of the 256-row tiles: row 256 = row 255, row 511 = row 256, row 512 = row 0"""
    rng = np.random.default_rng(2000 + n)
    x = _dense_base(rng, n, f)
    for i in rng.choice(n, n // 3, replace=False):
        x[i] = x[rng.integers(0, n)]
    for a, b in ((256, 255), (511, 256), (512, 0)):
        if a < n:
            x[a] = x[b]
    return x


def csr_arrays(rows):
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rowptr, np.concatenate([np.asarray(r, np.int32) for r in rows]).astype(np.int32)


def csr_case(m=400):
    """-> (rowptr, col, row_scale, pairs that must not merge in the pattern, pairs that must, named rows)"""
    rng = np.random.default_rng(31)
    rows = [np.sort(rng.choice(m, d, replace=False)) for d in rng.integers(1, 6, m)]
    scale = rng.choice(np.array([0.5, 0.25, 1.0], np.float32), m)
    for k, i in enumerate(rng.choice(np.arange(60, m), 180, replace=False)):
        j = rng.integers(0, m)
        rows[i] = rows[j]
        if k % 4:                                                 # (every fourth duplicate keeps a scale of its own)
            scale[i] = scale[j]
    hub = np.sort(rng.choice(m, 200, replace=False))
    spare = int(np.setdiff1d(np.arange(m), hub)[0])

    def hub_but(e):
        h = hub.copy()
        h[e] = spare
        return h

    named = {"empty": [7, 20, 59], "prefix": (10, 11), "order": (12, 13), "hub": 30, "hub_63": 31, "hub_64": 32, "hub_last": 33,
             "hub_copy": 34, "scale_zero": (40, 41), "scale_nan": (42, 43), "scale_differs": (44, 45)}
    for i in named["empty"]:
        rows[i] = np.zeros(0, np.int64)
    rows[10], rows[11] = np.array([3, 9, 20]), np.array([3, 9, 20, 31])
    rows[12], rows[13] = np.array([5, 8, 13]), np.array([8, 5, 13])
    rows[30], rows[31], rows[32], rows[33], rows[34] = hub, hub_but(63), hub_but(64), hub_but(199), hub.copy()
    for a, b in (named["scale_zero"], named["scale_nan"], named["scale_differs"]):
        rows[a] = rows[b] = np.array([a, a + 100, a + 200])
    scale[30:35] = 0.5
    scale[named["empty"]] = 1.0
    scale[[40, 41]] = 0.0, -0.0
    scale[[42, 43]] = np.nan
    scale[[44, 45]] = 0.5, 0.25
    apart = [named["prefix"], named["order"], (30, 31), (30, 32), (30, 33), (31, 32)]
    same = [(30, 34), (7, 20), (7, 59)]
    # a copy of the second row of the pairs that must stay apart (see dense_case: a hash blind to the difference shows in `rep`)
    for k, b in enumerate((11, 13, 31, 32, 33, 45)):
        rows[46 + k], scale[46 + k] = rows[b].copy(), scale[b]
        same.append((b, 46 + k))
    rowptr, col = csr_arrays(rows)
    return rowptr, col, scale, apart, same, named


def csr_values_case(m=400):
    """a graph whose stored values matter -> (rowptr, col, val, pairs apart WITH values that the pattern merges, pairs that merge)"""
    rng = np.random.default_rng(32)
    rows = [np.sort(rng.choice(m, d, replace=False)) for d in rng.integers(1, 6, m)]
    vals = [rng.choice(np.array([1.0, 2.0, 0.5], np.float32), len(r)) for r in rows]
    for i in rng.choice(np.arange(60, m), 170, replace=False):
        j = rng.integers(0, m)
        rows[i], vals[i] = rows[j], vals[j]
    hub = np.sort(rng.choice(m, 200, replace=False))
    hv = rng.choice(np.array([1.0, 2.0, 0.5], np.float32), 200)
    rows[10] = rows[11] = rows[12] = rows[13] = rows[14] = rows[15] = np.array([1, 50, 300])
    vals[10], vals[11] = np.float32([1, 2, 3]), np.float32([1, 2, 4])          # same columns, another value
    vals[12], vals[13] = np.float32([0.0, 2, 5]), np.float32([-0.0, 2, 5])     # +0 / -0
    vals[14], vals[15] = np.float32([np.nan, 2, 6]), np.float32([np.nan, 2, 6])
    rows[30], rows[31], rows[32], rows[33] = hub, hub, hub, hub
    vals[30], vals[31], vals[32], vals[33] = hv, hv.copy(), hv.copy(), hv.copy()
    vals[32][64] += 1.0                                                        # hub rows apart in one value behind the first 64
    vals[33][199] += 1.0
    apart = [(10, 11), (10, 12), (14, 15), (30, 32), (30, 33)]
    same = [(12, 13), (30, 31)]
    for k, b in enumerate((11, 32, 33)):                                       # copies of the second rows (see dense_case)
        rows[40 + k], vals[40 + k] = rows[b].copy(), vals[b].copy()
        same.append((b, 40 + k))
    rowptr, col = csr_arrays(rows)
    val = np.concatenate(vals).astype(np.float32)
    return rowptr, col, val, apart, same
