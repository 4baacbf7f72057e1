"""Reference and case builders for the aggregation Y = diag(r) A diag(c) X (tests/test_gpu_spmm_edges.py): plain numpy, no GPU.

The data is EXACT BY CONSTRUCTION: X holds integers in [-8, 8], stored values come from +-{0.25, 0.5, 1, 1.5, 2, 3}, column
scales from {0.5, 1, 2, 4}, row scales from +-2^k (k = -3 .. 3) and exact zeros.  Every term val * cs * x is then a multiple of
2^-3 of magnitude <= 96, and `make_case` asserts 8 * sum |term| < 2^24 for every row: every partial sum in every order is an
integer multiple of 2^-3 below 2^21, i.e. exact in fp32, and an fma equals a multiply followed by an add.  A kernel on any route
must therefore return `spmm64(...)` rounded to fp32 bit for bit; the same integers are exact in bf16.  held by tests/test_spmm_ref.py."""
import numpy as np

VAL_SET = np.array([0.25, 0.5, 1.0, 1.5, 2.0, 3.0, -0.25, -0.5, -1.0, -1.5, -2.0, -3.0], np.float32)
COL_SCALE_SET = np.array([0.5, 1.0, 2.0, 4.0], np.float32)
ROW_SCALE_SET = np.array([s * 2.0 ** k for k in range(-3, 4) for s in (1, -1)] + [0.0, 0.0], np.float32)
EXACT_LIMIT = float(1 << 24)

# the four ways every case runs: (use_values, row scale, column scale)
WAYS = [(True, False, False), (False, True, False), (False, True, True), (True, True, True)]
WAY_IDS = ["val", "pat-rs", "pat-rs-cs", "val-rs-cs"]

# designed row lengths: both sides of every length the kernels branch on
SLAB_LENS = [0, 0, 1, 3, 4, 5, 8, 9]                                                # the EPI = 4 steps of aggregate_rows, empty rows
GATHER_LENS = list(range(10))                                                       # the unroll of 4 and its tail
QUAD_SPLIT_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128]              # chunks of 16, pieces of 32, split form <= 128
QUAD_LONG_LENS = [129, 160]                                                         # one row more than 128: not split
QUAD_COL_BOUNDS = [2528, 2529, 5056, 5057, 10112]                                   # one block / half slab / two blocks / four
BAND_LENS = [0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32]                         # batches of B_NB = 8, the nb - i == 2 branch
NARROW_LENS = [0, 1, 15, 16, 17, 63, 64, 65, 128, 129, 255, 256, 257, 2048, 2049, 2100]  # three row classes, the 4 G unrolls
NARROW_BATCHED_LENS = list(range(71))


def spmm64(rowptr, col, val, x, row_scale, col_scale):
    """Y[i] = rs[i] * sum over the stored entries p of row i, in stored order, duplicates included, of val[p] * cs[col[p]] * x[col[p]]
    in fp64 -> fp64 [n_rows, F].  val / row_scale / col_scale may each be None (= 1)."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    x = np.asarray(x, np.float64)
    n_rows = rowptr.shape[0] - 1
    y = np.zeros((n_rows, x.shape[1]), np.float64)
    w = np.ones(col.shape[0], np.float64) if val is None else np.asarray(val, np.float64).copy()
    if col_scale is not None:
        with np.errstate(invalid="ignore"):
            w = w * np.asarray(col_scale, np.float64)[col]
    rows = np.repeat(np.arange(n_rows), np.diff(rowptr))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, col.shape[0], 8192):  # (np.add.at adds entry after entry, in stored order)
            b = min(a + 8192, col.shape[0])
            np.add.at(y, rows[a:b], w[a:b, None] * x[col[a:b]])
        if row_scale is not None:
            y = np.asarray(row_scale, np.float64)[:, None] * y
    return y


def dense64(rowptr, col, val, x, row_scale, col_scale):
    """the same product through the scattered dense matrix (duplicates summed) - an independent statement of spmm64"""
    n_rows, n_cols = len(rowptr) - 1, x.shape[0]
    a = np.zeros((n_rows, n_cols), np.float64)
    rows = np.repeat(np.arange(n_rows), np.diff(rowptr))
    np.add.at(a, (rows, np.asarray(col, np.int64)), 1.0 if val is None else np.asarray(val, np.float64))
    if col_scale is not None:
        a = a * np.asarray(col_scale, np.float64)[None, :]
    y = a @ np.asarray(x, np.float64)
    return y if row_scale is None else np.asarray(row_scale, np.float64)[:, None] * y


def seq32(rowptr, col, val, x, row_scale, col_scale, rng):
    """fp32 sequential sum of every row's terms in a RANDOM order (a multiply and an add per term, fp32 throughout)"""
    n_rows = len(rowptr) - 1
    x = np.asarray(x, np.float32)
    y = np.zeros((n_rows, x.shape[1]), np.float32)
    for i in range(n_rows):
        acc = np.zeros(x.shape[1], np.float32)
        for p in rng.permutation(np.arange(rowptr[i], rowptr[i + 1])):
            w = np.float32(1.0) if val is None else np.float32(val[p])
            if col_scale is not None:
                w = np.float32(w * np.float32(col_scale[col[p]]))
            acc = (acc + w * x[col[p]]).astype(np.float32)
        y[i] = acc if row_scale is None else np.float32(row_scale[i]) * acc
    return y


def classes(y):
    """per element: 0 finite, 1 NaN, 2 +inf, 3 -inf"""
    y = np.asarray(y)
    return np.where(np.isnan(y), 1, np.where(np.isposinf(y), 2, np.where(np.isneginf(y), 3, 0))).astype(np.int8)


def cycle(seq, n):
    """n row lengths cycling through seq"""
    return [seq[i % len(seq)] for i in range(n)]


def slab_lengths(n_rows):
    """SLAB_LENS cycled, with a run of 40 empty rows in the middle and at the end"""
    lens = np.array(cycle(SLAB_LENS, n_rows))
    if n_rows >= 120:
        lens[n_rows // 2:n_rows // 2 + 40] = 0
        lens[-40:] = 0
    return lens.tolist()


def make_case(rng, lens, n_cols, n_feat, cols_of_row=None):
    """A case with the given row lengths: sorted, unique columns per row (cols_of_row(i, length) -> columns overrides the random
    choice), values, scales and X from the exact sets.  -> dict(rowptr, col, val, x, rs, cs, n_rows, n_cols, n_feat)"""
    lens = np.asarray(lens, np.int64)
    n_rows = len(lens)
    assert lens.max(initial=0) <= n_cols, "a row of unique columns cannot be longer than n_cols"
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.empty(int(rowptr[-1]), np.int32)
    for i, k in enumerate(lens):
        c = None if cols_of_row is None else cols_of_row(i, int(k))
        if c is None:
            c = rng.choice(n_cols, int(k), replace=False) if k < n_cols else np.arange(n_cols)
        col[rowptr[i]:rowptr[i + 1]] = np.sort(np.asarray(c, np.int64))
    case = dict(rowptr=rowptr, col=col, val=rng.choice(VAL_SET, col.shape[0]).astype(np.float32),
                x=rng.integers(-8, 9, (n_cols, n_feat)).astype(np.float32), rs=rng.choice(ROW_SCALE_SET, n_rows).astype(np.float32),
                cs=rng.choice(COL_SCALE_SET, n_cols).astype(np.float32), n_rows=n_rows, n_cols=n_cols, n_feat=n_feat)
    assert_exact(case)
    return case


def term_bound(case):
    """per row: 8 * the largest (over the features and the four ways) sum of |term|"""
    rowptr, col = case["rowptr"], case["col"].astype(np.int64)
    w = np.maximum(np.abs(case["val"].astype(np.float64)), 1.0) * case["cs"].astype(np.float64)[col]  # (pattern-only ways: |val| = 1)
    w = np.maximum(w, np.maximum(np.abs(case["val"].astype(np.float64)), 1.0))                          # (ways without the column scale)
    out = np.zeros(case["n_rows"])
    if col.shape[0] and case["n_feat"]:
        xmax = np.abs(case["x"].astype(np.float64)).max(1)
        np.add.at(out, np.repeat(np.arange(case["n_rows"]), np.diff(rowptr)), w * xmax[col])
    return 8.0 * out


def assert_exact(case):
    """the builder's word: members of the exact sets only, no stored zero, and every row's sums exact in fp32 in any order"""
    assert np.isin(case["val"], VAL_SET).all() and np.isin(case["cs"], COL_SCALE_SET).all() and np.isin(case["rs"], ROW_SCALE_SET).all()
    assert (case["x"] == np.round(case["x"])).all() and np.abs(case["x"]).max(initial=0) <= 8
    assert case["col"].min(initial=0) >= 0 and case["col"].max(initial=-1) < max(case["n_cols"], 1)
    bound = term_bound(case)
    assert (bound < EXACT_LIMIT).all(), f"row {int(bound.argmax())}: 8 * sum |term| = {bound.max():.0f} >= 2^24"


def way_args(case, way):
    """(val, row_scale, col_scale) of one of WAYS"""
    use_values, rs, cs = way
    return case["val"] if use_values else None, case["rs"] if rs else None, case["cs"] if cs else None


def reference(case, way):
    val, rs, cs = way_args(case, way)
    return spmm64(case["rowptr"], case["col"], val, case["x"], rs, cs)


def reorder(case, mode, rng=None):
    """the same case with every row's entries stored "sorted" / "reversed" / "shuffled" (col and val move together)"""
    out = dict(case)
    col, val = case["col"].copy(), case["val"].copy()
    rp = case["rowptr"]
    for i in range(case["n_rows"]):
        a, b = int(rp[i]), int(rp[i + 1])
        if mode == "sorted":
            o = np.argsort(col[a:b], kind="stable")
        elif mode == "reversed":
            o = np.argsort(col[a:b], kind="stable")[::-1]
        else:
            o = rng.permutation(b - a)
        col[a:b], val[a:b] = col[a:b][o], val[a:b][o]
    out["col"], out["val"] = col, val
    return out


def with_duplicates(case, rng, fat_row=None, copies=40):
    """every third entry stored twice (the copy's value differs), the copies next to the original in a sorted row; fat_row: that row
    is replaced by ONE column stored `copies` times"""
    rp, col, val = case["rowptr"], case["col"], case["val"]
    new_col, new_val, lens = [], [], []
    for i in range(case["n_rows"]):
        a, b = int(rp[i]), int(rp[i + 1])
        if i == fat_row:
            c = np.full(copies, int(rng.integers(case["n_cols"])), np.int32)
            v = rng.choice(VAL_SET, copies).astype(np.float32)
        else:
            twice = np.arange(a, b)[(np.arange(a, b) % 3) == 0]
            c = np.concatenate([col[a:b], col[twice]])
            nxt = VAL_SET[(np.argmax(val[twice][:, None] == VAL_SET[None, :], axis=1) + 1) % len(VAL_SET)]  # the set's next member
            v = np.concatenate([val[a:b], nxt]).astype(np.float32)
            o = np.argsort(c, kind="stable")
            c, v = c[o], v[o]
        new_col.append(c)
        new_val.append(v)
        lens.append(len(c))
    out = dict(case)
    out["rowptr"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    out["col"] = np.concatenate(new_col).astype(np.int32) if new_col else col
    out["val"] = np.concatenate(new_val).astype(np.float32) if new_val else val
    assert_exact(out)
    return out


def poison(case):
    """B: X rows NaN (row 0), +inf (the last) and -inf (the middle one); one stored value inf, one row scale NaN, one column
    scale inf.  Stored values stay non-zero.  The case is no longer exact where these reach; `classes` of the reference says where."""
    out = dict(case)
    x, val, rs, cs = case["x"].copy(), case["val"].copy(), case["rs"].copy(), case["cs"].copy()
    m = case["n_cols"]
    if m:
        x[0] = np.nan
        x[m - 1] = np.inf
        x[m // 2] = -np.inf
        cs[m // 3] = np.inf
    if val.shape[0]:
        val[val.shape[0] // 2] = np.inf
    if rs.shape[0]:
        rs[rs.shape[0] // 2] = np.nan
    out.update(x=x, val=val, rs=rs, cs=cs)
    return out


def block_columns(n_cols, block_cols):
    """first and last column of every column block of block_cols columns"""
    out = []
    for b in range(0, n_cols, block_cols):
        out += [b, min(b + block_cols, n_cols) - 1]
    return sorted(set(out))


# ------------------------------------------------------------------------------------------- the cases of section A, route by route
def _offset_cycle(seq, n, start=3):
    """n lengths cycling through seq from position `start` (a one-row graph then has entries)"""
    return [seq[(i + start) % len(seq)] for i in range(n)]


def slab_case(seed=1, n_feat=35):
    return make_case(np.random.default_rng(seed), slab_lengths(1100), 300, n_feat)


def gather_case(n_feat, seed=2):
    return make_case(np.random.default_rng(seed + n_feat), cycle(GATHER_LENS, 50), 60, n_feat)


def quad_case(n_rows, n_feat, long_row=None, seed=3):
    """one column block of 160 columns; long_row: one row of that many entries (> 128: the graph is not in split form)"""
    lens = _offset_cycle(QUAD_SPLIT_LENS, n_rows)
    if long_row is not None:
        lens[n_rows // 2] = long_row
    return make_case(np.random.default_rng(seed + 7 * n_rows + n_feat), lens, 160, n_feat)


def sell16_block_cols(n_cols):
    """columns per block of the SELL-16 copy as include/wdg.h states it: the fewest blocks of <= 2528 columns, evenly, a multiple of
    4; 2529 .. 5056 columns: ONE block (half slabs).  The GPU tests compare it with wdg_sell16_block_cols."""
    if 2528 < n_cols <= 5056:
        return (n_cols + 3) & ~3
    blocks = -(-max(n_cols, 1) // 2528)
    return min((-(-max(n_cols, 1) // blocks) + 3) & ~3, 2528)


def quad_wide_case(n_rows, n_cols, n_feat, seed=4):
    """several column blocks or a half slab: every row has an entry in the first and the last column of every block (of the copy's
    own block width and of 2528, the width of an LDS slab), every fifth row ONLY entries of one block"""
    rng = np.random.default_rng(seed + n_cols + n_rows + n_feat)
    widths = sorted({2528, sell16_block_cols(n_cols)})
    edges = sorted({c for w in widths for c in block_columns(n_cols, w)})

    def cols(i, k):
        if i % 5 == 4:  # one block only: columns of block (i // 5) % n_blocks
            w = sell16_block_cols(n_cols)
            b = (i // 5) % -(-n_cols // w)
            lo, hi = b * w, min((b + 1) * w, n_cols)
            return rng.choice(np.arange(lo, hi), k, replace=False)
        rest = np.setdiff1d(np.arange(n_cols), edges)
        return np.concatenate([edges, rng.choice(rest, k - len(edges), replace=False)])

    lens = [(6 if i % 5 == 4 else len(edges) + (i % 7)) for i in range(n_rows)]
    return make_case(rng, lens, n_cols, n_feat, cols)


def quad_unsorted_case(n_rows, seed=5):
    """more than Q_SORT_MAX_ROWS = 16384 rows take the unsorted SELL-16 layout at 16385; lengths cycle 0 .. 5, row 16384 (where
    there is one) has all 40 columns"""
    lens = cycle([0, 1, 2, 3, 4, 5], n_rows)
    if n_rows > 16384:
        lens[16384] = 40
    return make_case(np.random.default_rng(seed + n_rows), lens, 40, 16)


def band_case(n_rows, n_feat, hub_len=None, seed=6):
    """400 columns; BAND_LENS from a position that gives a one-row graph entries; hub_len: rows of exactly hub_len, hub_len + 1,
    hub_len + 8 and 400 entries on top (n_rows >= 8)"""
    lens = _offset_cycle(BAND_LENS, n_rows, start=4)
    if hub_len is not None and n_rows >= 8:
        for k, length in enumerate((hub_len, hub_len + 1, hub_len + 8, 400)):
            lens[1 + 2 * k] = min(length, 400)
    return make_case(np.random.default_rng(seed + n_rows + n_feat), lens, 400, n_feat)


def band_large_case(seed=7):
    """16400 short rows: more than the in-LDS row sort takes (the bucket-sort plan)"""
    return make_case(np.random.default_rng(seed), cycle([0, 1, 2, 3, 9, 4], 16400), 400, 16)


def narrow_case(n_feat, seed=8):
    """2100 columns, 40 rows: NARROW_LENS, then rows whose entries all fall into ONE eighth of the columns and rows with none in the
    first half (the column parts of WDG_NARROW_PARTS = 2, 4, 8)"""
    rng = np.random.default_rng(seed + n_feat)
    lens = NARROW_LENS + [20] * 8 + [33] * 8 + cycle([3, 70, 130, 0], 8)
    eighth = -(-2100 // 8)

    def cols(i, k):
        if 16 <= i < 24:  # all in eighth i - 16
            lo = (i - 16) * eighth
            return rng.choice(np.arange(lo, min(lo + eighth, 2100)), k, replace=False)
        if 24 <= i < 32:  # none in the first half
            return rng.choice(np.arange(1050, 2100), k, replace=False)
        return None

    assert len(lens) == 40
    return make_case(rng, lens, 2100, n_feat, cols)


def narrow_batched_cases(n_feat, seed=9):
    """four jobs of 1, 16, 17 and 300 rows, row lengths 0 .. 70"""
    out = []
    for n in (1, 16, 17, 300):
        rng = np.random.default_rng(seed + n + 31 * n_feat)
        out.append(make_case(rng, _offset_cycle(NARROW_BATCHED_LENS, n, start=5 if n == 1 else 0), max(n, 80), n_feat))
    return out


def quad_batched_cases(n_feat, n_cols=160, seed=10):
    """six graphs of 1, 16, 17, 64, 65 and 300 rows over the same n_cols (the first three share one X: the caller passes case 0's)"""
    out = []
    for n in (1, 16, 17, 64, 65, 300):
        if n_cols > 2528:
            out.append(quad_wide_case(n, n_cols, n_feat, seed + n))
        else:
            out.append(make_case(np.random.default_rng(seed + n + n_feat), _offset_cycle(QUAD_SPLIT_LENS[:8], n), n_cols, n_feat))
    for c in out[1:3]:
        c["x"] = out[0]["x"]
        assert_exact(c)
    return out


def empty_case(n_rows, n_cols, n_feat, seed=11):
    return make_case(np.random.default_rng(seed), [0] * n_rows, n_cols, n_feat)


def small_case_lists():
    """name -> case for the CPU tests of the builders (tests/test_spmm_ref.py): one case of every builder"""
    return {"slab": slab_case(), "gather": gather_case(17), "quad": quad_case(130, 9), "quad-long": quad_case(65, 8, 160),
            "quad-half": quad_wide_case(70, 2529, 8), "quad-multi": quad_wide_case(70, 5057, 16), "quad-unsorted": quad_unsorted_case(16385),
            "band": band_case(300, 65, 40), "narrow": narrow_case(5), "narrow-batched": narrow_batched_cases(5)[3],
            "quad-batched": quad_batched_cases(20)[5]}
