"""tests/_spmm_ref.py held to its word (no GPU): the reference equals a dense fp64 product, the built data is exact in fp32 in any
order, the designed row lengths contain the lengths the kernels branch on, and the non-finite classes do not depend on the order."""
import numpy as np
import pytest

import _spmm_ref as R


@pytest.fixture(scope="module")
def cases():
    return R.small_case_lists()


NAMES = ["slab", "gather", "quad", "quad-long", "quad-half", "quad-multi", "quad-unsorted", "band", "narrow", "narrow-batched", "quad-batched"]


def test_case_list_is_complete(cases):
    assert sorted(cases) == sorted(NAMES)


@pytest.mark.parametrize("name", [n for n in NAMES if n != "quad-unsorted"])  # (16385 x 40 dense: the row-wise test below covers it)
@pytest.mark.parametrize("way", R.WAYS, ids=R.WAY_IDS)
def test_spmm64_equals_the_dense_product(cases, name, way):
    c = cases[name]
    val, rs, cs = R.way_args(c, way)
    np.testing.assert_array_equal(R.reference(c, way), R.dense64(c["rowptr"], c["col"], val, c["x"], rs, cs))


def test_spmm64_sums_duplicates_and_takes_any_order(cases):
    rng = np.random.default_rng(0)
    c = R.with_duplicates(cases["quad"], rng, fat_row=3)
    lens = np.diff(c["rowptr"])
    assert lens[3] == 40 and len(set(c["col"][c["rowptr"][3]:c["rowptr"][4]].tolist())) == 1
    assert c["col"].shape[0] >= cases["quad"]["col"].shape[0] * 4 // 3 - 130  # a third of the entries stored twice
    i = int(np.argmax(lens))
    a, b = int(c["rowptr"][i]), int(c["rowptr"][i + 1])
    dup = c["col"][a:b][1:] == c["col"][a:b][:-1]
    assert dup.any() and (c["val"][a:b][1:][dup] != c["val"][a:b][:-1][dup]).all()  # the copies carry other values
    for way in R.WAYS:
        val, rs, cs = R.way_args(c, way)
        want = R.dense64(c["rowptr"], c["col"], val, c["x"], rs, cs)
        for mode in ("sorted", "reversed", "shuffled"):
            d = R.reorder(c, mode, rng)
            assert sorted(zip(d["col"][a:b].tolist(), d["val"][a:b].tolist())) == sorted(zip(c["col"][a:b].tolist(), c["val"][a:b].tolist()))
            np.testing.assert_array_equal(R.reference(d, way), want)
    r = R.reorder(cases["quad"], "reversed")
    a, b = int(r["rowptr"][5]), int(r["rowptr"][6])
    assert b - a > 1 and (np.diff(r["col"][a:b]) < 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_fp32_sums_in_three_random_orders_equal_the_reference(cases, name):
    """what makes assert_array_equal the right comparison for EVERY kernel: any order of an fp32 sum gives the same bits"""
    c = cases[name]
    assert (R.term_bound(c) < R.EXACT_LIMIT).all()
    ways = R.WAYS if c["col"].shape[0] < 12000 else R.WAYS[3:]
    if c["col"].shape[0] >= 12000:  # the large cases: the 300 longest rows and 300 others
        lens = np.diff(c["rowptr"])
        pick = np.unique(np.concatenate([np.argsort(-lens, kind="stable")[:300], np.arange(0, c["n_rows"], max(1, c["n_rows"] // 300))]))
        rp = np.concatenate([[0], np.cumsum(lens[pick])])
        idx = np.concatenate([np.arange(c["rowptr"][i], c["rowptr"][i + 1]) for i in pick]).astype(np.int64)
        c = dict(c, rowptr=rp, col=c["col"][idx], val=c["val"][idx], rs=c["rs"][pick], n_rows=len(pick))
    for way in ways:
        val, rs, cs = R.way_args(c, way)
        want = R.reference(c, way)
        assert np.isfinite(want).all()
        np.testing.assert_array_equal(want.astype(np.float32).astype(np.float64), want)  # representable: the cast rounds nothing
        for seed in range(3):
            got = R.seq32(c["rowptr"], c["col"], val, c["x"], rs, cs, np.random.default_rng(seed))
            np.testing.assert_array_equal(got, want.astype(np.float32))


def test_the_builder_refuses_a_row_that_could_round():
    rng = np.random.default_rng(0)
    c = R.make_case(rng, [2100], 2100, 4)
    assert R.term_bound(c).max() < R.EXACT_LIMIT
    c["x"] = c["x"] * 64  # 2100 entries of up to 3 * 4 * 512: past 2^24 / 8
    with pytest.raises(AssertionError):
        R.assert_exact(c)
    c = R.make_case(rng, [5], 9, 4)
    c["val"][2] = 0.0
    with pytest.raises(AssertionError):
        R.assert_exact(c)


def _has(lens, wanted):
    missing = sorted(set(wanted) - set(int(v) for v in lens))
    assert not missing, f"row lengths {missing} are not in the case"


def test_designed_row_lengths_contain_the_boundaries():
    # slab: consecutive rows of a lane group with empty rows inside and at its end (1100 rows: SLAB = 4 -> 512 or 1024 groups own 3 or 2 rows)
    lens = np.diff(R.slab_case()["rowptr"])
    _has(lens, [0, 1, 3, 4, 5, 8, 9])
    assert (lens[550:590] == 0).all() and (lens[-40:] == 0).all() and lens[549] > 0 and -(-1100 // 512) == 3
    # SLAB = 4, 512 threads: a lane group owns three consecutive rows - runs that end in empty rows, runs that begin with them, and
    # (SLAB = 32, 64 groups of 18 rows) runs with empty rows between rows that have entries
    assert any(lens[i] > 0 and lens[i + 1] == 0 and lens[i + 2] == 0 for i in range(0, 300, 3))
    assert any(lens[i] == 0 and lens[i + 1] == 0 and lens[i + 2] > 0 for i in range(0, 300, 3))
    assert any(lens[i] > 0 and lens[i + 1] > 0 and lens[i + 2] == 0 for i in range(0, 300, 3))
    assert any((lens[i + 1:i + 17] == 0).any() and lens[i:i + 2].max() > 0 and lens[i + 16:i + 18].max() > 0 for i in range(0, 540, 18))
    # gather: the unroll of 4 and its tail
    _has(np.diff(R.gather_case(7)["rowptr"]), range(10))
    # quad: chunks of 16, pieces of 32, the split form's 128 and one past it
    for n in (15, 16, 17, 63, 64, 65, 130):
        _has(np.diff(R.quad_case(n, 8)["rowptr"]), R.QUAD_SPLIT_LENS)
    for k in (16, 17, 32, 33, 64, 65, 128):
        assert k in R.QUAD_SPLIT_LENS and k - 1 in R.QUAD_SPLIT_LENS
    assert np.diff(R.quad_case(1, 8)["rowptr"])[0] > 0
    for long_row in R.QUAD_LONG_LENS:
        lens = np.diff(R.quad_case(64, 8, long_row)["rowptr"])
        assert lens.max() == long_row > 128 and np.sort(lens)[-2] <= 128
    # quad, wide: every row but the one-block rows touches the first and the last column of every block; some rows stay in one block
    for n_cols in R.QUAD_COL_BOUNDS:
        c = R.quad_wide_case(70, n_cols, 8)
        w = R.sell16_block_cols(n_cols)
        edges = sorted(set(R.block_columns(n_cols, 2528) + R.block_columns(n_cols, w)))
        one_block = 0
        for i in range(70):
            cols = c["col"][c["rowptr"][i]:c["rowptr"][i + 1]]
            if i % 5 == 4:
                one_block += len(set((cols // w).tolist())) == 1
            else:
                assert np.isin(edges, cols).all()
        assert one_block == 14 and c["col"].max() == n_cols - 1 and c["col"].min() == 0
    assert [R.sell16_block_cols(m) for m in (160, 2528, 2529, 5056, 5057, 10112)] == [160, 2528, 2532, 5056, 1688, 2528]
    assert [2528, 2529] == R.QUAD_COL_BOUNDS[:2] and 5056 in R.QUAD_COL_BOUNDS and 5057 in R.QUAD_COL_BOUNDS
    # quad, unsorted layout: both sides of 16384 rows, the long row behind the boundary
    lens = np.diff(R.quad_unsorted_case(16385)["rowptr"])
    assert len(lens) == 16385 and lens[16384] == 40 and set(lens[:16384].tolist()) == {0, 1, 2, 3, 4, 5}
    assert len(np.diff(R.quad_unsorted_case(16384)["rowptr"])) == 16384
    # band: batches of 8 (B_NB), both sides; hub rows of hub_len, hub_len + 1, hub_len + 8 and all 400 columns
    _has(np.diff(R.band_case(300, 16)["rowptr"]), R.BAND_LENS)
    for k in (8, 16, 24, 32):
        assert k in R.BAND_LENS and k - 1 in R.BAND_LENS and (k + 1 in R.BAND_LENS or k == 32)
    _has(np.diff(R.band_case(300, 16, 37)["rowptr"]), [37, 38, 45, 400])
    assert np.diff(R.band_case(1, 16)["rowptr"])[0] > 0 and np.diff(R.band_large_case()["rowptr"]).shape[0] > 16384
    # narrow: 16 lanes / a wave / a workgroup per row: 128 | 129, 2048 | 2049; the 4 G unrolls at 64 | 65, 256 | 257
    c = R.narrow_case(5)
    lens = np.diff(c["rowptr"])
    _has(lens, R.NARROW_LENS)
    for k in (16, 64, 128, 256, 2048):
        assert k in R.NARROW_LENS and k + 1 in R.NARROW_LENS
    for i in range(16, 24):  # all in one eighth of the columns
        cols = c["col"][c["rowptr"][i]:c["rowptr"][i + 1]]
        assert len(set((cols // 263).tolist())) == 1 and cols[0] // 263 == i - 16
    for i in range(24, 32):  # none in the first part of 2, 4 or 8
        assert c["col"][c["rowptr"][i]] >= 1050
    for job in R.narrow_batched_cases(3):
        assert np.diff(job["rowptr"]).max() <= 70
    _has(np.diff(R.narrow_batched_cases(3)[3]["rowptr"]), range(71))
    assert [j["n_rows"] for j in R.quad_batched_cases(20)] == [1, 16, 17, 64, 65, 300]


@pytest.mark.parametrize("name", ["slab", "quad", "band", "narrow"])
def test_non_finite_classes_do_not_depend_on_the_order(cases, name):
    rng = np.random.default_rng(5)
    c = R.poison(cases[name])
    assert (c["val"] != 0).all()
    for way in R.WAYS:
        want = R.reference(c, way)
        cls = R.classes(want)
        assert (cls == 1).any() and (cls == 0).any()
        for mode in ("reversed", "shuffled", "shuffled"):
            got = R.reference(R.reorder(c, mode, rng), way)
            np.testing.assert_array_equal(R.classes(got), cls)
            np.testing.assert_array_equal(got[cls == 0], want[cls == 0])
        # a row that references none of the poisoned columns, values or scales is exactly the clean case's row
        clean = R.reference(cases[name], way)
        val, rs, cs = R.way_args(c, way)
        bad_col = ~np.isfinite(c["x"]).all(1) | (~np.isfinite(c["cs"]) if cs is not None else False)
        bad_entry = bad_col[c["col"]] | (~np.isfinite(c["val"]) if val is not None else False)
        rows = np.repeat(np.arange(c["n_rows"]), np.diff(c["rowptr"]))
        bad_row = np.bincount(rows, bad_entry, c["n_rows"]) > 0
        if rs is not None:
            bad_row |= ~np.isfinite(c["rs"])
        assert (~bad_row).any() and bad_row.any()
        np.testing.assert_array_equal(want[~bad_row], clean[~bad_row])
        assert (cls[bad_row] != 0).any(axis=1).all() or c["n_feat"] == 0
