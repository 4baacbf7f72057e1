"""Every GEMM kernel path of csrc/gemm.hip with EXACT products at its edges: gemm_f32_kernel in both column-tile widths, with and
without transb, alone, as a job table and as the partial products of split-K with gemm_splitk_reduce; gemm_bres_kernel; the four
skinny kernels (1 / 4 / 16 lanes per row and the wave per row); mlp2_split_kernel (row-major and tiled A) and mlp2_bres_kernel.

The data of tests/_gemm_ref.py is exact in fp32 in any summation order (tests/test_gemm_ref.py holds that), so every comparison
here is np.testing.assert_array_equal against the fp64 reference: no tolerance.  Every launch reads A and B through column slices
of wider buffers whose padding floats are NaN (lda = K + 4 where the route wants lda % 4 == 0, an odd pad elsewhere; ldb > N, or
> K under transb) and writes C into the interior of a buffer filled with the sentinel 7.0, C itself pre-filled with NaN: afterwards
the frame is intact and C holds no NaN.  Every case runs four ways (plain / bias / relu / bias + relu) and twice, and asserts the
route it took with wdg_gemm_resident_eligible, wdg_gemm_skinny_lanes, wdg_gemm_splitk_plan and the environment switches.
Sections: A exact products per kernel, B job tables, C split-K and its workspace, D the fused two-layer transform, E non-finite
inputs, F the empty sum K = 0 and refusals.

What the cases found: (1) ops.gemm / ops.gemm_skinny made a contiguous copy of every operand that was a column slice, so no
leading dimension other than the row length ever reached wdg_gemm_f32 / wdg_gemm_skinny_f32 through them (the "lda = K + pad" of
tests/test_gpu_configs.py::test_skinny_gemm_against_the_oracle was such a copy) - they now pass a matrix with contiguous rows as
it is.  (2) K = 0 was refused as "null matrix" - it is the empty sum now, act(bias), with A and B allowed to be NULL.  (3) the
GEMM epilogues' relu was fmaxf(v, 0), which turns a NaN into 0: a NaN in A left its row of C looking finite under relu - the
epilogues keep the NaN now (torch.relu's rule), section E asserts it in all four ways."""
import ctypes

import numpy as np
import pytest
import torch

import _gemm_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from wdg_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    """a kernel fault poisons the process: end the session there instead of starting the remaining tests on a faulted device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported a fault, no further test is started: {e}", returncode=3)


def _lib():
    from wdg_amd._lib import lib
    return lib


# ------------------------------------------------------------------------------------------- operands and checks
def _view(x, pad):
    """x [r, c] on the device as the leading columns of a buffer of c + pad columns whose other floats are NaN"""
    x = np.ascontiguousarray(x, np.float32)
    r, c = x.shape
    buf = torch.full((max(r, 1), c + pad), NAN, dtype=torch.float32, device="cuda")
    if x.size:
        buf[:r, :c] = torch.from_numpy(x).cuda()
    return buf[:r, :c]


def _vec(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def _cbuf(m, n, off=3, tail=4):
    """(buffer, C): C = rows 1 .. m and columns off .. off + n of a sentinel-filled buffer, pre-filled with NaN"""
    buf = torch.full((m + 2, off + n + tail), SENTINEL, dtype=torch.float32, device="cuda")
    c = buf[1:m + 1, off:off + n]
    c.fill_(NAN)
    return buf, c


def _same(got, want64, poisoned=False):
    with np.errstate(over="ignore", invalid="ignore"):
        want = want64.astype(np.float32)
    if not poisoned:
        assert np.isfinite(want64).all()
        np.testing.assert_array_equal(got, want)  # (a NaN left in C fails here: the reference has none)
        return
    cls = R.classes(want64)
    np.testing.assert_array_equal(R.classes(got), cls)
    np.testing.assert_array_equal(got[cls == 0], want[cls == 0])


def _check(buf, c, want64, poisoned=False):
    """every sentinel intact, C equal to the reference; C is NaN again afterwards"""
    torch.cuda.synchronize()
    got = c.cpu().numpy().copy()
    c.fill_(SENTINEL)
    assert bool((buf == SENTINEL).all()), "a write beside C"
    c.fill_(NAN)
    _same(got, want64, poisoned)
    return got


def _operands(case, transb=False, a_pad=3, b_pad=5):
    b = case["b"].T if transb else case["b"]
    return _view(case["a"], a_pad), _view(b, b_pad), _vec(case["bias"])


def _four_ways(call, case, want=None, poisoned=False):
    """call(bias, relu, out) four ways, each twice into the same NaN-filled C: both runs equal the reference (and so each other).
    -> {way: C as numpy}"""
    out = {}
    buf, c = _cbuf(case["m"], case["n"])
    for way in R.WAYS:
        ref = R.reference(case, way) if want is None else want(way)
        for _run in range(2):
            call(way[0], way[1], c)
            got = _check(buf, c, ref, poisoned)
            if way in out:
                assert got.tobytes() == out[way].tobytes(), "two runs differ"
            out[way] = got
    return out


def _gemm_call(ops, a, b, bias, transb=False):
    def call(use_bias, relu, out):
        assert ops.gemm(a, b, bias=bias if use_bias else None, relu=relu, transb=transb, out=out) is out
    return call


def _route(monkeypatch, kernel, splits=1):
    """the environment that sends ops.gemm to one kernel"""
    for env in ("WDG_GEMM_TILE", "WDG_GEMM_RESIDENT"):
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setenv({"tile": "WDG_GEMM_TILE", "resident": "WDG_GEMM_RESIDENT"}[kernel], "1")
    monkeypatch.setenv("WDG_GEMM_SPLITK", str(splits))


def _assert_route(kernel, m, n, k, splits=1, n_jobs=1):
    lib = _lib()
    assert int(lib.wdg_gemm_splitk_plan(m, n, k)) == splits
    assert bool(lib.wdg_gemm_resident_eligible(n_jobs, m, n, k)) == (kernel == "resident")


# =========================================================================================== A. exact products per kernel
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("transb", [False, True], ids=["b", "transb"])
def test_tile_kernel_pairwise_cover(ops, monkeypatch, transb, family):
    """gemm_f32_kernel<1 | 2, transb>: one and two column blocks of both widths, ragged rows and columns, K on both sides of the
    16-wide K step and K = 0; A with an odd pad, B with ldb = N + 5 (K + 5 under transb)"""
    _route(monkeypatch, "tile")
    for m, n, k in R.TILE_SHAPES:
        _assert_route("tile", m, n, k)
        case = R.make_case(family, m, n, k)
        a, b, bias = _operands(case, transb)
        assert tuple(b.shape) == ((n, k) if transb else (k, n))
        _four_ways(_gemm_call(ops, a, b, bias, transb), case)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_resident_kernel_pairwise_cover_has_the_tile_kernels_bits(ops, monkeypatch, family):
    """gemm_bres_kernel<1 | 2>: K without a whole group of 32, one group, odd and even group counts, a leftover, the LDS limit;
    M = 513 is two row parts.  The same operands through the tile kernel give the same bits (both are the reference's)."""
    for m, n, k in R.BRES_SHAPES:
        case = R.make_case(family, m, n, k)
        a, b, bias = _operands(case, a_pad=4)
        assert a.data_ptr() % 16 == 0 and a.stride(0) % 4 == 0 and a.stride(0) == k + 4
        _route(monkeypatch, "resident")
        _assert_route("resident", m, n, k)
        res = _four_ways(_gemm_call(ops, a, b, bias), case)
        _route(monkeypatch, "tile")
        _assert_route("tile", m, n, k)
        tile = _four_ways(_gemm_call(ops, a, b, bias), case)
        for way in R.WAYS:
            assert res[way].tobytes() == tile[way].tobytes()


@pytest.mark.parametrize("k", R.BRES_K_REFUSED)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_resident_kernel_declines_and_the_tile_kernel_answers(ops, monkeypatch, family, k):
    """K = 516 does not fit the LDS, K = 6 is no whole float4s: not eligible whatever WDG_GEMM_RESIDENT says, same bits"""
    for m, n in [(513, 64), (33, 33)]:
        case = R.make_case(family, m, n, k)
        a, b, bias = _operands(case, a_pad=4)
        _route(monkeypatch, "resident")
        assert not _lib().wdg_gemm_resident_eligible(1, m, n, k)
        asked = _four_ways(_gemm_call(ops, a, b, bias), case)
        _route(monkeypatch, "tile")
        tile = _four_ways(_gemm_call(ops, a, b, bias), case)
        for way in R.WAYS:
            assert asked[way].tobytes() == tile[way].tobytes()


@pytest.mark.parametrize("family", R.FAMILIES)
def test_skinny_kernels_pairwise_cover(ops, family):
    """gemm_skinny_kernel<1 | 4 | 16> and gemm_skinny_wave_kernel<N>: K on both sides of 16 | 17, 128 | 129 and 512 | 513, the
    butterflies over 4, 16 and 64 lanes, ragged row groups for every lanes-per-row value, whole waves past M; odd lda pad"""
    lib = _lib()
    for m, n, k in R.SKINNY_SHAPES:
        assert int(lib.wdg_gemm_skinny_lanes(k)) == R.SKINNY_LANES[R.SKINNY_K.index(k)]
        case = R.make_case(family, m, n, k)
        a, b, bias = _operands(case)

        def call(use_bias, relu, out):
            assert ops.gemm_skinny(a, b, bias=bias if use_bias else None, relu=relu, out=out) is out
        _four_ways(call, case)


# =========================================================================================== B. job tables
def _table(ops, jobs, bias_parity, relu, a_pad=4):
    """-> (GemmBatch, [(buffer, C, case, way)]): job i takes family i (cycled) and has a bias when i % 2 == bias_parity"""
    entries, checks = [], []
    for i, (m, n, k) in enumerate(jobs):
        case = R.make_case(R.FAMILIES[i % len(R.FAMILIES)], m, n, k, seed=1)
        a, b, bias = _operands(case, a_pad=a_pad)
        buf, c = _cbuf(m, n)
        use_bias = i % 2 == bias_parity
        entries.append((a, b, c, bias if use_bias else None))
        checks.append((buf, c, case, (use_bias, relu)))
    return ops.GemmBatch(entries, relu=relu), checks


@pytest.mark.parametrize("kernel", ["resident", "tile"])
@pytest.mark.parametrize("odd_k", [False, True], ids=["vec4", "one-job-K6"])
def test_batched_table_on_both_routes(ops, monkeypatch, kernel, odd_k):
    """GemmBatch: five jobs of different shapes, one of them empty (M = 0: its sentinel buffer stays untouched), every second with a
    bias; with one job's K = 6 the table clears GEMM_A_VEC4 and runs on the tile kernel whatever the environment asks for"""
    jobs = list(R.BATCH_JOBS)
    if odd_k:
        jobs[4] = (130, 33, 6)
    _route(monkeypatch, kernel)
    for bias_parity in (0, 1):
        for relu in (False, True):
            batch, checks = _table(ops, jobs, bias_parity, relu)
            assert batch.flags == (0 if odd_k else ops.GEMM_A_VEC4)
            assert (batch.n_jobs, batch.max_m, batch.max_n, batch.max_k) == (5, 513, 64, 512)
            eligible = bool(_lib().wdg_gemm_resident_eligible(5, batch.max_m, batch.max_n, batch.max_k))
            assert eligible == (kernel == "resident")  # (the shapes allow it; the K = 6 table never asks: its flag is clear)
            first = None
            for _run in range(2):
                batch.launch()
                got = [_check(buf, c, R.reference(case, way)) for buf, c, case, way in checks]
                assert checks[1][1].shape[0] == 0 and got[1].size == 0
                if first is not None:
                    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, got))
                first = got


# =========================================================================================== C. split-K
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("m,n,k,splits", R.SPLITK_SHAPES)
def test_split_k_ranges(ops, monkeypatch, m, n, k, splits, family):
    """gemm_f32_kernel as partial products + gemm_splitk_reduce: three EMPTY ranges (K = 1040 over 16: they store zero partials
    that the reduce adds), exact ranges, a ragged last range over two column blocks, and K < 16 splits, which is the single chain
    (equal bits, as everything here)"""
    _route(monkeypatch, "tile", splits)
    _assert_route("tile", m, n, k, splits)
    case = R.make_case(family, m, n, k)
    a, b, bias = _operands(case)
    split = _four_ways(_gemm_call(ops, a, b, bias), case)
    _route(monkeypatch, "tile", 1)
    _assert_route("tile", m, n, k, 1)
    single = _four_ways(_gemm_call(ops, a, b, bias), case)
    for way in R.WAYS:
        assert split[way].tobytes() == single[way].tobytes()


def _splitk_direct(ops, case, way, splits, c, ws_ptr, ws_bytes, a, b, bias):
    from wdg_amd._lib import stream_handle
    m, n, k = case["m"], case["n"], case["k"]
    return _lib().wdg_gemm_splitk_f32(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), bias.data_ptr() if way[0] else None,
                                      int(way[1]), c.data_ptr(), c.stride(0), m, n, k, splits, ws_ptr, ws_bytes, stream_handle())


@pytest.mark.parametrize("m,n,k,splits", R.SPLITK_SHAPES[:3])
def test_split_k_workspace_pointer_need_not_be_aligned(ops, monkeypatch, m, n, k, splits):
    """wdg_gemm_splitk_f32 directly: a workspace that starts 4 bytes behind a 256-byte boundary (the 256 spare bytes of
    wdg_gemm_splitk_workspace_bytes pay for the alignment) gives the same bits, and nothing before or behind it is written"""
    _route(monkeypatch, "tile", 1)
    lib = _lib()
    case = R.make_case("ints", m, n, k)
    a, b, bias = _operands(case)
    ws_bytes = int(lib.wdg_gemm_splitk_workspace_bytes(m, n, splits))
    assert ws_bytes == splits * m * ((n + 3) // 4 * 4) * 4 + 256
    raw = torch.full((4 + ws_bytes + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 256 == 0

    def call(use_bias, relu, out):
        assert _splitk_direct(ops, case, (use_bias, relu), splits, out, raw.data_ptr() + 4, ws_bytes, a, b, bias) == 0
    _four_ways(call, case)
    assert bool((raw[:4] == 0x5A).all()) and bool((raw[4 + ws_bytes:] == 0x5A).all()), "a write beside the workspace"


def test_split_k_refuses_a_workspace_one_byte_short(ops, monkeypatch):
    _route(monkeypatch, "tile", 1)
    lib = _lib()
    m, n, k, splits = R.SPLITK_SHAPES[0]
    case = R.make_case("ints", m, n, k)
    a, b, bias = _operands(case)
    ws_bytes = int(lib.wdg_gemm_splitk_workspace_bytes(m, n, splits))
    raw = torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device="cuda")
    buf, c = _cbuf(m, n)
    assert _splitk_direct(ops, case, (True, True), splits, c, raw.data_ptr(), ws_bytes - 1, a, b, bias) == -3  # WDG_ERR_WORKSPACE
    assert b"workspace" in lib.wdg_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(c).all()) and bool((raw == 0x5A).all()), "a refused call wrote"
    c.fill_(SENTINEL)
    assert bool((buf == SENTINEL).all())


# =========================================================================================== D. the fused two-layer transform
def _tiled(ops, a, k):
    """A [m, k] as ops.Tiled: 16-column groups with rows of 20 floats and a spare row per group, every float outside A NaN"""
    m = a.shape[0]
    groups = (k + 15) // 16
    store = torch.full((groups, m + 1, 20), NAN, dtype=torch.float32, device="cuda")
    padded = np.full((m, groups * 16), np.nan, np.float32)
    padded[:, :k] = a
    t = store[:, :m, :16]
    t.copy_(torch.from_numpy(np.ascontiguousarray(padded.reshape(m, groups, 16).transpose(1, 0, 2))).cuda())
    return ops.Tiled(t, k)


@pytest.mark.parametrize("family", R.MLP2_FAMILIES)
@pytest.mark.parametrize("kernel", ["split", "split-tiled", "chain"])
def test_fused_two_layer_transform_is_exact(ops, monkeypatch, kernel, family):
    """mlp2_split_kernel (row-major and tiled A) and mlp2_bres_kernel: Z equals the fp64 reference bit for bit on small integers
    and on both full-mantissa families - no bit of an input is dropped by the three-piece bf16 split.  lda = K + 4, ldw0 = H + 3,
    ldw1 = C + 5, Z in an ldz = 8 store whose other columns keep their NaN, between two sentinel rows"""
    monkeypatch.setenv("WDG_MLP2_SPLIT", "0" if kernel == "chain" else "1")
    for m, k, h, c_ in R.MLP2_SHAPES:
        case = R.make_mlp2_case(family, m, k, h, c_)
        a = _tiled(ops, case["a"], k) if kernel == "split-tiled" else _view(case["a"], 4)
        w0, w1, b0, b1 = _view(case["w0"], 3), _view(case["w1"], 5), _vec(case["b0"]), _vec(case["b1"])
        store = torch.full((m + 2, 8), NAN, dtype=torch.float32, device="cuda")
        store[0], store[m + 1] = SENTINEL, SENTINEL
        z = store[1:m + 1, :c_]
        for way in R.WAYS:
            entry = (a, w0, b0 if way[0] else None, w1, b1 if way[0] else None, z)
            assert ops.Mlp2Batch.eligible([entry]) and ops.Mlp2Batch.split_kernel() == (kernel != "chain")
            batch = ops.Mlp2Batch([entry], relu=way[1])
            assert batch.flags == {"split": 1, "split-tiled": 1 | 4, "chain": 2}[kernel]
            ref = R.mlp2_reference(case, way)
            for _run in range(2):
                batch.launch()
                torch.cuda.synchronize()
                got = store.cpu().numpy().copy()
                z.fill_(NAN)
                assert (got[0] == SENTINEL).all() and (got[m + 1] == SENTINEL).all() and np.isnan(got[1:m + 1, c_:]).all(), "a write beside Z"
                _same(got[1:m + 1, :c_], ref)


# =========================================================================================== E. non-finite inputs
@pytest.mark.parametrize("kernel,m,n,k", R.NONFINITE_SHAPES)
def test_a_nan_or_an_infinity_stays_in_its_row_or_column(ops, monkeypatch, kernel, m, n, k):
    """(the chain kernels and the skinny ones; the split-operand transform's rules are test_mlp2_split_operands_non_finite_inputs')
    one NaN at A[M - 1][K - 1]: the last row of C is NaN, in all four ways, every other row exact.  One +inf at B[K - 1][N - 1]: the
    last column holds +inf, -inf or NaN exactly where the fp64 reference has each, every other column exact."""
    transb = kernel == "tile-transb"
    if kernel != "skinny":
        splits = 7 if kernel == "splitk" else 1
        _route(monkeypatch, "resident" if kernel == "resident" else "tile", splits)
        _assert_route("resident" if kernel == "resident" else "tile", m, n, k, splits)
    else:
        assert n <= 8
    case = R.make_case("ints", m, n, k, seed=2)
    case["a"][:3, k - 1] = [1, -1, 0]  # (the column of the infinity meets a positive, a negative and a zero factor)
    a_nan, b_inf = case["a"].copy(), case["b"].copy()
    a_nan[m - 1, k - 1], b_inf[k - 1, n - 1] = np.nan, np.inf
    for a_np, b_np in ((a_nan, case["b"]), (case["a"], b_inf)):
        poisoned = dict(case, a=a_np, b=b_np)
        a, b, bias = _operands(poisoned, transb, a_pad=4 if kernel == "resident" else 3)
        want = lambda way: R.reference(case, way, a=a_np, b=b_np)  # noqa: E731
        cls = R.classes(want((False, False)))
        if a_np is a_nan:
            assert (cls[m - 1] == 1).all() and (cls[:m - 1] == 0).all()
        else:
            assert set(cls[:3, n - 1]) == {1, 2, 3} and (cls[:, :n - 1] == 0).all() and (cls[:, n - 1] != 0).all()
        if kernel == "skinny":
            def call(use_bias, relu, out):
                ops.gemm_skinny(a, b, bias=bias if use_bias else None, relu=relu, out=out)
        else:
            call = _gemm_call(ops, a, b, bias, transb)
        got = _four_ways(call, case, want=want, poisoned=True)
        if a_np is a_nan:
            for way in R.WAYS:
                assert np.isnan(got[way][m - 1]).all() and np.isfinite(got[way][:m - 1]).all()


# =========================================================================================== F. the empty sum and refusals
@pytest.mark.parametrize("m,n", [(1, 1), (130, 65), (257, 8)])
def test_k_zero_is_the_empty_sum_and_reads_no_operand(ops, monkeypatch, m, n):
    """A [M, 0] and B [0, N] are empty tensors: their pointers are NULL.  wdg_gemm_f32 (with and without transb), wdg_gemm_splitk_f32
    (its K < 16 splits rule) and wdg_gemm_skinny_f32 store act(bias), or act(0), into all of C"""
    case = R.make_case("ints", m, n, 0)
    case["bias"][0] = -3.0  # (a negative entry for the relu)
    a, bias = torch.empty((m, 0), device="cuda"), _vec(case["bias"])
    assert a.data_ptr() == 0
    for transb, splits in ((False, 1), (True, 1), (False, 16)):
        _route(monkeypatch, "tile", splits)
        b = torch.empty((n, 0) if transb else (0, n), device="cuda")
        assert b.data_ptr() == 0
        got = _four_ways(_gemm_call(ops, a, b, bias, transb), case)
        assert (got[(False, False)] == 0).all() and (got[(True, True)] == np.maximum(case["bias"], 0)[None, :]).all()
    if n <= 8:
        assert int(_lib().wdg_gemm_skinny_lanes(0)) == 1
        b = torch.empty((0, n), device="cuda")

        def call(use_bias, relu, out):
            ops.gemm_skinny(a, b, bias=bias if use_bias else None, relu=relu, out=out)
        _four_ways(call, case)


def test_skinny_stays_refused_for_nine_columns(ops):
    from wdg_amd._lib import stream_handle
    lib = _lib()
    case = R.make_case("ints", 65, 9, 17)
    a, b, _bias = _operands(case)
    buf, c = _cbuf(65, 9)
    assert lib.wdg_gemm_skinny_f32(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), None, 0, c.data_ptr(), c.stride(0), 65, 9, 17,
                                   stream_handle()) == -1  # WDG_ERR_INVALID
    assert b"8 columns" in lib.wdg_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(c).all()), "a refused call wrote"
    c.fill_(SENTINEL)
    assert bool((buf == SENTINEL).all())
