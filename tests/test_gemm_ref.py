"""The data of tests/_gemm_ref.py is what tests/test_gpu_gemm_edges.py assumes (no GPU): for every case that file launches, in all
four ways,
  * the fp64 reference is a set of fp32 numbers (cast to fp32 and back unchanged);
  * the bound that makes it order-free holds, computed from |A| |B| and not from the signed product: below 2^24 for the integer
    and selector families; at most ONE non-zero product per output, and no bias where there is one, for the full-mantissa family;
  * a forward, a reversed and a pairwise fp32 summation on the CPU give the reference's bits;
  * every small-integer entry is a bf16, and the full-mantissa operands need all three bf16 pieces of csrc/split_bf16.h - the
    kept piece products include (piece 2 of A) x (piece 0 of W0) and (piece 0 of A) x (piece 2 of W0).
Beside it: the library's two route queries (host entry points, they load without a GPU) against the case lists' own claims."""
import numpy as np
import pytest

import _gemm_ref as R


def _gemm_shapes():
    """every (M, N, K) of the GPU file, once"""
    shapes = set(R.TILE_SHAPES) | set(R.BRES_SHAPES) | set(R.SKINNY_SHAPES) | {s[:3] for s in R.SPLITK_SHAPES}
    shapes |= {(m, n, k) for m, n, _k in R.BRES_SHAPES[:4] for k in R.BRES_K_REFUSED} | {j for j in R.BATCH_JOBS if j[0] > 0}
    shapes |= {(130, 33, 6)} | {s[1:] for s in R.NONFINITE_SHAPES}
    return sorted(shapes)


GEMM_SHAPES = _gemm_shapes()


def _exact(ref64):
    assert np.isfinite(ref64).all()
    assert np.array_equal(ref64.astype(np.float32).astype(np.float64), ref64), "the reference is not a set of fp32 numbers"


def test_the_case_lists_cover_every_pair():
    for lists, shapes in (((R.TILE_M, R.TILE_N, R.TILE_K), R.TILE_SHAPES), ((R.BRES_M, R.BRES_N, R.BRES_K), R.BRES_SHAPES),
                          ((R.SKINNY_M, R.SKINNY_N, R.SKINNY_K), R.SKINNY_SHAPES)):
        assert len(shapes) < len(lists[0]) * len(lists[1]) * len(lists[2]) and len(set(shapes)) == len(shapes)
        for s in range(3):
            for t in range(s + 1, 3):
                assert {(c[s], c[t]) for c in shapes} == {(u, v) for u in lists[s] for v in lists[t]}
    assert max(k for _m, _n, k in GEMM_SHAPES) <= 4100 and max(n for _m, n, _k in GEMM_SHAPES) <= 100


@pytest.mark.parametrize("family", R.FAMILIES)
def test_gemm_data_is_exact_in_any_order(family):
    for m, n, k in GEMM_SHAPES:
        c = R.make_case(family, m, n, k)
        assert c["a"].shape == (m, k) and c["b"].shape == (k, n) and c["bias"].shape == (n,)
        assert all(v.dtype == np.float32 for v in (c["a"], c["b"], c["bias"]))
        if family.startswith("full"):
            terms = R.terms_per_output(c["a"], c["b"])
            assert terms.max(initial=0) <= 1 and not ((terms > 0) & (c["bias"] != 0)[None, :]).any(), (m, n, k)
            if k > 0 and n > 1:
                assert (terms > 0).any() and (c["bias"] != 0).any()
            whole = c["a"] if family == "full-a" else c["b"]
            assert ((whole.view(np.uint32) & 1) == 1)[whole != 0].all()  # the last significand bit is in use
        else:
            assert R.magnitude(c["a"], c["b"], c["bias"]).max(initial=0) < R.EXACT_LIMIT, (m, n, k)
        if family == "ints":
            for v in (c["a"], c["b"], c["bias"]):
                assert np.abs(v).max(initial=0) <= 8 and ((v.view(np.uint32) & 0xFFFF) == 0).all()  # integers, each a bf16
        if family == "selectors" and k > 0:
            assert ((c["a"] != 0).sum(axis=1) == 1).all() and c["a"][0, k - 1] == 1 and c["a"][-1, 0 if m > 1 else k - 1] == 1
        for way in R.WAYS:
            ref = R.reference(c, way)
            _exact(ref)
            if m * n * k <= 2_000_000:  # (the orders of the largest shapes are summed once, on the bias + relu way)
                orders = R.ORDERS
            else:
                orders = R.ORDERS if way == (True, True) else ()
            for order in orders:
                got = R.gemm_f32(c, way, order)
                assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), ref), (family, m, n, k, way, order)


@pytest.mark.parametrize("family", R.MLP2_FAMILIES)
def test_mlp2_data_is_exact_in_any_order(family):
    for m, k, h, c_ in R.MLP2_SHAPES:
        c = R.make_mlp2_case(family, m, k, h, c_)
        if family == "ints":
            for v in (c["a"], c["w0"], c["b0"], c["w1"], c["b1"]):
                assert np.abs(v).max() <= 4 and ((v.view(np.uint32) & 0xFFFF) == 0).all()
            hid = R.magnitude(c["a"], c["w0"], c["b0"])
            assert hid.max() <= 16 * 512 + 4
            assert (hid @ np.abs(c["w1"]).astype(np.float64) + np.abs(c["b1"])).max() < R.EXACT_LIMIT
        else:
            t0 = R.terms_per_output(c["a"], c["w0"])
            assert t0.max() <= 1 and not ((t0 > 0) & (c["b0"] != 0)[None, :]).any() and (t0 > 0).any()
            hidden_used = ((t0 > 0) | (c["b0"] != 0)[None, :]).astype(np.int64)
            t1 = hidden_used @ (c["w1"] != 0).astype(np.int64)
            assert t1.max() <= 1 and not ((t1 > 0) & (c["b1"] != 0)[None, :]).any()
            # all three pieces of the full operand are needed, and they meet piece 0 (the only one) of the power of two
            whole, other = (c["a"], c["w0"]) if family == "full-a" else (c["w0"], c["a"])
            wh, wm, wl = R.bf16_pieces(whole)
            oh, om, ol = R.bf16_pieces(other)
            assert np.array_equal(wh.astype(np.float64) + wm + wl, whole.astype(np.float64)) and not om.any() and not ol.any()
            if family == "full-a":  # (piece 2 of A) x (piece 0 of W0) reaches an output
                assert (((wl != 0).astype(np.int64) @ (oh != 0).astype(np.int64)) > 0).any()
            else:                   # (piece 0 of A) x (piece 2 of W0)
                assert (((oh != 0).astype(np.int64) @ (wl != 0).astype(np.int64)) > 0).any()
            assert (wm[whole != 0] != 0).mean() > 0.9 and (wl[whole != 0] != 0).mean() > 0.9
        for way in R.WAYS:
            ref = R.mlp2_reference(c, way)
            _exact(ref)
            for order in R.ORDERS:
                got = R.mlp2_f32(c, way, order)
                assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), ref), (family, m, k, h, c_, way, order)


def test_bf16_pieces_restate_the_split():
    x = R.full(np.random.default_rng(1), 4096)
    h, m, l = R.bf16_pieces(x)
    for p in (h, m, l):
        assert ((p.view(np.uint32) & 0xFFFF) == 0).all()
    assert np.array_equal(h.astype(np.float64) + m + l, x.astype(np.float64))
    assert (np.abs(x - h) <= np.abs(h) * 2.0 ** -8).all()  # round to nearest: half a unit of bf16's 8-bit significand


def test_split_k_ranges_are_what_the_cases_claim():
    """the range rule of gemm_f32_kernel, restated: ceil(K / splits) rounded up to whole K steps of 16"""
    def ranges(k, splits):
        kc = -(-(-(-k // splits)) // 16) * 16
        return [(min(k, z * kc), min(k, min(k, z * kc) + kc)) for z in range(splits)]
    r = ranges(1040, 16)
    assert r[12] == (960, 1040) and r[13:] == [(1040, 1040)] * 3
    assert ranges(1024, 16) == [(64 * z, 64 * z + 64) for z in range(16)]
    assert ranges(1100, 7)[-1] == (960, 1100) and ranges(1100, 7)[0] == (0, 160)
    assert 100 < 7 * 16


def test_route_queries_need_no_gpu(monkeypatch):
    """wdg_gemm_skinny_lanes on both sides of its three boundaries; wdg_gemm_resident_eligible where shape or switch decides alone"""
    import wdg_amd._lib as L
    assert [int(L.lib.wdg_gemm_skinny_lanes(k)) for k in R.SKINNY_K] == R.SKINNY_LANES
    for env in ("WDG_GEMM_TILE", "WDG_GEMM_RESIDENT"):
        monkeypatch.delenv(env, raising=False)
    for k in R.BRES_K_REFUSED + [0]:
        assert L.lib.wdg_gemm_resident_eligible(100, 513, 64, k) == 0
    assert L.lib.wdg_gemm_resident_eligible(100, 513, 65, 64) == 0
    monkeypatch.setenv("WDG_GEMM_RESIDENT", "1")
    for _m, n, k in R.BRES_SHAPES:
        assert L.lib.wdg_gemm_resident_eligible(1, 1, n, k) == 1
    assert L.lib.wdg_gemm_resident_eligible(1, 1, 64, 516) == 0 and L.lib.wdg_gemm_resident_eligible(1, 1, 64, 6) == 0
    monkeypatch.setenv("WDG_GEMM_TILE", "1")  # the tile switch wins
    assert L.lib.wdg_gemm_resident_eligible(1000, 513, 64, 64) == 0
