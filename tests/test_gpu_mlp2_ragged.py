"""GPU parity of the fused GCN-2 transform's partial K step (mlp2_split_kernel, csrc/gemm.hip).

The K loop runs whole 32-k steps; K % 32 != 0 leaves one partial step that is taken behind the loop, with addresses pulled back
inside the row and the values past K zeroed.  Zero-padding A (columns) and W0 (rows) to the next multiple of 32 sends the same
numbers down the whole-step path of the same build: exact zeros add nothing to an fp32 accumulator, so Z must be BITWISE equal.
Beside it: run-to-run equality, the fp64 yardstick of tests/test_gpu_kernels.py::test_mlp2_fused_transform (1e-5 of the
largest output) so that the pair cannot be wrong together, and the padding columns of an ldz = 8 row left alone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (M, K, H, C): K % 32 in {0, 4, 20, 28}; K < 32; K <= 128; a last quarter without a whole step (260 = 2 x 128 + 4); M off the
# 32-row tiles; fewer tiles than the workgroup has waves (16); one lane's worth of rows
WIDE = [(2000, 500, 64, 5), (700, 508, 40, 8), (999, 128, 64, 8), (513, 260, 64, 5), (100, 28, 40, 5), (300, 20, 64, 8),
        (1200, 384, 40, 1), (33, 68, 64, 1), (1, 4, 40, 1), (4500, 100, 64, 5)]
NARROW = [(2000, 500, 16, 5), (33, 68, 16, 1), (1, 4, 16, 1), (777, 124, 16, 8), (260, 96, 16, 5), (50, 12, 16, 8), (1500, 260, 16, 1)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from wdg_amd import ops as o
    return o


def _np(t):
    return t.detach().cpu().numpy()


def _entries(ops, shapes, tiled, bias, seed):
    """-> (entries at K, entries zero-padded to 32-multiples, fp64 inputs per job); Z is a view of NaN-filled [M, 8] storage"""
    rng = np.random.default_rng(seed)
    ragged, padded, f64 = [], [], []
    for m, k, h, c in shapes:
        kp = (k + 31) // 32 * 32
        a = rng.standard_normal((m, k)).astype(np.float32)
        w0 = (rng.standard_normal((k, h)) / np.sqrt(k)).astype(np.float32)
        w1 = (rng.standard_normal((h, c)) / np.sqrt(h)).astype(np.float32)
        b0 = rng.standard_normal(h).astype(np.float32) if bias else None
        b1 = rng.standard_normal(c).astype(np.float32) if bias else None
        a_pad, w0_pad = np.zeros((m, kp), np.float32), np.zeros((kp, h), np.float32)
        a_pad[:, :k], w0_pad[:k] = a, w0
        dev = lambda t: None if t is None else torch.from_numpy(t).cuda()
        if tiled:  # [groups, rows, 16]: the padded storage serves both (cols = K / the 32-multiple)
            t = dev(np.ascontiguousarray(a_pad.reshape(m, kp // 16, 16).transpose(1, 0, 2)))
            a_r, a_p = ops.Tiled(t, k), ops.Tiled(t, kp)
        else:      # the ragged job's rows are K long: a read past K would land in the next row
            a_r, a_p = dev(a), dev(a_pad)
        w1d, b0d, b1d = dev(w1), dev(b0), dev(b1)
        zs = [torch.full((m, 8), float("nan"), device="cuda") for _ in range(2)]
        ragged.append((a_r, dev(w0), b0d, w1d, b1d, zs[0][:, :c]))
        padded.append((a_p, dev(w0_pad), b0d, w1d, b1d, zs[1][:, :c]))
        f64.append(tuple(None if t is None else t.astype(np.float64) for t in (a, w0, b0, w1, b1)))
    return ragged, padded, f64


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("shapes", [WIDE, NARROW], ids=["two_column_tiles", "one_column_tile"])
def test_mlp2_split_partial_step_equals_whole_steps_on_zero_padding(ops, monkeypatch, shapes, tiled, relu, bias):
    monkeypatch.setenv("WDG_MLP2_SPLIT", "1")
    ragged, padded, f64 = _entries(ops, shapes, tiled, bias, seed=100 + 8 * tiled + 2 * relu + bias)
    assert ops.Mlp2Batch.eligible(ragged) and ops.Mlp2Batch.eligible(padded)
    br, bp = ops.Mlp2Batch(ragged, relu=relu), ops.Mlp2Batch(padded, relu=relu)
    br.launch()
    bp.launch()
    torch.cuda.synchronize()
    first = [e[5].clone() for e in ragged]
    br.launch()  # run to run
    torch.cuda.synchronize()
    for (m, k, h, c), er, ep, z1, (a, w0, b0, w1, b1) in zip(shapes, ragged, padded, first, f64):
        zr, zp = er[5], ep[5]
        assert torch.equal(zr, z1), f"{(m, k, h, c)}: two launches differ"
        assert not bool(torch.isnan(zr).any()), f"{(m, k, h, c)}: Z not fully written"
        assert torch.equal(zr, zp), f"{(m, k, h, c)}: partial step != whole steps on zero padding, max |d| = {float((zr - zp).abs().max())}"
        for z in (zr, zp):  # the caller's padding columns of an ldz = 8 row
            store = torch.as_strided(z, (m, 8), (8, 1))
            assert bool(torch.isnan(store[:, c:]).all()), f"{(m, k, h, c)}: stores outside Z[M, C]"
        hid = a @ w0 + (0 if b0 is None else b0)
        ref = (np.maximum(hid, 0) if relu else hid) @ w1 + (0 if b1 is None else b1)
        np.testing.assert_allclose(_np(zr), ref, rtol=1e-5, atol=1e-5 * max(np.abs(ref).max(), 1e-30))
