"""tests/_acm_ref.py (the numpy restatement of the ACM channel mix and of ACM-SGC-1 / ACM-GCN-2 that the GPU tests measure the
kernels against) pinned against torch autograd in fp64 on the CPU, and the refusals of the binding and of the entry points that
need no device."""
import ctypes

import numpy as np
import pytest
import torch

import _acm_ref as ref

SHAPES = [(1, 1), (7, 5), (65, 64), (33, 256)]
TOL = 1e-10


def _inputs(rows, cols, seed, with_agg=True):
    rng = np.random.default_rng(seed)
    d = dict(low=rng.standard_normal((rows, cols)), high=rng.standard_normal((rows, cols)),
             high_agg=rng.standard_normal((rows, cols)) if with_agg else None, ident=rng.standard_normal((rows, cols)),
             att=rng.uniform(-1, 1, (3, cols)) / np.sqrt(cols), wmix=rng.uniform(-1, 1, (3, 3)) / np.sqrt(3))
    return d, rng.standard_normal((rows, cols))


def _close(got, want, what):
    err = float(np.abs(got - want).max()) if want.size else 0.0
    assert err <= TOL * max(1.0, float(np.abs(want).max()) if want.size else 1.0), (what, err)


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_agg", [False, True])
def test_mix_matches_torch_autograd_fp64(rows, cols, relu, with_agg):
    d, d_out = _inputs(rows, cols, 100 * rows + cols, with_agg)
    t = {k: None if v is None else torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in d.items()}
    out_t = ref.torch_mix(t["low"], t["high"], t["high_agg"], t["ident"], t["att"], t["wmix"], relu)
    out_t.backward(torch.tensor(d_out))
    out, aux = ref.mix_forward(d["low"], d["high"], d["high_agg"], d["ident"], d["att"], d["wmix"], relu)
    assert out.dtype == np.float64 and aux.shape == (rows, 8)
    _close(out, out_t.detach().numpy(), "out")
    np.testing.assert_allclose(aux[:, :3].sum(1), 1.0, rtol=0, atol=1e-14)
    assert not aux[:, 6:].any()
    g = ref.mix_backward(d["low"], d["high"], d["high_agg"], d["ident"], d["att"], d["wmix"], relu, d_out)
    for k, name in (("d_low", "low"), ("d_high", "high"), ("d_ident", "ident"), ("d_att", "att"), ("d_wmix", "wmix")):
        _close(g[k], t[name].grad.numpy(), k)
    if with_agg:
        _close(-g["d_high"], t["high_agg"].grad.numpy(), "d_high_agg")


def test_restatement_follows_the_dtype_of_its_inputs():
    d, d_out = _inputs(33, 20, 5)
    d32 = {k: None if v is None else v.astype(np.float32) for k, v in d.items()}
    out32, aux32 = ref.mix_forward(d32["low"], d32["high"], d32["high_agg"], d32["ident"], d32["att"], d32["wmix"], True)
    g32 = ref.mix_backward(d32["low"], d32["high"], d32["high_agg"], d32["ident"], d32["att"], d32["wmix"], True, d_out.astype(np.float32))
    assert out32.dtype == np.float32 and aux32.dtype == np.float32 and all(v.dtype == np.float32 for v in g32.values())
    out64, _ = ref.mix_forward(d["low"], d["high"], d["high_agg"], d["ident"], d["att"], d["wmix"], True)
    err = float(np.abs(out32 - out64).max())
    assert 0 < err < 1e-4, err  # fp32 rounding: neither an fp64 evaluation in disguise nor a different function


def test_a_nan_input_stays_a_nan():
    d, _ = _inputs(4, 6, 9)
    d["ident"][2, 3] = np.nan
    for relu in (False, True):
        out, _ = ref.mix_forward(d["low"], d["high"], d["high_agg"], d["ident"], d["att"], d["wmix"], relu)
        assert np.isnan(out[2]).all() and not np.isnan(out[[0, 1, 3]]).any()


def _graph(n, seed):
    rng = np.random.default_rng(seed)
    a = (rng.random((n, n)) < 0.2).astype(np.float64) + np.eye(n)
    return a / a.sum(1, keepdims=True)  # the random-walk normalisation of a directed graph with self loops


def test_models_match_torch_autograd_fp64():
    n, f, hid, c = 23, 11, 6, 4
    rng = np.random.default_rng(3)
    a_hat, x = _graph(n, 4), rng.standard_normal((n, f))
    d_logits = rng.standard_normal((n, c))
    u = lambda *s: rng.uniform(-1, 1, s)  # noqa: E731
    # ACM-SGC-1
    p = dict(w=u(f, 3 * c), att=u(3, c) / np.sqrt(c), wmix=u(3, 3) / np.sqrt(3))
    t = {k: torch.tensor(v, requires_grad=True) for k, v in p.items()}
    lt = ref.torch_layer(torch.tensor(a_hat), torch.tensor(x), t["w"], t["att"], t["wmix"], False)
    lt.backward(torch.tensor(d_logits))
    _close(ref.acm_sgc1_forward(a_hat, x, p["w"], p["att"], p["wmix"]), lt.detach().numpy(), "sgc logits")
    g = ref.acm_sgc1_backward(a_hat, x, p["w"], p["att"], p["wmix"], d_logits)
    for k in p:
        _close(g[k], t[k].grad.numpy(), "sgc " + k)
    # ACM-GCN-2, evaluation (no mask) and training (a fixed mask times 1 / (1 - p))
    p = dict(w0=u(f, 3 * hid), att0=u(3, hid) / np.sqrt(hid), wmix0=u(3, 3) / np.sqrt(3), w1=u(hid, 3 * c), att1=u(3, c) / np.sqrt(c), wmix1=u(3, 3) / np.sqrt(3))
    for keep_scale in (None, (rng.random((n, hid)) < 0.5) * 2.0):
        t = {k: torch.tensor(v, requires_grad=True) for k, v in p.items()}
        ta = torch.tensor(a_hat)
        h = torch.relu(ref.torch_layer(ta, torch.tensor(x), t["w0"], t["att0"], t["wmix0"], True))
        if keep_scale is not None:
            h = h * torch.tensor(keep_scale)
        lt = ref.torch_layer(ta, h, t["w1"], t["att1"], t["wmix1"], False)
        lt.backward(torch.tensor(d_logits))
        _close(ref.acm_gcn2_forward(a_hat, x, p, keep_scale)[0], lt.detach().numpy(), "gcn logits")
        g = ref.acm_gcn2_backward(a_hat, x, p, d_logits, keep_scale)
        for k in p:
            _close(g[k], t[k].grad.numpy(), "gcn " + k)


def test_entry_points_refuse_malformed_tables_without_a_device():
    import wdg_amd._lib as L
    null = ctypes.c_void_p(0)
    for fn in (L.lib.wdg_acm_mix_batched_f32, L.lib.wdg_acm_mix_backward_batched_f32):
        assert fn(null, 0, 8, 8, null) == 0          # nothing to do
        assert fn(null, 3, 8, 8, null) != 0          # a null table with jobs
        assert b"null job table" in L.lib.wdg_last_error()
        assert fn(null, -1, 8, 8, null) != 0         # negative counts
        assert fn(null, 1, -8, 8, null) != 0
        assert fn(null, 1, 8, -8, null) != 0
        assert fn(null, 65536, 8, 8, null) != 0      # more jobs than one launch takes
        assert fn(null, 0, 8, 257, null) != 0        # a wider row than the kernel holds
        assert b"257" in L.lib.wdg_last_error()


def test_job_struct_matches_the_header(tmp_path):
    """size and field offsets of wdg_acm_mix_job as gcc lays them out == the ctypes mirror"""
    import os
    import subprocess
    import wdg_amd._lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(wdg_acm_mix_job));']
    lines += [f'printf("{name} %zu\\n", offsetof(wdg_acm_mix_job, {name}));' for name, _ in L.AcmMixJob._fields_]
    lines += ["return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.AcmMixJob)
    for name, _ in L.AcmMixJob._fields_:
        assert int(got[name]) == getattr(L.AcmMixJob, name).offset, name


def test_binding_refuses_what_the_kernel_does_not_take():
    """the checks of ops.AcmMixBatch that come before any device is touched"""
    from wdg_amd import ops
    z = lambda *s: torch.zeros(s)  # noqa: E731
    entry = lambda rows, cols: dict(low=z(rows, cols), high=z(rows, cols), ident=z(rows, cols), att=z(3, cols), wmix=z(3, 3), out=z(rows, cols))  # noqa: E731
    with pytest.raises(ValueError, match="257 columns"):
        ops.AcmMixBatch([entry(4, 257)], False)
    with pytest.raises(ValueError, match="0 columns"):
        ops.AcmMixBatch([entry(4, 0)], False)
    with pytest.raises(ValueError, match="one activation flag per entry"):
        ops.AcmMixBatch([entry(4, 4)], [True, False])
    with pytest.raises(ValueError, match="required"):
        ops.AcmMixBatch([{k: v for k, v in entry(4, 4).items() if k != "wmix"}], False)
    with pytest.raises(ValueError, match="unknown keys"):
        ops.AcmMixBatch([dict(entry(4, 4), bias=z(4))], False)
    with pytest.raises(ValueError, match="come together"):
        ops.AcmMixBatch([dict(entry(4, 4), d_out=z(4, 4))], False)
    with pytest.raises(ValueError, match="fp32 device matrix"):
        ops.AcmMixBatch([entry(4, 4)], False)  # host tensors
    with pytest.raises(ValueError, match="entries; one launch takes 65535"):
        ops.AcmMixBatch([None] * 65536, False)


def test_models_and_trainer_refuse_what_they_do_not_hold():
    from wdg_amd import models
    with pytest.raises(ValueError, match="256"):
        models.ACMGCN2(10, 3, nhid=300)
    with pytest.raises(ValueError, match="256"):
        models.ACMSGC1(10, 257)


def test_overlap_rule_of_the_binding():
    """train._views_may_overlap: disjoint column slices of one matrix do not overlap, intersecting ones and aliases do"""
    from wdg_amd.train import _views_may_overlap as may
    wide, other = torch.zeros(6, 12), torch.zeros(6, 4)
    assert not may(wide[:, :4], wide[:, 4:8]) and not may(wide[:, 8:], wide[:, :8]) and not may(wide[:, :4], other)
    assert may(wide[:, :4], wide[:, 3:7]) and may(wide[:, :4], wide[:, :4]) and may(wide[:, 2:6], wide[1:, :4])
    assert may(wide[:, :4], wide.view(12, 6)[:, :3])          # (another pitch inside the same bytes: reported)
    assert not may(wide[:3, :], wide[3:, :]) and not may(wide[:0], wide) and not may(wide[:1, :4], wide[:1, 4:])
