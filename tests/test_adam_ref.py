"""tests/_adam_ref.py (the numpy restatement of wdg_adam_batched_f32 that the GPU tests compare the kernel with, bit for bit) pinned
against torch.optim.Adam in float64 on the CPU, its power and its segment rule against plain definitions, and the boundary of the
entry point: the refusals that need no device, and the ctypes mirror of wdg_adam_job against the header's struct."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _adam_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10  # (the figure tests/test_acm_ref.py pins its restatement with)
INVALID = -1


@pytest.mark.parametrize("rows,cols,seg_rows,seg_cols", [(12, 10, 12, 4), (12, 8, 4, 8), (7, 9, 3, 4), (5, 5, 5, 5), (6, 6, 1, 1)])
def test_float64_restatement_matches_torch_adam_over_twenty_steps(rows, cols, seg_rows, seg_cols):
    """one tensor split into segments with different lr / weight_decay (ragged last segments included) against one torch parameter
    per segment, twenty steps with fresh gradients, within 1e-10"""
    rng = np.random.default_rng(rows * 100 + cols)
    seg = ref.segment_index(rows, cols, seg_rows, seg_cols)
    n_seg = ref.n_segments(rows, cols, seg_rows, seg_cols)
    assert n_seg == int(seg.max()) + 1
    hyper = np.stack([10.0 ** rng.uniform(-3, -1, n_seg), np.where(np.arange(n_seg) % 3 == 0, 0.0, 10.0 ** rng.uniform(-4, -2, n_seg))], 1)
    p = rng.standard_normal((rows, cols))
    m, v = np.zeros_like(p), np.zeros_like(p)
    params = [torch.nn.Parameter(torch.tensor(p[seg == s])) for s in range(n_seg)]
    opts = [torch.optim.Adam([q], lr=float(hyper[s, 0]), weight_decay=float(hyper[s, 1])) for s, q in enumerate(params)]
    for t in range(1, 21):
        g = rng.standard_normal((rows, cols)) * 10.0 ** rng.uniform(-4, 0)
        p, m, v = ref.adam_step(p, g, m, v, hyper, seg_rows, seg_cols, t)
        assert p.dtype == np.float64
        for s, (q, opt) in enumerate(zip(params, opts)):
            q.grad = torch.tensor(g[seg == s])
            opt.step()
            want = q.detach().numpy()
            err = float(np.abs(p[seg == s] - want).max())
            assert err <= TOL * max(1.0, float(np.abs(want).max())), (t, s, err)
    assert float(np.abs(v).min()) > 0


def test_ipow_is_the_power():
    for b in (0.9, 0.999, float(np.float32(0.9)), 0.0, 0.5):
        for t in (0, 1, 2, 3, 7, 1000, 100000):
            want = float(b) ** t
            assert abs(float(ref.ipow(b, t)) - want) <= 1e-12 * max(want, 1e-300), (b, t)
    assert ref.ipow(0.9, 100000) == 0.0 and ref.ipow(0.5, 1) == 0.5 and ref.ipow(0.0, 0) == 1.0


def test_segment_rule():
    seg = ref.segment_index(5, 10, 2, 4)
    assert seg.shape == (5, 10) and ref.n_segments(5, 10, 2, 4) == 9
    for r in range(5):
        for c in range(10):
            assert seg[r, c] == (r // 2) * 3 + c // 4
    # the trainer's layouts: w0 [F, R hidden] - a replica is a column block; w1 [R hidden, cs] - a replica is a row block
    assert ref.segment_index(7, 12, 7, 4)[:, 8:].min() == 2 == ref.segment_index(7, 12, 7, 4).max()
    assert (ref.segment_index(12, 8, 4, 8) == (np.arange(12) // 4)[:, None]).all()
    assert ref.n_segments(0, 5, 1, 1) == 0


def test_float32_restatement_keeps_its_dtype_and_its_special_cases():
    rng = np.random.default_rng(3)
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    p, g = f32(rng.standard_normal((6, 8))), f32(rng.standard_normal((6, 8)))
    p[:, 4:] = 0
    g[:, 4:] = 0  # a padding block
    g[1, 2] = np.nan
    hyper = f32([[0.01, 5e-4], [0.0, 5e-4]])
    p1, m1, v1 = ref.adam_step(p, g, np.zeros_like(p), np.zeros_like(p), hyper, 6, 4, 1)
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    for a in (p1, m1, v1):
        assert np.isnan(a[1, 2]) and int(np.isnan(a).sum()) == 1  # one NaN gradient: that element alone
        assert not a[:, 4:].any() and not np.signbit(a[:, 4:]).any()  # zero stays +0
    hyper = f32([[0.0, 0.0], [0.01, 0.0]])
    p2, m2, v2 = ref.adam_step(p, np.nan_to_num(g), np.zeros_like(p), np.zeros_like(p), hyper, 6, 4, 5)
    assert np.array_equal(p2[:, :4], p[:, :4]) and m2[:, :4].any() and v2[:, :4].any()  # lr = 0: p stays, the moments move
    p64, _, _ = ref.adam_step(p.astype(np.float64), np.nan_to_num(g).astype(np.float64), np.zeros((6, 8)), np.zeros((6, 8)),
                              f32([[0.01, 5e-4], [0.0, 5e-4]]).astype(np.float64), 6, 4, 1)
    p32, _, _ = ref.adam_step(p, np.nan_to_num(g), np.zeros_like(p), np.zeros_like(p), f32([[0.01, 5e-4], [0.0, 5e-4]]), 6, 4, 1)
    err = float(np.abs(p32 - p64).max())
    assert 0 < err < 1e-6, err  # fp32 rounding: neither a float64 evaluation in disguise nor another function


def test_refusals_need_no_gpu():
    import wdg_amd._lib as L
    f = L.lib.wdg_adam_batched_f32
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    assert f(null, 1, 8, 8, 0.9, 0.999, 1e-8, some, null) == INVALID           # a null table with jobs
    assert b"null job table" in L.lib.wdg_last_error()
    assert f(some, -1, 8, 8, 0.9, 0.999, 1e-8, some, null) == INVALID          # negative counts
    assert f(some, 1, -1, 8, 0.9, 0.999, 1e-8, some, null) == INVALID
    assert f(some, 1, 8, -1, 0.9, 0.999, 1e-8, some, null) == INVALID
    assert f(some, 1, 8, 8, 0.9, 0.999, 1e-8, null, null) == INVALID           # no step word
    assert b"step word" in L.lib.wdg_last_error()
    assert f(some, 65536, 8, 8, 0.9, 0.999, 1e-8, some, null) == INVALID       # more jobs than one launch takes
    for b1, b2 in ((1.0, 0.999), (-0.1, 0.999), (0.9, 1.0), (0.9, -1e-3), (float("nan"), 0.999), (0.9, float("nan"))):
        assert f(some, 1, 8, 8, b1, b2, 1e-8, some, null) == INVALID           # betas outside [0, 1)
    assert f(some, 1, 8, 8, 0.9, 0.999, float("nan"), some, null) == INVALID   # an eps that is not a number
    assert b"eps" in L.lib.wdg_last_error()
    assert f(null, 0, 8, 8, 0.9, 0.999, 1e-8, some, null) == 0                 # nothing to do
    assert f(null, 0, 0, 0, 0.0, 0.0, 0.0, some, null) == 0
    with pytest.raises(ValueError):
        L.check(f(null, 1, 8, 8, 0.9, 0.999, 1e-8, some, null), "wdg_adam_batched_f32")


def test_per_job_refusals_on_the_host_table():
    """what lies inside a job is checked on the host's copy of the table (wdg_adam_check_jobs): segments below 1 x 1 on a non-empty
    job, a leading dimension below the width, a null pointer; an empty job is not looked into"""
    import wdg_amd._lib as L
    from wdg_amd import train
    chk = L.lib.wdg_adam_check_jobs

    def job(**kw):
        tab = np.zeros(1, train._ADAM_JOB_DTYPE)
        for k in ("p", "g", "m", "v", "hyper"):
            tab[k] = 4096
        tab["rows"], tab["cols"], tab["seg_rows"], tab["seg_cols"], tab["ld"], tab["ld_s"] = 8, 12, 8, 4, 12, 12
        for k, val in kw.items():
            tab[k] = val
        return tab

    run = lambda tab: chk(ctypes.c_void_p(tab.ctypes.data), len(tab))  # noqa: E731
    assert run(job()) == 0
    assert run(job(seg_rows=0)) == INVALID and run(job(seg_cols=0)) == INVALID and run(job(seg_cols=-4)) == INVALID
    assert b"segments" in L.lib.wdg_last_error()
    assert run(job(ld=11)) == INVALID and run(job(ld_s=11)) == INVALID
    assert b"leading dimension" in L.lib.wdg_last_error()
    assert run(job(hyper=0)) == INVALID and run(job(rows=-1)) == INVALID
    assert run(job(rows=0, seg_rows=0, ld=0)) == 0 and run(job(cols=0, seg_cols=0, ld_s=0)) == 0  # empty: skipped
    assert chk(ctypes.c_void_p(0), 1) == INVALID and chk(ctypes.c_void_p(0), 0) == 0 and chk(ctypes.c_void_p(0), -1) == INVALID


def test_struct_layout_matches_header(tmp_path):
    """wdg_adam_job: size and field offsets as gcc lays them out == the ctypes mirror == the numpy record of the front end"""
    import wdg_amd._lib as L
    from wdg_amd import train
    mirror = L.AdamJob
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(wdg_adam_job));']
    for fname, _ in mirror._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(wdg_adam_job, {fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["size"] == ctypes.sizeof(mirror) == train._ADAM_JOB_DTYPE.itemsize
    assert [f for f, _ in mirror._fields_] == ["p", "g", "m", "v", "hyper", "ld", "ld_s", "rows", "cols", "seg_rows", "seg_cols"]
    for fname, _ in mirror._fields_:
        assert got[fname] == getattr(mirror, fname).offset == train._ADAM_JOB_DTYPE.fields[fname][1], fname

