"""CPU checks for wdg_head_train_batched_f32 (include/wdg.h): the numpy restatement the GPU tests compare the kernel with is pinned
against torch autograd + torch.optim.Adam, the ctypes mirror of its job struct against gcc's layout, and the entry's refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from _head_train_ref import head_train, split_ids, xavier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,f,c,lr", [(203, 67, 5, 0.01), (203, 67, 5, 0.05), (130, 515, 8, 0.05), (96, 1, 2, 0.01)])
def test_restatement_matches_torch_autograd_and_adam(n, f, c, lr):
    """12 epochs in float32 against log_softmax / nll_loss / backward / torch.optim.Adam(weight_decay=...) on the CPU: the same
    weights within atol 5e-5 + rtol 1e-3 (two fp32 evaluations in different summation orders, each within 7.3e-6 of float64 at these
    sizes: the bound of the GPU test), the same (validation hits, test hits, epoch) of the best epoch."""
    from wdg_amd import synth
    labels = np.arange(n) * c // n
    M = synth.features(n, f, 11, labels=labels)
    train, val, test = split_ids(n, 5)
    W0 = xavier(f, c, torch.Generator().manual_seed(2))
    epochs, wd = 12, 5e-4
    W, m, v, best = head_train(M, labels, train, val, test, W0.numpy(), epochs=epochs, lr=lr, weight_decay=wd, dtype=np.float32)
    assert W.dtype == np.float32 and m.dtype == np.float32

    w = torch.nn.Parameter(W0.clone())
    opt = torch.optim.Adam([w], lr=lr, weight_decay=wd)
    Mt, y = torch.from_numpy(M), torch.from_numpy(labels)
    tr, va, te = (torch.from_numpy(i.astype(np.int64)) for i in (train, val, test))
    ref_best = (-1, 0, 0)
    for e in range(epochs):
        opt.zero_grad()
        loss = torch.nn.functional.nll_loss(torch.log_softmax(Mt @ w, 1)[tr], y[tr])
        loss.backward()
        opt.step()
        with torch.no_grad():
            pred = (Mt @ w).argmax(1)
            hv, ht = int((pred[va] == y[va]).sum()), int((pred[te] == y[te]).sum())
        if hv > ref_best[0]:
            ref_best = (hv, ht, e)
    np.testing.assert_allclose(W, w.detach().numpy(), rtol=1e-3, atol=5e-5)
    st = opt.state[w]
    np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=2e-3, atol=1e-9)
    assert best == ref_best


def test_restatement_continues_from_its_own_state():
    """a + b epochs == a epochs, then b more from the returned (W, m, v, best) with step0 = a: bit for bit in the restatement too"""
    from wdg_amd import synth
    n, f, c = 120, 33, 4
    labels = np.arange(n) * c // n
    M = synth.features(n, f, 3, labels=labels)
    sets = split_ids(n, 1)
    W0 = xavier(f, c, torch.Generator().manual_seed(0)).numpy()
    whole = head_train(M, labels, *sets, W0, epochs=12, lr=0.05)
    a = head_train(M, labels, *sets, W0, epochs=5, lr=0.05)
    b = head_train(M, labels, *sets, a[0], m=a[1], v=a[2], best=a[3], epochs=7, step0=5, lr=0.05)
    for x, y in zip(whole[:3], b[:3]):
        assert np.array_equal(x, y)
    assert whole[3] == b[3]


def test_head_train_job_layout_matches_header(tmp_path):
    """wdg_head_train_job: size and field offsets as gcc lays the header's struct out == the ctypes mirror (and the numpy record the
    front end fills)"""
    import wdg_amd._lib as L
    from wdg_amd import train
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(wdg_head_train_job));']
    for fname, _ in L.HeadTrainJob._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(wdg_head_train_job, {fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert got["size"] == ctypes.sizeof(L.HeadTrainJob) == train._HEAD_JOB_DTYPE.itemsize
    for fname, _ in L.HeadTrainJob._fields_:
        assert got[fname] == getattr(L.HeadTrainJob, fname).offset == train._HEAD_JOB_DTYPE.fields[fname][1], fname
    assert [f for f, _ in L.HeadTrainJob._fields_] == list(train._HEAD_JOB_DTYPE.names)


def test_argument_refusals_need_no_gpu():
    """the entry refuses what it does not hold before any launch - an error code and a message, null pointers suffice"""
    import wdg_amd._lib as L
    null = ctypes.c_void_p(0)
    adam = (0.01, 5e-4, 0.9, 0.999, 1e-8)
    call = lambda n_jobs, max_f, max_c, epochs, step0=0: L.lib.wdg_head_train_batched_f32(null, n_jobs, max_f, max_c, epochs, step0, *adam, null)  # noqa: E731
    unsupported, invalid = -4, -1  # WDG_ERR_UNSUPPORTED, WDG_ERR_INVALID
    assert call(3, 64, 5, 10) == invalid                 # null job table
    assert b"null" in L.lib.wdg_last_error()
    assert call(-1, 64, 5, 10) == invalid                # negative job count
    assert call(3, 64, 5, -1) == invalid                 # negative epoch count
    assert call(3, 64, 5, 10, -2) == invalid             # negative first step
    assert call(3, 64, 9, 10) == unsupported             # more classes than a workgroup holds
    assert call(3, 64, 0, 10) == unsupported
    assert call(3, 4097, 5, 10) == unsupported           # a wider head than a workgroup holds
    assert call(3, 0, 5, 10) == unsupported
    assert call(0, 64, 5, 10) == 0                       # nothing to do: no launch
    assert call(0, 4096, 8, 0) == 0
    assert L.lib.wdg_head_train_batched_f32(null, 3, 64, 5, 10, 0, 0.01, 5e-4, 1.0, 0.999, 1e-8, null) == invalid  # beta1 = 1 divides by zero
