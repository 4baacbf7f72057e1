"""CPU checks for wdg_relu_dropout_batched_f32 (include/wdg.h): the numpy restatement the GPU tests compare the kernel with draws
masks of the right rate that differ by seed, stream and step; the ctypes mirror of the job struct matches gcc's layout; the entry
refuses malformed arguments before any HIP call; the front end takes the new arguments."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from _dropout_ref import SHAPES, cached_keep_mask, constants, keep_mask, relu_dropout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, STREAMS, STEPS = 3, range(6), range(12)


@pytest.mark.parametrize("p", [0.5, 0.2, 0.9])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_keep_rate_of_every_mask(rows, cols, p):
    """6 streams x 12 steps per (shape, p): every mask keeps 1 - p of its elements within 4 binomial standard deviations (864 masks
    in all: a fair generator fails one of that many two-sided 4-sigma checks with probability 0.05; the worst here is 3.34), and no
    two of the 72 are the same mask"""
    n = rows * cols
    sigma = (p * (1 - p) / n) ** 0.5
    seen, worst = set(), 0.0
    for stream in STREAMS:
        for step in STEPS:
            m = cached_keep_mask(rows, cols, p, SEED, stream, step)
            z = abs(m.mean() - (1 - p)) / sigma
            worst = max(worst, z)
            assert z <= 4.0, (rows, cols, p, stream, step, z)
            seen.add(m.tobytes())
    print(f"({rows}, {cols}) p = {p}: worst keep rate {worst:.2f} sigma from 1 - p")
    assert len(seen) == len(STREAMS) * len(STEPS)


def test_seed_stream_and_step_each_change_the_mask():
    base = keep_mask(130, 64, 0.5, 3, 1, 7)
    assert np.array_equal(base, keep_mask(130, 64, 0.5, 3, 1, 7))
    for other in (keep_mask(130, 64, 0.5, 4, 1, 7), keep_mask(130, 64, 0.5, 3, 2, 7), keep_mask(130, 64, 0.5, 3, 1, 8),
                  keep_mask(130, 64, 0.5, 3, 7, 1), keep_mask(130, 64, 0.5, 3, 1, 7 + (1 << 31))):
        # (two independent fair masks of 8320 elements agree on half of them, sigma = 0.0055: the window is 9 sigma wide each way)
        assert 0.45 < (base == other).mean() < 0.55


def test_constants_and_values_of_the_restatement():
    assert constants(0.0) == (0, np.float32(1.0))
    assert constants(0.5) == (1 << 31, np.float32(2.0))
    assert constants(0.2) == (858993459, np.float32(1.25))
    assert constants(1.0 - 2.0 ** -53)[0] == (1 << 32) - 1
    h = np.array([[-1.5, 0.0, -0.0, 2.0, np.nan, 3.0, 1e-30]], np.float32)
    out = relu_dropout(h, 0.0, 3, 0, 0)  # p = 0: a plain ReLU, the NaN kept, the negative zero made positive
    assert np.array_equal(out.view(np.uint32), np.array([[0.0, 0.0, 0.0, 2.0, np.nan, 3.0, 1e-30]], np.float32).view(np.uint32))
    h = np.full((67, 5), 3.0, np.float32)
    h[5, 2] = np.nan
    out = relu_dropout(h, 0.2, 3, 9, 4)
    keep = keep_mask(67, 5, 0.2, 3, 9, 4)
    keep[5, 2] = False
    assert np.isnan(out[5, 2]) and np.all(out[keep] == np.float32(3.75)) and not keep.all()
    rest = ~keep
    rest[5, 2] = False
    assert np.all(out[rest].view(np.uint32) == 0)
    assert relu_dropout(np.zeros((0, 7), np.float32), 0.5, 1, 2, 3).shape == (0, 7)


def test_dropout_job_layout_matches_header(tmp_path):
    """wdg_dropout_job: size and field offsets as gcc lays the header's struct out == the ctypes mirror and the numpy record the
    front end fills"""
    import wdg_amd._lib as L
    from wdg_amd import train
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(wdg_dropout_job));']
    for fname, _ in L.DropoutJob._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(wdg_dropout_job, {fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert got["size"] == ctypes.sizeof(L.DropoutJob) == train._DROPOUT_JOB_DTYPE.itemsize
    for fname, _ in L.DropoutJob._fields_:
        assert got[fname] == getattr(L.DropoutJob, fname).offset == train._DROPOUT_JOB_DTYPE.fields[fname][1], fname
    assert [f for f, _ in L.DropoutJob._fields_] == list(train._DROPOUT_JOB_DTYPE.names)  # (the tail padding is in the itemsize, unnamed)


def test_argument_refusals_need_no_gpu():
    """the entry refuses malformed arguments before any HIP call - an error code and a message; null or made-up pointers suffice"""
    import wdg_amd._lib as L
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (`some`: non-null, never dereferenced - every call below ends before a launch)
    call = lambda table, n_jobs, max_rows, max_cols, step=some, scale=2.0: L.lib.wdg_relu_dropout_batched_f32(  # noqa: E731
        table, n_jobs, max_rows, max_cols, 1 << 31, scale, 3, step, null)
    invalid = -1  # WDG_ERR_INVALID
    assert call(null, 3, 600, 16) == invalid                       # null job table
    assert b"null job table" in L.lib.wdg_last_error()
    assert call(some, -1, 600, 16) == invalid                      # negative counts
    assert call(some, 3, -1, 16) == invalid
    assert call(some, 3, 600, -1) == invalid
    assert call(some, 3, 600, 16, step=null) == invalid            # no step word
    assert b"step" in L.lib.wdg_last_error()
    assert call(some, 3, 1 << 30, 16) == invalid                   # 2^30 rows x 4 groups = 2^32 groups: one too many for a 32-bit counter word
    assert call(some, 3, 1 << 30, 13) == invalid                   # (ceil(13 / 4) = 4 groups a row)
    assert call(some, 3, 65536, 262144) == invalid                 # 2^16 x 2^16 groups
    assert call(some, 65536, 600, 16) == invalid                   # one launch takes 65535 jobs
    assert b"65535" in L.lib.wdg_last_error()
    assert call(some, 3, 16, 64 * 65535 + 1) == invalid            # ... and 65535 tiles of 64 columns
    assert call(some, 3, 600, 16, scale=float("nan")) == invalid
    assert call(null, 0, 600, 16) == 0                             # nothing to do: no launch
    assert call(null, 0, 0, 0) == 0


def test_front_end_refusals_and_signatures_need_no_gpu():
    from wdg_amd import models, ops, sweep
    for cls in (models.GCN2, models.MLP2):
        par = inspect.signature(cls.__init__).parameters
        assert par["dropout_rng"].default is None and par["dropout"].default == 0.5
        assert cls(8, 3, nhid=4).dropout_rng is None and cls(8, 3, nhid=4, dropout_rng=None).dropout == 0.5
    par = inspect.signature(sweep.TrainBatch.__init__).parameters
    assert par["dropout"].default == 0.0 and par["dropout_seed"].default is None
    par = inspect.signature(models.DeviceDropout.__init__).parameters
    assert list(par) == ["self", "seed", "stream"] and par["stream"].default == 0
    for p in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.DropoutBatch([], p, 3)
    with pytest.raises(ValueError):
        ops.DropoutBatch([], 0.5, 1 << 32)
    assert ops.dropout_constants(0.5) == (1 << 31, 2.0) and ops.dropout_constants(0.0) == (0, 1.0)
    assert ops.dropout_constants(0.9) == tuple(float(v) if i else v for i, v in enumerate(constants(0.9)))
