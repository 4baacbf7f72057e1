"""tests/_acm_split_ref.py (the restatement of one replica of acm_split_train.AcmSplitTrainBatch) pinned against plain torch autograd
in fp64 on the CPU; the ctypes mirror and the numpy record type of wdg_acm_packed_job against include/wdg.h; and the refusals of the
packed channel mix's entry points, of wdg_acm_mix_packed_check_jobs, of ops.AcmMixPackedBatch and of ops.AcmSplitTrainBatch that need
no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _acm_split_ref as sref
from _split_train_ref import dense_a_hat

TOL = 1e-10


def _problem(n=40, f=9, c=4, seed=2):
    rng = np.random.default_rng(seed)
    pattern = (rng.random((n, n)) < 0.15).astype(np.float64)
    pattern[np.arange(n), np.arange(n)] = 1.0
    labels = rng.integers(0, c, n)
    labels[:c] = np.arange(c)
    perm = rng.permutation(n)
    masks = np.zeros((3, n), bool)
    masks[0, perm[:20]], masks[1, perm[20:30]], masks[2, perm[30:38]] = True, True, True
    return dict(n=n, f=f, c=c, a=dense_a_hat(torch.from_numpy(pattern), 0), x=rng.standard_normal((n, f)), labels=labels, masks=masks)


@pytest.mark.parametrize("kind,dropout", [("acm_sgc", 0.0), ("acm_gcn", 0.0), ("acm_gcn", 0.5)])
def test_first_step_gradients_match_torch_autograd_fp64(kind, dropout):
    p = _problem()
    w = sref.init_params(kind, p["f"], p["c"], 6, 5, 1)
    rep = sref.AcmReplica(kind, p["a"], p["x"], p["labels"], p["masks"], w, dropout=dropout, dropout_seed=7, stream=1)
    rep.backward(rep.loss_gradient(rep.forward(train=True)))
    params = [q.detach().clone().requires_grad_() for q in rep.params]
    keep_scale = None if rep.keep_scale is None else torch.from_numpy(rep.keep_scale)
    assert (keep_scale is not None) == (dropout > 0)
    train = torch.from_numpy(rep.train)
    logits = sref.torch_logits(kind, p["a"], torch.from_numpy(p["x"]), params, keep_scale)
    torch.nn.functional.cross_entropy(logits[train], torch.from_numpy(p["labels"])[train]).backward()
    for key, got, want in zip(rep.keys, rep.params, params):
        err = float((got.grad - want.grad).abs().max())
        assert err <= TOL * max(1.0, float(want.grad.abs().max())), (key, err)
        assert float(want.grad.abs().max()) > 0, key
    if kind == "acm_gcn":
        assert 0 < rep.min_abs_pre < 1  # the pre-activation closest to the ReLU's kink is recorded


def test_restatement_runs_in_float32_and_selects_strictly():
    p = _problem()
    w = sref.init_params("acm_gcn", p["f"], p["c"], 6, 5, 0)
    runs = [sref.AcmReplica("acm_gcn", p["a"], p["x"], p["labels"], p["masks"], w, dtype=dt).run(3) for dt in (torch.float32, torch.float64)]
    assert all(q.dtype == torch.float32 for q in runs[0][0]) and all(q.dtype == torch.float64 for q in runs[1][0])
    err = max(float((a.double() - b).abs().max()) for a, b in zip(*[r[0] for r in runs]))
    assert 0 < err < 1e-4, err
    hv, ht, step = runs[1][1]
    assert 0 <= hv <= 10 and 0 <= ht <= 8 and 0 <= step < 3


def test_pack_and_unpack_are_inverse():
    rng = np.random.default_rng(0)
    blocks = [rng.standard_normal((5, 3)).astype(np.float32) for _ in range(4)]
    packed = sref.pack(blocks, 8, fill=9.0, ld=40, offset=4)
    assert packed.shape == (5, 40) and (packed[:, :4] == 9.0).all() and (packed[:, 36:] == 9.0).all()
    got, pad = sref.unpack(packed, 4, 8, 3, offset=4)
    assert all(np.array_equal(a, b) for a, b in zip(got, blocks)) and pad.shape == (5, 4, 5) and (pad == 9.0).all()
    att = sref.pack_att([b[:3] for b in blocks], 4)
    assert att.shape == (4, 3, 4) and not att[:, :, 3].any() and np.array_equal(att[2, :, :3], blocks[2][:3])


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_packed_job_struct_matches_the_header(tmp_path):
    """size and field offsets of wdg_acm_packed_job as gcc lays them out == the ctypes mirror"""
    import wdg_amd._lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(wdg_acm_packed_job));']
    lines += [f'printf("{name} %zu\\n", offsetof(wdg_acm_packed_job, {name}));' for name, _ in L.AcmPackedJob._fields_]
    lines += ["return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.AcmPackedJob)
    for name, _ in L.AcmPackedJob._fields_:
        assert int(got[name]) == getattr(L.AcmPackedJob, name).offset, name


def test_packed_record_type_is_the_mirrors_layout():
    import wdg_amd._lib as L
    from wdg_amd.train import _ACM_PACKED_JOB_DTYPE as dtype
    st = L.AcmPackedJob
    assert dtype.itemsize == ctypes.sizeof(st) and list(dtype.names) == [name for name, _ in st._fields_]
    for name, ctype in st._fields_:
        assert dtype.fields[name][1] == getattr(st, name).offset, name
        assert dtype.fields[name][0].itemsize == ctypes.sizeof(ctype), name


def test_packed_entry_points_refuse_malformed_tables_without_a_device():
    import wdg_amd._lib as L
    null = ctypes.c_void_p(0)
    for fn in (L.lib.wdg_acm_mix_packed_f32, L.lib.wdg_acm_mix_packed_backward_f32):
        assert fn(null, 0, 8, 8, null) == 0          # nothing to do
        assert fn(null, 3, 8, 8, null) != 0          # a null table with jobs
        assert b"null job table" in L.lib.wdg_last_error()
        assert fn(null, -1, 8, 8, null) != 0         # negative counts
        assert fn(null, 1, -8, 8, null) != 0
        assert fn(null, 1, 8, -8, null) != 0
        assert fn(null, 65536, 8, 8, null) != 0      # more jobs than one launch takes
        assert b"65536" in L.lib.wdg_last_error()
        assert fn(null, 0, 8, 64 * 65535 + 1, null) != 0  # more column blocks than one launch takes


def _host_job(**over):
    """a well-formed one-job table on the host (the pointers are never followed: aligned made-up addresses), with fields overridden"""
    from wdg_amd.train import _ACM_PACKED_JOB_DTYPE as dtype
    tab = np.zeros(1, dtype)
    ptrs = ("low", "high", "high_agg", "ident", "att", "wmix", "out", "aux", "d_out", "d_low", "d_high", "d_ident", "d_att", "d_wmix", "partials")
    for i, k in enumerate(ptrs):
        tab[k] = 0x10000 * (i + 1)
    for k in dtype.names:
        if k.startswith("ld_"):
            tab[k] = 24
    tab["rows"], tab["reps"], tab["cols"], tab["stride"] = 10, 3, 5, 8
    for k, v in over.items():
        tab[k] = v
    return tab


def _check(tab):
    import wdg_amd._lib as L
    tab = np.ascontiguousarray(tab)
    rc = L.lib.wdg_acm_mix_packed_check_jobs(ctypes.c_void_p(tab.ctypes.data), tab.shape[0])
    return rc, L.lib.wdg_last_error()


def test_check_jobs_refuses_every_malformed_job_without_a_device():
    import wdg_amd._lib as L
    assert _check(_host_job())[0] == 0
    assert _check(_host_job(high_agg=0, ld_high_agg=0))[0] == 0                         # no aggregated high-pass operand: fine
    assert _check(_host_job(d_out=0, d_low=0, d_high=0, d_ident=0, d_att=0, d_wmix=0, partials=0))[0] == 0  # a forward-only job
    assert _check(_host_job(rows=0))[0] == 0
    assert _check(_host_job(rows=0, low=0, high=0, high_agg=0, ident=0, out=0, aux=0, d_out=0, d_low=0, d_high=0, d_ident=0, partials=0))[0] == 0
    assert _check(_host_job(rows=0, att=0))[0] != 0 and _check(_host_job(rows=0, d_wmix=0))[0] != 0  # (the sums are written all the same)
    assert L.lib.wdg_acm_mix_packed_check_jobs(ctypes.c_void_p(0), 0) == 0
    assert L.lib.wdg_acm_mix_packed_check_jobs(ctypes.c_void_p(0), 2) != 0               # a null table with jobs
    assert L.lib.wdg_acm_mix_packed_check_jobs(ctypes.c_void_p(0), -1) != 0
    for stride in (0, 2, 6, 12, 32):
        rc, msg = _check(_host_job(stride=stride, cols=1))
        assert rc != 0 and b"stride" in msg, stride
    for cols in (0, 9, -1):
        rc, msg = _check(_host_job(cols=cols))
        assert rc != 0 and b"column count" in msg, cols
    for reps in (0, -3):
        rc, msg = _check(_host_job(reps=reps))
        assert rc != 0 and b"replica" in msg, reps
    assert _check(_host_job(rows=-1))[0] != 0
    for k in ("low", "high", "ident", "att", "wmix", "out", "aux"):                      # a null required pointer
        rc, msg = _check(_host_job(**{k: 0}))
        assert rc != 0 and b"null" in msg, k
    for k in ("d_out", "d_low", "d_high", "d_ident", "d_att", "d_wmix", "partials"):    # the gradient arrays come together
        rc, msg = _check(_host_job(**{k: 0}))
        assert rc != 0 and b"null" in msg, k
    for k in ("low", "high", "high_agg", "ident", "att", "out", "aux", "d_out", "d_low", "d_high", "d_ident", "d_att", "partials"):
        rc, msg = _check(_host_job(**{k: 0x10004}))                                      # misaligned
        assert rc != 0 and b"aligned" in msg, k
    for k in ("ld_low", "ld_high", "ld_high_agg", "ld_ident", "ld_out", "ld_d_out", "ld_d_low", "ld_d_high", "ld_d_ident"):
        rc, msg = _check(_host_job(**{k: 20}))                                           # shorter than 3 replicas of 8
        assert rc != 0 and b"leading dimension" in msg, k
        rc, msg = _check(_host_job(**{k: 26}))                                           # no multiple of 4
        assert rc != 0 and b"aligned" in msg, k
    two = np.concatenate([_host_job(), _host_job(stride=5)])
    rc, msg = _check(two)
    assert rc != 0 and b"job 1" in msg


# ------------------------------------------------------------------------------------------------------------ the front ends
def test_packed_binding_refuses_what_the_kernel_does_not_take():
    """the checks of ops.AcmMixPackedBatch that come before any device is touched"""
    from wdg_amd import ops
    z = lambda *s: torch.zeros(s)  # noqa: E731

    def entry(rows=4, reps=3, stride=8, cols=5):
        w = reps * stride
        return dict(cols=cols, low=z(rows, w), high=z(rows, w), ident=z(rows, w), att=z(reps, 3, stride), wmix=z(reps, 3, 3), out=z(rows, w))

    with pytest.raises(ValueError, match="stride of 12"):
        ops.AcmMixPackedBatch([entry(stride=12)], False)
    with pytest.raises(ValueError, match="9 columns"):
        ops.AcmMixPackedBatch([entry(cols=9)], False)
    with pytest.raises(ValueError, match="0 columns"):
        ops.AcmMixPackedBatch([entry(cols=0)], False)
    with pytest.raises(ValueError, match="one activation flag per entry"):
        ops.AcmMixPackedBatch([entry()], [True, False])
    with pytest.raises(ValueError, match="required"):
        ops.AcmMixPackedBatch([{k: v for k, v in entry().items() if k != "wmix"}], False)
    with pytest.raises(ValueError, match="required"):
        ops.AcmMixPackedBatch([{k: v for k, v in entry().items() if k != "cols"}], False)
    with pytest.raises(ValueError, match="unknown keys"):
        ops.AcmMixPackedBatch([dict(entry(), out_t=z(4))], False)  # (there is no transposed output)
    with pytest.raises(ValueError, match="come together"):
        ops.AcmMixPackedBatch([dict(entry(), d_out=z(4, 24))], False)
    with pytest.raises(ValueError, match=r"att must be a \[reps >= 1, 3, stride\]"):
        ops.AcmMixPackedBatch([dict(entry(), att=z(3, 8))], False)
    with pytest.raises(ValueError, match="fp32 device matrix"):
        ops.AcmMixPackedBatch([entry()], False)  # host tensors
    with pytest.raises(ValueError, match="entries; one launch takes 65535"):
        ops.AcmMixPackedBatch([None] * 65536, False)


def test_trainer_refuses_before_it_asks_for_a_device():
    from wdg_amd import acm_split_train, ops
    assert ops.AcmSplitTrainBatch is acm_split_train.AcmSplitTrainBatch
    n = 12
    masks = np.zeros((2, 3, n), bool)
    masks[:, 0, :5], masks[:, 1, 5:9], masks[:, 2, 9:] = True, True, True
    labels, x = np.arange(n) % 3, np.zeros((n, 4), np.float32)
    make = lambda **kw: ops.AcmSplitTrainBatch(None, kw.pop("x", x), kw.pop("labels", labels), kw.pop("masks", masks), **kw)  # noqa: E731
    for kind in ("gcn", "sgc", "mlp1", "mlp2", "acm"):
        with pytest.raises(ValueError, match="SplitTrainBatch's"):
            make(kind=kind)
    with pytest.raises(ValueError, match="no hidden layer"):
        make(kind="acm_sgc", dropout=0.5)
    with pytest.raises(ValueError, match="drop probability"):
        make(kind="acm_gcn", dropout=1.0)
    for hidden in (0, 257):
        with pytest.raises(ValueError, match="1..256"):
            make(kind="acm_gcn", hidden=hidden)
    with pytest.raises(ValueError, match="17 classes"):
        make(labels=np.where(np.arange(n) == 0, 16, labels))
    with pytest.raises(ValueError, match="one lr"):
        make(lr=[0.01, 0.02])
    with pytest.raises(ValueError, match="masks must be a bool array"):
        make(masks=masks.astype(np.int32))
    empty = masks.copy()
    empty[1, 0] = False
    with pytest.raises(ValueError, match="at least one train row"):
        make(masks=empty)
    both = masks.copy()
    both[0, 1, 0] = True
    with pytest.raises(ValueError, match="overlap"):
        make(masks=both)
    with pytest.raises(ValueError, match="replica_ids"):
        make(replica_ids=[0, -1])
    assert [acm_split_train.class_stride(c) for c in (1, 4, 5, 7, 8, 9, 16)] == [4, 4, 8, 8, 8, 16, 16]


def test_split_train_batch_still_refuses_the_acm_kinds_and_says_where_they_live():
    from wdg_amd import split_train
    assert "AcmSplitTrainBatch" in split_train.SplitTrainBatch.__doc__
    with pytest.raises(ValueError, match="unknown model kind"):
        split_train.SplitTrainBatch(None, None, None, None, kind="acm_sgc")
