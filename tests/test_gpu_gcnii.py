"""csrc/gcnii.hip on the device against tests/_gcnii_ref.py: ONE table of the shared jobs (n at one below, at and one above the row block,
at 1, three blocks and a ragged tail, no rows; w in 1, 3, 4, 5, 16, 17, 32, 64, 65, 128; leading dimensions above w; one job on pointers 4
bytes off a 16-byte boundary; three (alpha, beta)) - S, out, d_P, d_H0 (from a non-zero tensor), the partial sums and d_W bit for bit
against the fp32 restatement and within the derived bound of fp64; the epilogue against the existing DropoutBatch; every job alone against
the job in the table; a second launch against the first; the offset job against its aligned twin; where a NaN goes."""
import numpy as np
import pytest
import torch

import _gcnii_ref as ref

pytestmark = pytest.mark.gpu

def _pitched(a, extra, offset, dev):
    """a device copy of the fp32 matrix a as a view with leading dimension cols + extra that starts `offset` floats past a 16-byte
    boundary (the storage behind it is filled with a number no result may show)"""
    r, c = a.shape
    ld = c + extra
    store = torch.full((r * ld + 8,), 777.0, dtype=torch.float32, device=dev)
    assert store.data_ptr() % 16 == 0
    view = store[offset:offset + r * ld].view(r, ld)[:, :c]
    view.copy_(torch.from_numpy(np.array(a, np.float32)))
    return view


def _step_word(step):
    return torch.tensor([step - (1 << 32) if step >= 1 << 31 else step], dtype=torch.int32, device="cuda")


def _entry(index, dev, backward=True, s=True):
    n, w, extra, offset, (alpha, beta) = ref.JOBS[index]
    x = ref.job_inputs(index)
    zeros = np.zeros((n, w), np.float32)
    e = dict(p=_pitched(x["P"], extra, offset, dev), h0=_pitched(x["H0"], extra, offset, dev), w=_pitched(x["W"], extra, offset, dev),
             out=_pitched(zeros, extra, offset, dev), s=_pitched(zeros, extra, offset, dev) if s else None, alpha=alpha, beta=beta,
             stream=ref.stream_of(index))
    if backward:
        e.update(d_out=_pitched(x["d_out"], extra, offset, dev), d_p=_pitched(zeros, extra, offset, dev), d_h0=_pitched(x["d_H0"], extra, offset, dev),
                 d_w=_pitched(np.zeros((w, w), np.float32), extra, offset, dev))
    return e


def _run(indices, act, p=0.0, step=0, backward=True, launches=1):
    """the jobs `indices` as one table: forward, backward and weight gradient, `launches` times (d_h0 put back before each) -> per job a
    dict of host arrays (S, out, d_P, d_H0, partial, d_W)"""
    from wdg_amd import ops
    dev = torch.device("cuda")
    entries = [_entry(i, dev, backward) for i in indices]
    table = ops.GcniiBatch(entries, p, ref.SEED, act=act)
    word = _step_word(step)
    for _ in range(launches):
        for i, e in zip(indices, entries):
            if backward:
                e["d_h0"].copy_(torch.from_numpy(np.array(ref.job_inputs(i)["d_H0"])))
        table.launch(word)
        if backward:
            table.launch_backward()
            table.launch_weight_grad()
    torch.cuda.synchronize()
    got = []
    for k, e in enumerate(entries):
        g = dict(S=e["s"], out=e["out"])
        if backward:
            w = e["w"].shape[0]
            g.update(d_P=e["d_p"], d_H0=e["d_h0"], d_W=e["d_w"], partial=table.partial_of[k].view(-(-e["p"].shape[0] // ref.ROW_BLOCK), w, w))
        got.append({name: t.cpu().numpy() for name, t in g.items()})
        for t in e.values():  # nothing was written outside the views
            if isinstance(t, torch.Tensor) and t.shape[0] > 1 and t.stride(0) > t.shape[1]:
                pad = torch.as_strided(t, (t.shape[0] - 1, t.stride(0) - t.shape[1]), (t.stride(0), 1), t.storage_offset() + t.shape[1])
                assert bool((pad == 777.0).all())
    return got


_TABLE = {}


def _table(act, p=0.0, step=0):
    key = (act, p, step)
    if key not in _TABLE:
        _TABLE[key] = _run(list(range(len(ref.JOBS))), act, p, step)
    return _TABLE[key]


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("act,p,step", [(False, 0.0, 0), (True, 0.0, 0), (True, 0.5, 3)])
def test_every_output_equals_the_fp32_restatement_bit_for_bit(act, p, step):
    got = _table(act, p, step)
    for i, g in enumerate(got):
        want = ref.job_reference(i, act, p, step)
        for name in ("S", "out", "d_P", "d_H0", "partial", "d_W"):
            assert _same_bits(g[name], want[name]), (i, ref.JOBS[i], name, np.abs(g[name] - want[name]).max(initial=0))


def test_every_output_lies_within_the_derived_bound_of_fp64():
    worst = {}
    for act, p, step in ((False, 0.0, 0), (True, 0.5, 3)):
        scale = float(ref._dropout_ref.constants(p)[1])
        for i, g in enumerate(_table(act, p, step)):
            n, w = ref.JOBS[i][:2]
            alpha, beta = ref.JOBS[i][4]
            x = ref.job_inputs(i)
            S, S_abs, Z, Z_abs = ref.forward64(x["P"], x["H0"], x["W"], alpha, beta)
            keep = ref._dropout_ref.keep_mask(n, w, p, ref.SEED, ref.stream_of(i), step) if n else np.zeros((n, w), bool)
            out64 = np.where(keep, np.maximum(Z, 0.0) * scale, 0.0) if act else Z
            ratios = dict(S=ref.within("S", g["S"], S, S_abs, n, w), out=ref.within("out" if act else "Z", g["out"], out64, Z_abs * scale, n, w))
            b = ref.backward64(x["d_out"], g["out"], g["S"], x["W"], alpha, beta, x["d_H0"], act, scale)
            for name in ("d_P", "d_H0", "d_W"):
                ratios[name] = ref.within(name, g[name], *b[name], n, w)
            for name, r in ratios.items():
                worst[name] = max(worst.get(name, 0.0), r)
    print("largest error / derived bound:", {k: round(v, 4) for k, v in worst.items()})
    assert all(r <= 1.0 for r in worst.values()), worst


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("step", [0, ref._dropout_ref.STEP_SIGNED])
def test_the_epilogue_is_the_existing_dropout_kernel_applied_to_the_plain_output(p, step):
    """act = 1 gives out bit-equal to ops.DropoutBatch (same seed, stream, step word) applied in place to the act = 0 output"""
    from wdg_amd import ops
    dev = torch.device("cuda")
    plain = _table(False)
    fused = _run(list(range(len(ref.JOBS))), True, p, step, backward=False)
    hs = [torch.zeros(g["out"].shape, dtype=torch.float32, device=dev) for g in plain]
    for h, g in zip(hs, plain):
        h.copy_(torch.from_numpy(g["out"].copy()))
    word = _step_word(step)
    ops.DropoutBatch([(h, None, ref.stream_of(i)) for i, h in enumerate(hs)], p, ref.SEED).launch(word)
    torch.cuda.synchronize()
    for i, (h, g) in enumerate(zip(hs, fused)):
        assert _same_bits(h.cpu().numpy(), g["out"]), (i, ref.JOBS[i])
    if p > 0:
        assert any((g["out"] == 0).mean() > 0.6 for g in fused if g["out"].size > 1000)  # (something was dropped)


def test_every_job_alone_equals_the_job_in_the_table_and_a_second_launch_repeats_the_first():
    table = _table(True, 0.5, 3)
    for i in range(len(ref.JOBS)):
        alone = _run([i], True, 0.5, 3)[0]
        for name, a in alone.items():
            assert _same_bits(a, table[i][name]), (i, name)
    twice = _run([4, 5, 7, 8], True, 0.5, 3, launches=2)
    for k, i in enumerate((4, 5, 7, 8)):
        for name, a in twice[k].items():
            assert _same_bits(a, table[i][name]), (i, name)


def test_the_offset_job_equals_its_aligned_twin_and_inference_writes_no_s():
    from wdg_amd import ops
    a, b = ref.OFFSET_PAIR
    for act, p, step in ((False, 0.0, 0), (True, 0.5, 3)):
        t = _table(act, p, step)
        for name in t[a]:
            assert _same_bits(t[a][name], t[b][name]), name
    dev = torch.device("cuda")
    e = _entry(5, dev, backward=False, s=False)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.GcniiBatch([e], 0.0, ref.SEED).launch(word)
    torch.cuda.synchronize()
    assert _same_bits(e["out"].cpu().numpy(), ref.job_reference(5, True, 0.0, 0)["out"])


def test_a_sub_range_of_the_table_launches_those_jobs_alone():
    from wdg_amd import ops
    dev = torch.device("cuda")
    entries = [_entry(i, dev) for i in (4, 5, 6)]
    table = ops.GcniiBatch(entries, 0.0, ref.SEED, act=False)
    table.launch(first=1, count=1)
    table.launch_backward(first=1, count=1)
    table.launch_weight_grad(first=1, count=1)
    torch.cuda.synchronize()
    want = ref.job_reference(5, False)
    assert _same_bits(entries[1]["out"].cpu().numpy(), want["out"]) and _same_bits(entries[1]["d_w"].cpu().numpy(), want["d_W"])
    for k in (0, 2):
        assert float(entries[k]["out"].abs().max()) == 0.0 and float(entries[k]["d_w"].abs().max()) == 0.0
    with pytest.raises(ValueError):
        table.launch(first=2, count=2)


def _same_bits_or_nan(a, b):
    """the same elements are NaN, the others have the same bits"""
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and _same_bits(a[~nan], b[~nan])


def test_a_nan_in_p_reaches_its_row_of_s_and_out_and_its_row_of_d_w_and_nothing_else():
    """P[i, k] = NaN: S[i, k], row i of out and row k of d_W are NaN and nothing else is; every other number is the restatement's of the
    same input - rows other than i of out, d_P and d_H0 are those of the input without the NaN (an element depends on its own row)"""
    from wdg_amd import ops
    dev = torch.device("cuda")
    i, k = 40, 9
    for index, act in ((5, True), (4, False)):
        alpha, beta = ref.JOBS[index][4]
        e = _entry(index, dev)
        e["p"][i, k] = float("nan")
        table = ops.GcniiBatch([e], 0.0, ref.SEED, act=act)
        table.launch(torch.zeros(1, dtype=torch.int32, device=dev))
        table.launch_backward()
        table.launch_weight_grad()
        torch.cuda.synchronize()
        x = ref.job_inputs(index)
        p_nan = np.array(x["P"])
        p_nan[i, k] = np.nan
        s_ref, z_ref = ref.forward32(p_nan, x["H0"], x["W"], alpha, beta)
        out_ref = ref.relu_dropout32(z_ref, 0.0, ref.SEED, ref.stream_of(index), 0) if act else z_ref
        d_p_ref, d_h0_ref, _, d_w_ref = ref.backward32(x["d_out"], out_ref, s_ref, x["W"], alpha, beta, x["d_H0"], act, np.float32(1.0))
        s, out, d_w, d_p, d_h0 = (e[name].cpu().numpy() for name in ("s", "out", "d_w", "d_p", "d_h0"))
        assert np.isnan(s[i, k]) and np.isnan(s).sum() == 1 and np.isnan(out[i]).all() and np.isnan(d_w[k]).all()
        assert np.isnan(out).sum() == out.shape[1] and np.isnan(d_w).sum() == d_w.shape[1]
        for got, want_nan in ((s, s_ref), (out, out_ref), (d_w, d_w_ref), (d_p, d_p_ref), (d_h0, d_h0_ref)):
            assert _same_bits_or_nan(got, want_nan)
        want = ref.job_reference(index, act)
        rows = np.arange(out.shape[0]) != i
        assert _same_bits(out[rows], want["out"][rows]) and _same_bits(d_p[rows], want["d_P"][rows]) and _same_bits(d_h0[rows], want["d_H0"][rows])
        assert not np.isnan(d_p[rows]).any() and not np.isnan(d_h0[rows]).any()
        if act:  # (the ReLU's backward pass reads out > 0: a NaN there is not positive, the row's gradient is +0)
            assert not np.isnan(d_p).any() and not np.isnan(d_h0).any()
        else:    # (without it dZ = d_out: the other rows of d_W are those of the input without the NaN)
            assert _same_bits(np.delete(d_w, k, 0), np.delete(want["d_W"], k, 0))
