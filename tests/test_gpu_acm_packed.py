"""GPU tests of the packed ACM channel mix (csrc/acm_mix_packed.hip: wdg_acm_mix_packed_f32 and its backward pass, ops.AcmMixPackedBatch)
on one ragged table: every output against the fp64 restatement of tests/_acm_ref.py, per replica; bit equality with a one-job
ops.AcmMixBatch (csrc/acm_mix.hip) on every replica's column slices; and what the header promises of padding columns, repeated
launches, jobs alone, replicas in other jobs, NaN inputs and malformed jobs."""
import numpy as np
import pytest
import torch

import _acm_ref as ref
from _acm_split_ref import pack, pack_att, unpack

pytestmark = pytest.mark.gpu

ROWS = (0, 1, 63, 64, 65, 130)
SHAPES = ((4, 1), (4, 3), (4, 4), (8, 5), (8, 7), (8, 8), (16, 9), (16, 13), (16, 16))
# replicas per stride: a part-filled 64-column block, an exactly full one and a second one
REPS = {8: (1, 7, 8, 9), 4: (16, 17), 16: (4, 5)}
SENTINEL = 3.0e4   # what the padding columns of the inputs hold
MATS = ("low", "high", "high_agg", "ident", "d_out")
OUT_MATS = ("out", "d_low", "d_high", "d_ident")
OUTPUTS = ("out", "aux", "d_low", "d_high", "d_ident", "d_att", "d_wmix")


def _cases():
    """(rows, stride, cols, reps, relu, with high_agg, layout) - 24 jobs: every (stride, cols) with every replica count of its stride;
    the row counts cycle inside a stride (every stride meets every row count), the two flags and the layout cycle over all eight
    combinations"""
    out, i = [], 0
    for stride in (8, 4, 16):
        k = 0
        for s, cols in SHAPES:
            if s != stride:
                continue
            for reps in REPS[stride]:
                bits = (i + i // 8) % 8
                out.append((ROWS[k % 6], stride, cols, reps, bool(bits & 1), bool(bits & 2), "ranges" if bits & 4 else "plain"))
                i, k = i + 1, k + 1
    return out


CASES = _cases()


def _host(case, seed):
    """per-replica fp32 inputs of a job: {name: [reps] list of arrays}"""
    rows, stride, cols, reps, relu, with_agg, layout = case
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    h = {k: [f32(rng.standard_normal((rows, cols))) for _ in range(reps)] for k in MATS if k != "high_agg" or with_agg}
    h["att"] = [f32(rng.uniform(-1, 1, (3, cols)) / np.sqrt(cols)) for _ in range(reps)]
    h["wmix"] = [f32(rng.uniform(-1, 1, (3, 3)) / np.sqrt(3)) for _ in range(reps)]
    return h


def _device_matrix(per_replica, rows, reps, stride, layout, fill):
    """-> (the [rows, reps stride] device view, the tensor it is a view of)"""
    if per_replica is None:
        per_replica = [np.full((rows, stride), fill, np.float32)] * reps
    # (a device tensor first, the host array copied into it: numpy gives an array without elements strides of zero)
    if layout == "ranges":  # a column range of a wider matrix: 8 columns in, 12 more after it
        whole = torch.empty((rows, reps * stride + 20), device="cuda")
        whole.copy_(torch.from_numpy(pack(per_replica, stride, fill=fill, ld=reps * stride + 20, offset=8)))
        return whole[:, 8:8 + reps * stride], whole
    whole = torch.empty((rows, reps * stride), device="cuda")
    whole.copy_(torch.from_numpy(pack(per_replica, stride, fill=fill)))
    return whole, whole


def _entry(case, host, out_fill=float("nan")):
    """-> the entry of ops.AcmMixPackedBatch: inputs packed with SENTINEL in the padding columns, outputs prefilled with out_fill"""
    rows, stride, cols, reps, relu, with_agg, layout = case
    e = dict(cols=cols)
    for k in MATS:
        if k in host:
            e[k] = _device_matrix(host[k], rows, reps, stride, layout, SENTINEL)[0]
    for k in OUT_MATS:
        e[k], e["_whole_" + k] = _device_matrix(None, rows, reps, stride, layout, out_fill)
    e["att"] = torch.from_numpy(pack_att(host["att"], stride, fill=SENTINEL)).cuda()
    e["wmix"] = torch.from_numpy(np.stack(host["wmix"])).cuda()
    e["d_att"] = torch.full((reps, 3, stride), out_fill, device="cuda")
    e["d_wmix"] = torch.full((reps, 3, 3), out_fill, device="cuda")
    return e


def _public(e):
    return {k: v for k, v in e.items() if not k.startswith("_")}


def _results(entries, batch):
    got = [{k: e[k].cpu().numpy().copy() for k in OUTPUTS if k != "aux"} for e in entries]
    for g, aux in zip(got, batch.aux_of):
        g["aux"] = aux.cpu().numpy().copy()
    return got


def _replica(case, g, r):
    """replica r's outputs without the padding columns, in the shapes of a one-job ops.AcmMixBatch"""
    rows, stride, cols, reps = case[:4]
    res = {k: unpack(g[k], reps, stride, cols)[0][r] for k in OUT_MATS}
    res.update(aux=g["aux"][:, r], d_att=g["d_att"][r, :, :cols], d_wmix=g["d_wmix"][r])
    return res


@pytest.fixture(scope="module")
def table():
    """the ragged table, launched forward and backward once: (entries, host inputs, the batch, its results on the host)"""
    from wdg_amd import ops
    hosts = [_host(case, 50 + i) for i, case in enumerate(CASES)]
    entries = [_entry(case, h) for case, h in zip(CASES, hosts)]
    batch = ops.AcmMixPackedBatch([_public(e) for e in entries], [case[4] for case in CASES])
    batch.launch()
    batch.launch_backward()
    torch.cuda.synchronize()
    return entries, hosts, batch, _results(entries, batch)


def test_the_table_covers_what_it_is_meant_to():
    assert len(CASES) == 24
    assert {(c[1], c[2]) for c in CASES} == set(SHAPES)
    assert {(c[1], c[3]) for c in CASES} == {(s, r) for s, reps in REPS.items() for r in reps}
    assert {(c[1], c[0]) for c in CASES} == {(s, r) for s in (4, 8, 16) for r in ROWS}
    assert {(c[4], c[5], c[6]) for c in CASES} == {(a, b, l) for a in (False, True) for b in (False, True) for l in ("plain", "ranges")}
    # a part-filled column block, an exactly full one, a second one - at every stride
    for stride in (4, 8, 16):
        widths = {c[3] * stride for c in CASES if c[1] == stride}
        assert any(w < 64 or w % 64 for w in widths) and 64 in widths and any(w > 64 for w in widths), (stride, widths)


def _restated(host, r, relu, dtype):
    h = {k: v[r].astype(dtype) for k, v in host.items()}
    agg = h.get("high_agg")
    out, aux = ref.mix_forward(h["low"], h["high"], agg, h["ident"], h["att"], h["wmix"], relu)
    res = ref.mix_backward(h["low"], h["high"], agg, h["ident"], h["att"], h["wmix"], relu, h["d_out"])
    res.update(out=out, aux=aux)
    return res


def test_kernels_match_the_fp64_restatement(table):
    """every output of every replica of every job within 8 e32 + 2^-23 max |ref64| of the fp64 restatement, e32 = the largest
    difference between the restatement evaluated in fp32 and in fp64 on the same inputs (tests/test_gpu_acm.py's bound).  The largest
    error / bound per output is printed; DESIGN 4.19 records them."""
    entries, hosts, batch, got = table
    misses, worst = [], {}
    for i, (case, host, g) in enumerate(zip(CASES, hosts, got)):
        for r in range(case[3]):
            r64, r32, mine = _restated(host, r, case[4], np.float64), _restated(host, r, case[4], np.float32), _replica(case, g, r)
            for k in OUTPUTS:
                if r64[k].size == 0:
                    continue
                e32 = float(np.abs(r32[k].astype(np.float64) - r64[k]).max())
                bound = 8 * e32 + 2.0 ** -23 * float(np.abs(r64[k]).max())
                err = float(np.abs(mine[k].astype(np.float64) - r64[k]).max())
                ratio = err / bound if bound > 0 else (0.0 if err == 0 else np.inf)
                worst[k] = max(worst.get(k, 0.0), ratio)
                if not err <= bound:
                    misses.append(f"job {i} {case} replica {r} {k}: {err:.3e} > {bound:.3e}")
            assert not mine["aux"][:, 6:].any()
    print("largest error / bound per output:", {k: round(v, 3) for k, v in worst.items()})
    assert not misses, "\n".join(misses)


def test_every_replica_has_the_bits_of_a_one_job_acm_mix_batch(table):
    """out, aux, d_low, d_high, d_ident, d_att, d_wmix of every replica equal, elementwise with ==, what a one-job ops.AcmMixBatch
    computes for the replica's column slices of the SAME device matrices; the signs of zeros are compared on top of that (the packed
    kernel's ownership and orders of addition are acm_mix.hip's, so that this holds)"""
    from wdg_amd import ops
    entries, hosts, batch, got = table
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    differing = []
    for i, (case, e, host, g) in enumerate(zip(CASES, entries, hosts, got)):
        rows, stride, cols, reps, relu = case[:5]
        for r in range(reps):
            sl = slice(r * stride, r * stride + cols)
            one = dict(low=e["low"][:, sl], high=e["high"][:, sl], ident=e["ident"][:, sl], high_agg=e["high_agg"][:, sl] if "high_agg" in e else None,
                       att=e["att"][r, :, :cols].contiguous(), wmix=e["wmix"][r].contiguous(), out=z(rows, cols), d_out=e["d_out"][:, sl],
                       d_low=z(rows, cols), d_high=z(rows, cols), d_ident=z(rows, cols), d_att=z(3, cols), d_wmix=z(3, 3))
            b1 = ops.AcmMixBatch([one], relu)
            b1.launch()
            b1.launch_backward()
            want = {k: one[k].cpu().numpy() for k in OUTPUTS if k != "aux"}
            want["aux"] = b1.aux_of[0].cpu().numpy()
            mine = _replica(case, g, r)
            for k in OUTPUTS:
                if rows == 0 and k in OUT_MATS + ("aux",):
                    continue
                same = (mine[k] == want[k]) & (np.signbit(mine[k]) == np.signbit(want[k]))
                if not same.all():
                    differing.append(f"job {i} {case} replica {r} {k}: {int((~same).sum())} of {same.size} elements differ")
    assert not differing, "\n".join(differing[:40])


def test_padding_columns_are_written_as_plus_zero_and_nothing_else_is_touched(table):
    """the outputs were prefilled with NaN: the padding columns of out, d_low, d_high, d_ident and d_att are +0 (written, sign bit
    clear) although the inputs' padding holds a sentinel; the columns around a column range keep their NaN"""
    entries, hosts, batch, got = table
    for case, e, g in zip(CASES, entries, got):
        rows, stride, cols, reps, relu, with_agg, layout = case
        for k in OUT_MATS:
            body, pad = unpack(g[k], reps, stride, cols)
            assert not np.isnan(g[k]).any() and (pad == 0).all() and not np.signbit(pad).any(), (case, k)
            if layout == "ranges":
                whole = e["_whole_" + k].cpu().numpy()
                assert np.isnan(whole[:, :8]).all() and np.isnan(whole[:, 8 + reps * stride:]).all(), (case, k)
        pad = g["d_att"][:, :, cols:]
        assert not np.isnan(g["d_att"]).any() and (pad == 0).all() and not np.signbit(pad).any(), case
        assert not np.isnan(g["d_wmix"]).any() and not np.isnan(g["aux"]).any()
        if rows == 0:  # zero sums backward
            assert not g["d_att"].any() and not g["d_wmix"].any()


def test_a_second_launch_repeats_every_bit(table):
    entries, hosts, batch, got = table
    batch.launch()
    batch.launch_backward()
    torch.cuda.synchronize()
    for case, a, b in zip(CASES, got, _results(entries, batch)):
        for k in OUTPUTS:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (case, k)


@pytest.mark.parametrize("which", [1, 9, 14, 21])
def test_a_job_alone_answers_what_it_answers_in_the_table(table, which):
    from wdg_amd import ops
    entries, hosts, batch, got = table
    case = CASES[which]
    e = _entry(case, hosts[which])
    alone = ops.AcmMixPackedBatch([_public(e)], case[4])
    alone.launch()
    alone.launch_backward()
    torch.cuda.synchronize()
    res = _results([e], alone)[0]
    for k in OUTPUTS:
        assert np.array_equal(res[k].view(np.uint32), got[which][k].view(np.uint32)), (case, k)


def test_a_replica_answers_the_same_in_a_job_of_another_replica_count(table):
    """replicas 2 and 8 of the nine-replica jobs (the second of them sits in the second column block) as a job of two replicas, and as
    replicas 7 and 1 of a job of ten"""
    from wdg_amd import ops
    entries, hosts, batch, got = table
    for which, case in enumerate(CASES):
        if case[3] != 9:
            continue
        for reps, places in ((2, {0: 2, 1: 8}), (10, {7: 2, 1: 8})):
            host = {k: [v[places.get(r, 0)] for r in range(reps)] for k, v in hosts[which].items()}
            other = case[:3] + (reps,) + case[4:]
            e = _entry(other, host)
            b = ops.AcmMixPackedBatch([_public(e)], case[4])
            b.launch()
            b.launch_backward()
            torch.cuda.synchronize()
            res = _results([e], b)[0]
            for at, src in places.items():
                mine, want = _replica(other, res, at), _replica(case, got[which], src)
                for k in OUTPUTS:
                    assert np.array_equal(mine[k].view(np.uint32), want[k].view(np.uint32)), (case, reps, at, k)


@pytest.mark.parametrize("which", [5, 14, 21])
def test_a_nan_input_stays_in_its_replicas_row(table, which):
    """one NaN in `ident` of (row 1, one replica): out and the operand gradients are NaN in that replica's real columns of that row
    and nowhere else - the padding stays +0 -, d_att and d_wmix in that replica and in no other"""
    from wdg_amd import ops
    entries, hosts, batch, got = table
    case = CASES[which]
    rows, stride, cols, reps = case[:4]
    assert rows > 1
    bad = reps - 1
    host = {k: [a.copy() for a in v] for k, v in hosts[which].items()}
    host["ident"][bad][1, cols - 1] = np.nan
    e = _entry(case, host)
    b = ops.AcmMixPackedBatch([_public(e)], case[4])
    b.launch()
    b.launch_backward()
    torch.cuda.synchronize()
    res = _results([e], b)[0]
    for k in OUT_MATS:
        nan = np.isnan(res[k]).reshape(rows, reps, stride)
        want = np.zeros_like(nan)
        want[1, bad, :cols] = True
        if k != "out":  # (with the activation on, a unit that is switched off has the gradient 0: not NaN anywhere ELSE is the rule)
            assert not (nan & ~want).any(), k
            assert nan[1, bad, cols - 1] or k != "d_ident", k  # (the NaN unit itself keeps its NaN gradient)
        else:
            assert np.array_equal(nan, want), k
        pad = res[k].reshape(rows, reps, stride)[:, :, cols:]
        assert (pad == 0).all() and not np.signbit(pad).any(), k
    assert np.isnan(res["d_att"][bad, :, :cols]).any() and not np.isnan(np.delete(res["d_att"], bad, 0)).any()
    assert not res["d_att"][:, :, cols:].any()
    assert not np.isnan(np.delete(res["d_wmix"], bad, 0)).any()
    # every other replica's bits are those of the clean table
    for r in range(reps - 1):
        mine, want = _replica(case, res, r), _replica(case, got[which], r)
        for k in OUTPUTS:
            assert np.array_equal(mine[k].view(np.uint32), want[k].view(np.uint32)), (r, k)


@pytest.mark.parametrize("field,value", [("stride", 5), ("stride", 32), ("cols", 0), ("cols", 9), ("reps", 0), ("ld_low", 18), ("ld_out", 20),
                                         ("low", None), ("wmix", 0), ("d_att", 0)])
def test_a_malformed_job_in_a_table_is_left_untouched(table, field, value):
    """a table of two jobs whose second is damaged in device memory (the binding's own check is passed first, as a caller who fills the
    table by hand would bypass it): both launches leave every output of the damaged job as it was and answer the first as before"""
    from wdg_amd import ops
    from wdg_amd.train import _ACM_PACKED_JOB_DTYPE
    entries, hosts, batch, got = table
    a, bcase = 9, 2  # (job 2: stride 8, three replicas' worth of fields to damage)
    assert CASES[bcase][1] == 8 and CASES[bcase][0] > 1
    ea, eb = _entry(CASES[a], hosts[a]), _entry(CASES[bcase], hosts[bcase], out_fill=123.0)
    both = ops.AcmMixPackedBatch([_public(ea), _public(eb)], [CASES[a][4], CASES[bcase][4]])
    both.aux.fill_(123.0)
    tab = both.table.cpu().numpy().view(_ACM_PACKED_JOB_DTYPE).copy()
    tab[field][1] = tab[field][1] + 4 if value is None else value  # (None: a pointer moved off its 16-byte boundary)
    both.table.copy_(torch.from_numpy(tab.view(np.uint8)))
    both.launch()
    both.launch_backward()
    torch.cuda.synchronize()
    res = _results([ea, eb], both)
    for k in OUTPUTS:
        assert np.array_equal(res[0][k].view(np.uint32), got[a][k].view(np.uint32)), k
        assert (res[1][k] == 123.0).all(), (field, k)
