"""GPU tests of the attention-score kernels (csrc/gat_scores.hip: wdg_gat_scores_forward_batched_f32, wdg_gat_scores_backward_batched_f32)
through ops.GatScoresBatch: ONE table of jobs whose S, d_H and d_att must equal the fp32 numpy restatement of tests/_gat_scores_ref.py
BIT FOR BIT (include/wdg.h states every chain and every sum's order; tests/test_gat_scores_ref.py bounds that restatement against fp64 on
the CPU), and the exact properties the header states."""
import numpy as np
import pytest
import torch

import _gat_scores_ref as ref

pytestmark = pytest.mark.gpu

CANARY = 777.0
ROWS = (0, 1, 3, 65)  # 65 = two blocks of WDG_GAT_SCORES_ROW_BLOCK rows plus 1
# (G, heads, w): one group; groups of an odd width; a ragged last block (8 + 2); a width that is no multiple of 4; groups wider than the
# 16 columns a forward thread keeps in registers (33: scalar, 64: 16-byte loads); 15 forward tiles of 64 groups and 8 backward tiles
SHAPES = ((1, 1, 1), (3, 1, 5), (10, 8, 8), (16, 8, 7), (6, 2, 33), (4, 4, 64), (960, 8, 8))
# "plain" = contiguous operands, "slices" = every operand a column slice, one float in, of a wider matrix with an ODD leading dimension
# (scalar accesses), "wide16" = slices that keep the 16-byte alignment (the vector path on a slice, where w allows it)
LAYOUTS = ("plain", "slices", "wide16")
JOBS = [(n, shape, LAYOUTS[(i + k) % 3]) for i, shape in enumerate(SHAPES) for k, n in enumerate(ROWS)]
JOBS += [(65, shape, layout) for shape in SHAPES for layout in LAYOUTS if (65, shape, layout) not in JOBS]


def _view(rows, cols, layout, fill=None):
    """-> (view [rows, cols], the buffer around it): a canary row above and below and, in the sliced layouts, canary columns left and
    right of the view"""
    left, right = {"plain": (0, 0), "slices": (1, 1 if cols % 2 else 2), "wide16": (4, 4 + (-cols) % 4)}[layout]  # (slices: an odd pitch)
    full = torch.full((rows + 2, left + cols + right), CANARY, device="cuda")
    v = full[1:rows + 1, left:left + cols]
    if fill is not None:
        v.copy_(torch.from_numpy(fill))
    return v, full


def _canaries_intact(full, view):
    mask = torch.ones_like(full, dtype=torch.bool)
    r0 = (view.data_ptr() - full.data_ptr()) // 4 // full.stride(0)
    c0 = (view.data_ptr() - full.data_ptr()) // 4 % full.stride(0)
    mask[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = False
    return bool((full[mask] == CANARY).all())


def _entry(job, seed, att=None):
    """-> (the entry of ops.GatScoresBatch, its fp32 host inputs, the buffers around its outputs, the flat views of the outputs)"""
    n, (G, heads, w), layout = job
    rng = np.random.default_rng(seed)
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    host = dict(h=f32(n, G * w), att=f32(2, G, w) if att is None else att, d_s=f32(n, 2 * G), d_h=f32(n, G * w))  # (d_h: what is there already)
    e, around, flat = dict(heads=heads), {}, {}
    for k, cols in (("h", G * w), ("d_s", 2 * G)):
        e[k], _ = _view(n, cols, layout, host[k])
    flat["att"], _ = _view(2, G * w, layout, host["att"].reshape(2, G * w))
    e["att"] = flat["att"].unflatten(1, (G, w))
    e["s"], around["s"] = _view(n, 2 * G, layout)
    e["d_h"], around["d_h"] = _view(n, G * w, layout, host["d_h"])
    flat["d_att"], around["d_att"] = _view(2, G * w, layout)
    e["d_att"] = flat["d_att"].unflatten(1, (G, w))
    return e, host, around, flat


@pytest.fixture(scope="module")
def table():
    """the table over JOBS, launched forward and backward once -> dict(entries, hosts, arounds, want: the restatement, got: clones)"""
    from wdg_amd import ops
    made = [_entry(job, 100 + i) for i, job in enumerate(JOBS)]
    entries, hosts, arounds = [m[0] for m in made], [m[1] for m in made], [m[2] for m in made]
    tab = ops.GatScoresBatch(entries)
    tab.launch()
    tab.launch_backward()
    torch.cuda.synchronize()
    got = [{k: e[k].cpu().numpy().copy() for k in ("s", "d_h", "d_att")} for e in entries]
    want = []
    for (n, (G, heads, w), _), host in zip(JOBS, hosts):
        d_h, d_att, _ = ref.backward32(host["h"], host["att"], heads, host["d_s"], host["d_h"])
        want.append(dict(s=ref.forward32(host["h"], host["att"], heads), d_h=d_h, d_att=d_att))
    return dict(tab=tab, entries=entries, hosts=hosts, arounds=arounds, got=got, want=want)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_table_equals_the_fp32_restatement_bit_for_bit(table):
    for job, got, want, around, e in zip(JOBS, table["got"], table["want"], table["arounds"], table["entries"]):
        if job[0] == 0:  # the n = 0 job touches nothing: its d_att holds what it held
            assert (got["d_att"] == CANARY).all(), job
        else:
            for k in ("s", "d_h", "d_att"):
                assert _same_bits(got[k], want[k]), (job, k, float(np.abs(got[k] - want[k]).max()))
        for k, full in around.items():
            view = e[k] if k != "d_att" else e[k].flatten(1)
            assert _canaries_intact(full, view), (job, k)


def test_a_second_launch_repeats_the_first(table):
    for e, host in zip(table["entries"], table["hosts"]):
        e["s"].fill_(CANARY)
        e["d_h"].copy_(torch.from_numpy(host["d_h"]))  # (d_h is added to: what was there before the first launch)
    table["tab"].launch()
    table["tab"].launch_backward()
    torch.cuda.synchronize()
    for job, e, got in zip(JOBS, table["entries"], table["got"]):
        if job[0] == 0:
            continue
        for k in ("s", "d_h", "d_att"):
            assert _same_bits(e[k].cpu().numpy(), got[k]), (job, k)


def test_every_job_alone_equals_the_job_in_the_table(table):
    from wdg_amd import ops
    for i, (job, got) in enumerate(zip(JOBS, table["got"])):
        if job[0] == 0:
            continue
        e, _, _, _ = _entry(job, 100 + i)  # the same inputs, in buffers of its own
        alone = ops.GatScoresBatch([e])
        alone.launch()
        alone.launch_backward()
        for k in ("s", "d_h", "d_att"):
            assert _same_bits(e[k].cpu().numpy(), got[k]), (job, k)


@pytest.mark.parametrize("job", [(65, (10, 8, 8), "plain"), (65, (3, 1, 5), "slices"), (3, (6, 2, 33), "wide16")])
def test_unit_vector_and_zero_attention(job):
    from wdg_amd import ops
    n, (G, heads, w), _ = job
    dst, _ = ref.score_columns(G, heads)
    for k in (0, w - 1):
        att = np.zeros((2, G, w), np.float32)
        att[0, :, k] = 1.0  # a_dst = e_k: the dst score IS column k of the group
        e, host, _, _ = _entry(job, 7, att)
        ops.GatScoresBatch([e]).launch()
        assert _same_bits(e["s"].cpu().numpy()[:, dst], np.ascontiguousarray(host["h"].reshape(n, G, w)[:, :, k]))
    e, host, _, _ = _entry(job, 8, np.zeros((2, G, w), np.float32))
    tab = ops.GatScoresBatch([e])
    tab.launch_backward()
    assert _same_bits(e["d_h"].cpu().numpy(), host["d_h"])  # att = 0: d_h is unchanged
    assert (e["s"] == CANARY).all()  # (and a backward launch writes no score)


@pytest.mark.parametrize("job,i,g,k", [((65, (10, 8, 8), "plain"), 40, 9, 3), ((3, (3, 1, 5), "slices"), 2, 1, 4), ((65, (960, 8, 8), "wide16"), 64, 517, 0)])
def test_a_nan_reaches_its_own_scores_and_its_own_column_of_d_att(job, i, g, k):
    from wdg_amd import ops
    n, (G, heads, w), _ = job
    e, host, _, _ = _entry(job, 9)
    e["h"][i, g * w + k] = float("nan")
    tab = ops.GatScoresBatch([e])
    tab.launch()
    tab.launch_backward()
    dst, src = ref.score_columns(G, heads)
    s, d_h, d_att = (e[key].cpu().numpy() for key in ("s", "d_h", "d_att"))
    want_s = np.zeros((n, 2 * G), bool)
    want_s[i, dst[g]] = want_s[i, src[g]] = True
    assert np.array_equal(np.isnan(s), want_s)
    want_att = np.zeros((2, G, w), bool)
    want_att[:, g, k] = True
    assert np.array_equal(np.isnan(d_att), want_att) and not np.isnan(d_att[:, np.arange(G) != g]).any()
    assert not np.isnan(d_h).any()
