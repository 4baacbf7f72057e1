"""GPU tests of the polynomial-filter kernel (csrc/poly_filter.hip: wdg_poly_filter_batched_f32) through ops.PolyFilterBatch, against
the fp64 restatement of tests/_poly_filter_ref.py with a DERIVED bound: for every element |out - ref| <= K 2^-24 companion, K from
_poly_filter_ref.bound_factors (its docstring has the derivation: the roundings of a hop on the longest row, times the hops, plus the
accumulation).  The largest ratio error / bound is printed; DESIGN 4.28 records it.  The dot products are compared for EQUAL BITS with
the restatement of their fp64 order applied to the kernel's OWN T_k: the kernel does not expose T_k, but a job whose coefficients are
the unit vectors returns exactly T_k in segment k (the header says so), and a probe job of that kind runs beside every case.  And the
exact properties the header states.

One property is worded more narrowly than the issue that asked for these tests words it: all-zero input gives +0 in every bit when the
segment has a coefficient that is not negative (the cases have a +0 among theirs, as the issue asks); with only negative coefficients
gamma_0 * +0 is -0 and stays -0 - the arithmetic the same issue prescribes - which the order-0 test covers."""
import numpy as np
import pytest
import torch

import _poly_filter_ref as ref
from test_gpu_signed_att import CANARY, _canaries_intact, _p0, _p1, _p3, _p65, _p140, _rows_to_csr, _view  # noqa: F401

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TEAMS = 256        # 1024 threads in teams of 4
RING_N = 20448     # wdg_poly_filter_max_rows(1)


def _pteams():
    """one row more than the workgroup has teams: team 0 takes a second row; 0 .. 9 entries each, directed"""
    rng = np.random.default_rng(129)
    return _rows_to_csr([np.sort(rng.choice(TEAMS + 1, int(rng.integers(0, 10)), replace=False)) for _ in range(TEAMS + 1)])


def _p1025():
    """one row more than the workgroup has lanes: every team takes four rows, team 0 a fifth; 0 .. 8 entries each, directed"""
    rng = np.random.default_rng(1025)
    return _rows_to_csr([np.sort(rng.choice(1025, int(rng.integers(0, 9)), replace=False)) for _ in range(1025)])


def _plong():
    """300 directed rows around the long-row threshold: rows of 127, 128 (the last with a team of 4), 129 and 299 entries (a wave each;
    rows 3 and 64 share a block of 64 rows only with short ones, rows 130 and 131 sit side by side), 0 .. 12 elsewhere"""
    rng = np.random.default_rng(300)
    n, lengths = 300, {1: 127, 2: 128, 3: 129, 64: 299, 130: 129, 131: 300, 299: 130}
    return _rows_to_csr([np.sort(rng.choice(n, lengths.get(i, int(rng.integers(0, 13))), replace=False)) for i in range(n)])


def _ring():
    """row i stores i - 1 and i + 1 (mod n) at the largest n that one column admits"""
    i = np.arange(RING_N)
    return np.arange(RING_N + 1, dtype=np.int32) * 2, np.sort(np.stack([(i - 1) % RING_N, (i + 1) % RING_N], 1), 1).reshape(-1).astype(np.int32)


PATTERNS = {"p0": _p0, "p1": _p1, "p3": _p3, "p65": _p65, "p140": _p140, "pteams": _pteams, "p1025": _p1025, "plong": _plong, "ring": _ring}
WEIGHTED = {"p140w": "p140", "plongw": "plong"}   # the same patterns with stored values in 0.5 .. 2 (the others: a binary adjacency, no values)
# (pattern, cols, seg_cols, order, layout, scales, dots): layouts as in test_gpu_signed_att - "plain" contiguous, "slices" column slices
# with an ODD leading dimension, "wide16" slices that keep 16-byte alignment (gamma and dots follow the layout: slices of wider matrices)
CASES = [("p0", 4, 4, 2, "plain", "both", True), ("p1", 1, 1, 10, "plain", "row", True), ("p3", 3, 3, 2, "slices", "both", True),
         ("p3", 8, 1, 1, "plain", "none", True), ("p65", 5, 5, 10, "slices", "both", True), ("p65", 4, 4, 0, "wide16", "row", True),
         ("p140", 1, 1, 10, "plain", "both", True), ("p140", 7, 7, 10, "plain", "row", True), ("p140", 12, 4, 2, "wide16", "both", True),
         ("p140", 10, 5, 10, "slices", "both", True), ("p140", 8, 8, 1, "plain", "none", False), ("p140", 12, 12, 10, "slices", "none", True),
         ("pteams", 7, 7, 2, "plain", "both", True), ("plong", 5, 5, 2, "slices", "both", True), ("plong", 8, 4, 10, "plain", "row", True),
         ("ring", 1, 1, 3, "plain", "both", True), ("p140w", 7, 7, 10, "plain", "both", True), ("p140w", 10, 5, 2, "slices", "none", True),
         ("plongw", 4, 4, 10, "wide16", "both", True), ("p1025", 3, 3, 2, "slices", "both", True)]
RING = 15  # the ring's place in CASES
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731


@pytest.fixture(scope="module")
def graphs():
    """{name: (the CsrGraph, the host pattern, its fp32 values or None)}"""
    from wdg_amd import ops
    out = {}
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()  # noqa: E731
    for name, make in PATTERNS.items():
        rowptr, col = make()
        n = len(rowptr) - 1
        out[name] = (ops.CsrGraph(i32(rowptr), i32(col), None, n, n), (rowptr, col), None)
    for name, of in WEIGHTED.items():
        rowptr, col = out[of][1]
        val = np.random.default_rng(len(col)).uniform(0.5, 2.0, len(col)).astype(np.float32)
        out[name] = (ops.CsrGraph(i32(rowptr), i32(col), torch.from_numpy(val).cuda(), len(rowptr) - 1, len(rowptr) - 1), (rowptr, col), val)
        assert not out[name][0].unit_values and out[of][0].unit_values
    lengths = np.diff(out["plong"][1][0])
    assert {127, 128, 129, 300} <= set(lengths.tolist()) and np.diff(out["p140"][1][0]).max() == 130
    assert {0, 1, 8, 9} <= set(np.diff(out["p140"][1][0]).tolist()) | set(np.diff(out["p65"][1][0]).tolist())  # a lane's chain of one entry and of two
    return out


def _gamma(rng, order, n_seg):
    """coefficients of random sign; from order 2 on every segment has a positive gamma_0, a negative gamma_1 and a +0 among its others"""
    g = rng.uniform(0.3, 1.0, (order + 1, n_seg)) * rng.choice([-1.0, 1.0], (order + 1, n_seg))
    if order >= 2:
        g[0], g[1], g[order // 2 + 1 if order > 2 else 2] = np.abs(g[0]), -np.abs(g[1]), 0.0
    return g.astype(np.float32)


def _entry(case, seed, graphs, group=None):
    """-> (the entry of ops.PolyFilterBatch, its fp32 host inputs, the buffers around its outputs)"""
    name, cols, seg_cols, order, layout, scales, dots = case
    g, (rowptr, _), _ = graphs[name]
    n, rng, n_seg = g.n_rows, np.random.default_rng(seed), cols // seg_cols
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    deg = np.maximum(np.diff(rowptr), 1)
    host = dict(v=f32(rng.standard_normal((n, cols))), u=f32(rng.standard_normal((n, cols))) if dots else None, gamma=_gamma(rng, order, n_seg),
                row_scale=f32(rng.uniform(0.5, 1.5, n) / deg) if scales in ("both", "row") else None,   # about a random-walk normalisation
                col_scale=f32(rng.uniform(0.5, 1.5, n)) if scales == "both" else None)
    e, around = dict(graph=g, order=order, seg_cols=seg_cols), {}
    if group is not None:
        e["group"] = group
    for k, shape in (("v", (n, cols)), ("u", (n, cols)), ("gamma", (order + 1, n_seg))):
        if host[k] is not None:
            e[k], _ = _view(*shape, layout, host[k])
    for k in ("row_scale", "col_scale"):
        if host[k] is not None:
            e[k] = torch.from_numpy(host[k]).cuda()
    e["out"], around["out"] = _view(n, cols, layout)
    if dots:
        e["dots"], around["dots"] = _view(order + 1, n_seg, layout)
    return e, host, around


def _probe(case, e):
    """the job that returns the kernel's own T_k: the case's pattern, scales and v in order + 1 segments, segment k with the
    coefficients e_k (out = fmaf(1, T_k, +-0) there)"""
    cols, order = case[1], case[3]
    v = e["v"].repeat(1, order + 1).contiguous()
    p = dict(graph=e["graph"], order=order, seg_cols=max(cols, 1), v=v, out=torch.full_like(v, 5.0), gamma=torch.eye(order + 1, device="cuda"))
    p.update({k: e[k] for k in ("row_scale", "col_scale") if k in e})
    return p


def _restated(case, host, graphs):
    rowptr, col = graphs[case[0]][1]
    val = graphs[case[0]][2]
    x = {k: None if v is None else v.astype(np.float64) for k, v in host.items()}
    return ref.forward(rowptr, col, x["v"], x["gamma"], case[2], x["row_scale"], x["col_scale"], x["u"], None if val is None else val.astype(np.float64))


def _factors(case, graphs):
    """the bound's factors of a case: `weighted` where an entry's coefficient is the rounded product of a value and a col_scale"""
    return ref.bound_factors(graphs[case[0]][1][0], case[3], weighted=graphs[case[0]][2] is not None and case[5] == "both")


def _results(entries):
    return [{k: e[k].cpu().numpy().copy() for k in ("out", "dots") if k in e} for e in entries]


def _launch(entries):
    from wdg_amd import ops
    batch = ops.PolyFilterBatch(entries)
    batch.launch()
    torch.cuda.synchronize()
    return batch


@pytest.fixture(scope="module")
def table(graphs):
    """the mixed table - jobs of 0 .. 20448 rows, groups of 4, 2 and 1, with and without dots share a launch -, run once, and the
    probes' table: (entries, host inputs, the batch, results on the host, the buffers around the outputs, the fp64 restatement, the
    kernel's T_k of every case)"""
    built = [_entry(case, 70 + i, graphs) for i, case in enumerate(CASES)]
    entries, hosts, around = [b[0] for b in built], [b[1] for b in built], [b[2] for b in built]
    batch = _launch(entries)
    restated = [_restated(case, host, graphs) for case, host in zip(CASES, hosts)]  # (computed once, shared, never changed)
    probes = [_probe(case, e) for case, e in zip(CASES, entries)]
    _launch(probes)
    t_own = [[p["out"][:, k * c[1]:(k + 1) * c[1]].cpu().numpy().copy() for k in range(c[3] + 1)] for c, p in zip(CASES, probes)]
    return entries, hosts, batch, _results(entries), around, restated, t_own


def _ratio(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)), initial=0.0))


def test_the_table_mixes_groups_and_dots(table):
    batch = table[2]
    assert set(batch.groups) == {4, 1} and batch.max_dot_rows == 11 and batch.max_floats == RING_N and batch.max_groups == 8


def test_out_matches_the_fp64_restatement_within_the_derived_bound(table, graphs):
    got, restated, t_own = table[3], table[5], table[6]
    misses, worst = [], 0.0
    for i, (case, g_, r) in enumerate(zip(CASES, got, restated)):
        ks = _factors(case, graphs)
        if r["out"].size == 0:
            assert g_["out"].size == 0
            continue
        ratio = _ratio(np.abs(g_["out"].astype(np.float64) - r["out"]), ks["out"] * U * r["out_abs"])
        for k, tk in enumerate(t_own[i]):                            # the probes' T_k are outputs of the kernel as well: k r roundings, stated k r + 2
            ratio = max(ratio, _ratio(np.abs(tk.astype(np.float64) - r["t"][k]), (k * ks["r"] + 2) * U * r["t_abs"][k]))
        worst = max(worst, ratio)
        print(f"job {i} {case}: r {ks['r']} K {ks['out']:.0f} largest error / bound {ratio:.4f}")
        if not ratio <= 1.0:
            misses.append(f"job {i} {case}: error / bound {ratio:.3e}")
    print(f"largest error / bound (out, T_k): {worst:.4f}")
    assert not misses, "\n".join(misses)
    assert worst > 0                                                  # (the comparison is not vacuous)


def test_dots_equal_the_restated_order_on_the_kernels_own_hops_bit_for_bit(table, graphs):
    hosts, got, restated, t_own = table[1], table[3], table[5], table[6]
    seen, worst = 0, 0.0
    for i, case in enumerate(CASES):
        if not case[6]:
            continue
        want = ref.dots_bits(t_own[i], hosts[i]["u"], case[2])
        assert np.array_equal(bits(got[i]["dots"]), bits(want)), case
        ks = _factors(case, graphs)                                  # ... and within the derived bound of the fp64 value
        ratio = _ratio(np.abs(got[i]["dots"].astype(np.float64) - restated[i]["dots"]), ks["dots"][:, None] * U * restated[i]["dots_abs"])
        worst = max(worst, ratio)
        assert ratio <= 1.0, (case, ratio)
        seen += 1
    print(f"largest error / bound (dots): {worst:.4f}")
    assert seen == len(CASES) - 1


def test_rows_beyond_a_job_and_columns_beside_it_are_untouched(table):
    entries, around = table[0], table[4]
    for case, e, bufs in zip(CASES, entries, around):
        for k, full in bufs.items():
            assert _canaries_intact(full, e[k]), (case, k)


def test_a_second_launch_repeats_every_bit(table):
    entries, batch, got = table[0], table[2], table[3]
    for e in entries:  # (what the launch writes is cleared first: a stale value would not pass for a repeated one)
        e["out"].fill_(5.0)
        if "dots" in e:
            e["dots"].fill_(5.0)
    batch.partials.fill_(5.0)
    batch.launch()
    torch.cuda.synchronize()
    for case, a, b in zip(CASES, got, _results(entries)):
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), (case, k)


def test_a_job_alone_answers_what_it_answers_in_the_table(table, graphs):
    got = table[3]
    for i, case in enumerate(CASES):
        if case[0] == "ring":
            continue
        e, _, _ = _entry(case, 70 + i, graphs)
        _launch([e])
        res = _results([e])[0]
        for k in got[i]:
            assert np.array_equal(bits(got[i][k]), bits(res[k])), (case, k)


def test_group_widths_1_2_and_4_give_equal_bits(table, graphs):
    got = table[3]
    seen = 0
    for i, case in enumerate(CASES):
        if case[0] in ("ring", "p0", "p1"):
            continue
        built = [_entry(case, 70 + i, graphs, group=g) for g in (1, 2, 4)]
        batch = _launch([b[0] for b in built])                        # the three widths share a launch
        assert batch.groups == [1, 2, 4]
        for g, res in zip((1, 2, 4), _results([b[0] for b in built])):
            for k in got[i]:
                assert np.array_equal(bits(got[i][k]), bits(res[k])), (case, g, k)
        seen += 1
    assert seen >= 12


def test_a_segment_has_the_bits_of_a_one_segment_job_on_its_slice(table):
    """v, u, out and the segment's column of gamma are passed IN PLACE (slices with the job's leading dimensions)"""
    entries, got = table[0], table[3]
    seen = 0
    for i, case in enumerate(CASES):
        cols, seg_cols, order = case[1:4]
        n_seg = cols // seg_cols
        if n_seg == 1 or case[0] == "p0":
            continue
        e = entries[i]
        for s in {0, n_seg - 1, n_seg // 2}:
            sl = slice(s * seg_cols, (s + 1) * seg_cols)
            one = dict(graph=e["graph"], order=order, v=e["v"][:, sl], out=torch.full_like(e["out"][:, sl], 5.0), gamma=e["gamma"][:, s:s + 1])
            one.update({k: e[k] for k in ("row_scale", "col_scale") if k in e})
            if "u" in e:
                one["u"], one["dots"] = e["u"][:, sl], torch.full((order + 1, 1), 5.0, device="cuda")
            _launch([one])
            assert np.array_equal(bits(one["out"].cpu().numpy()), bits(got[i]["out"][:, sl])), (case, s)
            if "u" in e:
                assert np.array_equal(bits(one["dots"].cpu().numpy()[:, 0]), bits(got[i]["dots"][:, s])), (case, s)
            seen += 1
    assert seen >= 8


def test_order_zero_is_exactly_gamma_0_times_v(table, graphs):
    hosts, got = table[1], table[3]
    i = next(k for k, c in enumerate(CASES) if c[3] == 0)
    assert np.array_equal(bits(got[i]["out"]), bits(hosts[i]["gamma"][0, 0] * hosts[i]["v"]))
    g = graphs["p140"][0]
    v = torch.from_numpy(np.random.default_rng(1).standard_normal((140, 6)).astype(np.float32)).cuda()
    v[3, :] = 0.0                                                     # a +0 times a negative coefficient is -0: the product's sign
    gamma = torch.tensor([[-0.75, 2.5]], device="cuda")
    e = dict(graph=g, order=0, seg_cols=3, v=v, out=torch.full_like(v, 5.0), gamma=gamma)
    _launch([e])
    want = v.cpu().numpy() * np.repeat(gamma.cpu().numpy(), 3, axis=1)
    assert np.array_equal(bits(e["out"].cpu().numpy()), bits(want)) and np.signbit(want[3, 0]) and not np.signbit(want[3, 3])


def test_all_zero_input_gives_plus_zero(graphs):
    """v = +0 everywhere: every T_k, out and the dots are +0 in every bit (coefficients of mixed sign with a +0 among them)"""
    for i, case in enumerate(CASES):
        if case[0] not in ("p3", "p140", "plong", "p140w") or case[3] < 2 or not case[6]:
            continue
        e, _, _ = _entry(case, 70 + i, graphs)
        e["v"].zero_()
        _launch([e])
        assert not bits(e["out"].cpu().numpy()).any() and not bits(e["dots"].cpu().numpy()).any(), case


def test_padding_columns_of_plus_zero_stay_plus_zero(graphs):
    """segments of 5 columns whose last two hold +0 (the padding of a stacked layout): they stay +0 in every bit, and the live
    columns have the bits of the job without the padding"""
    g = graphs["p140"][0]
    rng = np.random.default_rng(8)
    v = rng.standard_normal((140, 10)).astype(np.float32)
    v[:, [3, 4, 8, 9]] = 0.0
    gamma = _gamma(rng, 10, 2)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    rs = dev((rng.uniform(0.5, 1.5, 140) / np.maximum(np.diff(graphs["p140"][1][0]), 1)).astype(np.float32))
    e = dict(graph=g, order=10, seg_cols=5, v=dev(v), out=torch.full((140, 10), 5.0, device="cuda"), gamma=dev(gamma), row_scale=rs)
    bare = dict(graph=g, order=10, seg_cols=3, v=dev(np.ascontiguousarray(v[:, [0, 1, 2, 5, 6, 7]])), out=torch.full((140, 6), 5.0, device="cuda"),
                gamma=dev(gamma), row_scale=rs)
    _launch([e, bare])
    out = e["out"].cpu().numpy()
    assert not bits(out[:, [3, 4, 8, 9]]).any()
    assert np.array_equal(bits(out[:, [0, 1, 2, 5, 6, 7]]), bits(bare["out"].cpu().numpy()))


def test_binding_refuses_on_the_device_what_the_kernel_does_not_take(graphs):
    from wdg_amd import ops
    e, _, _ = _entry(("p3", 4, 4, 2, "plain", "both", True), 1, graphs)
    with pytest.raises(ValueError, match="contiguous"):
        ops.PolyFilterBatch([dict(e, v=torch.zeros((4, 3), device="cuda").t())])
    with pytest.raises(ValueError, match="overlap"):
        ops.PolyFilterBatch([dict(e, out=e["u"])])
    with pytest.raises(ValueError, match="device"):
        ops.PolyFilterBatch([dict(e, row_scale=torch.ones(3))])
    with pytest.raises(ValueError, match="device"):
        ops.PolyFilterBatch([dict(e, gamma=torch.zeros(3, 1))])
    e_ring, _, _ = _entry(CASES[RING], 2, graphs)
    with pytest.raises(ValueError, match="20448 rows at group 2; at most 10224"):
        ops.PolyFilterBatch([dict(e_ring, group=2)])
    empty = ops.PolyFilterBatch([])
    empty.launch()
