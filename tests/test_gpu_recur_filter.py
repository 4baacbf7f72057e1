"""GPU tests of the recurrence-filter kernel (csrc/recur_filter.hip: wdg_recur_filter_batched_f32) through ops.RecurFilterBatch.

EQUAL BITS with tests/_recur_filter_ref.forward32 - the header's arithmetic restated operation by operation in fp32 - for the out of
every job of one mixed table and of the PROBE jobs beside it: a probe has the case's pattern, scales, v and recurrence in order + 1
segments whose coefficients are the unit vectors, so its segment k is fmaf(1, T_k, +-0) - the kernel's own T_k (the sign of a zero is
the accumulation's: the restatement of the probe job itself has it bit for bit, and T_k is compared with ==).  The dot products equal
_poly_filter_ref.dots_bits - the polynomial filter's fp64 order - on those T_k in every bit.  out, T_k and dots against the fp64
restatement under the DERIVED bound of _recur_filter_ref.bound_factors; the largest ratio is printed and DESIGN 4.36 records it.  With
the monomial table the kernel compares == with ops.PolyFilterBatch on the same inputs.  And the exact properties the header states."""
import numpy as np
import pytest
import torch

import _poly_filter_ref as pref
import _recur_filter_ref as ref
import test_gpu_poly_filter as poly
from test_gpu_poly_filter import RING_N, _ratio, bits, graphs  # noqa: F401  (graphs: the fixture - the patterns of the polynomial filter's tests)
from test_gpu_signed_att import _canaries_intact, _view

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# poly.CASES' fields (pattern, cols, seg_cols, order, layout, scales, dots) and the recurrence: "cheb", "jac11" = Jacobi(1, 1),
# "jac53" = Jacobi(0.5, -0.3) (b != 0: every term of the recurrence is live), "rand" = random signs, |entries| in 0.3 .. 1.5
CASES = [("p0", 4, 4, 2, "plain", "both", True, "cheb"), ("p1", 1, 1, 10, "plain", "row", True, "jac11"), ("p3", 3, 3, 2, "slices", "both", True, "rand"),
         ("p3", 8, 1, 1, "plain", "none", True, "jac53"), ("p3", 2, 2, 64, "plain", "row", True, "cheb"), ("p65", 5, 5, 10, "slices", "both", True, "cheb"),
         ("p65", 4, 4, 0, "wide16", "row", True, "jac11"), ("p140", 1, 1, 10, "plain", "both", True, "jac53"), ("p140", 7, 7, 10, "plain", "row", True, "cheb"),
         ("p140", 12, 4, 2, "wide16", "both", True, "rand"), ("p140", 10, 5, 10, "slices", "both", True, "jac11"), ("p140", 8, 8, 1, "plain", "none", False, "cheb"),
         ("p140", 12, 12, 3, "slices", "none", True, "rand"), ("pteams", 7, 1, 2, "plain", "both", True, "jac11"), ("plong", 5, 5, 2, "slices", "both", True, "jac53"),
         ("plong", 8, 4, 10, "plain", "row", True, "cheb"), ("ring", 1, 1, 3, "plain", "both", True, "jac11"), ("p140w", 7, 7, 10, "plain", "both", True, "rand"),
         ("p140w", 10, 5, 2, "slices", "none", False, "cheb"), ("plongw", 4, 4, 10, "wide16", "both", True, "jac53"), ("p1025", 3, 3, 2, "slices", "both", True, "jac11"),
         ("p65", 2, 2, 3, "wide16", "both", True, "rand")]
RING = 16  # the ring's place in CASES
assert {c[0] for c in CASES} == set(poly.PATTERNS) | set(poly.WEIGHTED) and {c[1] for c in CASES} >= {1, 2, 3, 4, 5, 7, 8, 12}
assert {c[2] for c in CASES} >= {1, 4, 5} and {c[3] for c in CASES} == {0, 1, 2, 3, 10, 64} and {c[4] for c in CASES} == {"plain", "slices", "wide16"}
assert {c[7] for c in CASES} == {"cheb", "jac11", "jac53", "rand"} and {c[6] for c in CASES} == {True, False} and CASES[RING][0] == "ring"


def _recurrence(kind, order, seed):
    from wdg_amd import models
    tab = {"cheb": lambda: models.recurrence_table("chebyshev", order), "jac11": lambda: models.recurrence_table("jacobi", order, 1.0, 1.0),
           "jac53": lambda: models.recurrence_table("jacobi", order, 0.5, -0.3), "mono": lambda: models.recurrence_table("monomial", order),
           "rand": lambda: ref.random_sign_table(np.random.default_rng(1000 + seed), order)}[kind]()
    return tab.astype(np.float32)


def _entry(case, seed, graphs, group=None, kind=None):  # noqa: F811
    """-> (the entry of ops.RecurFilterBatch, its fp32 host inputs, the buffers around its outputs): the polynomial filter's entry of the
    same case and seed, and the recurrence table - a view in the case's layout, so ld_recur is 3, 5 or 12"""
    e, host, around = poly._entry(case[:7], seed, graphs, group)
    host["recur"] = _recurrence(case[7] if kind is None else kind, case[3], seed)
    if case[3] > 0:
        e["recur"], _ = _view(case[3], 3, case[4], host["recur"])
    return e, host, around


def _probe(case, e):
    return dict(poly._probe(case[:7], e), **({"recur": e["recur"]} if "recur" in e else {}))


def _restated32(case, host, graphs, gamma=None, reps=1):  # noqa: F811
    (rowptr, col), val = graphs[case[0]][1], graphs[case[0]][2]
    v = np.tile(host["v"], (1, reps))
    return ref.forward32(rowptr, col, v, host["gamma"] if gamma is None else gamma, host["recur"], case[2] if gamma is None else max(case[1], 1), host["row_scale"],
                         host["col_scale"], val)


def _restated64(case, host, graphs):  # noqa: F811
    (rowptr, col), val = graphs[case[0]][1], graphs[case[0]][2]
    x = {k: None if v is None else v.astype(np.float64) for k, v in host.items()}
    return ref.forward64(rowptr, col, x["v"], x["gamma"], x["recur"], case[2], x["row_scale"], x["col_scale"], x["u"], None if val is None else val.astype(np.float64))


def _factors(case, graphs):  # noqa: F811
    return ref.bound_factors(graphs[case[0]][1][0], case[3], weighted=graphs[case[0]][2] is not None and case[5] == "both")


def _results(entries):
    return [{k: e[k].cpu().numpy().copy() for k in ("out", "dots") if k in e} for e in entries]


def _launch(entries, cls="RecurFilterBatch"):
    from wdg_amd import ops
    batch = getattr(ops, cls)(entries)
    batch.launch()
    torch.cuda.synchronize()
    return batch


@pytest.fixture(scope="module")
def table(graphs):  # noqa: F811
    """the mixed table - jobs of 0 .. 20448 rows, groups of 4 and 1, orders 0 .. 64, four kinds of recurrence, with and without dots
    share a launch -, run once, and the probes' table; the restatements are computed once, shared and never changed"""
    built = [_entry(case, 170 + i, graphs) for i, case in enumerate(CASES)]
    entries, hosts, around = [b[0] for b in built], [b[1] for b in built], [b[2] for b in built]
    batch = _launch(entries)
    probes = [_probe(case, e) for case, e in zip(CASES, entries)]
    _launch(probes)
    probe_out = [p["out"].cpu().numpy().copy() for p in probes]
    t_own = [[o[:, k * c[1]:(k + 1) * c[1]] for k in range(c[3] + 1)] for c, o in zip(CASES, probe_out)]
    r32 = [_restated32(case, host, graphs) for case, host in zip(CASES, hosts)]
    r64 = [_restated64(case, host, graphs) for case, host in zip(CASES, hosts)]
    return dict(entries=entries, hosts=hosts, batch=batch, got=_results(entries), around=around, r32=r32, r64=r64, t_own=t_own, probe_out=probe_out)


def test_the_table_mixes_groups_orders_and_dots(table):
    batch = table["batch"]
    assert set(batch.groups) == {4, 1} and batch.max_dot_rows == 65 and batch.max_floats == RING_N and batch.max_groups == 8
    lds = {e["recur"].stride(0) if "recur" in e else 0 for e in table["entries"]}
    assert lds == {3, 5, 12, 0}                                       # the recurrence as a plain matrix, as slices of wider ones, and absent (order 0)


def test_out_equals_the_fp32_restatement_in_every_bit(table):
    for case, g_, r in zip(CASES, table["got"], table["r32"]):
        assert g_["out"].shape == r["out"].shape and np.array_equal(bits(g_["out"]), bits(r["out"])), case
        assert np.isfinite(r["out"]).all(), case


def test_the_hops_equal_the_fp32_restatement(table, graphs):  # noqa: F811
    """the probe job's out in every bit (its restatement: the same rows with the unit-vector coefficients), and so T_k == the
    restatement's T_k (a zero's sign is the probe's accumulation's)"""
    for i, (case, host) in enumerate(zip(CASES, table["hosts"])):
        order = case[3]
        want = _restated32(case, host, graphs, gamma=np.eye(order + 1, dtype=np.float32), reps=order + 1)
        assert np.array_equal(bits(table["probe_out"][i]), bits(want["out"])), case
        for k in range(order + 1):
            assert np.array_equal(table["t_own"][i][k], table["r32"][i]["t"][k]), (case, k)
            nz = table["r32"][i]["t"][k] != 0
            assert np.array_equal(bits(table["t_own"][i][k])[nz], bits(table["r32"][i]["t"][k])[nz]), (case, k)


def test_dots_equal_the_polynomial_filters_order_on_the_kernels_own_hops_bit_for_bit(table):
    seen = 0
    for i, case in enumerate(CASES):
        if not case[6]:
            continue
        want = pref.dots_bits([np.ascontiguousarray(t) for t in table["t_own"][i]], table["hosts"][i]["u"], case[2])
        assert np.array_equal(bits(table["got"][i]["dots"]), bits(want)), case
        seen += 1
    assert seen == len(CASES) - 2


def test_out_hops_and_dots_match_the_fp64_restatement_within_the_derived_bound(table, graphs):  # noqa: F811
    misses, worst, worst_dots = [], 0.0, 0.0
    for i, (case, g_, r) in enumerate(zip(CASES, table["got"], table["r64"])):
        ks = _factors(case, graphs)
        if r["out"].size == 0:
            assert g_["out"].size == 0
            continue
        ratio = _ratio(np.abs(g_["out"].astype(np.float64) - r["out"]), ks["out"] * U * r["out_abs"])
        for k, tk in enumerate(table["t_own"][i]):
            ratio = max(ratio, _ratio(np.abs(tk.astype(np.float64) - r["t"][k]), ks["t"][k] * U * r["t_abs"][k]))
        dots = _ratio(np.abs(g_["dots"].astype(np.float64) - r["dots"]), ks["dots"][:, None] * U * r["dots_abs"]) if case[6] else 0.0
        worst, worst_dots = max(worst, ratio), max(worst_dots, dots)
        print(f"job {i} {case}: r {ks['r']} m {ks['m']} K {ks['out']:.0f} largest error / bound: out, T_k {ratio:.4f} dots {dots:.4f}")
        if not (ratio <= 1.0 and dots <= 1.0):
            misses.append(f"job {i} {case}: error / bound {ratio:.3e} (out, T_k) {dots:.3e} (dots)")
    print(f"largest error / bound (out, T_k): {worst:.4f}; (dots): {worst_dots:.4f}")
    assert not misses, "\n".join(misses)
    assert worst > 0 and worst_dots > 0                               # (the comparison is not vacuous)


def test_the_monomial_table_compares_equal_with_the_polynomial_filter(graphs):  # noqa: F811
    """(1, 0, 0) in every row: fmaf(1, P, 0 * T) is P up to the sign of a zero, so out and dots compare == (-0 == +0) with
    ops.PolyFilterBatch on the same finite inputs - every pattern, the ring included"""
    built = [_entry(case, 170 + i, graphs, kind="mono") for i, case in enumerate(CASES)]
    twins = [poly._entry(case[:7], 170 + i, graphs) for i, case in enumerate(CASES)]
    _launch([b[0] for b in built])
    _launch([b[0] for b in twins], "PolyFilterBatch")
    seen = 0
    for case, a, b in zip(CASES, _results([b[0] for b in built]), _results([b[0] for b in twins])):
        for k in a:
            assert np.isfinite(b[k]).all() and np.array_equal(a[k], b[k]), (case, k)
            seen += a[k].size > 0
    assert seen >= 2 * len(CASES) - 6


def test_rows_beyond_a_job_and_columns_beside_it_are_untouched(table):
    for case, e, bufs in zip(CASES, table["entries"], table["around"]):
        for k, full in bufs.items():
            assert _canaries_intact(full, e[k]), (case, k)


def test_a_second_launch_repeats_every_bit(table):
    entries, batch = table["entries"], table["batch"]
    for e in entries:  # (what the launch writes is cleared first: a stale value would not pass for a repeated one)
        e["out"].fill_(5.0)
        if "dots" in e:
            e["dots"].fill_(5.0)
    batch.partials.fill_(5.0)
    batch.launch()
    torch.cuda.synchronize()
    for case, a, b in zip(CASES, table["got"], _results(entries)):
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), (case, k)


def test_a_job_alone_answers_what_it_answers_in_the_table(table, graphs):  # noqa: F811
    for i, case in enumerate(CASES):
        if case[0] == "ring":
            continue
        e, _, _ = _entry(case, 170 + i, graphs)
        _launch([e])
        res = _results([e])[0]
        for k in table["got"][i]:
            assert np.array_equal(bits(table["got"][i][k]), bits(res[k])), (case, k)


def test_group_widths_1_2_and_4_give_equal_bits(table, graphs):  # noqa: F811
    seen = 0
    for i, case in enumerate(CASES):
        if case[0] in ("ring", "p0", "p1"):
            continue
        built = [_entry(case, 170 + i, graphs, group=g) for g in (1, 2, 4)]
        batch = _launch([b[0] for b in built])                        # the three widths share a launch
        assert batch.groups == [1, 2, 4]
        for g, res in zip((1, 2, 4), _results([b[0] for b in built])):
            for k in table["got"][i]:
                assert np.array_equal(bits(table["got"][i][k]), bits(res[k])), (case, g, k)
        seen += 1
    assert seen >= 14


def test_a_segment_has_the_bits_of_a_one_segment_job_on_its_slice(table):
    """v, u, out and the segment's column of gamma are passed IN PLACE (slices with the job's leading dimensions); the recurrence is the job's"""
    seen = 0
    for i, case in enumerate(CASES):
        cols, seg_cols, order = case[1:4]
        n_seg = cols // seg_cols
        if n_seg == 1 or case[0] == "p0":
            continue
        e, got = table["entries"][i], table["got"][i]
        for s in {0, n_seg - 1, n_seg // 2}:
            sl = slice(s * seg_cols, (s + 1) * seg_cols)
            one = dict(graph=e["graph"], order=order, v=e["v"][:, sl], out=torch.full_like(e["out"][:, sl], 5.0), gamma=e["gamma"][:, s:s + 1], recur=e["recur"])
            one.update({k: e[k] for k in ("row_scale", "col_scale") if k in e})
            if "u" in e:
                one["u"], one["dots"] = e["u"][:, sl], torch.full((order + 1, 1), 5.0, device="cuda")
            _launch([one])
            assert np.array_equal(bits(one["out"].cpu().numpy()), bits(got["out"][:, sl])), (case, s)
            if "u" in e:
                assert np.array_equal(bits(one["dots"].cpu().numpy()[:, 0]), bits(got["dots"][:, s])), (case, s)
            seen += 1
    assert seen >= 10


def test_order_zero_is_exactly_gamma_0_times_v(table, graphs):  # noqa: F811
    """... with no recurrence table at all, and with one that is not read"""
    hosts, got = table["hosts"], table["got"]
    i = next(k for k, c in enumerate(CASES) if c[3] == 0)
    assert "recur" not in table["entries"][i] and np.array_equal(bits(got[i]["out"]), bits(hosts[i]["gamma"][0, 0] * hosts[i]["v"]))
    g = graphs["p140"][0]
    v = torch.from_numpy(np.random.default_rng(1).standard_normal((140, 6)).astype(np.float32)).cuda()
    v[3, :] = 0.0                                                     # a +0 times a negative coefficient is -0: the product's sign
    gamma = torch.tensor([[-0.75, 2.5]], device="cuda")
    e = dict(graph=g, order=0, seg_cols=3, v=v, out=torch.full_like(v, 5.0), gamma=gamma, recur=torch.zeros(0, 3, device="cuda"))
    _launch([e])
    want = v.cpu().numpy() * np.repeat(gamma.cpu().numpy(), 3, axis=1)
    assert np.array_equal(bits(e["out"].cpu().numpy()), bits(want)) and np.signbit(want[3, 0]) and not np.signbit(want[3, 3])


def test_binding_refuses_on_the_device_what_the_kernel_does_not_take(graphs):  # noqa: F811
    from wdg_amd import ops
    e, _, _ = _entry(("p3", 4, 4, 2, "plain", "both", True, "cheb"), 1, graphs)
    with pytest.raises(ValueError, match="device"):
        ops.RecurFilterBatch([dict(e, recur=torch.zeros(2, 3))])
    with pytest.raises(ValueError, match="overlap"):
        ops.RecurFilterBatch([dict(e, out=e["u"])])
    e_ring, _, _ = _entry(CASES[RING], 2, graphs)
    with pytest.raises(ValueError, match="20448 rows at group 2; at most 10224"):
        ops.RecurFilterBatch([dict(e_ring, group=2)])
    ops.RecurFilterBatch([]).launch()
