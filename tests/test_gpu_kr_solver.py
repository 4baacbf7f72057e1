"""The kernel-regression solver (csrc/kernel_reg.hip: kr_solve_blocked_kernel, kr_deflate_kernel) against an fp64 pseudo-inverse,
probe by probe (tests/_kr_probe.py).  Every problem is asked twice - validation rows labelled with their designed arg-max (hit
count = n_val exactly) and with their runner-up (hit count = 0 exactly) - and its flags word must be the one the configuration
predicts.  Probes lead their runner-up by rho_hard = 1e-3 of |w|_1 max|alpha|; finer levels are printed, not asserted."""
import numpy as np
import pytest
import torch

import _kr_probe as kp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from wdg_amd import ops as o
    return o


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Built:
    """a case on the device: the hit problem and the control problem over one kernel matrix"""

    def __init__(self, case, rng, sort_train=True, ld_extra=0, rep=None):
        d = kp.assemble(case, rng, sort_train=sort_train, ld_extra=ld_extra)
        self.case, self.host = case, d
        self.K = _dev(d["K"])[:, :d["n"]]  # (a column slice: leading dimension n + ld_extra)
        self.tr, self.va = _dev(d["train"]), _dev(d["val"])
        self.lab_hit, self.lab_ctl = _dev(d["labels_hit"]), _dev(d["labels_ctl"])
        r = d["rep"] if rep is None else rep(d)
        self.rep = None if r is None else _dev(r)

    def problems(self, with_rep=True):
        extra = (self.rep,) if (with_rep and self.rep is not None) else ()
        return [(self.K, self.tr, self.va, self.lab_hit) + extra, (self.K, self.tr, self.va, self.lab_ctl) + extra]

    def want(self):
        return [self.case.n_probes, 0]


def _launch(ops, problems, classes):
    """one table (n_classes patched per job, as C is per job in wdg_kr_job) -> (correct, flags) host arrays"""
    from wdg_amd.kernel_regression import _KR_JOB_DTYPE
    kb = ops.KrBatch(problems, 8)
    tab = kb.table.cpu().numpy().view(_KR_JOB_DTYPE).copy()
    tab["n_classes"] = classes
    kb.table.copy_(torch.from_numpy(tab.view(np.uint8)))
    kb.flags.fill_(-1)
    kb.launch()
    torch.cuda.synchronize()
    return kb.correct[:kb.n_jobs].cpu().numpy(), kb.flags[:kb.n_jobs].cpu().numpy(), kb


def _flipped(ops, b, with_rep):
    """the probes of a failing case, one per problem: which of them the device predicts against the design"""
    p = []
    for i in range(b.case.n_probes):
        va = b.va[i:i + 1]
        extra = (b.rep,) if (with_rep and b.rep is not None) else ()
        p.append((b.K, b.tr, va, b.lab_hit) + extra)
    got, _, _ = _launch(ops, p, [b.case.c] * len(p))
    bad = np.flatnonzero(got != 1)
    return [(int(i), int(b.case.a[i]), int(b.case.b_[i]), float(b.case.ratio[i])) for i in bad[:12]]


def _check(ops, built, with_rep=None, label=""):
    """one table of every case's hit and control problem: exact counts and flags; a failing case is re-launched probe by probe"""
    with_rep = [True] * len(built) if with_rep is None else with_rep
    problems, classes, want, want_flags = [], [], [], []
    for b, wr in zip(built, with_rep):
        problems += b.problems(wr)
        classes += [b.case.c] * 2
        want += b.want()
        want_flags += [b.case.flags if wr else 0] * 2
    got, flags, kb = _launch(ops, problems, classes)
    assert np.array_equal(kb.dropped().cpu().numpy(), (flags & 4) != 0)
    bad = [(b.case.name, got[2 * i:2 * i + 2].tolist(), want[2 * i:2 * i + 2], flags[2 * i:2 * i + 2].tolist(), want_flags[2 * i])
           for i, b in enumerate(built)
           if got[2 * i:2 * i + 2].tolist() != want[2 * i:2 * i + 2] or flags[2 * i:2 * i + 2].tolist() != [want_flags[2 * i]] * 2]
    detail = {name: _flipped(ops, built[[b.case.name for b in built].index(name)], with_rep[[b.case.name for b in built].index(name)])
              for name, *_ in bad[:4]}
    assert not bad, (label, bad, "flipped probes (index, arg-max, runner-up, margin ratio):", detail)
    return got, flags


def _record(ops, cases, family, rng, with_rep=False, **kw):
    """finer probe levels on the same blocks: flips printed (not asserted) - the finest level with none is the device's resolution"""
    for rho in kp.RHO_RECORD[1:]:
        built = [Built(c.redesign(rng, rho), rng, **kw) for c in cases]
        problems, classes, want = [], [], []
        for b in built:
            problems += b.problems(with_rep)
            classes += [b.case.c] * 2
            want += b.want()
        got, _, _ = _launch(ops, problems, classes)
        n = sum(b.case.n_probes for b in built)
        print(f"[kr probe] {family}: rho {rho:g}: {int(np.abs(got - np.asarray(want)).sum())} flips of {n} probes")


@pytest.fixture(scope="module")
def spd():
    return kp.spd_cases()


def test_plain_entry_spd_blocks_at_every_block_edge(ops, spd):
    """n_train at every 32-row block edge from 1 to 320, condition 4 and 100, C over 1, 2, 3, 7, 8 (absent classes included)"""
    rng = np.random.default_rng(100)
    _check(ops, [Built(c, rng) for c in spd], label="spd")
    _record(ops, spd, "spd", rng)


def test_validation_counts_around_units_of_four(ops):
    """n_val 1 .. 5, 63 .. 65 and 4097: predictions are dealt in units of four validation rows"""
    rng = np.random.default_rng(101)
    case = kp.n_val_case()
    _check(ops, [Built(case.take(nv), rng) for nv in kp.N_VAL_EDGES], label="n_val")
    _record(ops, [case.take(nv) for nv in kp.N_VAL_EDGES], "n_val", rng)


def test_unsorted_train_ids_give_the_same_counts(ops, spd):
    rng = np.random.default_rng(102)
    _check(ops, [Built(c, rng, sort_train=False) for c in spd[1::3]], label="unsorted")


def _identity_rep(d):
    return np.arange(d["n"], dtype=np.int32)


def test_diagonal_spread_both_entries(ops):
    """B = D C D with min K_ii / max K_ii from 1e-2 to 1e-5: no flag, no flip, through the plain entry and the deflating one (every
    node its own representative) - the pre-pass drops no row the solver can factor"""
    rng = np.random.default_rng(103)
    cases = kp.spread_cases()
    _check(ops, [Built(c, rng) for c in cases], label="spread plain")
    _check(ops, [Built(c, rng, rep=_identity_rep) for c in cases], label="spread deflating")
    _record(ops, cases, "spread", rng)


def test_deflating_entry_on_exactly_singular_blocks(ops):
    """duplicate classes (2, 3, 33 members), all train rows one node, mixed-label classes, K_ii = 0 rows, an all-zero block and
    validation nodes that duplicate train nodes, with explicit row representatives: the fp64 pinv of the expanded block; flags bit 1
    (deflated) set, bit 0 (ridge) clear, bit 2 exactly where rows are dropped"""
    rng = np.random.default_rng(104)
    cases = kp.deflation_cases()
    _check(ops, [Built(c, rng) for c in cases], label="deflate")
    _record(ops, cases[:4], "deflate", rng, with_rep=True)


def test_plain_entry_ridge_on_exactly_rank_deficient_blocks(ops):
    """duplicate train nodes through the plain entry (no representatives): flags exactly bit 0 (the ridge retry), probes in range(B)
    exact at each case's level - rho_ridge = 1e-3 with pure-label duplicates, 1e-1 with mixed-label ones: 10x the finest level at
    which a host fp32 emulation of the retry flips nothing (tests/_kr_probe.py ridge_cases, test_kr_probe_oracle.py)"""
    rng = np.random.default_rng(108)
    cases = kp.ridge_cases()
    assert [c.rho for c in cases] == [1e-3, 1e-1] and all(c.flags == kp.FLAG_RIDGE for c in cases)
    _check(ops, [Built(c, rng) for c in cases], label="ridge")
    for c in cases:  # (recorded, not asserted: finer levels on the same blocks)
        for rho in (c.rho / 10, c.rho / 100):
            b = Built(c.redesign(rng, rho), rng)
            got, _, _ = _launch(ops, b.problems(), [c.c] * 2)
            print(f"[kr probe] {c.name}: rho {rho:g}: {int(abs(got[0] - b.case.n_probes) + got[1])} flips of {b.case.n_probes} probes")


def test_persistent_schedule_equals_one_problem_launches(ops, spd):
    """every family above in one shuffled table, longer than the device has CUs, with heterogeneous n_train, n_val, C and ldk: each
    problem answers what its own one-problem launch answers, bit for bit (plain table; deflating table with `rep` on some problems)"""
    rng = np.random.default_rng(105)
    cus = int(ops.lib.wdg_device_cus())
    spread = kp.spread_cases()
    nval = kp.n_val_case()
    plain = [Built(c, rng, ld_extra=13 * (i % 2)) for i, c in enumerate(spd)]
    plain += [Built(nval.take(nv), rng, ld_extra=7) for nv in (1, 3, 5, 65)]
    plain += [Built(c, rng, sort_train=False) for c in spread[::2]]
    plain += [Built(c, rng, ld_extra=3) for c in kp.ridge_cases()]
    defl = [Built(c, rng, ld_extra=5) for c in kp.deflation_cases()]
    defl += [Built(c, rng, rep=_identity_rep) for c in spread[1::2]]
    for deflating, pool in ((False, plain), (True, defl + plain[::3])):
        items = []
        for b in pool:
            for p in b.problems(with_rep=True):
                items.append((p, b.case.c))
        while len(items) <= cus + 17:
            items = items + items
        order = rng.permutation(len(items))
        items = [items[i] for i in order]
        got, flags, kb = _launch(ops, [p for p, _ in items], [c for _, c in items])
        assert (kb.ws is not None) == deflating
        one = {}
        for i, (p, c) in enumerate(items):
            key = tuple(int(t.data_ptr()) if t is not None else 0 for t in p)
            if key not in one:
                g1, f1, _ = _launch(ops, [p], [c])
                one[key] = (int(g1[0]), int(f1[0]))
            assert (int(got[i]), int(flags[i])) == one[key], (deflating, i, got[i], flags[i], one[key])


def test_layout_leading_dimensions_and_refusal(ops):
    """ldk = n + 13 (a column slice of a wider buffer) and ldk = 65 535; ldk = 65 536 patched into a table: that problem answers -1
    with flags 0, its neighbours are unaffected"""
    from wdg_amd.kernel_regression import _KR_JOB_DTYPE
    rng = np.random.default_rng(106)
    cases = kp.layout_cases()[:2]
    built = []
    for c in cases:
        n = c.nt + c.n_probes + 5
        built += [Built(c, rng, ld_extra=13), Built(c, rng, ld_extra=65535 - n)]
    assert {int(b.K.stride(0)) for b in built} == {b.host["n"] + 13 for b in built[::2]} | {65535}
    _check(ops, built, label="layout")
    _record(ops, cases, "layout", rng, ld_extra=13)
    problems, classes = [], []
    for b in built:
        problems += b.problems()
        classes += [b.case.c] * 2
    kb = ops.KrBatch(problems, 8)
    tab = kb.table.cpu().numpy().view(_KR_JOB_DTYPE).copy()
    tab["n_classes"] = classes
    tab["ldk"][3] = 65536
    kb.table.copy_(torch.from_numpy(tab.view(np.uint8)))
    kb.flags.fill_(12345)
    kb.correct.fill_(12345)
    kb.launch()
    torch.cuda.synchronize()
    got, flags = kb.correct[:len(problems)].cpu().numpy(), kb.flags[:len(problems)].cpu().numpy()
    want = np.array(sum((b.want() for b in built), []))
    want[3] = -1
    assert got.tolist() == want.tolist() and flags.tolist() == [0] * len(problems)


def test_element_offsets_past_two_to_the_31(ops):
    """train and probe rows above row 32 768 at ldk = 65 535: element offsets up to 4.3e9, past 2^31 - the solver's unsigned 32-bit
    offsets (an 8.6 GB kernel buffer)"""
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2**30:
        pytest.skip(f"needs 16 GB of free device memory for an 8.6 GB kernel buffer ({free / 2**30:.1f} GB free)")
    rng = np.random.default_rng(107)
    c = kp.layout_cases()[2]
    d = kp.assemble(c, rng)
    n, base, ldk = d["n"], 32769, 65535
    assert base * ldk > 2**31 and base + n < ldk
    big = torch.empty((base + n, ldk), dtype=torch.float32, device="cuda")
    rows = torch.zeros((n, ldk), dtype=torch.float32)
    rows[:, base:base + n] = torch.from_numpy(d["K"][:, :n])
    big[base:] = rows.cuda()
    lab_hit = np.full(base + n, -1, np.int32)
    lab_ctl = lab_hit.copy()
    lab_hit[base:], lab_ctl[base:] = d["labels_hit"], d["labels_ctl"]
    tr, va = _dev(d["train"] + base), _dev(d["val"] + base)
    kb = ops.KrBatch([(big, tr, va, _dev(lab_hit)), (big, tr, va, _dev(lab_ctl))], c.c)
    kb.launch()
    torch.cuda.synchronize()
    assert kb.correct[:2].cpu().tolist() == [c.n_probes, 0] and kb.flags[:2].cpu().tolist() == [0, 0]
    del big
    torch.cuda.empty_cache()
