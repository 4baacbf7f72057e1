"""GPU tests of wdg_auc_batched_i64 / ops.AucBatch (csrc/auc.hip): the AUC integers of stacked binary logits, the selection on them, the
patience counter and the curve rows, against the restatement (tests/_auc_ref.py) on the same fp32 logits.  Every comparison is exact
integer equality."""
import numpy as np
import pytest
import torch

import _auc_ref as ref

pytestmark = pytest.mark.gpu

# (n, R, cs, ld, values): one row; the row-block edges 64, 65 and 129; 1, 16, 17 and 33 replicas of cs = 4 (a 256-byte row group holds
# 16, then one past, then more than two); cs = 2 with a leading dimension that is no multiple of 4 (nothing aligned); the ragged pair
# (65, 3) beside (300, 1); a job without rows
CASES = [(1, 1, 2, 2, "normal"), (64, 1, 4, 4, "normal"), (65, 16, 4, 64, "levels"), (129, 17, 4, 72, "normal"), (97, 33, 4, 132, "equal"),
         (130, 3, 2, 7, "special"), (65, 3, 2, 6, "levels"), (300, 1, 2, 2, "normal"), (0, 2, 2, 4, "normal")]


def make_case(n, R, cs, ld, values, seed, frac_pos=0.2, odd_labels=True):
    """labels with 20 % positives and a few labels of -1 and 2, splits whose part sizes differ between the replicas (replica 0's test
    rows are all negatives: a part without positives), logits [n, ld] fp32 with NaN in every column the kernel must not read"""
    rng = np.random.default_rng(seed)
    labels = (rng.random(n) < frac_pos).astype(np.int32)
    if odd_labels and n > 8:
        labels[rng.choice(n, max(n // 16, 2), replace=False)] = rng.choice([-1, 2], max(n // 16, 2))
    split = np.zeros((n, R), np.uint8)
    for r in range(R):
        fr = 0.3 + 0.4 * rng.random()
        u = rng.random(n)
        split[:, r] = np.where(u < fr, 1, np.where(u < fr + (1 - fr) * 0.45, 2, np.where(u < 0.97, 3, 0)))
    if n > 8:
        split[(labels == 1) & (split[:, 0] == 3), 0] = 1
    if values == "equal":
        d = np.full((n, R), 0.25, np.float32)
    elif values == "levels":
        d = (rng.integers(0, 8, (n, R)) - 3).astype(np.float32) / 4 + labels.clip(0, 1)[:, None].astype(np.float32) * 0.25
    else:
        d = (rng.standard_normal((n, R)) + 0.7 * labels.clip(0, 1)[:, None]).astype(np.float32)
    z0 = rng.standard_normal((n, R)).astype(np.float32) if values == "normal" else np.zeros((n, R), np.float32)
    z = np.full((n, ld), np.nan, np.float32)
    for r in range(R):
        z[:, r * cs], z[:, r * cs + 1] = z0[:, r], z0[:, r] + d[:, r]
    if values == "special" and n >= 64:
        # +-0, +-inf and inf - inf = NaN in ONE validation row of replica 1 that counts
        picks = rng.choice(n, 24, replace=False)
        for k, i in enumerate(picks):
            z[i, 0::cs][:R] = 0.0
            z[i, 1::cs][:R] = [0.0, -0.0, np.inf, -np.inf][k % 4]
        i = int(np.nonzero((split[:, 1] == 2) & (labels >= 0) & (labels <= 1))[0][0])
        split[i, :] = np.where(np.arange(R) == 1, 2, 0)
        z[i, cs], z[i, cs + 1] = np.inf, np.inf
    c = dict(n=n, R=R, cs=cs, ld=ld, labels=labels, split=split, z=z)
    c["u2"], c["pairs"] = ref.auc_job(z, labels, split, R, cs)
    for a in (labels, split, z):
        a.setflags(write=False)
    return c


@pytest.fixture(scope="module")
def cases():
    return [make_case(*shape, seed=100 + j) for j, shape in enumerate(CASES)]


def _entry(c, z=None, **kw):
    z = np.array(c["z"] if z is None else z)
    logits = torch.empty(z.shape, dtype=torch.float32, device="cuda").copy_(torch.from_numpy(z))  # (row-major strides for the job without rows too)
    return dict(logits=logits, labels=torch.from_numpy(np.array(c["labels"])).cuda(),
                split=torch.from_numpy(np.array(c["split"])).cuda(), cs=c["cs"], **kw)


def _step(s):
    return torch.full((1,), s, dtype=torch.int32, device="cuda")


def _launch(entries, s=0):
    from wdg_amd import ops
    table = ops.AucBatch(entries)
    table.launch(_step(s))
    torch.cuda.synchronize()
    return table


def _same(table, j, c):
    assert np.array_equal(table.u2_of[j].cpu().numpy(), c["u2"]), (c["n"], c["R"], table.u2_of[j].cpu().numpy(), c["u2"])
    assert np.array_equal(table.pairs_of[j].cpu().numpy(), c["pairs"]), (c["n"], c["R"])


def test_the_ragged_table_equals_the_restatement(cases):
    """every shape and every kind of values in ONE table, twice from the same inputs: exact, and bit-identical"""
    tables = [_launch([_entry(c) for c in cases]) for _ in range(2)]
    for j, c in enumerate(cases):
        _same(tables[0], j, c)
    assert torch.equal(tables[0].u2, tables[1].u2) and torch.equal(tables[0].pairs, tables[1].pairs)
    sp = cases[5]
    assert sp["u2"][1, 1] == -1 and (sp["u2"][[0, 2]] >= 0).all() and (sp["u2"][1, [0, 2]] >= 0).all()  # the NaN row: one replica, one part
    assert all(c["pairs"][0, 2] == 0 and c["u2"][0, 2] == 0 for c in cases if c["n"] > 8)               # the part without positives
    eq = cases[4]
    assert np.array_equal(eq["u2"], eq["pairs"])                                                        # all scores equal: AUC 1/2
    auc = tables[0].auc(4)
    assert np.all((auc == 0.5) | np.isnan(auc))
    assert tables[0].auc(8).shape == (2, 3) and (tables[0].pairs_of[8] == 0).all()                      # the job without rows


def test_a_job_alone_has_the_numbers_it_has_in_the_table(cases):
    for j in (2, 3, 5, 7):
        for max_rows in (None, 4096):
            from wdg_amd import ops
            table = ops.AucBatch([_entry(cases[j])])
            if max_rows:
                table.max_rows = max_rows
            table.launch(_step(0))
            torch.cuda.synchronize()
            _same(table, 0, cases[j])


@pytest.mark.parametrize("bins_log2", [1, 4, 12, 16])
def test_the_bin_count_moves_no_number(cases, bins_log2):
    picked = [cases[j] for j in (2, 3, 5, 6, 7)]
    table = _launch([_entry(c, bins_log2=bins_log2) for c in picked])
    for j, c in enumerate(picked):
        _same(table, j, c)


def test_a_bin_several_times_the_tile():
    """5000 rows of ONE part with scores in [1, 2) - one binade - and bins_log2 = 1: a single bin holds about 4000 negatives, four times the
    LDS tile of 1024 keys (the last tile partly filled), and about 900 positives, four rounds of the workgroup's threads"""
    rng = np.random.default_rng(7)
    n = 5000
    c = make_case(n, 1, 2, 2, "normal", 8, odd_labels=False)
    z = np.zeros((n, 2), np.float32)
    z[:, 1] = 1 + rng.integers(0, 1 << 12, n).astype(np.float32) / (1 << 12)  # (ties among them)
    split = np.full((n, 1), 2, np.uint8)
    u2, pairs = ref.auc_job(z, c["labels"], split, 1, 2)
    assert int((np.array(c["labels"]) == 0).sum()) > 3 * 1024 and int((np.array(c["labels"]) == 1).sum()) > 3 * 256
    table = _launch([dict(logits=torch.from_numpy(z).cuda(), labels=torch.from_numpy(np.array(c["labels"])).cuda(),
                          split=torch.from_numpy(split).cuda(), bins_log2=1)])
    assert np.array_equal(table.u2_of[0].cpu().numpy(), u2) and np.array_equal(table.pairs_of[0].cpu().numpy(), pairs)
    assert u2[0, 1] > 0 and u2[0, 0] == 0 and u2[0, 2] == 0


def test_twenty_thousand_rows_at_the_default():
    c = make_case(20000, 2, 2, 4, "normal", 9)
    table = _launch([_entry(c)])
    _same(table, 0, c)
    want = ref.auc_of(c["u2"], c["pairs"])
    assert np.array_equal(np.isnan(want), np.isnan(table.auc())) and np.array_equal(np.nan_to_num(want), np.nan_to_num(table.auc()))


def _sequence(cases):
    """three sets of logits per job: even replicas score high, low, high again (the tie at the third step never replaces), odd replicas
    low, high, low"""
    out = []
    for c in cases:
        n, R, cs = c["n"], c["R"], c["cs"]
        rng = np.random.default_rng(n + R)
        lab = np.array(c["labels"]).clip(0, 1).astype(np.float32)[:, None]
        noise = rng.standard_normal((n, R)).astype(np.float32)
        hi, lo = noise + 2.0 * lab, noise + 0.25 * lab
        even = (np.arange(R) % 2 == 0)[None, :]
        zs = []
        for first in (True, False, True):
            d = np.where(even == first, hi, lo)
            z = np.zeros((n, c["ld"]), np.float32)
            z[:, 1:R * cs:cs] = d
            zs.append(z)
        out.append(zs)
    return out


def _check_sequence(table, cases, seqs, steps, select, patience, curve_rows, run_step):
    states = [ref.new_state(c["R"], curve_rows) for c in cases]
    for k, s in enumerate(steps):
        run_step(k, s)
        torch.cuda.synchronize()
        for j, c in enumerate(cases):
            u2, pairs = ref.auc_job(seqs[j][k], c["labels"], c["split"], c["R"], c["cs"])
            st = ref.step(states[j], u2, s, select, patience)
            assert np.array_equal(table.u2_of[j].cpu().numpy(), u2), (j, k)
            assert np.array_equal(table.pairs_of[j].cpu().numpy(), pairs), (j, k)
            assert np.array_equal(table.best_u2_of[j].cpu().numpy(), st["best_u2"]), (j, k)
            assert np.array_equal(table.best_of[j].cpu().numpy(), st["best"]), (j, k)
            assert np.array_equal(table.state_of[j].cpu().numpy(), st["state"]), (j, k)
            if curve_rows:
                assert np.array_equal(table.curve_of[j].cpu().numpy(), st["curve"]), (j, k)
    return states


@pytest.mark.parametrize("select,patience", [(1, 0), (1, 1), (0, 1)])
def test_selection_patience_and_curve_over_three_calls(cases, select, patience):
    """steps 5, 9, 11 with the step word advanced ON THE DEVICE; curve_rows = 10: rows 5 and 9 are written, row 11 is dropped.  With
    patience 1 the even replicas stop at step 9 and ignore step 11; select = 0 scores and never selects"""
    from wdg_amd import ops
    picked = [cases[j] for j in (2, 3, 6, 7)]
    seqs = _sequence(picked)
    entries = [_entry(c, z=seqs[j][0], select=select, patience=patience, curve_rows=10) for j, c in enumerate(picked)]
    table = ops.AucBatch(entries)
    word = _step(5)

    def run_step(k, s):
        for e, zs in zip(entries, seqs):
            e["logits"].copy_(torch.from_numpy(zs[k]))
        table.launch(word)
        word.add_(4 if k == 0 else 2)

    states = _check_sequence(table, picked, seqs, (5, 9, 11), select, patience, 10, run_step)
    if select == 1:
        assert states[0]["best"][0].tolist() == [0, 0, 5] and states[0]["best"][1].tolist() == [0, 0, 9]
        assert states[0]["state"][0, 1] == (9 if patience else -1)
    else:
        assert all((st["best"][:, 0] == -1).all() for st in states)


def test_a_captured_call_replays_without_a_memset_of_its_own(cases):
    """the launch captured once and replayed three times, the logits and the step word changed between the replays: every replay equals
    the restatement - the work space is left as the next call needs it"""
    from wdg_amd import ops
    picked = [cases[j] for j in (2, 3, 6, 7)]
    seqs = _sequence(picked)
    entries = [_entry(c, z=seqs[j][0], select=1, patience=2, curve_rows=4) for j, c in enumerate(picked)]
    table = ops.AucBatch(entries)
    word = _step(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        table.launch(word)  # (warm-up; rewound below)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    table.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        table.launch(word)
        word.add_(1)
    word.zero_()
    table.reset()

    def run_step(k, s):
        for e, zs in zip(entries, seqs):
            e["logits"].copy_(torch.from_numpy(zs[k]))
        graph.replay()

    _check_sequence(table, picked, seqs, (0, 1, 2), 1, 2, 4, run_step)
    assert int(word.item()) == 3
