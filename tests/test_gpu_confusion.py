"""GPU tests of wdg_confusion_batched_i32 (csrc/confusion.hip, ops.ConfusionBatch) against tests/_confusion_ref.py: predictions and
counts are integers, so the bound is equality."""
import ctypes

import numpy as np
import pytest
import torch

import _confusion_ref as ref

pytestmark = pytest.mark.gpu

NS = (0, 1, 63, 64, 65, 130)      # none, one, around one workgroup's 64 rows, three workgroups
RS = (1, 3, 17)                   # 17 replicas of 16 classes: two chunks of the workgroup's counters (10 + 7)
CS = (1, 2, 5, 7, 16)
STRIDES = ("C", "x4", 16)         # the replica stride: C itself, the next multiple of 4, 16
CASES = [(n, R, C, C if cs == "C" else (-(-C // 4) * 4 if cs == "x4" else 16)) for n in NS for R in RS for C in CS for cs in STRIDES]


def _pad(i):
    """the floats between a row's R cs columns and the next row, job by job: 4 (with cs a multiple of 4 the pitch is one of 16 bytes:
    the kernel's 16-byte loads) or 3 (never: the scalar loads).  Jobs i and i + 45 (the same R, C and stride at the next n) differ."""
    return 4 if i % 2 == 0 else 3


def _host(case, seed, pad):
    """-> (logits [n, R cs + pad] - a leading dimension wider than R cs -, labels [n], split [n, R]).  The logits are small integers, so
    exact ties are the rule; some rows are all -inf, some carry a NaN among their classes, the padding columns carry NaNs nobody may
    read; labels run over -1 .. C (both ends out of range); split codes over 0 .. 4"""
    n, R, C, cs = case
    rng = np.random.default_rng(seed)
    logits = rng.integers(-2, 3, (n, R * cs + pad)).astype(np.float32)
    logits[rng.random(logits.shape) < 0.03] = np.inf
    for r in range(R):
        kind = rng.random(n)
        logits[kind < 0.08, r * cs:r * cs + C] = -np.inf
        rows = np.nonzero((kind >= 0.08) & (kind < 0.16))[0]
        logits[rows, r * cs + rng.integers(0, C, len(rows))] = np.nan
        logits[:, r * cs + C:(r + 1) * cs] = np.nan
    logits[:, R * cs:] = np.nan
    labels = rng.integers(-1, C + 1, n).astype(np.int32)
    split = rng.choice(np.arange(5, dtype=np.uint8), (n, R), p=[0.15, 0.4, 0.2, 0.2, 0.05])
    return logits, labels, np.ascontiguousarray(split)


def _jobs(hosts):
    # (a column range of a wider matrix; the empty job is a plain empty matrix - torch gives an empty slice no strides to speak of)
    wide = lambda lg, w: torch.from_numpy(lg).cuda()[:, :w] if lg.shape[0] else torch.zeros((0, w), device="cuda")  # noqa: E731
    return [dict(logits=wide(lg, case[1] * case[3]), labels=torch.from_numpy(lab).cuda(), split=torch.from_numpy(sp).cuda(),
                 C=case[2], cs=case[3]) for case, (lg, lab, sp) in zip(CASES, hosts)]


def _vector_path(job):
    """the kernel's rule (csrc/confusion.hip: vec_in): 16-byte loads of a replica's classes, four at a time, when the logits' pointer and
    pitch are multiples of 16 bytes and cs is a multiple of 4 - used for the groups of four that lie inside the C classes"""
    t = job["logits"]
    return t.shape[0] > 0 and job["C"] >= 4 and job["cs"] % 4 == 0 and t.data_ptr() % 16 == 0 and (max(t.stride(0), t.shape[1]) * 4) % 16 == 0


@pytest.fixture(scope="module")
def hosts():
    return [_host(case, 300 + i, _pad(i)) for i, case in enumerate(CASES)]


@pytest.fixture(scope="module")
def expected(hosts):
    return [ref.confusion(lg, lab, sp, case[2], case[3]) for case, (lg, lab, sp) in zip(CASES, hosts)]


@pytest.fixture(scope="module")
def table(hosts):
    from wdg_amd import ops
    batch = ops.ConfusionBatch(_jobs(hosts))
    batch.launch()
    torch.cuda.synchronize()
    return batch, [c.cpu().numpy().copy() for c in batch.counts_of], [p.cpu().numpy().copy() for p in batch.pred_of]


def test_counts_and_predictions_equal_the_restatement(table, expected):
    _, counts, preds = table
    misses = []
    for i, (case, c, p, (wc, wp)) in enumerate(zip(CASES, counts, preds, expected)):
        assert c.dtype == np.int32 and p.dtype == np.uint8 and c.shape == (case[1], 3, case[2], case[2] + 1) and p.shape == (case[0], case[1])
        if not np.array_equal(p, wp):
            misses.append(f"job {i} {case}: {int((p != wp).sum())} predictions differ")
        if not np.array_equal(c, wc):
            misses.append(f"job {i} {case}: {int((c != wc).sum())} counters differ")
    assert not misses, "\n".join(misses[:20])
    every = np.concatenate([p.reshape(-1) for p in preds])
    assert (every == 255).sum() > 1000 and sum(int(c.sum()) for c in counts) > 30000 and sum(int(c[..., -1].sum()) for c in counts) > 1000
    assert len(CASES) == 270 and max(c[1] * 3 * c[2] * (c[2] + 1) for c in CASES) > 8192  # (more counters than a workgroup holds at once)


def test_the_table_covers_both_load_paths(table, expected):
    """the adversarial rows - ties, all -inf, NaNs, NaN padding - meet the 16-byte loads as well as the scalar ones: for every R and
    every C >= 4 there are jobs on either path, among them jobs of more than one workgroup, and the larger jobs of both paths hold
    unpredicted rows and counted rows"""
    jobs = table[0].keep
    vec = {(c[1], c[2], c[3]) for c, j in zip(CASES, jobs) if _vector_path(j)}
    scalar = {(c[1], c[2], c[3]) for c, j in zip(CASES, jobs) if c[0] and not _vector_path(j)}
    assert {(R, C) for R, C, _ in vec} == {(R, C) for R in RS for C in (5, 7, 16)}, vec
    assert {(R, C) for R, C, _ in scalar} == {(R, C) for R in RS for C in CS}, scalar
    assert {cs for _, _, cs in vec} == {8, 16} and (17, 16, 16) in vec and (17, 16, 16) in scalar
    for path in (True, False):
        big = [w for c, j, w in zip(CASES, jobs, expected) if c[0] >= 63 and c[1] >= 3 and c[2] >= 5 and _vector_path(j) == path]
        assert len(big) >= 20 and all(int((wp == 255).sum()) > 0 and int(wc.sum()) > 0 for wc, wp in big), path
        assert any(c[0] == 130 and _vector_path(j) == path for c, j in zip(CASES, jobs))


def test_a_second_launch_repeats_and_the_counts_add_onto_a_pool(table, expected):
    batch, counts, preds = table
    batch.launch()
    torch.cuda.synchronize()
    assert all(np.array_equal(c.cpu().numpy(), w) for c, w in zip(batch.counts_of, counts))
    assert all(np.array_equal(p.cpu().numpy(), w) for p, w in zip(batch.pred_of, preds))
    pool = np.random.default_rng(9).integers(0, 1000, batch.counts.shape[0]).astype(np.int32)
    batch.counts.copy_(torch.from_numpy(pool))
    batch.launch(zero=False)
    torch.cuda.synchronize()
    flat = np.concatenate([w.reshape(-1) for w, _ in expected])
    assert np.array_equal(batch.counts.cpu().numpy()[:len(flat)].astype(np.int64), pool[:len(flat)] + flat)
    batch.launch()  # (and the front end's own launch starts from zero again)
    assert all(np.array_equal(c.cpu().numpy(), w) for c, w in zip(batch.counts_of, counts))


def test_a_replica_alone_answers_as_in_the_table(table):
    """a job alone in a table, and single replicas of it as jobs of their own (R = 1 over a column range of the logits)"""
    from wdg_amd import ops
    batch, counts, preds = table
    jobs = batch.keep
    picked = [k for k, c in enumerate(CASES) if c[0] == 130 and c[1] == 17 and c[2] in (5, 16)]
    assert {_vector_path(jobs[k]) for k in picked} == {True, False}  # (a slice of one replica, r cs floats on, keeps its job's path)
    for i in picked:
        n, R, C, cs = CASES[i]
        alone = ops.ConfusionBatch([jobs[i]])
        alone.launch()
        assert np.array_equal(alone.counts_of[0].cpu().numpy(), counts[i]) and np.array_equal(alone.pred_of[0].cpu().numpy(), preds[i])
        singles = ops.ConfusionBatch([dict(logits=jobs[i]["logits"][:, r * cs:(r + 1) * cs], labels=jobs[i]["labels"],
                                           split=jobs[i]["split"][:, r:r + 1].contiguous(), C=C, cs=cs) for r in (0, 9, 10, 16)])
        assert all(_vector_path(s) == _vector_path(jobs[i]) for s in singles.keep)
        singles.launch()
        for k, r in enumerate((0, 9, 10, 16)):
            assert np.array_equal(singles.counts_of[k].cpu().numpy()[0], counts[i][r]), (i, r)
            assert np.array_equal(singles.pred_of[k].cpu().numpy()[:, 0], preds[i][:, r]), (i, r)


@pytest.mark.parametrize("path", ["16-byte loads", "scalar loads"])
def test_a_job_damaged_in_device_memory_is_skipped(table, path):
    from wdg_amd import ops, train
    from wdg_amd._lib import lib
    jobs = table[0].keep
    i = next(k for k, c in enumerate(CASES) if c[0] in (65, 130) and c[1:] == (3, 5, 8) and _vector_path(jobs[k]) == (path == "16-byte loads"))
    job, n = jobs[i], CASES[i][0]
    batch = ops.ConfusionBatch([job, job])
    batch.launch()
    want = batch.counts_of[1].cpu().numpy().copy()
    sound = batch.table.cpu().numpy().view(train._CONFUSION_JOB_DTYPE).copy()
    for field, value in [("C", 0), ("C", 17), ("cs", 4), ("ld_logits", 23), ("logits", 0), ("labels", 0), ("split", 0), ("counts", 0), ("R", 0), ("n", -1)]:
        tab = sound.copy()
        tab[field][0] = value  # ("ld_logits" 23: below R cs = 24)
        dev = torch.from_numpy(tab.view(np.uint8)).cuda()
        batch.counts.zero_()
        batch.pred.fill_(77)
        assert lib.wdg_confusion_batched_i32(ctypes.c_void_p(dev.data_ptr()), 2, n, 5, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        assert not batch.counts_of[0].any() and bool((batch.pred_of[0] == 77).all()), (field, value)
        assert np.array_equal(batch.counts_of[1].cpu().numpy(), want), (field, value)


def test_refusals():
    from wdg_amd import ops
    n, R, C, cs = 10, 3, 5, 8
    ok = lambda **kw: {**dict(logits=torch.zeros((n, R * cs), device="cuda"), labels=torch.zeros(n, dtype=torch.int32, device="cuda"),  # noqa: E731
                              split=torch.zeros((n, R), dtype=torch.uint8, device="cuda"), C=C, cs=cs), **kw}
    ops.ConfusionBatch([ok()]).launch()
    ops.ConfusionBatch([]).launch()  # an empty table launches nothing
    ops.ConfusionBatch([ok(cs=C, logits=torch.zeros((n, R * C), device="cuda"))])
    for kw in (dict(C=0), dict(C=17, cs=17), dict(cs=4), dict(logits=torch.zeros((n, R * cs - 1), device="cuda")),
               dict(logits=torch.zeros((n + 1, R * cs), device="cuda")), dict(logits=torch.zeros((n, R * cs), device="cuda").double()),
               dict(logits=torch.zeros((n, R * cs))), dict(labels=torch.zeros(n, dtype=torch.int64, device="cuda")),
               dict(labels=torch.zeros(n + 1, dtype=torch.int32, device="cuda")), dict(split=torch.zeros((n, R), dtype=torch.int32, device="cuda")),
               dict(split=torch.zeros((R, n), dtype=torch.uint8, device="cuda").t()), dict(extra=1)):
        with pytest.raises(ValueError):
            ops.ConfusionBatch([ok(**kw)])
