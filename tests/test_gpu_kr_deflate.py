"""The deflation pre-pass of the two kernel-regression solvers (csrc/kr_deflate.h: kr_deflate_kernel through route "registers",
kr_large_deflate_kernel through route "large"), read from the workspace it leaves: the same problems through both routes, both
workspaces decoded by the layout (P = 320 / P = n_train rounded up to 32) and compared with each other and with a numpy restatement
of the pass.  The train-row counts are the smallest at which a mechanism of the pass can break: 1; 8 and 9 (the first-match search
takes eight ids at a time); 33 (P = 64 != n_train on the large route); 63, 64, 65 (the ballot prefix across a wave edge); 320 (the
register route's last thread); 321 and 1024 (the large route alone).  Diagonals of K are exactly 0 or at least 1e-3 of the largest:
the drop threshold n eps max K_ii / 64 (< 2e-6 of the largest at 1024 rows) is never near a tested value."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_VAL, N_CLASSES, MAX_C = 5, 5, 8
NTS_BOTH = [1, 8, 9, 33, 63, 64, 65, 320]
NTS_LARGE = [321, 1024]
P_REGISTERS = 320


def pad32(n):
    return (n + 31) & ~31


def make_case(nt, rng, with_rep=True):
    """a problem of `nt` train rows over nt + 12 nodes -> dict of host arrays (K SPD apart from its zero rows, with the diagonal `d`)"""
    n = nt + 12
    train = np.sort(rng.choice(n - 6, nt, replace=False)).astype(np.int32)
    val = np.arange(n - N_VAL, n, dtype=np.int32)
    labels = rng.integers(0, N_CLASSES, n).astype(np.int32)
    rep = np.arange(n, dtype=np.int32)
    d = rng.uniform(0.01, 1.0, n).astype(np.float32)
    d[train[0]] = 1.0
    used = {0}

    def merge(a, b, same_label):  # train row b joins the class of train row a (a < b: the representative is the smallest id)
        rep[train[b]] = rep[train[a]]
        labels[train[b]] = labels[train[a]] if same_label else (labels[train[a]] + 1) % N_CLASSES
        used.update((a, b))

    if nt == 8:
        merge(0, 7, True)  # (the match sits in the one group of eight that thread 7 reads)
    if nt >= 9:
        merge(1, nt - 1, True)        # a duplicate class, first and later member in different waves from 65 rows up
        merge(2, nt - 2, False)       # a class with mixed labels
        if nt >= 12:
            merge(2, 3, True)         # (two members with one label, one with another)
        d[train[5]] = 0.0             # a zero row: dropped
        d[train[6]] = 1e-3            # the smallest diagonal that is kept
        used.update((5, 6))
        for _ in range(nt // 16):     # further pairs, so that the compaction moves rows in every wave
            a, b = sorted(rng.choice(nt, 2, replace=False).tolist())
            if a not in used and b not in used:
                merge(a, b, True)
        rep[val[0]] = rep[train[4]]   # a validation id that duplicates a train row
        rep[val[1]] = rep[train[1]]   # ... and one that duplicates a merged class
    val = val[rng.permutation(N_VAL)]
    sign = rng.choice([-1.0, 1.0], n)
    corr = 0.5 * np.eye(n) + 0.5 * np.outer(sign, sign)  # unit diagonal, eigenvalues >= 0.5
    s = np.sqrt(d.astype(np.float64))
    K = (corr * np.outer(s, s)).astype(np.float32)
    K[np.arange(n), np.arange(n)] = d
    return dict(nt=nt, K=K, train=train, val=val, labels=labels, rep=rep if with_rep else None)


def restate(case, P):
    """the pre-pass in numpy -> the workspace's fields at stride P"""
    train, val, labels, K = case["train"], case["val"], case["labels"], case["K"]
    rep = case["rep"] if case["rep"] is not None else np.arange(K.shape[0], dtype=np.int32)
    slot_of, reps, members, counts = {}, [], [], []
    dropped = False
    for g in train:
        r = int(rep[g])
        if K[r, r] == 0:
            dropped = True
            continue
        if r not in slot_of:  # the first occurrence in train order keeps the class: slots in that order
            slot_of[r] = len(reps)
            reps.append(r), members.append(0), counts.append(np.zeros(MAX_C, np.int64))
        members[slot_of[r]] += 1
        if 0 <= labels[g] < MAX_C:
            counts[slot_of[r]][labels[g]] += 1
    kept = len(reps)
    lab, mixed = np.full(P, -1, np.int32), []
    for s_, (m, cnt) in enumerate(zip(members, counts)):
        nz = np.flatnonzero(cnt)
        if nz.size == 1 and cnt[nz[0]] == m:
            lab[s_] = nz[0]
        elif nz.size:
            lab[s_] = -2
            mixed += [(s_ << 16) | (int(c) << 12) | int(cnt[c]) for c in nz]
    tr = np.full(P, -1, np.int32)
    tr[:kept] = reps
    return dict(header=[kept, int(kept != train.shape[0]), len(mixed), int(dropped)], train=tr, lab=lab, mixed=sorted(mixed),
                members=np.asarray(members, np.int64), val_rep=rep[val], val_lab=labels[val])


def decode(words, P, n_val=N_VAL):
    """a problem's workspace words -> its fields (csrc/kr_deflate.h: four header words, four arrays of P words, the validation rows)"""
    kept, n_mixed = int(words[0]), int(words[2])
    o_lab, o_scale, o_mix, o_val = 4 + P, 4 + 2 * P, 4 + 3 * P, 4 + 4 * P
    return dict(header=words[:4].tolist(), train=words[4:4 + P], lab=words[o_lab:o_lab + P], scale_bits=words[o_scale:o_scale + P],
                scale=words[o_scale:o_scale + P].view(np.float32), mixed=sorted(words[o_mix:o_mix + n_mixed].tolist()),
                val_rep=words[o_val:o_val + n_val], val_lab=words[o_val + n_val:o_val + 2 * n_val], kept=kept)


def run(ops, cases, route):
    """one table of `cases` through `route` -> every job's workspace words"""
    up = {id(c): {k: (None if v is None or k == "nt" else torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in c.items()} for c in cases}
    dev = [up[id(c)] for c in cases]  # (a case listed many times is uploaded once)
    kb = ops.KrBatch([(c["K"], c["train"], c["val"], c["labels"], c["rep"]) for c in dev], N_CLASSES, route=route)
    assert kb.large == (route == "large") and kb.ws is not None
    kb.ws.fill_(0x5A)  # (what the pass does not write is not mistaken for a result)
    kb.launch()
    torch.cuda.synchronize()
    return kb.ws.cpu().numpy().view(np.int32).reshape(len(cases), -1)


def check(got, want, P, label):
    print(f"[kr deflate] {label}: header {got['header']} want {want['header']}, mixed {got['mixed']} want {want['mixed']}")
    assert got["header"] == want["header"], label
    for k in ("train", "lab", "val_rep", "val_lab"):
        assert np.array_equal(got[k], want[k]), (label, k)
    assert got["mixed"] == want["mixed"], label
    kept = want["header"][0]
    # (members <= 1024: an ulp of sqrtf moves scale^2 by 2.4e-7 of it, far from half a unit)
    assert np.array_equal(np.rint(got["scale"][:kept].astype(np.float64) ** 2).astype(np.int64), want["members"]), label
    assert np.array_equal(got["scale"][kept:], np.ones(P - kept, np.float32)), label


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from wdg_amd import ops as o
    return o


@pytest.fixture(scope="module")
def tables(ops):
    """every case once, through both routes where the register solver holds it: {nt: (case, words registers | None, words large)}"""
    rng = np.random.default_rng(320)
    cases = [make_case(nt, rng) for nt in NTS_BOTH + NTS_LARGE]
    reg = run(ops, cases[:len(NTS_BOTH)], "registers")
    large = run(ops, cases, "large")
    return {c["nt"]: (c, reg[i] if i < len(NTS_BOTH) else None, large[i]) for i, c in enumerate(cases)}


@pytest.mark.parametrize("nt", NTS_BOTH + NTS_LARGE)
def test_workspace_matches_the_restatement(tables, nt):
    case, reg, large = tables[nt]
    if reg is not None:
        check(decode(reg, P_REGISTERS), restate(case, P_REGISTERS), P_REGISTERS, f"registers, {nt} rows")
    check(decode(large, pad32(nt)), restate(case, pad32(nt)), pad32(nt), f"large, {nt} rows")


@pytest.mark.parametrize("nt", NTS_BOTH)
def test_routes_agree(tables, nt):
    _case, reg, large = tables[nt]
    P = pad32(nt)
    a, b = decode(reg, P_REGISTERS), decode(large, P)
    assert a["header"] == b["header"] and a["mixed"] == b["mixed"]
    for k in ("train", "lab", "scale_bits"):
        assert np.array_equal(a[k][:P], b[k]), k
    for k in ("val_rep", "val_lab"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["train"][P:] == -1).all() and (a["lab"][P:] == -1).all()


@pytest.mark.parametrize("route", ["registers", "large"])
def test_job_without_representatives_beside_one_with(ops, route):
    """one table, one job with `rep` and one without: both get a workspace, the second runs with identity representatives (its zero
    row is still dropped)"""
    rng = np.random.default_rng(321)
    cases = [make_case(33, rng), make_case(33, rng, with_rep=False)]
    words = run(ops, cases, route)
    P = P_REGISTERS if route == "registers" else pad32(33)
    for i, c in enumerate(cases):
        want = restate(c, P)
        check(decode(words[i], P), want, P, f"{route}, job {i}")
    assert restate(cases[1], P)["header"] == [32, 1, 0, 1]


def test_table_longer_than_the_persistent_grid(ops):
    """more jobs of 9 rows than the 2 x CUs workgroups of kr_large_deflate_kernel: a workgroup runs the pass on several problems, one
    after the other, over the same shared arrays"""
    from wdg_amd._lib import lib
    cus = int(lib.wdg_kr_large_scratch_bytes()) // (528 * 4096)
    assert cus >= 1
    rng = np.random.default_rng(322)
    m = 7 if (2 * cus) % 7 else 5  # (problems i and i + 2 x CUs, one workgroup's consecutive ones, are then different cases)
    distinct = [make_case(9, rng) for _ in range(m)]
    cases = [distinct[i % m] for i in range(2 * cus + 5)]
    words = run(ops, cases, "large")
    want = [restate(c, 32) for c in distinct]
    for i in range(len(cases)):
        got = decode(words[i], 32)
        assert got["header"] == want[i % m]["header"] and got["mixed"] == want[i % m]["mixed"], i
        for k in ("train", "lab", "val_rep", "val_lab"):
            assert np.array_equal(got[k], want[i % m][k]), (i, k)
        assert np.array_equal(got["scale_bits"], decode(words[i % m], 32)["scale_bits"]), i
