"""GPU tests of wdg_keep_best_batched_f32 (csrc/keep_best.hip, ops.KeepBestBatch) against tests/_keep_ref.py, BIT FOR BIT: the kernel
moves 32-bit words, so the bound is equality - of the copied segments and of everything around them."""
import ctypes

import numpy as np
import pytest
import torch

import _keep_ref as ref

pytestmark = pytest.mark.gpu

ROWS = (0, 1, 2, 65)
COLS = (1, 4, 5, 64, 72)
SEG_COLS = (1, 4, 5, 8, 64)
SEG_ROWS = (1, 3, "rows")
LAYOUTS = ("plain", "slices", "offset")
STEP = 7
SENTINEL = 0x7FC0BEEF  # (a NaN with a payload: a kernel that moved VALUES through an arithmetic unit could not keep it either)


def _cases():
    """every (rows, cols) in all three layouts; seg_cols and seg_rows cycle so that each meets every layout and the ragged last segments
    occur (72 columns in segments of 5 and 64, 65 rows in segments of 3); reps cycles through the segment count, a third of it (reps
    below the segment count: channels x replicas) and 5 -> (rows, cols, seg_rows, seg_cols, reps, layout)"""
    out, k = [], 0
    for rows in ROWS:
        for cols in COLS:
            for layout in LAYOUTS:
                sc, sr = SEG_COLS[k % len(SEG_COLS)], SEG_ROWS[(k // len(SEG_COLS)) % len(SEG_ROWS)]
                sr = max(rows, 1) if sr == "rows" else sr
                segs = max(-(-rows // sr) * -(-cols // sc), 1)
                reps = (segs, max(segs // 3, 1), 5)[k % 3 if segs > 1 else 0]
                out.append((rows, cols, sr, sc, reps, layout))
                k += 1
    # the channel-major ACM weight: 3 channels x 5 replicas = 15 column blocks (the last one ragged: 72 = 14 x 5 + 2) for 5 replicas
    out.append((65, 72, 65, 5, 5, "slices"))
    out.append((2, 64, 2, 4, 5, "plain"))  # ... and 16 blocks of four columns for 5 replicas on the 16-byte path
    # 16-byte groups beside a ragged right edge (5 = 4 + 1, 72 = 18 x 4 over row blocks of 3), and a range of a wider matrix in row blocks
    out += [(65, 5, 65, 4, 2, "slices"), (65, 72, 3, 4, 7, "slices"), (65, 64, 3, 8, 5, "slices"), (65, 72, 65, 4, 18, "plain")]
    return out


CASES = _cases()


def _views(rows, cols, layout):
    """-> (wide_src, src, wide_dst, dst): src / dst are [rows, cols] views of the wide device matrices.  "plain": the matrices
    themselves; "slices": a column range, starting at a multiple of 16 bytes, of a matrix whose pitch is one as well (the 16-byte path
    where seg_cols allows); "offset": a pitch of cols + 3 floats and a start one float in (the word path)"""
    z = lambda c: torch.zeros((rows, c), dtype=torch.float32, device="cuda")  # noqa: E731
    if layout == "plain":
        a, b = z(cols), z(cols)
        return a, a, b, b
    if layout == "offset":
        a, b = z(cols + 3), z(cols + 3)
        return a, a[:, 1:1 + cols], b, b[:, 1:1 + cols]
    w = -(-cols // 4) * 4
    a, b = z(w + 8), z(2 * w + 4)
    return a, a[:, 4:4 + cols], b, b[:, w:w + cols]


def _host(case, seed):
    """-> (src words uint32 [rows, cols] with NaNs that carry payloads, -0, infinities and ordinary numbers; best int32 [reps, 3])"""
    rows, cols, _, _, reps, _ = case
    rng = np.random.default_rng(seed)
    src = rng.standard_normal((rows, cols)).astype(np.float32).view(np.uint32).copy()
    kind = rng.random((rows, cols))
    src[kind < 0.1] = 0x7F800001 + rng.integers(0, 1 << 22, (rows, cols), dtype=np.uint32)[kind < 0.1]   # signalling and quiet NaNs
    src[(kind >= 0.1) & (kind < 0.15)] = 0xFFC12345                                                       # a negative NaN with a payload
    src[(kind >= 0.15) & (kind < 0.25)] = 0x80000000                                                      # -0
    src[(kind >= 0.25) & (kind < 0.3)] = 0xFF800000                                                       # -inf
    # per replica: selected now / a stale step / "none yet" beside a matching step / the step before / the step after
    states = np.array([(3, 1, STEP), (4, 2, STEP - 3), (-1, 0, STEP), (2, 2, STEP - 1), (5, 0, STEP + 1), (0, 0, STEP)], np.int32)
    best = states[(np.arange(reps) + seed) % len(states)]
    return src, np.ascontiguousarray(best)


def _sentinel(t):
    t.view(torch.int32).fill_(SENTINEL)


@pytest.fixture(scope="module")
def table():
    """the ragged table, launched once: dict(entries, wides, hosts, batch, got = [(wide dst words, wide src words)], step)"""
    from wdg_amd import ops
    hosts = [_host(case, 50 + i) for i, case in enumerate(CASES)]
    entries, wides = [], []
    for case, (src_w, best) in zip(CASES, hosts):
        wa, a, wb, b = _views(case[0], case[1], case[5])
        entries.append((a, b, case[2], case[3], case[4], torch.from_numpy(best).cuda()))
        wides.append((wa, wb))
    batch = ops.KeepBestBatch(entries)
    step = torch.tensor([STEP], dtype=torch.int32, device="cuda")
    _fill(entries, wides, hosts)
    batch.launch(step)
    torch.cuda.synchronize()
    return dict(entries=entries, wides=wides, hosts=hosts, batch=batch, got=_read(wides), step=step)


def _fill(entries, wides, hosts):
    for (a, b, *_), (wa, wb), (src_w, _) in zip(entries, wides, hosts):
        _sentinel(wa)
        _sentinel(wb)
        if a.numel():
            a.view(torch.int32).copy_(torch.from_numpy(src_w.view(np.int32)))


def _read(wides):
    return [(wb.cpu().numpy().view(np.uint32).copy(), wa.cpu().numpy().view(np.uint32).copy()) for wa, wb in wides]


def _expected(case, host, entry, wide):
    """the words of the whole wide dst and of the whole wide src after the launch, from the restatement"""
    rows, cols, seg_rows, seg_cols, reps, _ = case
    src_w, best = host
    wa, wb = wide
    want_dst = np.full(tuple(wb.shape), SENTINEL, np.uint32)
    want_src = np.full(tuple(wa.shape), SENTINEL, np.uint32)
    off_a = (entry[0].data_ptr() - wa.data_ptr()) // 4 if rows else 0
    off_b = (entry[1].data_ptr() - wb.data_ptr()) // 4 if rows else 0
    want_src[:, off_a:off_a + cols] = src_w
    new, mask = ref.keep_best(src_w.view(np.float32), np.full((rows, cols), SENTINEL, np.uint32).view(np.float32), seg_rows, seg_cols, reps, best, STEP)
    want_dst[:, off_b:off_b + cols] = new.view(np.uint32)
    return want_dst, want_src, mask


def test_the_kernel_equals_the_restatement_bit_for_bit_and_touches_nothing_else(table):
    misses, copied, left = [], 0, 0
    for i, (case, host, entry, wide, (got_dst, got_src)) in enumerate(zip(CASES, table["hosts"], table["entries"], table["wides"], table["got"])):
        want_dst, want_src, mask = _expected(case, host, entry, wide)
        copied, left = copied + int(mask.sum()), left + int((~mask).sum())
        if not np.array_equal(got_src, want_src):
            misses.append(f"job {i} {case}: src was written")
        if not np.array_equal(got_dst, want_dst):
            bad = np.argwhere(got_dst != want_dst)
            r, c = bad[0]
            misses.append(f"job {i} {case}: {len(bad)} words of dst differ, first at ({r}, {c}): {got_dst[r, c]:#x} against {want_dst[r, c]:#x}")
    assert not misses, "\n".join(misses[:20])
    assert copied > 2000 and left > 2000  # both outcomes are well represented


def test_the_table_covers_both_access_paths_and_every_state(table):
    def vec(case, e):
        a, b = e[0], e[1]
        return case[0] > 0 and case[1] >= 4 and case[3] % 4 == 0 and all(
            t.data_ptr() % 16 == 0 and (max(t.stride(0), t.shape[1]) * 4) % 16 == 0 for t in (a, b))
    on = {(c[1], c[3], c[5]) for c, e in zip(CASES, table["entries"]) if vec(c, e)}
    off = {(c[1], c[3], c[5]) for c, e in zip(CASES, table["entries"]) if c[0] > 0 and not vec(c, e)}
    assert {layout for _, _, layout in on} == {"plain", "slices"} and {sc for _, sc, _ in on} >= {4, 8, 64}, on
    assert {layout for _, _, layout in off} == set(LAYOUTS) and {sc for _, sc, _ in off} >= {1, 5}, off
    assert any(c[5] == "offset" and c[3] % 4 == 0 and c[1] >= 4 for c in CASES)  # the word path by the pointer alone
    assert any(c[5] == "slices" and c[1] in (5, 72) and c[3] == 4 for c in CASES)  # 16-byte groups beside a ragged right edge
    segs = [(-(-c[0] // c[2]) * -(-c[1] // c[3]), c[4]) for c in CASES if c[0]]
    assert any(r < s for s, r in segs) and any(r == s for s, r in segs)
    assert {c[2] for c in CASES} >= {1, 3, 65} and {c[3] for c in CASES} == set(SEG_COLS)
    assert any(c[0] and c[1] % c[3] and c[1] > c[3] for c in CASES) and any(c[0] % c[2] and c[0] > c[2] for c in CASES)  # ragged last segments


def test_a_second_launch_and_a_job_alone_give_the_same_bits(table):
    from wdg_amd import ops
    _fill(table["entries"], table["wides"], table["hosts"])
    table["batch"].launch(table["step"])
    torch.cuda.synchronize()
    for i, (again, first) in enumerate(zip(_read(table["wides"]), table["got"])):
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1]), i
    _fill(table["entries"], table["wides"], table["hosts"])
    for e in table["entries"]:
        ops.KeepBestBatch([e]).launch(table["step"])
    torch.cuda.synchronize()
    for i, (alone, first) in enumerate(zip(_read(table["wides"]), table["got"])):
        assert np.array_equal(alone[0], first[0]), (i, CASES[i])


def test_the_step_word_is_read_on_the_device(table):
    """the same table one step later: now the replicas recorded at STEP + 1 are the selected ones"""
    i = next(k for k, c in enumerate(CASES) if c[0] == 65 and c[4] >= 6)  # (six states: every one occurs)
    case, (src_w, best), e = CASES[i], table["hosts"][i], table["entries"][i]
    from wdg_amd import ops
    step = torch.tensor([STEP], dtype=torch.int32, device="cuda")
    _fill([e], [table["wides"][i]], [table["hosts"][i]])
    batch = ops.KeepBestBatch([e])
    step.add_(1)
    batch.launch(step)
    torch.cuda.synchronize()
    want, mask = ref.keep_best(src_w.view(np.float32), np.full(src_w.shape, SENTINEL, np.uint32).view(np.float32), case[2], case[3], case[4], best, STEP + 1)
    assert mask.any() and np.array_equal(e[1].cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_a_job_damaged_in_device_memory_is_left_untouched():
    """the table lives in device memory: a record that is wrong THERE (the host predicate saw the sound one) is skipped by the kernel,
    and its neighbour in the table is served as ever"""
    from wdg_amd import ops, train
    from wdg_amd._lib import lib
    rows, cols = 6, 16
    src = [torch.randn((rows, cols), device="cuda") for _ in range(2)]
    dst = [torch.zeros((rows, cols), device="cuda") for _ in range(2)]
    best = torch.tensor([[1, 1, STEP], [2, 0, STEP]], dtype=torch.int32, device="cuda")
    step = torch.tensor([STEP], dtype=torch.int32, device="cuda")
    batch = ops.KeepBestBatch([(src[k], dst[k], rows, 8, 2, best) for k in range(2)])
    sound = batch.table.cpu().numpy().view(train._KEEP_JOB_DTYPE).copy()
    for field, value in [("seg_rows", 0), ("seg_cols", 0), ("seg_cols", -8), ("reps", 0), ("ld_src", cols - 1), ("ld_dst", cols - 1), ("src", 0),
                         ("dst", 0), ("best", 0), ("dst", src[0].data_ptr()), ("dst", src[0].data_ptr() + 4 * cols)]:
        tab = sound.copy()
        tab[field][0] = value
        assert lib.wdg_keep_best_check_jobs(ctypes.c_void_p(tab.ctypes.data), 2) == -1, field
        dev = torch.from_numpy(tab.view(np.uint8)).cuda()
        for d in dst:
            _sentinel(d)
        keep_src = src[0].clone()
        assert lib.wdg_keep_best_batched_f32(ctypes.c_void_p(dev.data_ptr()), 2, rows, cols, ctypes.c_void_p(step.data_ptr()),
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        assert bool((dst[0].view(torch.int32) == SENTINEL).all()) and torch.equal(src[0], keep_src), (field, value)
        assert torch.equal(dst[1], src[1]), (field, value)


def test_refusals():
    from wdg_amd import ops
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    best = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    ok = (z(4, 8), z(4, 8), 4, 4, 2, best)
    ops.KeepBestBatch([ok])
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.KeepBestBatch([]).launch(step)  # an empty table launches nothing
    wide = z(4, 16)
    bad = [(z(4, 8), z(4, 8), 0, 4, 2, best), (z(4, 8), z(4, 8), 4, 0, 2, best), (z(4, 8), z(4, 8), 4, 4, 0, best),      # below 1
           (z(4, 8), z(4, 8), 4, 4, 3, best), (z(4, 8), z(4, 8), 4, 4, 2, best.long()), (z(4, 8), z(4, 8), 4, 4, 2, best.cpu()),  # best
           (z(4, 8), z(4, 7), 4, 4, 2, best), (z(4, 8).double(), z(4, 8).double(), 4, 4, 2, best), (z(8, 4).t(), z(8, 4).t(), 4, 4, 2, best),
           (z(4, 8).cpu(), z(4, 8), 4, 4, 2, best), (z(32), z(32), 4, 4, 2, best), (wide[:, :8], wide[:, 4:12], 4, 4, 2, best),
           (z(4, 8), z(4, 8), 4, 4, 2)]
    for e in bad:
        with pytest.raises(ValueError):
            ops.KeepBestBatch([e])
    ops.KeepBestBatch([(wide[:, :8], wide[:, 8:], 4, 4, 2, best)])  # (disjoint column ranges of one matrix are fine)
    ops.KeepBestBatch([(z(4, 8), z(4, 12)[:, 2:10], 4, 4, 2, best)])  # (and so are two leading dimensions)
    batch = ops.KeepBestBatch([ok])
    for word in (None, 3, torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32)):
        with pytest.raises(ValueError):
            batch.launch(word)
