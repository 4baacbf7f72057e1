"""The numpy restatement of csrc/neighbor_sample.hip as include/wdg.h defines it: the step key, an entry's 64-bit key, the threshold tau
of a forward row (a full sort: not the kernel's register-held candidate set), the kept mask of a forward and of a transposed job and the
thinned CSR with its scale, on _synth_ref.philox4x32_10 and _drop_edge_ref.scale_of / transpose / kept_pairs."""
import numpy as np

from _drop_edge_ref import kept_pairs, scale_of, transpose  # noqa: F401  (the tests read all three through this module)
from _synth_ref import philox4x32_10

TRANSPOSED, KEEP_DIAGONAL, NORM_SYM = 2, 4, 8  # WDG_NEIGHBOR_SAMPLE_*
KEY_TAG = 0x53414745  # "SAGE"
NOTHING = np.uint64(0xFFFFFFFFFFFFFFFF)
SENTINEL = (-7, -7, -7.0, 0x0123456789ABCDEF)  # kept_col, kept_len, scale, tau


def step_key(seed, stream, step):
    """(k0, k1): output words 0 and 1 of Philox4x32-10 with counter {step, stream, 0, 0} and key {seed, 0x53414745}"""
    w = philox4x32_10(np.uint64(step & 0xFFFFFFFF), np.uint64(stream), seed, KEY_TAG)
    return int(w[..., 0]), int(w[..., 1])


def keys(fi, fj, seed, stream, step):
    """key(i, j) of the entries with FORWARD coordinates (fi, fj) -> uint64: word 0 of Philox{i, j, 0, 0} under the step key above the
    column.  Coordinates are taken as the uint32 the kernel sees."""
    i, j = np.asarray(fi, np.int64) & 0xFFFFFFFF, np.asarray(fj, np.int64) & 0xFFFFFFFF
    k0, k1 = step_key(seed, stream, step)
    w = philox4x32_10(i.astype(np.uint64), j.astype(np.uint64), k0, k1)[..., 0].astype(np.uint64)
    return (w << np.uint64(32)) | j.astype(np.uint64)


def sample(rowptr, col, n_cols, flags, fanout, seed, stream, step, sentinel=SENTINEL):
    """a FORWARD job -> (kept_col [nnz], kept_len [n], scale [n], tau [n] uint64) as phase 0 leaves them over outputs pre-filled with
    `sentinel`: a row whose extent lies outside [0, nnz] keeps it"""
    assert not flags & TRANSPOSED and 1 <= fanout <= 64
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n, nnz = rowptr.shape[0] - 1, col.shape[0]
    kept_col, kept_len, scale = np.full(nnz, sentinel[0], np.int32), np.full(n, sentinel[1], np.int32), np.full(n, sentinel[2], np.float32)
    tau = np.full(n, sentinel[3], np.uint64)
    for i in range(n):
        beg, end = int(rowptr[i]), int(rowptr[i + 1])
        if not 0 <= beg <= end <= nnz:
            continue
        cols = col[beg:end]
        valid = (cols >= 0) & (cols < n_cols)
        protected = valid & (cols == i) if flags & KEEP_DIAGONAL else np.zeros(end - beg, bool)
        key = keys(np.full(end - beg, i), cols, seed, stream, step)
        eligible = np.sort(key[valid & ~protected])  # with multiplicity
        tau[i] = eligible[fanout - 1] if len(eligible) >= fanout else NOTHING
        keep = valid & (protected | (key <= tau[i]))
        c = int(keep.sum())
        kept_col[beg:beg + c], kept_col[beg + c:end], kept_len[i] = cols[keep], -1, c
        scale[i] = scale_of([c], flags)[0]
    return kept_col, kept_len, scale, tau


def thin_transposed(rowptr, col, n_cols, flags, tau, seed, stream, step, sentinel=SENTINEL):
    """a TRANSPOSED job (its n_cols = the forward job's rows, tau [n_cols] = the forward job's) -> (kept_col, kept_len, scale) as phase 1
    leaves them"""
    assert flags & TRANSPOSED
    rowptr, col, tau = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(tau, np.uint64)
    n, nnz = rowptr.shape[0] - 1, col.shape[0]
    kept_col, kept_len, scale = np.full(nnz, sentinel[0], np.int32), np.full(n, sentinel[1], np.int32), np.full(n, sentinel[2], np.float32)
    for i in range(n):
        beg, end = int(rowptr[i]), int(rowptr[i + 1])
        if not 0 <= beg <= end <= nnz:
            continue
        cols = col[beg:end]
        valid = (cols >= 0) & (cols < n_cols)
        protected = valid & (cols == i) if flags & KEEP_DIAGONAL else np.zeros(end - beg, bool)
        key = keys(cols, np.full(end - beg, i), seed, stream, step)  # the forward coordinates of (i, j) are (j, i)
        t = np.where(valid, tau[np.where(valid, cols, 0)] if len(tau) else np.uint64(0), np.uint64(0)) if end > beg else np.zeros(0, np.uint64)
        keep = valid & (protected | (key <= t))
        c = int(keep.sum())
        kept_col[beg:beg + c], kept_col[beg + c:end], kept_len[i] = cols[keep], -1, c
        scale[i] = scale_of([c], flags)[0]
    return kept_col, kept_len, scale
