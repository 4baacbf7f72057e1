"""wdg_keep_best_batched_f32's definition (include/wdg.h) restated in numpy: which elements of a job are copied, and the copy itself on
the 32-bit words."""
import numpy as np


def replica_of(rows, cols, seg_rows, seg_cols, reps):
    """-> int64 [rows, cols]: the replica of every element - segment (i // seg_rows) * ceil(cols / seg_cols) + j // seg_cols, modulo reps"""
    i, j = np.arange(rows, dtype=np.int64)[:, None], np.arange(cols, dtype=np.int64)[None, :]
    segs_per_row = -(-cols // seg_cols)
    return ((i // seg_rows) * segs_per_row + j // seg_cols) % reps


def selected(best, step):
    """best: int [reps, 3], step: the step word -> bool [reps]: the replicas whose best epoch is this step"""
    best = np.asarray(best)
    return (best[:, 0] >= 0) & (best[:, 2] == step)


def keep_best(src, dst, seg_rows, seg_cols, reps, best, step):
    """src, dst: float32 [rows, cols] -> (the new dst, the bool mask of the copied elements); bits are copied, never values"""
    src, dst = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32)
    assert src.shape == dst.shape and src.ndim == 2
    rows, cols = src.shape
    if rows == 0 or cols == 0:
        return dst.copy(), np.zeros(src.shape, bool)
    mask = selected(best, step)[replica_of(rows, cols, seg_rows, seg_cols, reps)]
    out = dst.view(np.uint32).copy()
    out[mask] = src.view(np.uint32)[mask]
    return out.view(np.float32), mask
