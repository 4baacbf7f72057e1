"""numpy restatement of wdg_relu_dropout_batched_f32 as include/wdg.h defines it: the mask of an element from Philox4x32-10
(_synth_ref.philox4x32_10) at (seed, stream, step, row, column group), ReLU and the inverted-dropout scale in fp32."""
import functools
import math

import numpy as np

from _synth_ref import philox4x32_10

# the shapes of the mask statistics and of the device comparison
SHAPES = [(600, 16), (67, 5), (130, 64), (257, 33)]
STEP_SIGNED = (1 << 31) + 5  # a step word whose top bit is set: read as a signed number anywhere, it draws another mask


def constants(p):
    """-> (drop_threshold uint32 as int, scale np.float32): floor(p 2^32) computed in fp64, (float)(1 / (1 - p))"""
    assert 0.0 <= p < 1.0
    return int(math.floor(float(p) * 4294967296.0)), np.float32(1.0 / (1.0 - float(p)))


def words(rows, cols, seed, stream, step):
    """the generator word of every element -> uint32 [rows, cols]: word c & 3 of the block with counter {r ceil(cols / 4) + (c >> 2),
    step, 0, 0} and key {seed, stream}"""
    gpr = (cols + 3) // 4
    assert rows * gpr < 1 << 32
    g = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(gpr) + np.arange(gpr, dtype=np.uint64)[None, :]
    w = philox4x32_10(g, np.uint64(step & 0xFFFFFFFF), seed & 0xFFFFFFFF, stream & 0xFFFFFFFF)  # [rows, gpr, 4]
    return w.reshape(rows, 4 * gpr)[:, :cols]


def keep_mask(rows, cols, p, seed, stream, step):
    """-> bool [rows, cols]: the elements that are kept"""
    return words(rows, cols, seed, stream, step) >= np.uint32(constants(p)[0])


@functools.lru_cache(maxsize=None)
def cached_keep_mask(rows, cols, p, seed, stream, step):
    """keep_mask, computed once per process (the tests share the masks and never write to them)"""
    m = keep_mask(rows, cols, p, seed, stream, step)
    m.setflags(write=False)
    return m


def relu_dropout(h, p, seed, stream, step):
    """-> float32 array like h: h * scale (one fp32 multiply) where kept and h > 0, a NaN where h is one (the same bits), +0.0 elsewhere"""
    h = np.asarray(h, np.float32)
    rows, cols = h.shape
    scale = constants(p)[1]
    keep = keep_mask(rows, cols, p, seed, stream, step) if rows and cols else np.zeros((rows, cols), bool)
    out = np.where(keep & (h > 0), (h * scale).astype(np.float32), np.float32(0.0)).astype(np.float32)
    nan = np.isnan(h)
    out[nan] = h[nan]
    return out
