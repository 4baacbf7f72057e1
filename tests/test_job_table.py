"""job_table.py without a device: the offsets of the buffers a table owns, the byte stride of a unit, the count test before the entry
checks, and the two leading-dimension rules of the stacked-logits tables being one number."""
import numpy as np
import pytest
import torch

from wdg_amd import ops
from wdg_amd._rt import _ld
from wdg_amd.job_table import block_offsets, unit_bytes


def test_no_jobs_give_the_minimum_and_one_offset():
    off, total = block_offsets([])
    assert off.tolist() == [0] and off.dtype == np.int64 and total == 1


def test_a_job_of_no_elements_between_two_others():
    off, total = block_offsets([3, 0, 2])
    assert off.tolist() == [0, 3, 3, 5] and total == 5


def test_blocks_start_at_multiples_of_the_alignment():
    off, total = block_offsets([15, 1], align=4)
    assert off.tolist() == [0, 16, 20] and total == 20


def test_the_minimum_total_of_adam_is_four_floats():
    off, total = block_offsets([], align=4)
    assert off.tolist() == [0] and total == 4
    assert block_offsets([0], align=4)[1] == 4 and block_offsets([0, 0], align=4)[0].tolist() == [0, 0, 0]
    assert block_offsets([5], align=4)[1] == 8


@pytest.mark.parametrize("dtype, unit, want", [(torch.int32, (3,), 12), (torch.int64, (3,), 24), (torch.int32, (2,), 8), (torch.float64, (), 8),
                                               (torch.uint8, (), 1)])
def test_the_byte_stride_comes_from_the_dtype_and_the_unit(dtype, unit, want):
    assert unit_bytes(dtype, unit) == want


TOO_MANY = [None] * 65536  # (no entry of it would pass a check: the count is tested first)


@pytest.mark.parametrize("build, noun", [
    (lambda: ops.AcmMixBatch(TOO_MANY, False), "entries"), (lambda: ops.AcmMixPackedBatch(TOO_MANY, False), "entries"),
    (lambda: ops.XentEvalBatch(TOO_MANY), "entries"), (lambda: ops.XentCurveBatch(TOO_MANY), "entries"), (lambda: ops.AucBatch(TOO_MANY), "entries"),
    (lambda: ops.AdamBatch(TOO_MANY), "entries"), (lambda: ops.KeepBestBatch(TOO_MANY), "entries"), (lambda: ops.ConfusionBatch(TOO_MANY), "jobs"),
    (lambda: ops.SparseDenseBatch(TOO_MANY), "entries")])
def test_the_count_is_tested_before_any_entry(build, noun):
    with pytest.raises(ValueError, match=f": 65536 {noun}; one launch takes 65535"):
        build()


def test_the_tables_without_a_limit_have_none():
    assert ops.HeadTrainBatch.MAX_JOBS is None and ops.DropoutBatch.MAX_JOBS is None


@pytest.mark.parametrize("view", [torch.zeros(1, 8), torch.zeros(8, 1).t(), torch.zeros(5, 12)[:, :8], torch.zeros(5, 12)[:, 4:]])
def test_max_of_ld_and_the_replicas_columns_is_ld(view):
    """what _stacked_logits_entry admits - R cs <= the row's length, and R cs <= _ld where there is more than one row - never exceeds
    _ld: XentEvalBatch's plain _ld(logits) of old and max(_ld(logits), R cs) are one number"""
    n, width = view.shape
    assert width == 8 and (n == 1 or view.stride(0) == 12)
    admitted = [rcs for rcs in range(0, 64) if not (rcs > width or (n > 1 and rcs > _ld(view)))]
    assert admitted == list(range(9))
    for rcs in admitted:
        assert max(_ld(view), rcs) == _ld(view)
