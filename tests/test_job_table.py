"""job_table.py without a device: the offsets of the buffers a table owns, the byte stride of a unit, the count test before the entry
checks, and the two leading-dimension rules of the stacked-logits tables being one number."""
import numpy as np
import pytest
import torch

from wdg_amd import ops
from wdg_amd._rt import _ld
from wdg_amd.csbmh import QdaBatch
from wdg_amd.job_table import JobTable, block_offsets, unit_bytes


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
    (lambda: ops.SparseDenseBatch(TOO_MANY), "entries"), pytest.param(lambda: ops.TwoHopBatch(TOO_MANY), "graphs", id="TwoHopBatch"),
    pytest.param(lambda: ops.TopkRowsBatch(TOO_MANY), "jobs", id="TopkRowsBatch")])
def test_the_count_is_tested_before_any_entry(build, noun):
    with pytest.raises(ValueError, match=f": 65536 {noun}; one launch takes 65535"):
        build()


def test_the_tables_without_a_limit_have_none():
    assert ops.HeadTrainBatch.MAX_JOBS is None and ops.DropoutBatch.MAX_JOBS is None
    for table in (ops.RowRepBatch, ops.GramBatch, ops.EdgeGramBatch, ops.KrSets, ops.KrBatch, ops.GnbBatch, ops.SvmBatch, ops.StatsBatch,
                  ops.LasBatch, ops.GemmBatch, ops.Mlp2Batch, ops.ClassGraphBatch, ops.GaussFeatureBatch, QdaBatch):
        assert issubclass(table, JobTable) and table.MAX_JOBS is None, table.__name__


def _qda_job(mean_shape):
    return (torch.zeros(4, 2), torch.zeros(4, 2), torch.zeros(4, dtype=torch.int32), (np.zeros(mean_shape), np.zeros((3, 2)), np.zeros((3, 2))))


@pytest.mark.parametrize("build, text", [
    (lambda: ops.RowRepBatch(), "RowRepBatch: dense or csr"),
    (lambda: ops.RowRepBatch(dense=[torch.zeros(2, 3, dtype=torch.float64)]), "RowRepBatch: A must be fp32 with unit inner stride"),
    (lambda: ops.GramBatch([torch.zeros(3, 2).t()]), "GramBatch: A must be fp32 with unit inner stride"),
    (lambda: ops.KrSets([(torch.zeros(3, dtype=torch.int32), np.ones(65, np.int32), np.ones(65, np.int32), 1)], 2), "KrSets: more than 64 classes"),
    (lambda: ops.KrBatch([], 3, route="fast"), r"KrBatch: unknown route 'fast' \(one of auto, registers, large\)"),
    (lambda: ops.KrBatch.from_arrays(*([np.ones(1, np.int64)] * 5), [321], [1], 3, route="registers"),
     r"KrBatch: 321..321 train rows, the solver holds blocks of 1..320 \(route 'registers'; the large solver holds 1..1024\)"),
    (lambda: ops.KrBatch.from_arrays(*([np.ones(1, np.int64)] * 7), 9), r"KrBatch: 9 classes, the solver holds 1..8 \(class_windows=True: 1..16\)"),
    (lambda: ops.GnbBatch([None], 17), "GnbBatch: 17 classes, the kernel holds 1..16"),
    (lambda: ops.GnbBatch([(torch.zeros(4, 2), torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))], 2),
     "GnbBatch: X must be a row-major fp32 device matrix"),
    (lambda: ops.SvmBatch([], 3, "sigmoid", 1.0, "scale"), "SvmBatch: unknown kernel 'sigmoid'"),
    (lambda: ops.SvmBatch([], 3, "rbf", 1.0, 0.0), "SvmBatch: gamma must be positive or 'scale'"),
    (lambda: ops.GemmBatch([(torch.zeros(2, 3), torch.zeros(4, 2), torch.zeros(2, 2), None)]), "GemmBatch: shape / layout mismatch"),
    (lambda: ops.Mlp2Batch([]), "Mlp2Batch: needs H <= 64, C <= 8, K <= 512, K % 4 == 0, 16-byte aligned rows of A"),
    (lambda: ops.TwoHopBatch([], flags=4), r"TwoHopBatch: flags = 4 \(TWO_HOP_KEEP_ONE_HOP = 1 and TWO_HOP_KEEP_SELF = 2 are defined\)"),
    (lambda: ops.TopkRowsBatch([dict(scores=torch.zeros(2, 3), k=65)]), "TopkRowsBatch: entry 0 has k = 65; 1 .. 64 are supported"),
    (lambda: ops.ClassGraphBatch([((1,) * 17, (0,) * 17, (0,) * 17, 1)]), "class_graphs_device: graph 0: 1 .. 16 classes with a size, a k and a d each"),
    (lambda: ops.GaussFeatureBatch([torch.zeros(2, dtype=torch.int32)], np.zeros((2, 3)), np.zeros(2), [1], ld=2),
     "gauss_features_device: ld = 2 below F = 3"),
    (lambda: QdaBatch([_qda_job((3, 2, 3))]), r"QdaBatch: job 0: mean of shape \(3, 2, 3\) for F = 2 \(at most 16 features\)"),
])
def test_an_entry_check_raises_its_own_error_before_a_device_is_asked_for(build, text):
    """(on a machine without a GPU the constructors used to stop at require_gpu(): the checks now come first, as the base's sequence has it)"""
    with pytest.raises(ValueError, match=text):
        build()


def test_a_sparse_dense_entry_of_the_wrong_type_is_a_type_error():
    with pytest.raises(TypeError, match="SparseDenseBatch: entry 0: a DeviceFeatures expected, not NoneType"):
        ops.SparseDenseBatch([(None, False, None, None)])


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
