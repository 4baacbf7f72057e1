"""The device generators' DEFINITION (include/wdg.h: wdg_synth_regular_batched, wdg_synth_feature_rows), pinned on the host before any
device sees it: the numpy restatement (tests/_synth_ref.py) has the family's structure and the reference files' distribution, and the
entry refuses malformed tables without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from scipy.stats import chi2

import _synth_ref as ref
from _golden import SYN, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("loops", [0, 1])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restated_graphs_have_the_familys_structure(shape, loops):
    """strictly ascending rows of d (d + 1 with loops) columns, exactly k of them in the row's own class (the loop not counted),
    column i in row i exactly when loops are asked for; labels = i // m"""
    n, C, k, d = shape
    rowptr, col, labels = ref.cached_graph(n, C, k, d, 1234567 + n, ref.SELF_LOOPS * loops)
    m, D = n // C, d + loops
    assert np.array_equal(rowptr, np.arange(n + 1) * D) and np.array_equal(labels, np.arange(n) // m)
    rows = col.reshape(n, D).astype(np.int64)
    assert rows.min() >= 0 and rows.max() < n
    assert (np.diff(rows, axis=1) > 0).all()
    is_self = rows == np.arange(n)[:, None]
    assert (is_self.sum(1) == loops).all()
    same = (labels[rows] == labels[:, None]) & ~is_self
    assert (same.sum(1) == k).all()


def test_loops_only_add_the_diagonal():
    for n, C, k, d in ref.SHAPES[:5]:
        a = ref.cached_graph(n, C, k, d, 99)[1].reshape(n, d)
        b = ref.cached_graph(n, C, k, d, 99, ref.SELF_LOOPS)[1].reshape(n, d + 1)
        for i in range(n):
            assert np.array_equal(np.sort(np.append(a[i], i)), b[i])


def _bounds(n, C):
    return chi2.ppf(1e-6, n - C), chi2.ppf(1 - 1e-6, n)


def test_restated_draws_are_uniform():
    """n = 200, C = 5, k = 4, h = 0.2 (d = 20), 64 seeds: the in-degree chi-square of the same-class and of the other-class edges"""
    n, C, k, d = 200, 5, 4, 20
    graphs = [ref.regular_graph(n, C, k, d, ref.mix64(s, 200, n, k, ref.SYNTH_TAG))[1].reshape(n, d).astype(np.int64) for s in range(64)]
    lo, hi = _bounds(n, C)
    stat_s, stat_o = ref.column_chi2(graphs, n, C, k, d)
    print(f"same-class {stat_s:.1f}, other-class {stat_o:.1f}, bounds [{lo:.1f}, {hi:.1f}]")
    assert lo < stat_s < hi and lo < stat_o < hi


@pytest.mark.parametrize("name", SYN)
def test_reference_files_follow_the_restated_rule(name):
    """the five fixture graphs written by the reference's (absent) generator: the structure of the rule, and the same in-degree
    statistic inside the same kind of interval - the evidence that the restated rule is the reference's distribution"""
    g = load(name)
    n, C = int(g["n_nodes"]), 5
    m = n // C
    row, col, lab = g["adj_row"].astype(np.int64), g["adj_col"].astype(np.int64), g["labels"].astype(np.int64)
    assert np.array_equal(lab, np.arange(n) // m)
    d = len(row) // n
    assert np.array_equal(np.bincount(row, minlength=n), np.full(n, d))
    order = np.lexsort((col, row))
    rows = col[order].reshape(n, d)
    assert (np.diff(rows, axis=1) > 0).all() and not (rows == np.arange(n)[:, None]).any()
    k = int(((lab[rows] == lab[:, None]).sum(1))[0])
    assert ((lab[rows] == lab[:, None]).sum(1) == k).all()
    h = float(name.split("_")[2])
    assert d == int(k / h) and k == int(name.split("_")[1]) // 400
    lo, hi = _bounds(n, C)
    stat_s, stat_o = ref.column_chi2([rows], n, C, k, d)
    print(f"{name}: same-class {stat_s:.1f}, other-class {stat_o}, bounds [{lo:.1f}, {hi:.1f}]")
    assert lo < stat_s < hi
    if d > k:  # (the d = k fixture has no other-class edges)
        assert lo < stat_o < hi
    else:
        assert stat_o is None


def test_feature_rows_come_from_the_nodes_class_and_are_uniform():
    rng = np.random.default_rng(11)
    base = rng.integers(0, 7, 2708)
    n, C = 2100, 7
    m = n // C
    picks = [ref.feature_rows(base, n, C, ref.mix64(s, 77)) for s in range(64)]
    for p in picks[:4]:
        assert np.array_equal(base[p], np.arange(n) // m)
    c = 3
    members = np.flatnonzero(base == c)
    M = len(members)
    cnt = np.bincount(np.concatenate([p[c * m:(c + 1) * m] for p in picks]), minlength=len(base))[members].astype(np.float64)
    assert cnt.sum() == 64 * m
    e = 64 * m / M
    stat = float(((cnt - e) ** 2 / (e * (1 - 1 / M))).sum())
    lo, hi = chi2.ppf(1e-6, M - 1), chi2.ppf(1 - 1e-6, M)
    print(f"class {c}: {M} members, statistic {stat:.1f}, bounds [{lo:.1f}, {hi:.1f}]")
    assert lo < stat < hi
    with pytest.raises(ValueError):
        ref.feature_rows(np.zeros(10, np.int64), 10, 2, 1)  # class 1 has no base rows


def test_job_seed_is_the_packages():
    from wdg_amd import sweep
    j = sweep.Job(0.3, 7, 10, 2000, 5)
    assert sweep.synth_seed(j) == ref.job_seed(7, 0.3, 2000, 10) == sweep._mix64(7, 300, 2000, 10, ref.SYNTH_TAG)
    assert sweep.synth_specs([j]) == [(2000, 5, 10, 33, ref.job_seed(7, 0.3, 2000, 10))]


# ------------------------------------------------------------------------------------------------------------- the ABI, without a GPU
def _table(*specs):
    """host table of wdg_synth_job with (fake, never dereferenced) non-null outputs"""
    import wdg_amd._lib as L
    jobs = (L.SynthJob * len(specs))()
    for j, (n, C, k, d, flags) in zip(jobs, specs):
        j.rowptr = j.col = j.val = j.labels = 0x1000
        j.n, j.n_classes, j.k, j.d, j.flags, j.seed = n, C, k, d, flags, 5
    return jobs


def test_generator_entry_refuses_bad_tables_before_any_launch():
    import wdg_amd._lib as L
    call, null, fake = L.lib.wdg_synth_regular_batched, ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
    assert call(null, null, 0, null) == 0                                      # nothing to do
    assert call(null, null, 3, null) == -1                                     # a null table
    good = _table((2000, 5, 10, 66, 0))
    assert call(ctypes.cast(good, ctypes.c_void_p), null, 1, null) == -1       # a null device table
    assert call(ctypes.cast(good, ctypes.c_void_p), fake, 65536, null) == -1   # more jobs than one grid dimension
    assert call(ctypes.cast(good, ctypes.c_void_p), fake, -1, null) == -1
    for bad in [(2001, 5, 10, 66, 0),      # C does not divide n
                (2000, 5, 400, 400, 0),    # k > m - 1
                (2000, 5, 0, 10, 0),       # k < 1
                (2000, 5, 10, 9, 0),       # d < k
                (2000, 5, 10, 1611, 0),    # d - k > n - m
                (16385, 1, 2, 2, 0),       # n > 16384
                (2000, 5, 10, 66, 2)]:     # unknown flag
        t = _table((10, 5, 1, 1, 0), bad)
        assert call(ctypes.cast(t, ctypes.c_void_p), fake, 2, null) == -1, bad
        assert L.lib.wdg_last_error()
    t = _table((10, 5, 1, 1, 0))
    t[0].col = 0
    assert call(ctypes.cast(t, ctypes.c_void_p), fake, 1, null) == -1          # a null output
    rows = L.lib.wdg_synth_feature_rows
    assert rows(null, 10, 0, 5, 1, null, null, 0, null) == 0                   # no nodes
    assert rows(null, 10, 7, 5, 1, null, null, 0, null) == -1                  # C does not divide n
    assert rows(null, 10, 10, 5, 1, null, null, 0, null) == -1                 # null pointers
    assert rows(fake, 10, 10, 5, 1, fake, fake, 8, null) == -3                 # workspace too small
    assert L.lib.wdg_synth_feature_rows_workspace_bytes(2708, 7) == (2708 * 7 + 7) * 4


def test_synth_job_layout_matches_header(tmp_path):
    """size and field offsets of wdg_synth_job as gcc lays them out == the ctypes mirror"""
    import wdg_amd._lib as L
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(wdg_synth_job));']
    for fname, _ in L.SynthJob._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(wdg_synth_job, {fname}));')
    lines += ['printf("loops %d\\n", WDG_SYNTH_SELF_LOOPS);', "return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.SynthJob)
    for fname, _ in L.SynthJob._fields_:
        assert int(got[fname]) == getattr(L.SynthJob, fname).offset, fname
    assert int(got["loops"]) == ref.SELF_LOOPS
    assert {"rowptr", "col", "val", "labels", "seed", "n", "n_classes", "k", "d", "flags"} <= {f for f, _ in L.SynthJob._fields_}


def test_python_refusals_need_no_gpu():
    from wdg_amd import ops, sweep
    with pytest.raises(ValueError):
        ops.GraphBatch.generated([(10, 5, 1, 1, 0)], ops.COO_SYMMETRISE)
    with pytest.raises(ValueError):
        sweep.SweepBatch([], generate="gpu")
    with pytest.raises(ValueError):
        sweep._check_generate("Device")
    jobs = sweep.make_jobs([0.5], [0], k=2, n_nodes=100)
    for kw in (dict(inputs=[(None, None, None, None)]), dict(share=object()), dict(build="per_graph")):
        with pytest.raises(ValueError):
            sweep.SweepBatch(jobs, generate="device", **kw)


def test_new_kernels_spill_nothing():
    """build/synth.rsrc (written by the Makefile): two kernels, no spilled VGPR, no scratch"""
    import glob
    import re
    if not glob.glob(os.path.join(ROOT, "build", "*.rsrc")):
        pytest.skip("no resource reports (the library was built without the Makefile)")
    path = os.path.join(ROOT, "build", "synth.rsrc")
    assert os.path.exists(path), "the Makefile did not compile csrc/synth.hip"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 2 and any("synth_regular_kernel" in x for x in names) and any("synth_feature_rows_kernel" in x for x in names)
    assert [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", text)] == [0, 0]
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)] == [0, 0]
