"""CPU-only checks of the boundary of the neighbour sampler (csrc/neighbor_sample.hip): the ctypes mirror of wdg_neighbor_sample_job against
the layout gcc gives the header's, the front end's record type against the mirror, every refusal include/wdg.h lists - through ctypes, with
a NULL stream and no device -, the host predicate on damaged tables, the refusals of ops.NeighborSampleBatch and models.NeighborSampleAdj
that come before they ask for a device, and the statements the header and the source owe (a `replaces:` line with a citation)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
FIELDS = ["rowptr", "col", "kept_col", "kept_len", "scale", "tau", "n", "n_cols", "nnz", "stream", "flags", "fanout"]


def test_struct_layout_matches_the_header(tmp_path):
    """size and field offsets as gcc lays them out == the ctypes mirror == the numpy record of the front end; the flag values"""
    import wdg_amd._lib as L
    from wdg_amd import neighbor_sample as S
    cname, mirror, dtype = "wdg_neighbor_sample_job", L.NeighborSampleJob, S._NEIGHBOR_SAMPLE_JOB_DTYPE
    assert [f for f, _ in mirror._fields_] == FIELDS == list(dtype.names)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {',
             'printf("flags x %d %d %d %d\\n", WDG_NEIGHBOR_SAMPLE_TRANSPOSED, WDG_NEIGHBOR_SAMPLE_KEEP_DIAGONAL, WDG_NEIGHBOR_SAMPLE_NORM_SYM, '
             'WDG_NEIGHBOR_SAMPLE_MAX_FANOUT);',
             f'printf("{cname} size %zu 0\\n", sizeof({cname}));']
    for fname in FIELDS:
        lines.append(f'printf("{cname} {fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname} *)0)->{fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {tuple(line.split()[:2]): [int(v) for v in line.split()[2:]] for line in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got[("flags", "x")] == [S.NEIGHBOR_SAMPLE_TRANSPOSED, S.NEIGHBOR_SAMPLE_KEEP_DIAGONAL, S.NEIGHBOR_SAMPLE_NORM_SYM, S.MAX_FANOUT] == [2, 4, 8, 64]
    assert got[(cname, "size")][0] == ctypes.sizeof(mirror) == dtype.itemsize == 72
    for fname, ctype in mirror._fields_:
        assert got[(cname, fname)][0] == getattr(mirror, fname).offset == dtype.fields[fname][1], fname
        assert got[(cname, fname)][1] == ctypes.sizeof(ctype) == dtype.fields[fname][0].itemsize, fname
    assert dtype.fields["stream"][0] == np.uint32 and S.NeighborSampleBatch.MAX_JOBS == 65535


def _sample(table, n_jobs, max_rows, phase=0, step=4096):
    import wdg_amd._lib as L
    return L.lib.wdg_neighbor_sample_batched(table, n_jobs, max_rows, phase, 7, ctypes.c_void_p(step), ctypes.c_void_p(0))


def test_launch_refusals_need_no_gpu():
    import wdg_amd._lib as L
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    err = L.lib.wdg_last_error
    assert _sample(null, 1, 8) == INVALID and b"null job table" in err()
    assert _sample(some, -1, 8) == INVALID and b"negative count" in err()
    assert _sample(some, 1, -1) == INVALID and b"negative count" in err()
    assert _sample(some, 65536, 8) == INVALID and b"65535" in err()
    for phase in (-1, 2, 3):
        assert _sample(some, 1, 8, phase=phase) == INVALID and b"unknown phase" in err()
    for phase in (0, 1):
        assert _sample(some, 1, 8, phase=phase, step=0) == INVALID and b"null step word" in err()
        assert _sample(some, 0, 8, phase=phase, step=0) == INVALID                       # (refused before the test for an empty table)
        assert _sample(null, 0, 8, phase=phase) == 0 and _sample(some, 0, 8, phase=phase) == 0 and _sample(some, 3, 0, phase=phase) == 0  # nothing to do
    with pytest.raises(ValueError):
        L.check(_sample(null, 1, 8), "wdg_neighbor_sample_batched")


def _check(tab):
    import wdg_amd._lib as L
    host = np.ascontiguousarray(tab)
    return L.lib.wdg_neighbor_sample_check_jobs(ctypes.c_void_p(host.ctypes.data), len(host))


def _table():
    """a well-formed forward job and its transposed job over made-up addresses (the predicate reads the records, never the memory)"""
    from wdg_amd import neighbor_sample as S
    tab = np.zeros(2, S._NEIGHBOR_SAMPLE_JOB_DTYPE)
    for k, name in enumerate(("rowptr", "col", "kept_col", "kept_len", "scale", "tau")):
        tab[name] = 0x100000 * (k + 1)
    tab["scale"][1] = 0
    tab["n"], tab["n_cols"], tab["nnz"], tab["stream"], tab["flags"], tab["fanout"] = [10, 12], [12, 10], [40, 40], [3, 0xFFFFFFFF], [4 | 8, 2 | 4 | 8], [25, 0]
    return tab


def test_check_jobs_on_damaged_tables():
    import wdg_amd._lib as L
    f = L.lib.wdg_neighbor_sample_check_jobs
    assert _check(_table()) == 0
    assert f(None, 0) == 0 and f(None, 1) == INVALID and f(None, -1) == INVALID
    big = np.zeros(65536, _table().dtype)
    assert f(ctypes.c_void_p(big.ctypes.data), 65536) == INVALID and b"65535" in L.lib.wdg_last_error()
    damage = [("n", -1), ("n_cols", -1), ("nnz", -1), ("flags", 1), ("flags", 4 | 1), ("flags", 16), ("flags", -2), ("fanout", 0), ("fanout", 65), ("fanout", -3),
              ("rowptr", 0), ("col", 0), ("kept_col", 0), ("kept_len", 0), ("tau", 0),
              ("kept_col", 0x200000), ("kept_col", 0x200000 + 4 * 39), ("kept_col", 0x200000 - 4 * 39)]  # (the last three: kept_col inside col's bytes)
    for field, value in damage:
        tab = _table()
        tab[field][0] = value
        assert _check(tab) == INVALID, (field, value)
        assert L.lib.wdg_last_error().startswith(b"neighbor_sample_check_jobs: "), (field, L.lib.wdg_last_error())
    tab = _table()
    tab["flags"][0] = 1
    assert _check(tab) == INVALID and b"no tied form" in L.lib.wdg_last_error()
    for value in (1, 64):
        tab = _table()
        tab["fanout"][0] = value
        assert _check(tab) == 0
    for value in (0, 65, -9):                                                               # a transposed job's fan-out is not read
        tab = _table()
        tab["fanout"][1] = value
        assert _check(tab) == 0
    for field, value in (("flags", 2 | 1), ("flags", 2 | 16), ("tau", 0), ("kept_col", 0x200000), ("rowptr", 0)):   # ... its other fields are
        tab = _table()
        tab[field][1] = value
        assert _check(tab) == INVALID, (field, value)
    tab = _table()
    tab["kept_col"][0] = 0x200000 + 4 * 40                                                  # ... right behind col: no overlap
    assert _check(tab) == 0
    tab = _table()
    for field in ("n", "rowptr", "kept_len", "col", "kept_col", "tau"):                    # an empty job needs no memory
        tab[field][0] = 0
    assert _check(tab) == 0
    tab = _table()
    tab["nnz"], tab["col"], tab["kept_col"] = 0, 0, 0                                       # a pattern without entries needs no columns
    tab["tau"][1] = 0                                                                       # ... and its transposed job no thresholds
    assert _check(tab) == 0
    tab["tau"][0] = 0                                                                       # (the forward job still writes them)
    assert _check(tab) == INVALID


def _graph(n=6, n_cols=None, nnz=12):
    """a CsrGraph over HOST tensors: it passes every check that needs no device"""
    from wdg_amd import ops
    return ops.CsrGraph(torch.zeros(n + 1, dtype=torch.int32), torch.zeros(nnz, dtype=torch.int32), None, n, n if n_cols is None else n_cols)


def test_the_table_refuses_before_it_asks_for_a_device():
    from wdg_amd import ops
    B, g = ops.NeighborSampleBatch, _graph()
    for fanout in (0, 65, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="fan-out of 1 .. 64"):
            B([dict(graph=g)], fanout, 0)
    with pytest.raises(ValueError, match="entry 0: a fan-out of 1 .. 64"):
        B([dict(graph=g, fanout=65)], 5, 0)
    with pytest.raises(ValueError, match="seed of 32 bits"):
        B([dict(graph=g)], 5, 1 << 32)
    with pytest.raises(ValueError, match="65536 jobs .two per entry.; one launch takes 65535"):
        B([None] * 32768, 5, 0)
    with pytest.raises(ValueError, match="unknown keys .'tied'."):  # there is no tied form
        B([dict(graph=g, tied=True)], 5, 0)
    with pytest.raises(ValueError, match="a dict with `graph`"):
        B([dict(stream=1)], 5, 0)
    with pytest.raises(TypeError, match="CsrGraph"):
        B([dict(graph=torch.zeros(3, 3))], 5, 0)
    with pytest.raises(ValueError, match="not the transpose"):
        B([dict(graph=g, graph_t=_graph(nnz=11))], 5, 0)
    with pytest.raises(ValueError, match="stream of 32 bits"):
        B([dict(graph=g, stream=-1)], 5, 0)
    with pytest.raises(ValueError, match="norm must be"):
        B([dict(graph=g, norm=2)], 5, 0)
    if not torch.cuda.is_available():  # a well-formed entry passes every host-side check: what stops it is the missing device
        for entries in ([dict(graph=_graph(6, 7), graph_t=_graph(7, 6), keep_diagonal=True, norm=ops.NORM_SYM, stream=9, fanout=64)], []):
            with pytest.raises(Exception, match="no HIP device"):
                B(entries, 25, 0)


def test_neighbor_sample_adj_argument_checks_need_no_device():
    from wdg_amd import models
    a = torch.eye(3)
    for fanout in (0, 65, 1.5):
        with pytest.raises(ValueError, match="NeighborSampleAdj: a fan-out of 1 .. 64"):
            models.NeighborSampleAdj(a, fanout, 0)
    with pytest.raises(ValueError, match="NeighborSampleAdj: a seed and a stream of 32 bits"):
        models.NeighborSampleAdj(a, 5, 1 << 32)
    with pytest.raises(ValueError, match="NeighborSampleAdj: a seed and a stream of 32 bits"):
        models.NeighborSampleAdj(a, 5, 0, stream=-1)
    assert issubclass(models.NeighborSampleAdj, models._ResampledAdj) and issubclass(models.DropEdgeAdj, models._ResampledAdj)  # one machinery
    assert models.NeighborSampleAdj.resample is models.DropEdgeAdj.resample and models.NeighborSampleAdj._product is models.DropEdgeAdj._product
    torch.manual_seed(0)
    m1, m2 = models.SAGE1(10, 3), models.SAGE2(10, 3, nhid=8)
    assert tuple(m1.w.shape) == (10, 6) and tuple(m2.w0.shape) == (10, 16) and tuple(m2.w1.shape) == (8, 6)
    assert [n for n, _ in m2.named_parameters()] == ["w0", "w1"] and m2.dropout_rng is None  # bias-free


def test_header_and_source_state_what_they_owe():
    header = open(os.path.join(ROOT, "include", "wdg.h")).read()
    for name in ("wdg_neighbor_sample_batched", "wdg_neighbor_sample_check_jobs"):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n|typedef struct (wdg_\w+) \{.*?\} \2;\s*)*int " + name + r"\(", header, re.S)
        assert m and re.search(r"replaces:.*?[\w/]+\.py:\d+", m.group(1), re.S), name
        assert "utils/util_funcs.py:29-36" in m.group(1) and "365-380" in m.group(1), name
    for said in ("{*step_dev, jobs[j].stream, 0, 0}", "{seed, 0x53414745}", "{fi, fj, 0, 0}", "<< 32 | (uint32_t) fj", "fanout-th smallest", "2^64 - 1",
                 "key <= tau[fi]", "goes to the lower column", "no tied form", "left untouched", "no atomics", "HOST", "gnns_on_syn.py:9-53",
                 "NO multi-wave path", "NOT bounded", "a pure function of (pattern, fanout, flags, seed, stream, step)"):
        assert said in header, said
    source = open(os.path.join(ROOT, "when-do-gnns-help_amd", "csrc", "neighbor_sample.hip")).read()
    assert "replaces:" in source and "utils/util_funcs.py:29-36" in source and "utils/util_funcs.py:365-380" in source and "gnns_on_syn.py:9-53" in source
    assert '#include "philox.h"' in source and "0x53414745u" in source
    code = re.sub(r"//[^\n]*", "", source)
    assert '#include "wave_rows.h"' in code and "topk_rows" not in code  # (the row helpers shared, the candidate set restated)
    shared = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "when-do-gnns-help_amd", "csrc", "wave_rows.h")).read())  # the helpers the unit takes from there
    for text in (code, shared):
        assert "atomic" not in text.lower() and "__shared__" not in text  # (no atomics, no LDS)
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^LAST\s*\+=\s*\$\(CSRC\)/neighbor_sample\.hip$", make, re.M)
    assert make.index("neighbor_sample.hip") > make.index("drop_edge.hip") and make.index("LAST     +=") < make.index("SRCS     := $(filter-out")
