"""CPU-only checks of the boundary of the DropEdge kernels (csrc/drop_edge.hip): the ctypes mirrors of wdg_drop_edge_job and
wdg_thinned_spmm_job against the layout gcc gives the header's, the front end's record types against the mirrors, every refusal
include/wdg.h lists - through ctypes, with a NULL stream and no device -, the host predicates on damaged tables, the refusals of
ops.DropEdgeBatch / ops.ThinnedSpmmBatch and of models.DropEdgeAdj that come before they ask for a device, and the statements the header
and the source owe (a `replaces:` line with a citation, contraction off)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
THIN_FIELDS = ["rowptr", "col", "kept_col", "kept_len", "scale", "n", "n_cols", "nnz", "stream", "flags", "reserved"]
SPMM_FIELDS = ["rowptr", "kept_col", "kept_len", "row_scale", "col_scale", "X", "Y", "ldx", "ldy", "n_rows", "n_cols", "n_feat", "nnz", "reserved"]


def test_struct_layouts_match_the_header(tmp_path):
    """size and field offsets as gcc lays them out == the ctypes mirrors == the numpy records of the front end; the flag values"""
    import wdg_amd._lib as L
    from wdg_amd import drop_edge as D
    structs = [("wdg_drop_edge_job", L.DropEdgeJob, D._DROP_EDGE_JOB_DTYPE, THIN_FIELDS), ("wdg_thinned_spmm_job", L.ThinnedSpmmJob, D._THINNED_SPMM_JOB_DTYPE, SPMM_FIELDS)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {',
             'printf("flags x %d %d %d %d\\n", WDG_DROP_EDGE_TIED, WDG_DROP_EDGE_TRANSPOSED, WDG_DROP_EDGE_KEEP_DIAGONAL, WDG_DROP_EDGE_NORM_SYM);']
    for cname, mirror, dtype, fields in structs:
        assert [f for f, _ in mirror._fields_] == fields == list(dtype.names)
        lines.append(f'printf("{cname} size %zu 0\\n", sizeof({cname}));')
        for fname in fields:
            lines.append(f'printf("{cname} {fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname} *)0)->{fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {tuple(line.split()[:2]): [int(v) for v in line.split()[2:]] for line in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got[("flags", "x")] == [D.DROP_EDGE_TIED, D.DROP_EDGE_TRANSPOSED, D.DROP_EDGE_KEEP_DIAGONAL, D.DROP_EDGE_NORM_SYM] == [1, 2, 4, 8]
    for cname, mirror, dtype, _ in structs:
        assert got[(cname, "size")][0] == ctypes.sizeof(mirror) == dtype.itemsize, cname
        for fname, ctype in mirror._fields_:
            assert got[(cname, fname)][0] == getattr(mirror, fname).offset == dtype.fields[fname][1], (cname, fname)
            assert got[(cname, fname)][1] == ctypes.sizeof(ctype) == dtype.fields[fname][0].itemsize, (cname, fname)
    assert D._DROP_EDGE_JOB_DTYPE.fields["stream"][0] == np.uint32 and D.DropEdgeBatch.MAX_JOBS == D.ThinnedSpmmBatch.MAX_JOBS == 65535


def _thin(table, n_jobs, max_rows, step=4096):
    import wdg_amd._lib as L
    return L.lib.wdg_drop_edge_thin_batched(table, n_jobs, max_rows, 1 << 31, 7, ctypes.c_void_p(step), ctypes.c_void_p(0))


def _spmm(table, n_jobs, max_rows, max_feat):
    import wdg_amd._lib as L
    return L.lib.wdg_spmm_thinned_batched_f32(table, n_jobs, max_rows, max_feat, ctypes.c_void_p(0))


def test_launch_refusals_need_no_gpu():
    import wdg_amd._lib as L
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    err = L.lib.wdg_last_error
    assert _thin(null, 1, 8) == INVALID and b"null job table" in err()
    assert _thin(some, -1, 8) == INVALID and b"negative count" in err()
    assert _thin(some, 1, -1) == INVALID and b"negative count" in err()
    assert _thin(some, 65536, 8) == INVALID and b"65535" in err()
    assert _thin(some, 1, 8, step=0) == INVALID and b"null step word" in err()
    assert _thin(some, 0, 8, step=0) == INVALID                                       # (refused before the test for an empty table)
    assert _thin(null, 0, 8) == 0 and _thin(some, 0, 8) == 0 and _thin(some, 3, 0) == 0  # nothing to do
    assert _spmm(null, 1, 8, 8) == INVALID and b"null job table" in err()
    assert _spmm(some, -1, 8, 8) == INVALID and _spmm(some, 1, -1, 8) == INVALID and _spmm(some, 1, 8, -1) == INVALID and b"negative count" in err()
    assert _spmm(some, 65536, 8, 8) == INVALID and b"65535" in err()
    assert _spmm(some, 1, 8, 256 * 65535 + 1) == INVALID and b"columns" in err()
    assert _spmm(null, 0, 8, 8) == 0 and _spmm(some, 0, 8, 8) == 0 and _spmm(some, 1, 0, 8) == 0 and _spmm(some, 1, 8, 0) == 0
    with pytest.raises(ValueError):
        L.check(_thin(null, 1, 8), "wdg_drop_edge_thin_batched")


def _check(name, tab):
    import wdg_amd._lib as L
    host = np.ascontiguousarray(tab)
    return getattr(L.lib, name)(ctypes.c_void_p(host.ctypes.data), len(host))


def _thin_table():
    """two well-formed jobs over made-up addresses (the predicate reads the records, never the memory behind them)"""
    from wdg_amd import drop_edge as D
    tab = np.zeros(2, D._DROP_EDGE_JOB_DTYPE)
    for k, name in enumerate(("rowptr", "col", "kept_col", "kept_len", "scale")):
        tab[name] = 0x100000 * (k + 1)
    tab["scale"][1] = 0
    tab["n"], tab["n_cols"], tab["nnz"], tab["stream"], tab["flags"] = [10, 7], [10, 12], [40, 30], [3, 0xFFFFFFFF], [1 | 4 | 8, 2]
    return tab


def test_drop_edge_check_jobs_on_damaged_tables():
    import wdg_amd._lib as L
    f, name = L.lib.wdg_drop_edge_check_jobs, "wdg_drop_edge_check_jobs"
    assert _check(name, _thin_table()) == 0
    assert f(None, 0) == 0 and f(None, 1) == INVALID and f(None, -1) == INVALID
    big = np.zeros(65536, _thin_table().dtype)
    assert f(ctypes.c_void_p(big.ctypes.data), 65536) == INVALID
    damage = [("n", -1), ("n_cols", -1), ("nnz", -1), ("flags", 16), ("flags", -1), ("reserved", 1), ("rowptr", 0), ("col", 0), ("kept_col", 0), ("kept_len", 0),
              ("kept_col", 0x200000), ("kept_col", 0x200000 + 4 * 39), ("kept_col", 0x200000 - 4 * 39)]  # (the last three: kept_col inside col's bytes)
    for field, value in damage:
        tab = _thin_table()
        tab[field][0] = value
        assert _check(name, tab) == INVALID, (field, value)
        assert L.lib.wdg_last_error().startswith(b"drop_edge_check_jobs: "), (field, L.lib.wdg_last_error())
    tab = _thin_table()
    tab["kept_col"][0] = 0x200000 + 4 * 40                                                # ... right behind col: no overlap
    assert _check(name, tab) == 0
    tab = _thin_table()
    tab["n"][1], tab["rowptr"][1], tab["kept_len"][1], tab["col"][1], tab["kept_col"][1] = 0, 0, 0, 0, 0  # an empty job needs no memory
    assert _check(name, tab) == 0
    tab = _thin_table()
    tab["nnz"][1], tab["col"][1], tab["kept_col"][1] = 0, 0, 0                            # a pattern without entries needs no columns
    assert _check(name, tab) == 0


def _spmm_table():
    from wdg_amd import drop_edge as D
    tab = np.zeros(2, D._THINNED_SPMM_JOB_DTYPE)
    for k, name in enumerate(("rowptr", "kept_col", "kept_len", "row_scale", "col_scale", "X", "Y")):
        tab[name] = 0x100000 * (k + 1)
    tab["row_scale"][1], tab["col_scale"][1] = 0, 0
    tab["n_rows"], tab["n_cols"], tab["n_feat"], tab["nnz"], tab["ldx"], tab["ldy"] = [10, 7], [10, 12], [64, 5], [40, 30], [64, 9], [80, 5]
    return tab


def test_spmm_thinned_check_jobs_on_damaged_tables():
    import wdg_amd._lib as L
    f, name = L.lib.wdg_spmm_thinned_check_jobs, "wdg_spmm_thinned_check_jobs"
    assert _check(name, _spmm_table()) == 0
    assert f(None, 0) == 0 and f(None, 1) == INVALID and f(None, -1) == INVALID
    big = np.zeros(65536, _spmm_table().dtype)
    assert f(ctypes.c_void_p(big.ctypes.data), 65536) == INVALID
    for field, value in [("n_rows", -1), ("n_cols", -1), ("n_feat", -1), ("nnz", -1), ("reserved", 1), ("ldx", 63), ("ldy", 63), ("rowptr", 0), ("kept_len", 0),
                         ("Y", 0), ("kept_col", 0), ("X", 0), ("Y", 0x600000)]:
        tab = _spmm_table()
        tab[field][0] = value
        assert _check(name, tab) == INVALID, (field, value)
        assert L.lib.wdg_last_error().startswith(b"spmm_thinned_check_jobs: "), (field, L.lib.wdg_last_error())
    for empty in ("n_rows", "n_feat"):                                                    # an empty job needs no memory
        tab = _spmm_table()
        tab[empty][1] = 0
        for field in ("rowptr", "kept_col", "kept_len", "X", "Y", "ldx", "ldy"):
            tab[field][1] = 0
        assert _check(name, tab) == 0, empty


def _graph(n=6, n_cols=None, nnz=12):
    """a CsrGraph over HOST tensors: it passes every check that needs no device"""
    from wdg_amd import ops
    return ops.CsrGraph(torch.zeros(n + 1, dtype=torch.int32), torch.zeros(nnz, dtype=torch.int32), None, n, n if n_cols is None else n_cols)


def test_the_tables_refuse_before_they_ask_for_a_device():
    from wdg_amd import ops
    B, g = ops.DropEdgeBatch, _graph()
    with pytest.raises(ValueError, match=r"drop probability in \[0, 1\)"):
        B([dict(graph=g)], 1.0, 0)
    with pytest.raises(ValueError, match="seed of 32 bits"):
        B([dict(graph=g)], 0.5, 1 << 32)
    with pytest.raises(ValueError, match="65536 jobs .two per entry.; one launch takes 65535"):
        B([None] * 32768, 0.5, 0)
    with pytest.raises(ValueError, match="unknown keys"):
        B([dict(graph=g, layerwise=True)], 0.5, 0)
    with pytest.raises(ValueError, match="a dict with `graph`"):
        B([dict(tied=True)], 0.5, 0)
    with pytest.raises(TypeError, match="CsrGraph"):
        B([dict(graph=torch.zeros(3, 3))], 0.5, 0)
    with pytest.raises(ValueError, match="not the transpose"):
        B([dict(graph=g, graph_t=_graph(nnz=11))], 0.5, 0)
    with pytest.raises(ValueError, match="tied needs a square pattern"):
        B([dict(graph=_graph(6, 7), tied=True)], 0.5, 0)
    with pytest.raises(ValueError, match="stream of 32 bits"):
        B([dict(graph=g, stream=-1)], 0.5, 0)
    with pytest.raises(ValueError, match="norm must be"):
        B([dict(graph=g, norm=2)], 0.5, 0)
    if not torch.cuda.is_available():  # a well-formed entry passes every host-side check: what stops it is the missing device
        for entries in ([dict(graph=g, graph_t=_graph(), tied=True, keep_diagonal=True, norm=ops.NORM_SYM, stream=9)], []):
            with pytest.raises(Exception, match="no HIP device"):
                B(entries, 0.5, 0)
    S = ops.ThinnedSpmmBatch
    pat = ops.ThinnedPattern(torch.zeros(7, dtype=torch.int32), torch.zeros(12, dtype=torch.int32), torch.zeros(6, dtype=torch.int32), None, 6, 6)
    with pytest.raises(ValueError, match="65536 entries; one launch takes 65535"):
        S([None] * 65536)
    with pytest.raises(ValueError, match="a dict with pattern, x, y"):
        S([dict(pattern=pat, x=torch.zeros(6, 4))])
    with pytest.raises(TypeError, match="ThinnedPattern"):
        S([dict(pattern=_graph(), x=torch.zeros(6, 4), y=torch.zeros(6, 4))])
    with pytest.raises(ValueError, match=r"x must be a \[6, any\] fp32 device matrix"):  # (_check_matrix: a host tensor, a wrong dtype, a wrong shape)
        S([dict(pattern=pat, x=torch.zeros(6, 4), y=torch.zeros(6, 4))])


def test_drop_edge_adj_argument_checks_need_no_device():
    from wdg_amd import models
    a = torch.eye(3)
    with pytest.raises(ValueError, match=r"drop probability in \[0, 1\)"):
        models.DropEdgeAdj(a, 1.0, 0)
    with pytest.raises(ValueError, match=r"drop probability in \[0, 1\)"):
        models.DropEdgeAdj(a, -0.1, 0)
    with pytest.raises(ValueError, match="32 bits"):
        models.DropEdgeAdj(a, 0.5, 1 << 32)
    with pytest.raises(ValueError, match="32 bits"):
        models.DropEdgeAdj(a, 0.5, 0, stream=-1)
    for name in ("aggregate", "aggregate_t"):  # what the served models call on either kind of adjacency
        assert callable(getattr(models.NormAdj, name)) and callable(getattr(models._ThinnedAdj, name))
    view = models._ThinnedAdj.__new__(models._ThinnedAdj)
    for read in (lambda: view.graph, lambda: view.graph_t, lambda: view.row_scale, lambda: view.col_scale, view.attention_plan):
        with pytest.raises(TypeError, match="GCN2, ACMGCN2, GPRGNN1 / GPRGNN2 with fused=False, GCNII"):
            read()


def test_header_and_source_state_what_they_owe():
    header = open(os.path.join(ROOT, "include", "wdg.h")).read()
    for name in ("wdg_drop_edge_thin_batched", "wdg_drop_edge_check_jobs", "wdg_spmm_thinned_batched_f32", "wdg_spmm_thinned_check_jobs"):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n|typedef struct (wdg_\w+) \{.*?\} \2;\s*)*int " + name + r"\(", header, re.S)
        assert m and re.search(r"replaces:.*?[\w/]+\.py:\d+", m.group(1), re.S), name
        assert "utils/util_funcs.py:29-36" in m.group(1) and "365-380" in m.group(1), name
    for said in ("{*step_dev, jobs[j].stream, 0, 0}", "{seed, 0x45444745}", "{a, b, 0, 0}", "(min, max)", "is >= drop_threshold", "1.0f / sqrtf((float)c)",
                 "fmaf(col_scale ? col_scale[j] : 1.0f, X[j, f], acc)", "left untouched", "no atomics", "HOST", "gnns_on_syn.py:9-53", "30 steps of one wave"):
        assert said in header, said
    source = open(os.path.join(ROOT, "when-do-gnns-help_amd", "csrc", "drop_edge.hip")).read()
    assert "replaces:" in source and "utils/util_funcs.py:29-36" in source and "utils/util_funcs.py:365-380" in source and "gnns_on_syn.py:9-53" in source
    assert "#pragma clang fp contract(off)" in source and '#include "philox.h"' in source
    code = re.sub(r"//[^\n]*", "", source)
    assert '#include "wave_rows.h"' in code and "gat_lanes.h" not in code  # (the row helpers shared, the chains restated)
    shared = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "when-do-gnns-help_amd", "csrc", "wave_rows.h")).read())  # the helpers the unit takes from there
    assert "gat_lanes.h" not in shared
    for text in (code, shared):
        assert "atomic" not in text.lower() and "__shared__" not in text  # (no atomics, no LDS)
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "FLAGS_drop_edge := -ffp-contract=off" in make and re.search(r"^LAST\s*:=.*gcnii\.hip \$\(CSRC\)/drop_edge\.hip$", make, re.M)
