"""CPU-only checks of the boundary of the neighbour-maximum kernels (csrc/neighbor_max.hip): the ctypes mirrors of wdg_neighbor_max_job
and wdg_neighbor_max_backward_job against the layout gcc gives the header's, the front end's record types against the mirrors, every
refusal include/wdg.h lists - through ctypes, with a NULL stream and no device -, the host predicates on damaged tables, the refusals of
ops.NeighborMaxBatch / ops.NeighborMaxBackwardBatch / ops.neighbor_max that come before they ask for a device, and the statements the
header, the source and the Makefile owe."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
FWD_FIELDS = ["rowptr", "col", "kept_len", "X", "Y", "arg", "ldx", "ldy", "lda", "n_rows", "n_cols", "n_feat", "nnz", "flags", "reserved"]
BWD_FIELDS = ["rowptr", "col", "kept_len", "G", "arg", "D", "ldg", "lda", "ldd", "n_rows", "n_src", "n_feat", "nnz", "reserved", "reserved2"]
ENTRIES = ("wdg_neighbor_max_batched_f32", "wdg_neighbor_max_backward_batched_f32")
PREDICATES = ("wdg_neighbor_max_check_jobs", "wdg_neighbor_max_backward_check_jobs")


def test_struct_layouts_match_the_header(tmp_path):
    """size and field offsets as gcc lays them out == the ctypes mirrors == the numpy records of the front end; the flag value"""
    import wdg_amd._lib as L
    from wdg_amd import neighbor_max as M
    structs = [("wdg_neighbor_max_job", L.NeighborMaxJob, M._NEIGHBOR_MAX_JOB_DTYPE, FWD_FIELDS),
               ("wdg_neighbor_max_backward_job", L.NeighborMaxBackwardJob, M._NEIGHBOR_MAX_BACKWARD_JOB_DTYPE, BWD_FIELDS)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {', 'printf("flags x %d\\n", WDG_NEIGHBOR_MAX_MIN);']
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
    assert got[("flags", "x")] == [M.NEIGHBOR_MAX_MIN] == [1]
    for cname, mirror, dtype, _ in structs:
        assert got[(cname, "size")][0] == ctypes.sizeof(mirror) == dtype.itemsize, cname
        for fname, ctype in mirror._fields_:
            assert got[(cname, fname)][0] == getattr(mirror, fname).offset == dtype.fields[fname][1], (cname, fname)
            assert got[(cname, fname)][1] == ctypes.sizeof(ctype) == dtype.fields[fname][0].itemsize, (cname, fname)
    assert M.NeighborMaxBatch.MAX_JOBS == M.NeighborMaxBackwardBatch.MAX_JOBS == 65535


@pytest.mark.parametrize("entry", ENTRIES)
def test_launch_refusals_need_no_gpu(entry):
    import wdg_amd._lib as L
    f = lambda table, n_jobs, max_rows, max_feat: getattr(L.lib, entry)(table, n_jobs, max_rows, max_feat, ctypes.c_void_p(0))  # noqa: E731
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    err = L.lib.wdg_last_error
    assert f(null, 1, 8, 8) == INVALID and b"null job table" in err()
    assert f(some, -1, 8, 8) == INVALID and b"negative count" in err()
    assert f(some, 1, -1, 8) == INVALID and b"negative count" in err()
    assert f(some, 1, 8, -1) == INVALID and b"negative count" in err()
    assert f(some, 65536, 8, 8) == INVALID and b"65535" in err()
    assert f(some, 1, 8, 256 * 65535 + 1) == INVALID and b"columns" in err()
    assert err().startswith(entry[4:-4].encode() + b": ")
    assert f(null, 0, 8, 8) == 0 and f(some, 0, 8, 8) == 0 and f(some, 1, 0, 8) == 0 and f(some, 1, 8, 0) == 0  # nothing to do
    with pytest.raises(ValueError):
        L.check(f(null, 1, 8, 8), entry)


def _check(name, tab):
    import wdg_amd._lib as L
    host = np.ascontiguousarray(tab)
    return getattr(L.lib, name)(ctypes.c_void_p(host.ctypes.data), len(host))


def _table(backward):
    """two well-formed jobs over made-up addresses (the predicate reads the records, never the memory behind them)"""
    from wdg_amd import neighbor_max as M
    tab = np.zeros(2, M._NEIGHBOR_MAX_BACKWARD_JOB_DTYPE if backward else M._NEIGHBOR_MAX_JOB_DTYPE)
    for k, name in enumerate(tab.dtype.names[:6]):
        tab[name] = 0x100000 * (k + 1)
    tab["kept_len"][1] = 0  # a plain pattern
    tab["n_rows"], tab["n_feat"], tab["nnz"] = [10, 7], [64, 5], [40, 30]
    tab["n_src" if backward else "n_cols"] = [10, 12]
    for ld, values in zip(tab.dtype.names[6:9], ([64, 9], [80, 5], [64, 6])):
        tab[ld] = values
    if not backward:
        tab["flags"], tab["arg"][1], tab["lda"][1] = [1, 0], 0, 0  # evaluation: no arg
    return tab


@pytest.mark.parametrize("backward", [False, True])
def test_check_jobs_on_damaged_tables(backward):
    import wdg_amd._lib as L
    name = PREDICATES[backward]
    f, x, y = getattr(L.lib, name), ("G" if backward else "X"), ("D" if backward else "Y")
    assert _check(name, _table(backward)) == 0
    assert f(None, 0) == 0 and f(None, 1) == INVALID and f(None, -1) == INVALID
    big = np.zeros(65536, _table(backward).dtype)
    assert f(ctypes.c_void_p(big.ctypes.data), 65536) == INVALID
    damage = [("n_rows", -1), ("n_src" if backward else "n_cols", -1), ("n_feat", -1), ("nnz", -1), ("reserved", 1), ("rowptr", 0), (y, 0), ("col", 0), (x, 0)]
    damage += [(ld, 63) for ld in _table(backward).dtype.names[6:9]] + [(y, _table(backward)[x][0])]  # (the last: one matrix read and written)
    damage += [("reserved2", 1), ("arg", 0)] if backward else [("flags", 2), ("flags", -1)]
    for field, value in damage:
        tab = _table(backward)
        tab[field][0] = value
        assert _check(name, tab) == INVALID, (field, value)
        assert L.lib.wdg_last_error().startswith(name[4:].encode() + b": "), (field, L.lib.wdg_last_error())
    for empty in ("n_rows", "n_feat"):  # an empty job needs no memory
        tab = _table(backward)
        tab[empty][1] = 0
        for field in tab.dtype.names[:9]:
            tab[field][1] = 0
        assert _check(name, tab) == 0, empty
    tab = _table(backward)  # a pattern without entries, or with nothing to gather from, needs no col and no sources
    tab["nnz"][1], tab["col"][1], tab[x][1] = 0, 0, 0
    assert _check(name, tab) == 0
    if not backward:
        tab = _table(backward)
        tab["lda"][1] = 1  # (not read where arg is NULL)
        assert _check(name, tab) == 0


def _graph(n=6, n_cols=None, nnz=12):
    """a CsrGraph over HOST tensors: it passes every check that needs no device"""
    from wdg_amd import ops
    return ops.CsrGraph(torch.zeros(n + 1, dtype=torch.int32), torch.zeros(nnz, dtype=torch.int32), None, n, n if n_cols is None else n_cols)


def test_the_tables_refuse_before_they_ask_for_a_device():
    from wdg_amd import ops
    F, B, g = ops.NeighborMaxBatch, ops.NeighborMaxBackwardBatch, _graph()
    pat = ops.ThinnedPattern(torch.zeros(7, dtype=torch.int32), torch.zeros(12, dtype=torch.int32), torch.zeros(6, dtype=torch.int32), None, 6, 6)
    host = torch.zeros(6, 4)
    for T in (F, B):
        with pytest.raises(ValueError, match="65536 entries; one launch takes 65535"):
            T([None] * 65536)
    with pytest.raises(ValueError, match="a dict with pattern, x, y"):
        F([dict(pattern=g, x=host)])
    with pytest.raises(ValueError, match="a dict with pattern, x, y"):
        F([dict(pattern=g, x=host, y=host, maximum=True)])
    with pytest.raises(ValueError, match="a dict with pattern, g, arg and d"):
        B([dict(pattern=g, g=host, d=host)])
    for p in (torch.zeros(3, 3), None):
        with pytest.raises(TypeError, match="CsrGraph or a ThinnedPattern"):
            F([dict(pattern=p, x=host, y=host)])
        with pytest.raises(TypeError, match="CsrGraph or a ThinnedPattern"):
            B([dict(pattern=p, g=host, arg=host, d=host)])
    for p in (g, pat):  # (_check_matrix: a host tensor, a wrong dtype, a wrong shape)
        with pytest.raises(ValueError, match=r"x must be a \[6, any\] fp32 device matrix"):
            F([dict(pattern=p, x=host, y=host)])
        with pytest.raises(ValueError, match=r"g must be a \[6, any\] fp32 device matrix"):
            B([dict(pattern=p, g=host, arg=host, d=host)])
    with pytest.raises(ValueError, match=r"x must be a \[6, any\] fp32 device matrix"):
        ops.neighbor_max(g, host)
    if not torch.cuda.is_available():  # an empty table passes every host-side check: what stops it is the missing device
        for T in (F, B):
            with pytest.raises(Exception, match="no HIP device"):
                T([])


def test_the_adjacencies_and_models_are_there():
    from wdg_amd import models
    for cls in (models.NormAdj, models._ThinnedAdj):
        assert callable(cls.neighbor_max)
    m1, m2 = models.SAGEPool1(5, 3, npool=8), models.SAGEPool2(5, 3, nhid=6, npool=8)
    assert [tuple(p.shape) for p in m1.parameters()] == [(5, 8), (5, 3), (8, 3)]  # w_p, w_s, w_n: bias-free
    assert [tuple(p.shape) for p in m2.parameters()] == [(5, 8), (5, 6), (8, 6), (6, 8), (6, 3), (8, 3)]
    torch.manual_seed(3)
    a = models.SAGEPool1(5, 3, npool=8)
    torch.manual_seed(3)
    draws = [models._xavier(5, 8), models._xavier(5, 3), models._xavier(8, 3)]  # the stated order
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), draws))
    view = models._ThinnedAdj.__new__(models._ThinnedAdj)
    with pytest.raises(TypeError, match="SAGE1 / SAGE2 - or pool through neighbor_max - SAGEPool1 / SAGEPool2"):
        view.graph


def test_header_source_and_makefile_state_what_they_owe():
    header = open(os.path.join(ROOT, "include", "wdg.h")).read()
    for name in ENTRIES + PREDICATES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n|typedef struct (wdg_\w+) \{.*?\} \2;\s*)*int " + name + r"\(", header, re.S)
        assert m and re.search(r"replaces:.*?[\w/]+\.py:\d+", m.group(1), re.S), name
        assert "utils/util_funcs.py:29-36" in m.group(1) and "365-380" in m.group(1), name
    for said in ("a NaN above everything", "-0 == +0", "the LOWER j", "its BITS, copied", "stores +0 and -1", "left untouched", "for any stored order",
                 "with\n * duplicates, alone or in any table, and for a column at any job width", "SHARES of the row's entries", "sixteen entries are in flight",
                 "associative and commutative", "acc = acc + G[i, f]", "the duplicate rule", "MERGES duplicates", "adjacent copies stay adjacent",
                 "counts them per occurrence", "NO multi-wave path", "No LDS, no atomics", "HOST", "gnns_on_syn.py:9-53"):
        assert said in header, said
    source = open(os.path.join(ROOT, "when-do-gnns-help_amd", "csrc", "neighbor_max.hip")).read()
    assert "replaces:" in source and "utils/util_funcs.py:29-36" in source and "utils/util_funcs.py:365-380" in source and "gnns_on_syn.py:9-53" in source
    assert "#pragma clang fp contract(off)" in source
    code = re.sub(r"//[^\n]*", "", source)
    assert '#include "wave_rows.h"' in code
    shared = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "when-do-gnns-help_amd", "csrc", "wave_rows.h")).read())  # the helpers the unit takes from there
    for text in (code, shared):
        assert "atomic" not in text.lower() and "__shared__" not in text and "fmaf" not in text  # (no atomics, no LDS, a plain add chain)
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "FLAGS_neighbor_max := -ffp-contract=off" in make
    last = re.findall(r"^LAST\s*\+=\s*(.*)$", make, re.M)
    assert last == ["$(CSRC)/neighbor_sample.hip", "$(CSRC)/neighbor_max.hip"]  # on a line of its own, behind the sampler
    rsrc = os.path.join(ROOT, "build", "neighbor_max.rsrc")
    if os.path.exists(rsrc):  # (tests/test_abi.py reads every unit's report for spills; scratch is checked here)
        report = open(rsrc).read()
        assert report.count("Function Name") == 2 and set(re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", report)) == {"0"}
