"""CPU-only checks of the boundary of the neighbour-moments kernels (csrc/neighbor_moments.hip): the ctypes mirrors of
wdg_neighbor_moments_job and wdg_neighbor_moments_backward_job against the layout gcc gives the header's, the front end's record types
against the mirrors, every refusal include/wdg.h lists - through ctypes, with a NULL stream and no device -, the host predicates on damaged
tables, the refusals of ops.NeighborMomentsBatch / ops.NeighborMomentsBackwardBatch / ops.neighbor_moments that come before they ask for
a device, the models' parameters, and the statements the header, the sources and the Makefile owe."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
FWD_FIELDS = ["rowptr", "col", "kept_len", "X", "mean", "std", "mx", "mn", "arg_max", "arg_min", "cnt", "ldx", "ld_mean", "ld_std", "ld_mx", "ld_mn", "ld_amax",
              "ld_amin", "n_rows", "n_cols", "n_feat", "nnz", "eps", "flags", "reserved", "reserved2"]
BWD_FIELDS = ["rowptr", "col", "kept_len", "X", "g_mean", "g_std", "g_max", "g_min", "mean", "std", "arg_max", "arg_min", "cnt", "A", "B", "D", "ldx", "ld_gmean",
              "ld_gstd", "ld_gmax", "ld_gmin", "ld_mean", "ld_std", "ld_amax", "ld_amin", "ldw", "ldd", "n_rows", "n_src", "n_feat", "nnz", "flags", "reserved"]
ENTRIES = ("wdg_neighbor_moments_batched_f32", "wdg_neighbor_moments_backward_batched_f32")
PREDICATES = ("wdg_neighbor_moments_check_jobs", "wdg_neighbor_moments_backward_check_jobs")


def test_struct_layouts_match_the_header(tmp_path):
    """size and field offsets as gcc lays them out == the ctypes mirrors == the numpy records of the front end"""
    import wdg_amd._lib as L
    from wdg_amd import neighbor_moments as M
    structs = [("wdg_neighbor_moments_job", L.NeighborMomentsJob, M._NEIGHBOR_MOMENTS_JOB_DTYPE, FWD_FIELDS),
               ("wdg_neighbor_moments_backward_job", L.NeighborMomentsBackwardJob, M._NEIGHBOR_MOMENTS_BACKWARD_JOB_DTYPE, BWD_FIELDS)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {']
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
    for cname, mirror, dtype, _ in structs:
        assert got[(cname, "size")][0] == ctypes.sizeof(mirror) == dtype.itemsize, cname
        for fname, ctype in mirror._fields_:
            assert got[(cname, fname)][0] == getattr(mirror, fname).offset == dtype.fields[fname][1], (cname, fname)
            assert got[(cname, fname)][1] == ctypes.sizeof(ctype) == dtype.fields[fname][0].itemsize, (cname, fname)
    assert dtype.fields["reserved"][0] == np.int32 and M._NEIGHBOR_MOMENTS_JOB_DTYPE.fields["eps"][0] == np.float32
    assert M.NeighborMomentsBatch.MAX_JOBS == M.NeighborMomentsBackwardBatch.MAX_JOBS == 65535


@pytest.mark.parametrize("entry", ENTRIES)
def test_launch_refusals_need_no_gpu(entry):
    import wdg_amd._lib as L
    backward = entry.endswith("backward_batched_f32")
    counts = lambda rows, feat: (rows, 8, feat) if backward else (rows, feat)  # noqa: E731  (max_rows, [max_src,] max_feat)
    f = lambda table, n_jobs, max_rows, max_feat: getattr(L.lib, entry)(table, n_jobs, *counts(max_rows, max_feat), ctypes.c_void_p(0))  # noqa: E731
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    err = L.lib.wdg_last_error
    assert f(null, 1, 8, 8) == INVALID and b"null job table" in err()
    assert f(some, -1, 8, 8) == INVALID and b"negative count" in err()
    assert f(some, 1, -1, 8) == INVALID and b"negative count" in err()
    assert f(some, 1, 8, -1) == INVALID and b"negative count" in err()
    if backward:
        assert L.lib.wdg_neighbor_moments_backward_batched_f32(some, 1, 8, -1, 8, ctypes.c_void_p(0)) == INVALID and b"negative count" in err()
    assert f(some, 65536, 8, 8) == INVALID and b"65535" in err()
    assert f(some, 1, 8, 256 * 65535 + 1) == INVALID and b"columns" in err()
    assert err().startswith(entry[4:-4].encode() + b": ")
    assert f(null, 0, 8, 8) == 0 and f(some, 0, 8, 8) == 0 and f(some, 1, 8, 0) == 0  # nothing to do
    if not backward:
        assert f(some, 1, 0, 8) == 0
    else:
        assert L.lib.wdg_neighbor_moments_backward_batched_f32(some, 1, 0, 0, 8, ctypes.c_void_p(0)) == 0
    with pytest.raises(ValueError):
        L.check(f(null, 1, 8, 8), entry)


def _check(name, tab):
    import wdg_amd._lib as L
    host = np.ascontiguousarray(tab)
    return getattr(L.lib, name)(ctypes.c_void_p(host.ctypes.data), len(host))


def _table(backward):
    """two well-formed jobs over made-up addresses (the predicate reads the records, never the memory behind them)"""
    from wdg_amd import neighbor_moments as M
    tab = np.zeros(2, M._NEIGHBOR_MOMENTS_BACKWARD_JOB_DTYPE if backward else M._NEIGHBOR_MOMENTS_JOB_DTYPE)
    pointers = [n for n in tab.dtype.names if tab.dtype.fields[n][0] == np.uint64]
    for k, name in enumerate(pointers):
        tab[name] = 0x100000 * (k + 1)
    tab["kept_len"][1] = 0  # a plain pattern
    tab["n_rows"], tab["n_feat"], tab["nnz"] = [10, 7], [64, 5], [40, 30]
    tab["n_src" if backward else "n_cols"] = [10, 12]
    for ld in (n for n in tab.dtype.names if n.startswith("ld")):
        tab[ld] = [64, 9]
    if not backward:
        tab["eps"] = [1e-5, 0.0]
        for name, ld in (("arg_max", "ld_amax"), ("arg_min", "ld_amin"), ("std", "ld_std")):  # evaluation without the deviation
            tab[name][1], tab[ld][1] = 0, 0
    else:
        for name, ld in (("g_std", "ld_gstd"), ("g_max", "ld_gmax")):  # gradients that are not there read as +0
            tab[name][1], tab[ld][1] = 0, 0
    return tab


@pytest.mark.parametrize("backward", [False, True])
def test_check_jobs_on_damaged_tables(backward):
    import wdg_amd._lib as L
    name = PREDICATES[backward]
    f = getattr(L.lib, name)
    good = _table(backward)
    assert _check(name, good) == 0
    assert f(None, 0) == 0 and f(None, 1) == INVALID and f(None, -1) == INVALID
    big = np.zeros(65536, good.dtype)
    assert f(ctypes.c_void_p(big.ctypes.data), 65536) == INVALID
    damage = [("n_rows", -1), ("n_src" if backward else "n_cols", -1), ("n_feat", -1), ("nnz", -1), ("reserved", 1), ("flags", 1), ("flags", -1), ("rowptr", 0),
              ("cnt", 0), ("col", 0), ("X", 0)]
    damage += [(ld, 63) for ld in good.dtype.names if ld.startswith("ld")]
    if backward:
        damage += [("D", 0), ("A", 0), ("B", 0), ("mean", 0), ("std", 0), ("arg_max", 0), ("arg_min", 0), ("D", good["X"][0]), ("D", good["g_min"][0]),
                   ("A", good["B"][0]), ("B", good["std"][0])]
    else:
        damage += [("reserved2", 1), ("eps", -1e-5), ("eps", np.inf), ("eps", np.nan), ("mean", good["X"][0]), ("mn", good["mx"][0]), ("cnt", good["arg_min"][0])]
    for field, value in damage:
        tab = _table(backward)
        tab[field][0] = value
        assert _check(name, tab) == INVALID, (field, value)
        assert L.lib.wdg_last_error().startswith(name[4:].encode() + b": "), (field, L.lib.wdg_last_error())
    for empty in ("n_rows", "n_feat"):  # an empty job needs no memory
        tab = _table(backward)
        tab[empty][1] = 0
        if backward and empty == "n_rows":
            tab["n_src"][1] = 0
        for field in tab.dtype.names:
            if tab.dtype.fields[field][0] in (np.uint64, np.int64):
                tab[field][1] = 0
        assert _check(name, tab) == 0, empty
    tab = _table(backward)  # a pattern without entries needs no col (and no X to aggregate)
    tab["nnz"][1], tab["col"][1] = 0, 0
    if not backward:
        tab["X"][1] = 0
    assert _check(name, tab) == 0
    if not backward:
        tab = _table(backward)
        tab["ld_std"][1] = 1  # (not read where the result is NULL)
        assert _check(name, tab) == 0


def _graph(n=6, n_cols=None, nnz=12):
    """a CsrGraph over HOST tensors: it passes every check that needs no device"""
    from wdg_amd import ops
    return ops.CsrGraph(torch.zeros(n + 1, dtype=torch.int32), torch.zeros(nnz, dtype=torch.int32), None, n, n if n_cols is None else n_cols)


def test_the_tables_refuse_before_they_ask_for_a_device():
    from wdg_amd import ops
    F, B, g = ops.NeighborMomentsBatch, ops.NeighborMomentsBackwardBatch, _graph()
    pat = ops.ThinnedPattern(torch.zeros(7, dtype=torch.int32), torch.zeros(12, dtype=torch.int32), torch.zeros(6, dtype=torch.int32), None, 6, 6)
    host, cnt = torch.zeros(6, 4), torch.zeros(6, dtype=torch.int32)
    for T in (F, B):
        with pytest.raises(ValueError, match="65536 entries; one launch takes 65535"):
            T([None] * 65536)
    with pytest.raises(ValueError, match="a dict with pattern, x, cnt"):
        F([dict(pattern=g, x=host)])
    with pytest.raises(ValueError, match="a dict with pattern, x, cnt"):
        F([dict(pattern=g, x=host, cnt=cnt, var=host)])
    with pytest.raises(ValueError, match="a dict with pattern, x, d, cnt"):
        B([dict(pattern=g, x=host, d=host)])
    for p in (torch.zeros(3, 3), None):
        with pytest.raises(TypeError, match="CsrGraph or a ThinnedPattern"):
            F([dict(pattern=p, x=host, cnt=cnt)])
        with pytest.raises(TypeError, match="CsrGraph or a ThinnedPattern"):
            B([dict(pattern=p, x=host, d=host, cnt=cnt)])
    for p in (g, pat):  # (_check_matrix: a host tensor, a wrong dtype, a wrong shape)
        with pytest.raises(ValueError, match=r"x must be a \[6, any\] fp32 device matrix"):
            F([dict(pattern=p, x=host, cnt=cnt)])
        with pytest.raises(ValueError, match=r"x must be a \[6, any\] fp32 device matrix"):
            B([dict(pattern=p, x=host, d=host, cnt=cnt)])
    with pytest.raises(ValueError, match=r"x must be a \[6, any\] fp32 device matrix"):
        ops.neighbor_moments(g, host)
    if not torch.cuda.is_available():  # an empty table passes every host-side check: what stops it is the missing device
        for T in (F, B):
            with pytest.raises(Exception, match="no HIP device"):
                T([])


def test_eps_and_delta_are_checked():
    from wdg_amd import models
    from wdg_amd.neighbor_moments import _check_eps
    assert _check_eps("t", 0) == 0.0 and _check_eps("t", 1e-5) == 1e-5
    for bad in (-1e-9, float("inf"), float("nan"), None, True, "1"):
        with pytest.raises(ValueError, match="eps must be a finite number >= 0"):
            _check_eps("t", bad)
    for bad in (0, -1.0, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="delta must be a finite number > 0"):
            models.PNA1(5, 3, bad)


def test_the_adjacencies_and_models_are_there():
    from wdg_amd import models
    for cls in (models.NormAdj, models._ThinnedAdj):
        assert callable(cls.neighbor_moments)
    assert callable(models.pna_delta)
    m1, m2 = models.PNA1(5, 3, 1.5, nagg=8), models.PNA2(5, 3, 1.5, nhid=6, nagg=8)
    assert [tuple(p.shape) for p in m1.parameters()] == [(5, 8), (5, 3), (32, 9)]  # w_pre, w_self, w_post: bias-free
    assert [tuple(p.shape) for p in m2.parameters()] == [(5, 8), (5, 6), (32, 18), (6, 8), (6, 3), (32, 9)]
    torch.manual_seed(3)
    a = models.PNA1(5, 3, 1.5, nagg=8)
    torch.manual_seed(3)
    draws = [models._xavier(5, 8), models._xavier(5, 3), models._xavier(32, 9)]  # the stated order
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), draws))
    view = models._ThinnedAdj.__new__(models._ThinnedAdj)
    with pytest.raises(TypeError, match="aggregate through neighbor_moments - PNA1 / PNA2"):
        view.graph


def test_header_source_and_makefile_state_what_they_owe():
    header = open(os.path.join(ROOT, "include", "wdg.h")).read()
    for name in ENTRIES + PREDICATES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n|typedef struct (wdg_\w+) \{.*?\} \2;\s*)*int " + name + r"\(", header, re.S)
        assert m and re.search(r"replaces:.*?[\w/]+\.py:\d+", m.group(1), re.S), name
        assert "utils/util_funcs.py:29-36" in m.group(1) and "365-380" in m.group(1), name
    for said in ("DEFINED here (DESIGN 4.37)", "FOUR CHAINS BY POSITION", "e % 4 == k", "s1 = (c0 + c1) + (c2 + c3)", "acc = fmaf(d, d, acc)", "sqrtf(var + eps)",
                 "s1 / (float)c", "EXACTLY the Y and arg of wdg_neighbor_max_batched_f32", "count per occurrence", "mean = std = mx = mn = +0",
                 "left untouched", "a column the same bits at any job width", "its payload is not\n *                part of the contract",
                 "B = g_std[i, f] / ((float)c * std[i, f])", "A = fmaf(-B, mean[i, f], g_mean[i, f] / (float)c)", "D[j, f] = fmaf(X[j, f], SB, (SA + RM) + Rm)",
                 "routes nothing", "May any two operands alias?  None", "NO multi-wave path", "No LDS, no atomics", "HOST", "gnns_on_syn.py:9-53"):
        assert said in header, said
    csrc = os.path.join(ROOT, "when-do-gnns-help_amd", "csrc")
    source = open(os.path.join(csrc, "neighbor_moments.hip")).read()
    assert "replaces:" in source and "utils/util_funcs.py:29-36" in source and "utils/util_funcs.py:365-380" in source and "gnns_on_syn.py:9-53" in source
    assert "#pragma clang fp contract(off)" in source
    code = re.sub(r"//[^\n]*", "", source)
    order = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "neighbor_order.h")).read())
    assert '#include "wave_rows.h"' in code and '#include "neighbor_order.h"' in code
    assert '#include "neighbor_order.h"' in re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "neighbor_max.hip")).read())  # the order is stated once
    assert "nm_key" in order and code.count("uint32_t nm_key(") == 0
    for text in (code, order):
        assert "atomic" not in text.lower() and "__shared__" not in text  # (no atomics, no LDS)
    assert "fmaf" not in order and "float" not in order  # integer work only: the header means the same in any unit
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "FLAGS_neighbor_moments := -ffp-contract=off" in make
    assert re.findall(r"^AFTER\s*\+=\s*(.*)$", make, re.M) == ["$(CSRC)/neighbor_moments.hip"]  # on a line of its own, behind everything else
    rsrc = os.path.join(ROOT, "build", "neighbor_moments.rsrc")
    if os.path.exists(rsrc):  # (tests/test_abi.py reads every unit's report for spills; scratch is checked here)
        report = open(rsrc).read()
        assert report.count("Function Name") == 3 and set(re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", report)) == {"0"}
        assert set(re.findall(r"VGPRs Spill: (\d+)", report)) == {"0"}
