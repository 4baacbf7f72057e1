"""CPU-only checks of the boundary of the two-hop build (csrc/two_hop.hip): the ctypes mirror of wdg_two_hop_job against the layout gcc
gives the header's, the limit and its LDS arithmetic, every refusal include/wdg.h lists - through ctypes and with no device -, and the
front end's own refusals and its reading of the totals, which need no device either."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -4
FIELDS = ["rowptr", "col", "n", "flags", "out_rowptr", "out_col", "total"]
LDS_BYTES, WAVES = 160 * 1024 - 256, 8
LIMIT = LDS_BYTES // (4 * WAVES) * 32


def test_struct_layout_and_limits_match_header(tmp_path):
    import wdg_amd._lib as L
    mirror, cname = L.TwoHopJob, "wdg_two_hop_job"
    assert [f for f, _ in mirror._fields_] == FIELDS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdg.h"', 'int main(void) {', f'printf("size %zu\\n", sizeof({cname}));',
             'printf("limits %d %d %d %d %d\\n", WDG_TWO_HOP_KEEP_ONE_HOP, WDG_TWO_HOP_KEEP_SELF, WDG_TWO_HOP_WAVES, WDG_TWO_HOP_LDS_BYTES, WDG_TWO_HOP_MAX_ROWS);']
    for fname in FIELDS:
        lines.append(f'printf("{fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname} *)0)->{fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got["size"][0] == ctypes.sizeof(mirror) == 48
    assert got["limits"] == [1, 2, WAVES, LDS_BYTES, LIMIT]
    for fname, ctype in mirror._fields_:
        assert got[fname][0] == getattr(mirror, fname).offset, fname
        assert got[fname][1] == ctypes.sizeof(ctype), fname
    from wdg_amd import ops
    assert (ops.TWO_HOP_KEEP_ONE_HOP, ops.TWO_HOP_KEEP_SELF) == (1, 2)
    import _two_hop_ref as ref
    assert (ref.KEEP_ONE_HOP, ref.KEEP_SELF) == (1, 2)


def test_the_limit_is_eight_bitmaps_in_the_lds_budget():
    import wdg_amd._lib as L
    from wdg_amd import ops
    limit = L.lib.wdg_csr_two_hop_max_rows()
    assert limit == LIMIT == 163584 == ops.TwoHopBatch.max_rows() and limit >= 32768
    assert WAVES * 4 * ((limit + 31) // 32) <= LDS_BYTES < WAVES * 4 * ((limit + 32 + 31) // 32)  # one more word per wave does not fit


def _jobs(count=1, **fields):
    """well-formed jobs over made-up addresses (the predicate reads the records, never the memory behind them)"""
    import wdg_amd._lib as L
    jobs = (L.TwoHopJob * count)()
    for j in jobs:
        j.rowptr, j.col, j.out_rowptr, j.out_col, j.total, j.n, j.flags = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 2000, 0
        for k, v in fields.items():
            setattr(j, k, v)
    return jobs


def _check(jobs, count=None):
    import wdg_amd._lib as L
    return L.lib.wdg_csr_two_hop_check_jobs(ctypes.cast(jobs, ctypes.c_void_p), len(jobs) if count is None else count)


def test_check_jobs_refusals():
    import wdg_amd._lib as L
    err = L.lib.wdg_last_error
    assert _check(_jobs(3)) == 0
    assert L.lib.wdg_csr_two_hop_check_jobs(None, 0) == 0                         # n_jobs = 0: nothing to check
    assert L.lib.wdg_csr_two_hop_check_jobs(None, 1) == INVALID and b"null job table" in err()
    assert L.lib.wdg_csr_two_hop_check_jobs(None, -1) == INVALID
    assert _check(_jobs(n=-1)) == INVALID and b"negative n" in err()
    assert _check(_jobs(n=LIMIT)) == 0                                            # the limit itself is accepted
    assert _check(_jobs(n=LIMIT + 1)) == UNSUPPORTED and str(LIMIT).encode() in err()
    for flags in (4, 8, 7, -1, 1 << 30):
        assert _check(_jobs(flags=flags)) == INVALID and b"flags" in err(), flags
    for flags in (0, 1, 2, 3):
        assert _check(_jobs(flags=flags)) == 0
    assert _check(_jobs(rowptr=0)) == INVALID and b"null rowptr" in err()
    assert _check(_jobs(out_rowptr=0)) == INVALID and b"out_rowptr" in err()
    assert _check(_jobs(total=0)) == INVALID and b"total" in err()
    assert _check(_jobs(out_col=0)) == 0                                          # out_col may be null for the count pass
    assert _check(_jobs(col=0)) == 0                                              # a pattern without entries
    assert _check(_jobs(n=0, rowptr=0, col=0)) == 0                               # an empty job needs no input
    jobs = _jobs(3)
    jobs[2].n = -5
    assert _check(jobs) == INVALID and err().startswith(b"csr_two_hop_check_jobs: job 2 ")
    big = _jobs(65536)
    assert _check(big) == INVALID and b"65535" in err()
    assert _check(big, 65535) == 0


def test_launch_refusals_need_no_gpu():
    import wdg_amd._lib as L
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # (never dereferenced: every call below returns before any HIP call)
    for f in (L.lib.wdg_csr_two_hop_count_batched, L.lib.wdg_csr_two_hop_fill_batched):
        assert f(null, 1, 100, null) == INVALID and b"null job table" in L.lib.wdg_last_error()
        assert f(some, -1, 100, null) == INVALID and f(some, 1, -1, null) == INVALID
        assert f(some, 65536, 100, null) == INVALID and b"65535" in L.lib.wdg_last_error()
        assert f(some, 1, LIMIT + 1, null) == UNSUPPORTED and str(LIMIT).encode() in L.lib.wdg_last_error()
        assert f(null, 0, 100, null) == 0 and f(some, 0, 0, null) == 0           # n_jobs = 0: nothing is launched
        assert f(some, 3, 0, null) == 0                                          # nothing but n = 0 jobs: nothing is launched
    with pytest.raises(ValueError):
        L.check(L.lib.wdg_csr_two_hop_count_batched(null, 1, 100, null), "wdg_csr_two_hop_count_batched")


def _graph(n_rows, n_cols):
    """an empty pattern of HOST tensors: enough for every check that comes before the device is asked for"""
    from wdg_amd import ops
    return ops.CsrGraph(torch.zeros(n_rows + 1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), None, n_rows, n_cols)


def test_two_hop_batch_refuses_before_it_asks_for_a_device():
    from wdg_amd import ops
    with pytest.raises(ValueError, match="graph 1 is 6 x 7; a square pattern"):
        ops.TwoHopBatch([_graph(6, 6), _graph(6, 7)])
    with pytest.raises(ValueError, match=f"graph 0 has {LIMIT + 1} rows; .* at most {LIMIT}"):
        ops.TwoHopBatch([_graph(LIMIT + 1, LIMIT + 1)])
    with pytest.raises(ValueError, match="flags = 4"):
        ops.TwoHopBatch([_graph(6, 6)], flags=4)
    with pytest.raises(ValueError, match="65536 graphs; one launch takes 65535"):
        ops.TwoHopBatch([_graph(1, 1)] * 65536)
    with pytest.raises(ValueError, match="square"):
        ops.two_hop(_graph(3, 4))
    with pytest.raises(ValueError, match="square"):
        _graph(3, 4).two_hop()
    if not torch.cuda.is_available():  # a well-formed list passes every host-side check: what stops it is the missing device
        with pytest.raises(Exception, match="no HIP device"):
            ops.TwoHopBatch([_graph(6, 6), _graph(LIMIT, LIMIT)], flags=3)
        with pytest.raises(Exception, match="no HIP device"):
            ops.TwoHopBatch([])


def test_the_totals_helper():
    from wdg_amd import ops
    assert ops.two_hop_totals([0, 5, (1 << 31) - 1]) == [0, 5, (1 << 31) - 1]
    assert ops.two_hop_totals(torch.tensor([3, 4], dtype=torch.int64).tolist()) == [3, 4] and ops.two_hop_totals([]) == []
    with pytest.raises(IndexError, match="graph 1 "):
        ops.two_hop_totals([7, -1, 2])
    with pytest.raises(OverflowError, match="graph 0 has 2147483648"):
        ops.two_hop_totals([1 << 31])


def test_models_names_exist():
    from wdg_amd import models
    assert issubclass(models.H2GCN1, torch.nn.Module) and issubclass(models.H2GCN2, torch.nn.Module) and hasattr(models, "TwoHopAdj")
    torch.manual_seed(0)
    m = models.H2GCN2(10, 3, nhid=4)
    assert [k for k, _ in m.named_parameters()] == ["w_e", "w_c"] and m.w_e.shape == (10, 4) and m.w_c.shape == (28, 3)
    torch.manual_seed(0)
    we = torch.nn.init.xavier_uniform_(torch.empty(10, 4))
    wc = torch.nn.init.xavier_uniform_(torch.empty(28, 3))
    assert torch.equal(m.w_e.detach(), we) and torch.equal(m.w_c.detach(), wc)   # drawn in the stated order
    assert models.H2GCN1(10, 3, nhid=4).w_c.shape == (12, 3)
