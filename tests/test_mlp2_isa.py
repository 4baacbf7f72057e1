"""CPU-only check of the generated code of the fused GCN-2 transform (mlp2_split_kernel, csrc/gemm.hip): the K loop's waits
stay counted - the next step's loads in flight while the held step is split and multiplied - and the stores of Z are issued
back to back (scripts/check_mlp2_isa.py).  The kernel computes the same bits either way: only its code shows it."""
import importlib.util
import os

from _device_code import device_code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("mlp2_split_kernelILi1E", "mlp2_split_kernelILi2E")


def _checker():
    spec = importlib.util.spec_from_file_location("check_mlp2_isa", os.path.join(ROOT, "scripts", "check_mlp2_isa.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    return chk


def test_mlp2_split_loop_keeps_its_prefetch_in_flight(tmp_path):
    """both instantiations, as shipped: (a) between a step's four A loads and the end of the MFMAs behind them no wait asks for
    fewer than four requests in flight, (b) no vmcnt wait between the first and the last store of Z, (c) no scratch"""
    chk, text = _checker(), device_code("gemm", tmp_path)
    for name in KERNELS:
        res = chk.check_kernel(text, name)
        assert res["loops"] == 1 and res["groups"] == 4, (name, res)  # the quarter loop: four steps, each behind a group of four loads
        assert res["stores"] == 16, (name, res)                         # 2 sub-tiles x 8 classes, one dword each
        assert not res["loop_waits"], f"{name}: the K loop drains its prefetch: {res['loop_waits'][:6]}"
        assert not res["store_waits"], f"{name}: waits between the stores of Z: {res['store_waits'][:6]}"
        assert not res["scratch"], f"{name}: scratch memory: {res['scratch'][:3]}"


LOADS = ["global_load_dwordx4 v[70:73], v[12:13], off offset:16", "global_load_dwordx4 v[74:77], v[12:13], off",
         "global_load_dwordx4 v[62:65], v[14:15], off offset:16", "global_load_dwordx4 v[66:69], v[14:15], off"]
SPLIT = ["v_cvt_pk_bf16_f32 v80, v46, v47", "v_lshlrev_b32_e32 v81, 16, v80"]
MFMAS = ["v_mfma_f32_16x16x32_bf16 v[0:3], v[90:93], v[80:83], v[0:3]"] * 6


def _loop(first_wait, second_wait):
    """a hand-written quarter loop of two steps: loads of the next step, wait, split, wait, MFMAs"""
    step = LOADS + [f"s_waitcnt vmcnt({first_wait})"] + SPLIT + [f"s_waitcnt vmcnt({second_wait})"] + SPLIT + MFMAS
    return [".LBB0_1:"] + step + step + ["s_waitcnt lgkmcnt(0)", "s_barrier", "s_cbranch_scc0 .LBB0_1"]


def _stores(between):
    out = []
    for c in range(4):
        out += between + [f"global_store_dword v[2:3], v{40 + c}, off offset:{4 * c}"]
    return out


def test_mlp2_isa_check_sees_drained_waits_and_serialised_stores():
    """the checker itself, on short instruction lists: the counted waits (vmcnt(6) / vmcnt(4)) and back-to-back stores pass; the
    pattern this kernel had before its partial step was taken out of the loop - vmcnt(2) in front of the held step's first use,
    vmcnt(0) in the middle of its split, a bias load and vmcnt(0) in front of every store - is reported, and so is scratch"""
    chk = _checker()
    good = chk.check_body("\n".join(_loop(6, 4) + _stores([])))
    assert good["loops"] == 1 and good["groups"] == 2 and good["stores"] == 4, good
    assert not good["loop_waits"] and not good["store_waits"] and not good["scratch"], good
    bad = chk.check_body("\n".join(_loop(2, 0) + _stores(["global_load_dword v42, v11, s[24:25]", "s_waitcnt vmcnt(0)"])))
    assert [n for _i, _t, n in bad["loop_waits"]] == [2, 0, 2, 0], bad
    assert len(bad["store_waits"]) == 3, bad  # (the wait in front of the FIRST store delays nothing behind a store)
    spill = chk.check_body("\n".join(_loop(6, 4) + ["scratch_store_dword off, v2, off offset:8"] + _stores([])))
    assert spill["scratch"] and not spill["loop_waits"], spill
    # a wait behind the MFMAs (W0's rows for the next quarter, four A requests behind them) is not the step's business
    late = _loop(6, 4)
    late.insert(len(late) - 3, "s_waitcnt vmcnt(4)")
    assert not chk.check_body("\n".join(late))["loop_waits"]
