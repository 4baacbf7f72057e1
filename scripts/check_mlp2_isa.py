#!/usr/bin/env python3
"""Static check of the generated code of mlp2_split_kernel<1> / <2> (csrc/gemm.hip): does the K loop keep its prefetch in flight?

The loop requests the NEXT 32-k step's four `global_load_dwordx4` and then splits and multiplies the step it holds.  The
compiler writes the waits; it counts them (`s_waitcnt vmcnt(4)`: "everything but the four requests just issued") only while
no memory operation in the loop is conditional - with one, its wait insertion merges the paths and the wait in front of the
held step's first use degrades to `vmcnt(2)` .. `vmcnt(0)`: the wave issues its prefetch and stands still until it has
arrived.  The results are the same either way, so only the generated code shows it.  Checked per kernel:

  (a) in the steady-state loop (the innermost loop that holds the bf16 MFMAs) no `s_waitcnt vmcnt(n)` between a step's group
      of A loads and the end of the MFMA group that follows has n below the number of A loads of that group (four);
  (b) no `s_waitcnt vmcnt` between the first and the last store of Z (a wait there also waits for the store before it);
  (c) no `scratch_` instruction.

Used by tests/test_mlp2_isa.py.  By hand (the compiler and the unit's flags as the Makefile hands them out):
    $(make -s hipcc-line UNIT=gemm) --cuda-device-only -S when-do-gnns-help_amd/csrc/gemm.hip -o gemm.s && \\
          python scripts/check_mlp2_isa.py gemm.s
(`python scripts/check_mlp2_isa.py gram.s gram_split_kernel`, on csrc/gram.hip's code, reports (a) and (c) for another kernel of the
same scheme.)
"""
import re
import sys

A_LOADS = 4  # global_load_dwordx4 per step: two rows x (k 0..3, k 4..7) of the lane's eight
KERNEL_RE = r"^(_Z\S*%s\S*):[^\n]*\n(.*?)s_endpgm"
MFMA = "v_mfma_f32_16x16x32_bf16"


def instructions(body):
    """the kernel's lines in layout order without comments and directives; labels stay"""
    out = []
    for line in body.split("\n"):
        t = line.split(";")[0].strip()
        if not t or (t.startswith(".") and not re.match(r"^\.LBB\d+_\d+:", t)):
            continue
        out.append(t)
    return out


def steady_loops(ins):
    """[(first, last)] of the innermost loops (a label and a later branch to it) that hold a bf16 MFMA"""
    at = {m.group(1): i for i, t in enumerate(ins) for m in [re.match(r"^(\.LBB\d+_\d+):", t)] if m}
    loops = []
    for j, t in enumerate(ins):
        m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", t)
        if m and m.group(1) in at and at[m.group(1)] < j:
            i = at[m.group(1)]
            if any(x.startswith(MFMA) for x in ins[i:j]):
                loops.append((i, j))
    return [l for l in loops if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in loops)]


def check_body(body):
    """-> dict(loops, groups, stores, loop_waits=[(index, text, n)], store_waits=[(index, text)], scratch=[text])"""
    ins = instructions(body)
    loops = steady_loops(ins)
    loop_waits, n_groups = [], 0
    for first, last in loops:
        loads = [i for i in range(first, last + 1) if ins[i].startswith("global_load_dwordx4")]
        groups = [loads[g:g + A_LOADS] for g in range(0, len(loads) - A_LOADS + 1, A_LOADS)]
        for g, grp in enumerate(groups):
            stop = groups[g + 1][0] if g + 1 < len(groups) else last + 1
            if any(ins[i].startswith(MFMA) for i in range(grp[0], grp[-1])):
                raise ValueError("a step's A loads are not issued as one group")
            mfmas = [i for i in range(grp[-1], stop) if ins[i].startswith(MFMA)]
            if not mfmas:
                continue  # (nothing is multiplied behind this group)
            n_groups += 1
            for i in range(grp[-1] + 1, mfmas[-1]):
                m = re.match(r"s_waitcnt\b.*vmcnt\((\d+)\)", ins[i])
                if m and int(m.group(1)) < A_LOADS:
                    loop_waits.append((i, ins[i], int(m.group(1))))
    stores = [i for i, t in enumerate(ins) if t.startswith("global_store")]
    store_waits = []
    if stores:
        store_waits = [(i, ins[i]) for i in range(stores[0], stores[-1]) if re.match(r"s_waitcnt\b.*vmcnt", ins[i])]
    return {"loops": len(loops), "groups": n_groups, "stores": len(stores), "loop_waits": loop_waits, "store_waits": store_waits,
            "scratch": [t for t in ins if t.startswith("scratch_")]}


def check_kernel(text, name):
    m = re.search(KERNEL_RE % name, text, re.M | re.S)
    if not m:
        raise ValueError(f"{name} not found")
    return check_body(m.group(2))


def main():
    text = open(sys.argv[1]).read()
    names = sys.argv[2:] or ["mlp2_split_kernelILi1E", "mlp2_split_kernelILi2E"]
    bad = 0
    for name in names:
        res = check_kernel(text, name)
        print(name, {k: (v if isinstance(v, int) else len(v)) for k, v in res.items()})
        for key in ("loop_waits", "store_waits", "scratch"):
            for v in res[key][:12]:
                print("   ", key, v)
            bad += len(res[key])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
