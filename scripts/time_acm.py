#!/usr/bin/env python3
"""Times sweep.TrainBatch's captured epoch of the kinds "acm_sgc" / "acm_gcn" beside "sgc" / "gcn", and the two launches of
csrc/acm_mix.hip (wdg_acm_mix_batched_f32 and its backward pass) beside the same mix written as torch operations on the stacked
tensors - what a user would write without the kernel.

  shard    the C3 shard of bench.py's `train` block (50 graphs, N = 2000, F = 500, k = 10, hidden 64), the captured epoch, --epochs
           epochs, best of --runs after a warm-up.  The ACM kinds and the existing kinds are timed in alternating processes:
           acm, base, acm, base - one process each, in that order, on the same device.
  kernel   layer 1's mix of "acm_gcn" on that shard ([50, 2000, 64], activation on, high_agg and the transposed output) and the logits
           mix ([50, 2000, 5], no activation): the launch against the torch composition, forward and forward + backward, interleaved
           rounds in one process, device time from events around --kernel-iters back-to-back calls

    python scripts/time_acm.py [--runs 3] [--epochs 200] [--out profiles/acm_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails: nothing more runs on the device after a step that faults, aborts or times out.  A child writes its part of the
document next to --out and the parent joins them.  (`device` in the document is torch.cuda.get_device_name(0): an MI355X reports
"AMD Radeon Graphics" under ROCm builds that have no marketing name for gfx950.)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _shard_batch, _time_arms, best_of, flags, run_step, run_steps, write  # noqa: E402

GROUPS = {"acm": ("acm_sgc", "acm_gcn"), "base": ("sgc", "gcn")}


def step_shard(a):
    from wdg_amd import sweep
    jobs, sb = _shard_batch()
    out = {"workload": f"{len(jobs)} graphs, N = 2000, F = 500, k = 10, hidden 64, {a.epochs} captured epochs, best of {a.runs} after a warm-up; "
                       "wall clock around the epoch loop, the device drained before and after"}
    for kind in GROUPS[a.group]:
        tb = sweep.TrainBatch(sb, kind=kind, hidden=64, seed=1)
        tb.run(epochs=3, capture=True)
        r = {}
        s = best_of(lambda: r.update(tb.run(epochs=a.epochs, capture=True)) or r["seconds"], a.runs)
        out[kind] = {"seconds": s, "ms_per_epoch": s / a.epochs * 1e3, "mean_val_acc": float(r["val_acc"].mean()),
                     "mean_test_acc": float(r["test_acc"].mean())}
        print(json.dumps({kind: out[kind]}), flush=True)
        del tb
    return out


def torch_mix(low, high, high_agg, ident, att, wmix, relu):
    """the mix of include/wdg.h on stacked tensors ([J, n, w] operands, att [J, 3, w], wmix [J, 3, 3]) -> (out, out_t)"""
    import torch
    h = torch.stack([low, high - high_agg, ident], 1)
    if relu:
        h = torch.relu(h)
    s = torch.sigmoid(torch.einsum("jcnk,jck->jnc", h, att))
    alpha = torch.softmax((s / 3) @ wmix, 2)
    out = 3 * torch.einsum("jnc,jcnk->jnk", alpha, h)
    return out, out.transpose(1, 2).contiguous()


def step_kernel(a):
    import torch
    from wdg_amd import ops
    J, n = 50, 2000
    out = {"workload": f"{J} layers of {n} rows, {a.kernel_rounds} interleaved rounds of {a.kernel_iters} back-to-back calls, device time from "
                       "events; us per call.  torch: the composition on the stacked tensors, its backward pass by autograd (timed as "
                       "forward + backward: autograd needs the forward's graph)"}
    for w, relu in ((64, True), (5, False)):
        g = lambda *s: torch.randn((J,) + s, device="cuda")  # noqa: E731
        t = dict(low=g(n, w), high=g(n, w), high_agg=g(n, w), ident=g(n, w), att=g(3, w) / w ** 0.5, wmix=g(3, 3) / 3 ** 0.5, d_out=g(n, w))
        z = lambda *s: torch.zeros((J,) + s, device="cuda")  # noqa: E731
        o = dict(out=z(n, w), out_t=z(w, n), d_low=z(n, w), d_high=z(n, w), d_ident=z(n, w), d_att=z(3, w), d_wmix=z(3, 3))
        batch = ops.AcmMixBatch([dict({k: v[j] for k, v in t.items()}, **{k: v[j] for k, v in o.items()}) for j in range(J)], relu)
        leaves = {k: t[k].clone().requires_grad_() for k in ("low", "high", "high_agg", "ident", "att", "wmix")}

        def torch_forward():
            with torch.no_grad():
                torch_mix(t["low"], t["high"], t["high_agg"], t["ident"], t["att"], t["wmix"], relu)

        def torch_both():
            res, _ = torch_mix(leaves["low"], leaves["high"], leaves["high_agg"], leaves["ident"], leaves["att"], leaves["wmix"], relu)
            torch.autograd.grad(res, list(leaves.values()), grad_outputs=t["d_out"])

        arms = {"wdg_acm_mix_batched_f32 (1 launch)": batch.launch, "wdg_acm_mix_backward_batched_f32 (2 launches)": batch.launch_backward,
                "kernels, forward + backward": lambda: (batch.launch(), batch.launch_backward()),
                "torch forward": torch_forward, "torch forward + backward": torch_both}
        times = _time_arms(arms, a.kernel_rounds, a.kernel_iters)
        mb = J * n * w * 4 / 1e6
        key = f"width {w}, activation {'on' if relu else 'off'}"
        out[key] = {"bytes": f"forward: 4 reads of {mb:.1f} MB, out and out_t of {mb:.1f} MB each, aux {J * n * 32 / 1e6:.1f} MB; "
                             f"backward: 5 reads and 3 writes of {mb:.1f} MB, aux"}
        for name, summary in times.items():
            out[key][name] = summary
            print(json.dumps({key: {name: out[key][name]}}), flush=True)
    return out


STEP_FNS = {"shard": step_shard, "kernel": step_kernel}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--kernel-rounds", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=100)
    ap.add_argument("--step", choices=["shard", "kernel"])
    ap.add_argument("--group", choices=sorted(GROUPS), help="(with --step shard) the kinds the step times")
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acm_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    """acm, base, acm, base - one process each -, then the kernel"""
    return [Step(f"shard {group} {i}", "shard", 300, ("--group", group)) for i in (1, 2) for group in ("acm", "base")] + [Step("kernel", "kernel", 240)]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    parts = run_steps(__file__, invocations(a), flags(a, "runs", "epochs", "kernel_rounds", "kernel_iters"), a.out)
    doc = dict({"order": [key for key, _ in parts]}, **dict(parts))
    best = lambda group, kind: min(doc[f"shard {group} {i}"][kind]["ms_per_epoch"] for i in (1, 2))  # noqa: E731
    doc["ms per captured epoch, best of each side's two processes"] = {k: best(g, k) for g, kinds in GROUPS.items() for k in kinds}
    doc["acm over base"] = {"acm_sgc / sgc": best("acm", "acm_sgc") / best("base", "sgc"), "acm_gcn / gcn": best("acm", "acm_gcn") / best("base", "gcn")}
    write(a.out, doc)


if __name__ == "__main__":
    main()
