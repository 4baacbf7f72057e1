#!/usr/bin/env python3
"""Times the GCNII layer of csrc/gcnii.hip (wdg_gcnii_forward_batched_f32, wdg_gcnii_backward_batched_f32 and the one
wdg_gcnii_weight_grad_batched_f32 launch of a model) beside the same layer composed from what existed before it - ops.spmm, torch.lerp,
ops.gemm, torch.lerp, ops.DropoutBatch: five launches per layer forward -, and records, for DESIGN 4.31, GCNII's accuracy on the generated
graphs beside GCN-2 and MLP-2 and the largest error / derived bound of every output of the kernels against fp64.

  layers    the Cora fixture's topology (tests/golden/real_cora.npz, symmetric scales, self loops) at w = 64, L = 8 and L = 32 layers on a
            random H0: the forward pass alone (no gradients: the inference table, S = NULL) and forward + backward (models._GcniiLayers
            against the composition under autograd: adj.matmul, torch.lerp, models._Linear, torch.lerp, DeviceDropout.relu_dropout), both
            at dropout 0.5 with a DeviceDropout; and ONE layer of a 50-graph shard (N = 2000, k = 10, ten homophily levels x five seeds,
            w = 64) as ONE table of 50 jobs, forward and backward, behind 50 ops.spmm calls in both arms - the composition: one torch.lerp
            over the concatenated rows, 50 ops.gemm (a weight per graph), one torch.lerp, one DropoutBatch of 50 entries; its backward
            pass is not composed (not measured).  The arms alternate inside every round; device time from events around --iters
            back-to-back calls; median, minimum and maximum over the rounds (the method of scripts/_timing.py).
  epochs    the captured models.train_eval_graphed epoch (training step + evaluation) of models.GCNII and of the composed model, on Cora's
            topology with 128 generated features and 7 generated classes, L = 8 and L = 32, hidden 64: seconds / epochs of 200 replays,
            the two models alternating, three rounds.
  accuracy  N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, h in 0.2, 0.5, 0.9, seeds 0 - 4: validation and test accuracy at the
            selected epoch of GCNII (hidden 64, 8 layers, alpha 0.1, theta 0.5; NormAdj(symmetric=1)), GCN2 and MLP2 (NormAdj(symmetric=0)),
            dropout 0.5 - the graphs, features and seeds of scripts/time_gat.py.
  errors    the jobs of tests/_gcnii_ref.py on the device: the largest |fp32 - fp64| / derived bound of S, out, d_P, d_H0 and d_W.

    python scripts/time_gcnii.py [--out profiles/gcnii_timing.json]

Without --step the script runs its steps as child processes, each under its own `timeout`, one after the other, and stops at the
first that fails: nothing more runs on the device after a step that faults, aborts or times out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import ROOT, Step, _accuracy_sweep, _cora_coo, _generated_features, _time_arms, _time_epochs, flags, run_step, run_steps, write  # noqa: E402

ALPHA, THETA, P, W = 0.1, 0.5, 0.5, 64


def composed_model():
    """the GCNII of models.py with every layer composed from the operations that existed before csrc/gcnii.hip"""
    import torch
    from wdg_amd import models

    class ComposedGCNII(models._HiddenDropout, torch.nn.Module):
        def __init__(self, nfeat, nclass, nhid=64, layers=8, alpha=ALPHA, theta=THETA, dropout=P, dropout_rng=None):
            super().__init__()
            ref = models.GCNII(nfeat, nclass, nhid, layers, alpha, theta, dropout, None)  # (the same draws and the same beta)
            self.w_in, self.weights, self.w_out = ref.w_in, ref.weights, ref.w_out
            self.alpha, self.betas = float(alpha), [float(b) for b in ref.filter_strength()]
            self.dropout, self.dropout_rng = dropout, dropout_rng
            self._rngs = [models.DeviceDropout(dropout_rng.seed, dropout_rng.stream + l + 1) for l in range(layers)] if dropout_rng is not None else None

        def layers(self, adj, h0):
            h = h0
            for l, (w, beta) in enumerate(zip(self.weights, self.betas)):
                s = torch.lerp(adj.matmul(h), h0, self.alpha)
                z = torch.lerp(s, models._Linear.apply(s, w, False), beta)
                h = self._rngs[l].relu_dropout(z, self.dropout, self.training) if self._rngs is not None else self._torch_dropout(torch.relu(z))
            return h

        def forward(self, adj, x):
            return models._Linear.apply(self.layers(adj, self._relu_dropout_of_product(x, self.w_in)), self.w_out, False)

    return ComposedGCNII


def _cora_adj():
    from wdg_amd import models
    coo, n = _cora_coo()
    return models.NormAdj(coo, symmetric=1), n


def _stack_case(adj, n, layers, a):
    """L layers on Cora: the fused stack against the composition, forward alone and forward + backward"""
    import torch
    from wdg_amd import models, ops
    torch.manual_seed(0)
    fused = models.GCNII(8, 7, W, layers, ALPHA, THETA, P, models.DeviceDropout(1, 0)).cuda().train()
    comp = composed_model()(8, 7, W, layers, ALPHA, THETA, P, models.DeviceDropout(1, 0)).cuda().train()
    h0 = torch.rand(n, W, device="cuda")
    h0g = h0.clone().requires_grad_()
    d_out = torch.randn(n, W, device="cuda")
    weights = [w.detach() for w in fused.weights]
    # the composition's forward pass on raw operations: exactly five launches per layer, in place where the operation allows
    buf = {k: torch.zeros(n, W, device="cuda") for k in ("p", "s", "t")}
    outs = [torch.zeros(n, W, device="cuda") for _ in range(2)]
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    drops = [ops.DropoutBatch([(o, None, 1)], P, 1) for o in outs]

    def composed_forward():
        h = h0
        for l, (w, beta) in enumerate(zip(weights, comp.betas)):
            ops.spmm(adj.graph, h, row_scale=adj.row_scale, col_scale=adj.col_scale, out=buf["p"])
            torch.lerp(buf["p"], h0, ALPHA, out=buf["s"])
            ops.gemm(buf["s"], w, out=buf["t"])
            torch.lerp(buf["s"], buf["t"], beta, out=outs[l & 1])
            drops[l & 1].launch(word)
            h = outs[l & 1]

    def fused_forward():
        with torch.no_grad():
            fused._stack.forward(False, adj, h0, weights, P, 0.0)

    def fused_both():
        torch.autograd.grad(models._GcniiLayers.apply(fused._stack, adj, P, 0.0, h0g, *fused.weights), [h0g, *fused.weights], grad_outputs=d_out)

    def composed_both():
        torch.autograd.grad(comp.layers(adj, h0g), [h0g, *comp.weights], grad_outputs=d_out)

    def aggregations():
        for _ in range(layers):
            ops.spmm(adj.graph, h0, row_scale=adj.row_scale, col_scale=adj.col_scale, out=buf["p"])

    arms = {"fused forward (L aggregations + L launches + 2 copies)": fused_forward, "composed forward (5 L launches)": composed_forward,
            "fused forward + backward (autograd function over the stack)": fused_both, "composed forward + backward (autograd)": composed_both,
            "the L aggregations alone (ops.spmm)": aggregations}
    return _time_arms(arms, a.rounds, a.iters)


def _shard_case(a):
    """ONE layer of a 50-graph shard as one table of 50 jobs"""
    import torch
    from wdg_amd import ops, synth
    specs = [(2000, 5, 10, synth.out_degree(10, h), seed) for h in synth.H_LEVELS_10_K10 for seed in range(5)]
    graphs = ops.GraphBatch.generated(specs, flags=0, quad=False).graphs
    norm = [ops.degree_norm(g, ops.NORM_SYM, ops.PREC_F32)["dinv"] for g in graphs]
    n, G = 2000, len(graphs)
    z = lambda *shape: torch.zeros(shape, device="cuda")  # noqa: E731
    h_all, h0_all, p_all, s_all, t_all, out_all, out2_all = torch.rand(G * n, W, device="cuda"), torch.rand(G * n, W, device="cuda"), z(G * n, W), z(G * n, W), z(G * n, W), z(G * n, W), z(G * n, W)
    d_out, d_p, d_h0 = torch.randn(G * n, W, device="cuda"), z(G * n, W), z(G * n, W)
    ws, d_ws = torch.randn(G, W, W, device="cuda") / 8, z(G, W, W)
    rows = lambda t, i: t[i * n:(i + 1) * n]  # noqa: E731
    beta = 0.4
    entries = [dict(p=rows(p_all, i), h0=rows(h0_all, i), w=ws[i], out=rows(out_all, i), s=rows(s_all, i), alpha=ALPHA, beta=beta, stream=i,
                    d_out=rows(d_out, i), d_p=rows(d_p, i), d_h0=rows(d_h0, i), d_w=d_ws[i]) for i in range(G)]
    table = ops.GcniiBatch(entries, P, 1)
    drop = ops.DropoutBatch([(rows(out2_all, i), None, i) for i in range(G)], P, 1)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")

    def aggregate():
        for i, (g, d) in enumerate(zip(graphs, norm)):
            ops.spmm(g, rows(h_all, i), row_scale=d, col_scale=d, out=rows(p_all, i))

    def fused_forward():
        aggregate()
        table.launch(word)

    def composed_forward():
        aggregate()
        torch.lerp(p_all, h0_all, ALPHA, out=s_all)
        for i in range(G):
            ops.gemm(rows(s_all, i), ws[i], out=rows(t_all, i))
        torch.lerp(s_all, t_all, beta, out=out2_all)
        drop.launch(word)

    def fused_backward():
        table.launch_backward()
        table.launch_weight_grad()

    fused_forward()
    composed_forward()
    torch.cuda.synchronize()
    res = _time_arms({"fused forward (50 ops.spmm + 1 launch)": fused_forward, "composed forward (50 ops.spmm + lerp + 50 ops.gemm + lerp + DropoutBatch)": composed_forward,
                      "the 50 aggregations alone (ops.spmm)": aggregate, "fused backward + weight gradient (2 launches, no aggregation)": fused_backward},
                     a.rounds, max(1, a.iters // 5))
    res["composed backward"] = "not measured"
    res["largest |fused - composed| of out"] = float((out_all - out2_all).abs().max())
    return res


def step_layers(a):
    out = {"workload": f"{a.rounds} interleaved rounds of {a.iters} back-to-back calls (the shard: a fifth of that), device time from events; us per call"}
    adj, n = _cora_adj()
    for layers in (8, 32):
        name = f"cora, w = {W}, L = {layers}"
        out[name] = _stack_case(adj, n, layers, a)
        print(json.dumps({name: out[name]}), flush=True)
    name = f"one layer of a shard of 50 graphs (N = 2000, k = 10), w = {W}, one table"
    out[name] = _shard_case(a)
    print(json.dumps({name: out[name]}), flush=True)
    return out


def step_epochs(a):
    import torch
    from wdg_amd import models
    adj, n = _cora_adj()
    x, labels = _generated_features(n, 7)
    out = {"workload": "models.train_eval_graphed(capture=True), 200 epochs on Cora's topology, 128 generated features, 7 generated classes, hidden 64, "
                       "dropout 0.5 with a DeviceDropout: ms per epoch (training step + evaluation, two graph replays), three alternating rounds"}
    for layers in (8, 32):
        def arm(mk):
            def run(rnd):
                torch.manual_seed(0)
                model = mk(128, 7, W, layers, ALPHA, THETA, P, models.DeviceDropout(1, 0))
                torch.manual_seed(0)
                return models.train_eval_graphed(model, adj, x, labels, epochs=200, lr=0.01, capture=True)
            return run

        out[f"L = {layers}"] = _time_epochs({"models.GCNII": arm(models.GCNII), "composed": arm(composed_model())}, 3, 200)
        print(json.dumps({f"L = {layers}": out[f"L = {layers}"]}), flush=True)
    return out


def step_accuracy(a):
    from wdg_amd import models
    out = {"workload": "N = 2000, F = 128, signal 0.5, k = 10, 80 epochs, lr 0.05, weight decay 5e-4, dropout 0.5, random 60/20/20 splits; validation "
                       "and test accuracy at the selected epoch, seeds 0 - 4"}
    adj = lambda coo, seed: models.NormAdj(coo, symmetric=0)  # noqa: E731
    out.update(_accuracy_sweep((("GCNII (hidden 64, 8 layers, alpha 0.1, theta 0.5)", models.GCNII, lambda coo, seed: models.NormAdj(coo, symmetric=1)),
                                ("GCN2 (hidden 64)", models.GCN2, adj), ("MLP2 (hidden 64)", models.MLP2, adj))))
    return out


def step_errors(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import _gcnii_ref as ref
    from wdg_amd import ops
    worst = {}
    for act, p, step in ((False, 0.0, 0), (True, 0.5, 3)):
        scale = float(ref._dropout_ref.constants(p)[1])
        for i, (n, w, _extra, _offset, (alpha, beta)) in enumerate(ref.JOBS):
            z = lambda *shape: torch.zeros(shape, device="cuda")  # noqa: E731
            x = {k: z(*v.shape).copy_(torch.from_numpy(np.array(v))) for k, v in ref.job_inputs(i).items()}
            e = dict(p=x["P"], h0=x["H0"], w=x["W"], out=z(n, w), s=z(n, w), alpha=alpha, beta=beta, stream=ref.stream_of(i), d_out=x["d_out"], d_p=z(n, w),
                     d_h0=x["d_H0"].clone(), d_w=z(w, w))
            table = ops.GcniiBatch([e], p, ref.SEED, act=act)
            table.launch(torch.tensor([step], dtype=torch.int32, device="cuda"))
            table.launch_backward()
            table.launch_weight_grad()
            torch.cuda.synchronize()
            g = {k: e[k].cpu().numpy() for k in ("s", "out", "d_p", "d_h0", "d_w")}
            h = ref.job_inputs(i)
            S, S_abs, Z, Z_abs = ref.forward64(h["P"], h["H0"], h["W"], alpha, beta)
            keep = ref._dropout_ref.keep_mask(n, w, p, ref.SEED, ref.stream_of(i), step) if n else np.zeros((n, w), bool)
            out64 = np.where(keep, np.maximum(Z, 0.0) * scale, 0.0) if act else Z
            ratios = dict(S=ref.within("S", g["s"], S, S_abs, n, w), out=ref.within("out" if act else "Z", g["out"], out64, Z_abs * scale, n, w))
            b = ref.backward64(h["d_out"], g["out"], g["s"], h["W"], alpha, beta, h["d_H0"], act, scale)
            for name, key in (("d_P", "d_p"), ("d_H0", "d_h0"), ("d_W", "d_w")):
                ratios[name] = ref.within(name, g[key], *b[name], n, w)
            for name, r in ratios.items():
                worst[name] = max(worst.get(name, 0.0), r)
    return {"workload": f"the {len(ref.JOBS)} jobs of tests/_gcnii_ref.py, without an activation and with ReLU + dropout 0.5: the largest |fp32 - fp64| / "
                        "((k + 2) 2^-24 * companion), k = the roundings counted in tests/_gcnii_ref.py (1.0 = the bound)",
            "largest error / derived bound": {k: round(v, 4) for k, v in worst.items()}}


STEP_FNS = {"layers": step_layers, "epochs": step_epochs, "accuracy": step_accuracy, "errors": step_errors}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step", choices=["layers", "epochs", "accuracy", "errors"])
    ap.add_argument("--part", help="(with --step) where the step writes its part of the document")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcnii_timing.json"))
    return ap.parse_args(argv)


def invocations(a):
    return [Step("errors", "errors", 120), Step("layers", "layers", 240), Step("epochs", "epochs", 240), Step("accuracy", "accuracy", 300)]


def main():
    a = parse()
    if a.step:
        return run_step(a, STEP_FNS)
    write(a.out, dict(run_steps(__file__, invocations(a), flags(a, "rounds", "iters"), a.out)))


if __name__ == "__main__":
    main()
