#!/usr/bin/env python3
"""Line-level host time of SweepBatch.__init__ and of KrPlan's construction inside the whole sweep (dev tool; sys.settrace on those
frames)."""
import linecache
import os
import sys
import time
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

import bench
from wdg_amd import sweep


class A:
    nodes, kr_epochs = 2000, 100


inp = bench.whole_inputs(A)
pairs, graphs, feats = inp["pairs"], inp["graphs"], inp["feats"]
graph_of = lambda j: graphs[(j.h, j.seed)]  # noqa: E731
sweep.whole_sweep_rank(pairs[:4], graph_of, feats, 1, 0)
sweep.whole_sweep_rank(pairs, graph_of, feats, 1, 0)
torch.cuda.synchronize()
acc = defaultdict(float)
last = {}
SB = sweep.SweepBatch  # (sweep_batch.py: the constructor and its stages; KrPlan's are in kr_plan.py - a line is named with its file)
targets = {f.__code__ for f in (SB.__init__, SB._plan_columns, SB._host_graphs, SB._feature_blocks, SB._with_label_block, SB._finish_graphs,
                                 SB._upload_labels, SB._layout_y, SB._aggregation_tables, SB._gcn_tables, sweep.KrPlan.__init__,
                                 sweep.KrPlan._build_grams, sweep.KrPlan._group_jobs, sweep.KrPlan._draw_sets, sweep.KrPlan._regression_table)}


def tracer(frame, event, arg):
    if frame.f_code not in targets:
        return None

    def local(frame, event, arg):
        now = time.perf_counter()
        key = id(frame)
        if key in last:
            path, code, line, t0 = last[key]
            acc[(path, code, line)] += now - t0
        if event == "return":
            last.pop(key, None)
        else:
            last[key] = (frame.f_code.co_filename, frame.f_code.co_name, frame.f_lineno, time.perf_counter())
        return local
    last[id(frame)] = (frame.f_code.co_filename, frame.f_code.co_name, frame.f_lineno, time.perf_counter())
    return local


W, R = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1, 0)
sweep.whole_sweep_rank(pairs, graph_of, feats, W, R)
torch.cuda.synchronize()
sys.settrace(tracer)
t0 = time.perf_counter()
sweep.whole_sweep_rank(pairs, graph_of, feats, W, R)
torch.cuda.synchronize()
sys.settrace(None)
print(f"traced pass: {(time.perf_counter() - t0) * 1e3:.0f} ms")
for (path, code, line), t in sorted(acc.items(), key=lambda kv: -kv[1])[:40]:
    print(f"{t * 1e3:8.1f} ms  {os.path.basename(path)}:{code}:{line}  {linecache.getline(path, line).strip()[:110]}")
