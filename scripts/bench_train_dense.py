#!/usr/bin/env python
"""Training step on the dense box (shape B: N = 504 atoms at 0.1 / A^3, r = 8 A, ~120 neighbours per atom; k = 1024,
depth 6, fp32): ms per step and peak device memory of `train_conv_mode` "factored" and "materialized" on the same
batches, in that order per batch size.  One JSON line per (batch size, mode); a mode that does not fit reports
"oom".  For the per-kernel split of a factored step run this script with `--modes factored --batch-sizes 1` under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_train_dense.py ...` in a run of its own.

    python scripts/bench_train_dense.py --batch-sizes 1 2 4 8 --steps 3 --warmup 1
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from molecular_dynamics_neural_operator_amd import ops, synthetic as syn  # noqa: E402
from molecular_dynamics_neural_operator_amd.dataset import PairData  # noqa: E402
from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN, LpLoss  # noqa: E402
from molecular_dynamics_neural_operator_amd.training import collate, train_forward  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--atoms", type=int, default=504)
ap.add_argument("--kernel-width", type=int, default=1024)
ap.add_argument("--depth", type=int, default=6)
ap.add_argument("--window", type=int, default=10)
ap.add_argument("--batch-sizes", type=int, nargs="+", default=[1, 2, 4, 8])
ap.add_argument("--modes", nargs="+", default=["factored", "materialized"], choices=["factored", "materialized"])
ap.add_argument("--gemm-mode", default="split_f16", choices=["split_f16", "split_bf16", "f32"])
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
a = ap.parse_args()

dev = torch.device("cuda:0")


def sample(seed):
    base = syn.box_frame(a.atoms, 0.1, seed=seed)
    win = torch.from_numpy(syn.jitter_window(base, a.window, seed=seed)).to(dev)
    g = ops.radius_graph(win[-1].contiguous(), a.atoms, 8.0)
    ei = g.to_edge_index()
    ea = torch.cat([win[-1][ei[0]], win[-1][ei[1]]], dim=1)
    y = win[-1] + 0.05 * torch.randn(a.atoms, 3, device=dev, generator=torch.Generator(dev).manual_seed(seed))
    return PairData(torch.from_numpy(syn.amino_acids(a.atoms, seed=seed)).to(dev), win, y, ea, ei)


torch.manual_seed(0)
model = KernelNN(64, a.kernel_width, a.depth, 6, 7, 3, 20, 4)
with torch.no_grad():
    for p_ in model.conv1.net.layers[4].parameters():
        p_.mul_(0.05)
model.to(dev).train()
model.gemm_mode, model.train_precision = a.gemm_mode, "fp32"
loss_fn = LpLoss(size_average=False)

for B in a.batch_sizes:
    batch = collate([sample(s) for s in range(B)])
    E = int(batch.edge_index.shape[1])
    for mode in a.modes:
        model.train_conv_mode = mode
        rec = dict(atoms=a.atoms, k=a.kernel_width, depth=a.depth, batch=B, edges=E, mode=mode, gemm_mode=a.gemm_mode)
        try:
            times = []
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            for it in range(a.warmup + a.steps):
                model.zero_grad(set_to_none=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = train_forward(model, batch)
                loss_fn(out.view(B, -1), batch.y.view(B, -1)).backward()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times.append((time.perf_counter() - t0) * 1e3)
            rec.update(ms_per_step=float(np.median(times)), ms_all=[round(t, 3) for t in times],
                       peak_mib=torch.cuda.max_memory_allocated() / 2 ** 20)
        except torch.cuda.OutOfMemoryError:
            rec.update(ms_per_step=None, peak_mib=None, note="oom")
            out = None
            model.zero_grad(set_to_none=True)
        print(json.dumps(rec), flush=True)
