#!/usr/bin/env python
"""One training step through K unrolled model steps (training.unrolled_forward): ms per step, by device events after
warm-up, at K = 1, 2 and 4 in two configurations —

  chain   cfg4's shape: N = 28 chains, batch 128, k = 1024, depth 6, fp32, materialised
  dense   N = 504 box at 0.1 / A^3 (r = 8 A, ~120 neighbours per atom), batch 1, k = 1024, depth 6, fp32, factored

— and `mdno_edge_mlp_input_bwd` alone at E = 60,588, k = 1024 (one N = 504 sample): its time and E k 4 bytes / time
as a fraction of 8 TB/s.  A step = zero_grad, the K forwards, the mean of the K relative-L2 losses, backward and one
Adam step.  K = 1 is `train_forward`, the one-step path; the figure to hold an unrolled step against is K x that one.
One JSON line per measurement.  Nothing here is a gate.

    python scripts/bench_train_unrolled.py --steps 10 --warmup 3
    python scripts/bench_train_unrolled.py --unroll 1 --configs chain      # (runs on a tree without unrolled_forward too)
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from molecular_dynamics_neural_operator_amd import ops, synthetic as syn, training  # noqa: E402
from molecular_dynamics_neural_operator_amd.dataset import PairData  # noqa: E402
from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN, LpLoss  # noqa: E402

CONFIGS = {"chain": dict(atoms=28, batch=128, mode="materialized"), "dense": dict(atoms=504, batch=1, mode="factored")}

ap = argparse.ArgumentParser()
ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
ap.add_argument("--unroll", type=int, nargs="+", default=[1, 2, 4])
ap.add_argument("--detach", action="store_true", help="cut the gradient at the fed-back frames (pushforward)")
ap.add_argument("--kernel-width", type=int, default=1024)
ap.add_argument("--depth", type=int, default=6)
ap.add_argument("--window", type=int, default=10)
ap.add_argument("--gemm-mode", default="split_f16", choices=["split_f16", "split_bf16", "f32"])
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--kernel-edges", type=int, default=60588, help="0: skip the stand-alone kernel timing")
a = ap.parse_args()
dev = torch.device("cuda:0")
unrolled_forward = getattr(training, "unrolled_forward", None)


def sample(atoms, seed, steps):
    base = syn.chain_frame(atoms, seed=seed) if atoms <= 64 else syn.box_frame(atoms, 0.1, seed=seed)
    win = torch.from_numpy(syn.jitter_window(base, a.window, seed=seed)).to(dev)
    g = ops.radius_graph(win[-1].contiguous(), atoms, 8.0)
    ei = g.to_edge_index()
    ea = torch.cat([win[-1][ei[0]], win[-1][ei[1]]], dim=1)
    gen = torch.Generator(dev).manual_seed(seed)
    ys = win[-1][None] + 0.05 * torch.randn(steps, atoms, 3, device=dev, generator=gen)
    s = PairData(torch.from_numpy(syn.amino_acids(atoms, seed=seed)).to(dev), win, ys[0].contiguous(), ea, ei)
    return s, ys


def timed(fn, warmup, steps):
    times = []
    for it in range(warmup + steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            times.append(t0.elapsed_time(t1))
    return times


loss_fn = LpLoss(size_average=False)
for name in a.configs:
    cfg = CONFIGS[name]
    B, K_max = cfg["batch"], max(a.unroll)
    pairs = [sample(cfg["atoms"], s, K_max) for s in range(B)]
    batch = training.collate([p[0] for p in pairs])
    y_all = torch.cat([p[1] for p in pairs], dim=1).contiguous()          # [K_max, B*N, 3]
    torch.manual_seed(0)
    model = KernelNN(64, a.kernel_width, a.depth, 6, 7, 3, 20, 4)
    with torch.no_grad():
        for p_ in model.conv1.net.layers[4].parameters():
            p_.mul_(0.05)
    model.to(dev).train()
    model.gemm_mode, model.train_precision, model.train_conv_mode = a.gemm_mode, "fp32", cfg["mode"]
    opt = training.Adam(model.parameters(), lr=1e-5)
    for K in a.unroll:
        def step():
            opt.zero_grad()
            if K == 1:
                outs = [training.train_forward(model, batch)]
            else:
                outs, _ = unrolled_forward(model, batch, K, detach=a.detach)
            loss = loss_fn(outs[0].view(B, -1), y_all[0].view(B, -1))
            for k in range(1, K):
                loss = loss + loss_fn(outs[k].view(B, -1), y_all[k].view(B, -1))
            (loss / K).backward()
            opt.step()
        if K > 1 and unrolled_forward is None:
            continue
        torch.cuda.reset_peak_memory_stats()
        times = timed(step, a.warmup, a.steps)
        print(json.dumps(dict(what="train_step", config=name, atoms=cfg["atoms"], batch=B, k=a.kernel_width, depth=a.depth,
                              mode=cfg["mode"], gemm_mode=a.gemm_mode, unroll=K, detach=bool(a.detach and K > 1),
                              edges_step1=int(batch.edge_index.shape[1]), ms_per_step=float(np.median(times)),
                              ms_min=min(times), ms_max=max(times), peak_mib=torch.cuda.max_memory_allocated() / 2 ** 20)),
              flush=True)
    del model, opt, batch

if a.kernel_edges and hasattr(ops, "edge_mlp_input_bwd"):
    E, k = a.kernel_edges, a.kernel_width
    # four inputs in turn (1 GB at the default size): no call finds its 248 MB in the 256 MiB Infinity Cache
    bufs = [torch.randn(E, k, device=dev) for _ in range(4)]
    w0 = torch.randn(k, 6, device=dev)
    ne = torch.tensor([E], dtype=torch.int32, device=dev)
    out = torch.empty(E, 6, device=dev)
    turn = [0]

    def call():
        ops.edge_mlp_input_bwd(bufs[turn[0] % 4], w0, ne, out=out)
        turn[0] += 1
    times = timed(call, 8, 40)
    ms = float(np.median(times))
    nbytes = E * k * 4
    print(json.dumps(dict(what="mdno_edge_mlp_input_bwd", edges=E, k=k, ker_in=6, ms=ms, ms_min=min(times), ms_max=max(times),
                          bytes_read=nbytes, tb_per_s=nbytes / (ms * 1e-3) / 1e12,
                          fraction_of_8_tb_per_s=nbytes / (ms * 1e-3) / 8e12)), flush=True)
