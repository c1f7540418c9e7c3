"""Time the internal-coordinate featuriser (ops.internal_features, csrc/internal.hip) against the same features composed
from torch gathers in fp64 on the same device.  Shapes: 1,000 steps x 504 atoms at 8 and at 64 members with
Featurizer.backbone(504, 3, 4), and 1,000 steps x 64 members x 28 atoms with the full backbone set.  Per shape ONE JSON line:
the median of `--calls` calls of each (HIP events around one call, after `--warmup` calls of that shape), the achieved
bytes/s of the kernel against what it must move — the frames in plus the features out, computed from the shapes —, the ratio
to the torch composition, the peak of the torch composition's temporaries (torch.cuda.max_memory_allocated above what was
held before the call) and the largest difference between the two results.  The column histogram of the same matrix is
timed beside them.

    python scripts/bench_internal.py [--calls 50] [--warmup 3] [--steps 1000]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def torch_features(frames, ft):
    """The rule of include/mdno_internal.h composed from torch operations in fp64 (not its bits: torch sums in its own
    order) -> f32 [F, D]."""
    x = frames.to(torch.float64)
    bond = lambda a, b: x[:, b.long()] - x[:, a.long()]
    p, t, q = ft.pairs, ft.triples, ft.quads
    cols = [bond(p[:, 0], p[:, 1]).norm(dim=-1)]
    u, w = bond(t[:, 1], t[:, 0]), bond(t[:, 1], t[:, 2])
    cols.append(((u * w).sum(-1) / (u.norm(dim=-1) * w.norm(dim=-1))).clamp(-1.0, 1.0))
    b1, b2, b3 = bond(q[:, 0], q[:, 1]), bond(q[:, 1], q[:, 2]), bond(q[:, 2], q[:, 3])
    n1, n2 = torch.linalg.cross(b1, b2), torch.linalg.cross(b2, b3)
    xx, yy = (n1 * n2).sum(-1), b2.norm(dim=-1) * (b1 * n2).sum(-1)
    h = torch.sqrt(xx * xx + yy * yy)
    cols.append(torch.stack([(xx / h).clamp(-1.0, 1.0), (yy / h).clamp(-1.0, 1.0)], -1).reshape(x.shape[0], -1))
    return torch.cat(cols, 1).to(torch.float32)


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_internal.py needs a GPU (there is no CPU path)")
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    dev = torch.device("cuda:0")
    for members, atoms, (min_sep, stride) in ((8, 504, (3, 4)), (64, 504, (3, 4)), (64, 28, (3, 1))):
        base = syn.box_frame(atoms, seed=1) if atoms > 128 else syn.chain_frame(atoms, seed=1)
        traj = torch.from_numpy(syn.ou_trajectory(base, a.steps, seed=2)).to(dev)                  # [S, N, 3]
        frames = (traj[:, None] + 0.05 * torch.randn(a.steps, members, atoms, 3, device=dev, generator=torch.Generator(dev).manual_seed(3)))
        frames = frames.to(torch.float32).contiguous()
        flat = frames.reshape(-1, atoms, 3)
        ft = forecast.Featurizer.backbone(atoms, min_sep, stride).to(dev)
        F, D = flat.shape[0], ft.dim()
        moved = F * atoms * 12 + F * D * 4
        out = {}
        k_ms = timed(lambda: out.__setitem__("k", forecast.internal_coordinates(frames, ft)), a.calls, a.warmup)
        g_ms = timed(lambda: out.__setitem__("g", ops.internal_features(flat, ft.pairs, ft.triples, ft.quads, form="global")), a.calls, a.warmup)
        lo, hi = forecast.feature_ranges(out["k"])
        h_ms = timed(lambda: forecast.feature_histograms(out["k"], lo, hi, 32), min(a.calls, 10), 1)   # (host-bound: D / 128 launches)
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t_ms = timed(lambda: out.__setitem__("t", torch_features(flat, ft)), a.calls, a.warmup)
        peak = torch.cuda.max_memory_allocated() - held
        diff = float((out["k"].reshape(F, D).double() - out["t"].double()).abs().max())
        same = bool(torch.equal(out["k"].reshape(F, D).view(torch.int32), out["g"].view(torch.int32)))
        print(json.dumps({
            "members": members, "atoms": atoms, "steps": a.steps, "frames": F, "features": D, "min_separation": min_sep, "stride": stride,
            "calls": a.calls, "kernel_ms_median": k_ms[0], "kernel_ms_min_max": k_ms[1:], "kernel_global_form_ms_median": g_ms[0],
            "forms_bit_equal": same, "bytes_moved": moved, "kernel_bytes_per_s": moved / (k_ms[0] * 1e-3),
            "torch_fp64_ms_median": t_ms[0], "torch_fp64_ms_min_max": t_ms[1:], "torch_over_kernel": t_ms[0] / k_ms[0],
            "torch_peak_temporaries_bytes": peak, "output_bytes": F * D * 4, "max_abs_difference": diff,
            "histogram_32_bins_ms_median": h_ms[0]}), flush=True)
        del out, frames, flat, traj
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
