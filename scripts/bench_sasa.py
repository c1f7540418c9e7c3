"""Time the Shrake-Rupley counts (ops.exposed_points; csrc/surface.hip) against the same counts composed from torch in fp64 on
the same device.  Shapes: 1,000 steps x 8 and x 64 members x 504 atoms at P = 96 and at P = 960 points, and 1,000 steps x 64
members x 28 atoms at P = 96; one radius of 1.9 A plus a probe of 1.4 A for every atom.  Per shape ONE JSON line: the median of
`--calls` calls (HIP events around one call, after `--warmup` calls of that shape) of
    exposed_points in the form "auto" picks (the frame staged in LDS) and in the tiled form;
    exposed_points with a ONE-point table: the neighbour search alone, so the difference is the point tests;
    the counts of that shape per second, and the share of fully buried and fully exposed atoms (what the early exits see);
    the torch composition on the first `--torch-frames` frames — the [frames, N, P, N] tests chunked so that their fp64
    temporaries stay under `--torch-bytes` — its time per frame, that time scaled to all frames, its ratio to the kernel and
    the peak of its temporaries (torch.cuda.max_memory_allocated above what was held before);
and whether the torch counts equal the kernel's on those frames.

    python scripts/bench_sasa.py [--calls 50] [--warmup 3] [--steps 1000] [--torch-frames 32]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def torch_counts(frames, R, U, budget):
    """counts i32 [F, N] by the rule of include/mdno_surface.h from elementwise torch operations in fp64 (each rounded once, in
    the header's order), the [rows, P, N] tests chunked over frames and atoms so that four fp64 temporaries fit `budget` bytes."""
    F, N = frames.shape[:2]
    P = U.shape[0]
    q = R[:, None, None] * U[None]                                   # [N, P, 3]
    reach = R[:, None] + R[None, :]
    r2 = (R * R)[None, None, None, :]
    off = ~torch.eye(N, dtype=torch.bool, device=frames.device)
    rows = max(1, budget // (32 * P * N))
    fc, ic = (rows // N, N) if rows >= N else (1, rows)
    out = torch.empty((F, N), dtype=torch.int32, device=frames.device)
    for f0 in range(0, F, fc):
        x = frames[f0:f0 + fc].to(torch.float64)
        d = x[:, None, :, :] - x[:, :, None, :]                      # [c, i, j, 3]: x_j - x_i
        s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        nb = (s.sqrt() < reach) & off
        for i0 in range(0, N, ic):
            di, t = d[:, i0:i0 + ic], None
            for a in range(3):
                e = q[None, i0:i0 + ic, :, None, a] - di[:, :, None, :, a]          # [c, rows, P, j]
                t = e * e if t is None else t + e * e
            buried = ((t < r2) & nb[:, i0:i0 + ic, None, :]).any(-1)
            out[f0:f0 + fc, i0:i0 + ic] = P - buried.sum(-1, dtype=torch.int32)
    return out


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


def with_peak(fn, calls, warmup):
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = timed(fn, calls, warmup)
    return ms, torch.cuda.max_memory_allocated() - held


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--torch-frames", type=int, default=32, help="frames the torch composition is timed on (it is the slow side)")
    ap.add_argument("--torch-calls", type=int, default=3)
    ap.add_argument("--torch-bytes", type=int, default=4 << 30, help="bound on the torch composition's fp64 temporaries")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sasa.py needs a GPU (there is no CPU path)")
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    dev = torch.device("cuda:0")
    for members, atoms, n_points in ((8, 504, 96), (64, 504, 96), (8, 504, 960), (64, 504, 960), (64, 28, 96)):
        base = syn.box_frame(atoms, seed=1) if atoms > 128 else syn.chain_frame(atoms, seed=1)
        traj = torch.from_numpy(syn.ou_trajectory(base, a.steps, seed=2)).to(dev)                  # [S, N, 3]
        frames = (traj[:, None] + 0.05 * torch.randn(a.steps, members, atoms, 3, device=dev, generator=torch.Generator(dev).manual_seed(3)))
        frames = frames.to(torch.float32).contiguous()
        sp = forecast.Spheres(1.9, probe=1.4, n_points=n_points, n_atoms=atoms).to(dev)
        one = sp.points[:1].contiguous()
        out = {}
        auto_ms = timed(lambda: out.__setitem__("c", ops.exposed_points(frames, sp.R, sp.points, reach=sp.reach)), a.calls, a.warmup)
        tiled_ms = timed(lambda: ops.exposed_points(frames, sp.R, sp.points, reach=sp.reach, form="tiled"), a.calls, a.warmup)
        search_ms = timed(lambda: ops.exposed_points(frames, sp.R, one, reach=sp.reach), a.calls, a.warmup)
        counts = out.pop("c")
        flat = frames.reshape(-1, atoms, 3)
        tf = min(a.torch_frames, flat.shape[0])
        (t_ms, t_peak) = with_peak(lambda: out.__setitem__("t", torch_counts(flat[:tf], sp.R, sp.points, a.torch_bytes)), a.torch_calls, 1)
        equal = bool(torch.equal(out.pop("t"), counts.reshape(-1, atoms)[:tf]))
        n_frames = flat.shape[0]
        neighbours = (ops.contact_maps(flat[:tf], sp.reach).sum((-1, -2)).double().mean().item() / atoms) - 1.0
        print(json.dumps({
            "members": members, "atoms": atoms, "steps": a.steps, "points": n_points, "frames": n_frames, "calls": a.calls,
            "exposed_points_ms_median": auto_ms[0], "exposed_points_ms_min_max": auto_ms[1:],
            "exposed_points_tiled_form_ms_median": tiled_ms[0], "exposed_points_tiled_form_ms_min_max": tiled_ms[1:],
            "neighbour_search_alone_ms_median": search_ms[0],
            "atom_counts_per_s": n_frames * atoms / (auto_ms[0] * 1e-3),
            "mean_neighbours_per_atom": neighbours,
            "share_fully_buried": float((counts == 0).double().mean()), "share_fully_exposed": float((counts == n_points).double().mean()),
            "mean_exposed_fraction": float(counts.double().mean() / n_points),
            "torch_frames": tf, "torch_fp64_ms_median": t_ms[0], "torch_fp64_ms_per_frame": t_ms[0] / tf,
            "torch_fp64_ms_scaled_to_all_frames": t_ms[0] / tf * n_frames,
            "torch_over_exposed_points": (t_ms[0] / tf * n_frames) / auto_ms[0],
            "torch_fp64_peak_temporaries_bytes": t_peak, "torch_counts_equal": equal}), flush=True)
        del out, frames, traj, counts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
