"""Time the dynamical-scoring entry points (csrc/dynamics.hip) against the torch composition of the same statistics on the
same device: displacement statistics (sum2, sum4 and the 64-bin histogram), the velocity autocorrelation and unwrapping of
a synthetic random walk f32 [S, M, N, 3] at the default lags, HIP events after a warm-up.  The yardstick forms every lag
on its own in fp64 (differences, squares, a masked bincount per lag for the histogram), which is how one would write it
without the kernels; where it runs out of memory the line says so.  Prints ONE JSON line per M.

    python scripts/bench_dynamics.py [--steps 1000] [--members 8 64] [--atoms 504] [--bins 64] [--r-max 4.0] [--reps 5]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def timed(fn, reps):
    """(best ms over `reps` after one warm-up, the last result)."""
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return min(ms), out


def torch_displacement_stats(x, lags, r_max, n_bins):
    """The composition: per lag, fp64 differences over all origins, their squares, and a masked bincount."""
    S, M, N, _ = x.shape
    sum2 = torch.empty((M, len(lags)), dtype=torch.float64, device=x.device)
    sum4 = torch.empty_like(sum2)
    counts = torch.empty((M, len(lags), n_bins), dtype=torch.int64, device=x.device)
    inv_dr = n_bins / r_max
    member = (torch.arange(M, device=x.device) * n_bins)[None, :, None]
    for l, tau in enumerate(lags):
        d = x[tau:].double() - x[:S - tau].double()
        s = (d * d).sum(-1)                                                  # [origins, M, N]
        sum2[:, l] = s.sum((0, 2))
        sum4[:, l] = (s * s).sum((0, 2))
        r = s.sqrt()
        b = (r * inv_dr).long().clamp_max(n_bins - 1) + member
        counts[:, l] = torch.bincount(b[r < r_max], minlength=M * n_bins).reshape(M, n_bins)
    return sum2, sum4, counts


def torch_velocity_autocorrelation(x, lags):
    S, M = x.shape[:2]
    v = x[1:].double() - x[:-1].double()
    corr = torch.empty((M, len(lags)), dtype=torch.float64, device=x.device)
    for l, tau in enumerate(lags):
        corr[:, l] = (v[:S - 1 - tau] * v[tau:]).sum((0, 2, 3))
    return corr


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--members", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--atoms", type=int, default=504)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--r-max", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()

    from molecular_dynamics_neural_operator_amd import forecast, ops

    if not torch.cuda.is_available():
        raise SystemExit("bench_dynamics.py needs a GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    S, N = a.steps, a.atoms
    lags = forecast.default_lags(S)
    vlags = forecast.default_lags(S, 1)
    for M in a.members:
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.rand((1, M, N, 3), generator=g, device=dev, dtype=torch.float64) * 17.1
        x = (x + torch.cumsum(torch.randn((S, M, N, 3), generator=g, device=dev, dtype=torch.float64) * 0.3, 0)).float()
        samples = sum(ops.n_origins(S, t) for t in lags) * M * N
        res = {"steps": S, "members": M, "atoms": N, "lags": len(lags), "bins": a.bins, "samples": samples}
        ms, out = timed(lambda: ops.displacement_stats(x, lags, 1, False, a.r_max, a.bins), a.reps)
        res["displacement_stats_ms"] = ms
        res["samples_per_s"] = samples / (ms * 1e-3)
        res["displacement_stats_remove_com_ms"] = timed(lambda: ops.displacement_stats(x, lags, 1, True, a.r_max, a.bins), a.reps)[0]
        res["displacement_stats_no_histogram_ms"] = timed(lambda: ops.displacement_stats(x, lags), a.reps)[0]
        vms, vout = timed(lambda: ops.velocity_autocorrelation(x, vlags), a.reps)
        res["velocity_autocorrelation_ms"] = vms
        res["unwrap_ms"] = timed(lambda: ops.unwrap_frames(x, (17.1, 17.1, 17.1)), a.reps)[0]
        try:
            tms, ref = timed(lambda: torch_displacement_stats(x, lags, a.r_max, a.bins), a.reps)
            res["torch_displacement_stats_ms"] = tms
            res["torch_over_kernel"] = tms / ms
            res["counts_equal"] = bool(torch.equal(ref[2], out[2]))
            res["sum2_max_rel_diff"] = float(((ref[0] - out[0]).abs() / ref[0].abs().clamp_min(1e-300)).max())
            del ref
        except torch.cuda.OutOfMemoryError:
            res["torch_displacement_stats_ms"] = "out of memory"
        torch.cuda.empty_cache()
        try:
            tms, ref = timed(lambda: torch_velocity_autocorrelation(x, vlags), a.reps)
            res["torch_velocity_autocorrelation_ms"] = tms
            res["torch_over_kernel_vacf"] = tms / vms
            res["corr_max_rel_diff"] = float(((ref - vout).abs() / ref.abs().clamp_min(1e-300)).max())
            del ref
        except torch.cuda.OutOfMemoryError:
            res["torch_velocity_autocorrelation_ms"] = "out of memory"
        res["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated())
        print(json.dumps(res), flush=True)
        del x, out, vout
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()


if __name__ == "__main__":
    main()
