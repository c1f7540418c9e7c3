"""Time the ensemble-verification entry point (csrc/ensemble.hip) against the torch composition of the same statistics on
the same device: the sums behind the error of the ensemble mean, the spread and the CRPS, and the rank histogram, per step
of a synthetic ensemble f32 [S, M, N, 3] against a truth [S, N, 3]; HIP events after warm-up calls.  The yardstick is how
one would write it without the kernel: the members in fp64, a sort over the (strided) member axis for the pair term, a
scatter_add for the histogram.  Prints ONE JSON line per M: the median, minimum and maximum of the repetitions, the
effective bandwidth against the frames' bytes, and whether the two agree.

    python scripts/bench_ensemble.py [--steps 1000] [--members 8 64] [--atoms 504] [--reps 20] [--warmup 3]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def timed(fn, reps, warmup):
    """(ms of every repetition after `warmup` calls, the last result)."""
    for _ in range(warmup):
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
    return ms, out


def torch_ensemble_score(x, y):
    """The composition in fp64: (sums [S, 4], rank_hist [S, M + 1])."""
    S, M, N, _ = x.shape
    d = x.double().reshape(S, M, 3 * N) - y.double().reshape(S, 1, 3 * N)
    mean = d.mean(1)
    var = d.var(1, unbiased=True) if M >= 2 else torch.zeros_like(mean)
    srt = d.sort(1).values
    coef = (2.0 * torch.arange(M, device=x.device, dtype=torch.float64) - (M - 1))[None, :, None]
    sums = torch.stack([(mean * mean).sum(1), var.sum(1), d.abs().sum((1, 2)), (coef * srt).sum((1, 2))], 1)
    rank = (d < 0).sum(1)                                                   # [S, 3 N]
    hist = torch.zeros((S, M + 1), dtype=torch.int64, device=x.device)
    hist.scatter_add_(1, rank, torch.ones_like(rank))
    return sums, hist


def spread_of(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--members", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--atoms", type=int, default=504)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    from molecular_dynamics_neural_operator_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble.py needs a GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    S, N = a.steps, a.atoms
    for M in a.members:
        g = torch.Generator(device=dev).manual_seed(1)
        base = torch.rand((S, 1, N, 3), generator=g, device=dev, dtype=torch.float64) * 17.1
        x = (base + torch.randn((S, M, N, 3), generator=g, device=dev, dtype=torch.float64) * 0.3).float()
        y = (base[:, 0] + torch.randn((S, N, 3), generator=g, device=dev, dtype=torch.float64) * 0.3).float()
        del base
        frame_bytes = x.numel() * 4 + y.numel() * 4
        res = {"steps": S, "members": M, "atoms": N, "samples": S * 3 * N, "frame_bytes": frame_bytes}
        forms = ["auto", "lds"] if M <= ops.MAX_REGISTER_MEMBERS else ["auto"]
        out = None
        for form in forms:
            ms, o = timed(lambda: ops.ensemble_score(x, y, form), a.reps, a.warmup)
            key = "ensemble_score" if form == "auto" else "ensemble_score_lds"
            res[key] = spread_of(ms)
            res[key]["effective_gb_per_s"] = frame_bytes / (statistics.median(ms) * 1e-3) / 1e9
            if form == "auto":
                out = o
            else:
                res["forms_equal"] = all(bool(torch.equal(u, v)) for u, v in zip(out, o))
        torch.cuda.reset_peak_memory_stats()
        try:
            tms, ref = timed(lambda: torch_ensemble_score(x, y), a.reps, a.warmup)
            res["torch_composition"] = spread_of(tms)
            res["torch_over_kernel"] = statistics.median(tms) / res["ensemble_score"]["median_ms"]
            res["rank_hist_equal"] = bool(torch.equal(ref[1], out[1]))
            res["sums_max_rel_diff"] = float(((ref[0] - out[0]).abs() / ref[0].abs().clamp_min(1e-300)).max())
            del ref
        except torch.cuda.OutOfMemoryError:
            res["torch_composition"] = "out of memory"
        res["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated())
        print(json.dumps(res), flush=True)
        del x, y, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
