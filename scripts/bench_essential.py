"""Time the essential-dynamics entry points (csrc/essential.hip) against the torch composition of the same statistics on the
same device: superposition of a synthetic run f32 [S, M, N, 3] onto one reference, the column sums, the 3 N x 3 N covariance
sums at lag 0 and the projection onto k = 10 directions; HIP events after warm-up calls.  The yardstick is how one would
write it without the kernels, in fp64: centred frames, a batched 3 x 3 covariance against the reference, Horn's 4 x 4 matrix,
torch.linalg.eigh, the quaternion's rotation; then the fp64 copy of the aligned frames, its mean, (X - mean)^T (X - mean) and
(X - mean) V — with its peak temporaries.  Prints ONE JSON line per M: the median, minimum and maximum of the repetitions per
stage, and the fp64 TFLOP/s the covariance's median implies against 2 K D^2 flop (the full product; at lag 0 the kernel
computes the upper tiles only, so its own arithmetic is about half of that) — to be read beside the 77.4 TFLOP/s issue loop
of scripts/micro/mfma_f64_issue.hip.

    python scripts/bench_essential.py [--steps 1000] [--members 8 64] [--atoms 504] [--components 10] [--reps 50] [--warmup 3]
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


def spread_of(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def torch_superpose(x, q):
    """The composition in fp64: aligned f32 [S, M, N, 3]."""
    a = x.double()
    a = a - a.mean(2, keepdim=True)
    cq = q.double().mean(0)
    b = q.double() - cq
    c = torch.einsum("smkr,kc->smrc", a, b)
    K = torch.empty(c.shape[:2] + (4, 4), dtype=torch.float64, device=x.device)
    xx, xy, xz, yx, yy, yz, zx, zy, zz = (c[..., r, s] for r in range(3) for s in range(3))
    K[..., 0, 0], K[..., 1, 1], K[..., 2, 2], K[..., 3, 3] = xx + yy + zz, xx - yy - zz, yy - xx - zz, zz - xx - yy
    K[..., 0, 1] = K[..., 1, 0] = yz - zy
    K[..., 0, 2] = K[..., 2, 0] = zx - xz
    K[..., 0, 3] = K[..., 3, 0] = xy - yx
    K[..., 1, 2] = K[..., 2, 1] = xy + yx
    K[..., 1, 3] = K[..., 3, 1] = zx + xz
    K[..., 2, 3] = K[..., 3, 2] = yz + zy
    v = torch.linalg.eigh(K)[1][..., -1]
    q0, q1, q2, q3 = v.unbind(-1)
    R = torch.stack([q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2),
                     2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1),
                     2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3], -1).reshape(c.shape[:2] + (3, 3))
    return (torch.einsum("smij,smkj->smki", R, a) + cq).float()


def torch_covariance(x):
    """The composition in fp64 on aligned frames f32 [S, M, N, 3]: (mean [D], sums [D, D], the centred fp64 copy)."""
    X = x.reshape(x.shape[0] * x.shape[1], -1).double()
    mean = X.mean(0)
    X = X - mean
    return mean, X.transpose(0, 1) @ X, X


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--members", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--atoms", type=int, default=504)
    ap.add_argument("--components", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="time the kernels only")
    a = ap.parse_args()

    from molecular_dynamics_neural_operator_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("bench_essential.py needs a GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    S, N, k = a.steps, a.atoms, a.components
    D = 3 * N
    for M in a.members:
        g = torch.Generator(device=dev).manual_seed(1)
        q = (torch.rand((N, 3), generator=g, device=dev, dtype=torch.float64) * 17.1).float()
        x = (q.double() + torch.randn((S, M, N, 3), generator=g, device=dev, dtype=torch.float64) * 0.5).float()
        V = torch.linalg.qr(torch.randn((D, k), generator=g, device=dev, dtype=torch.float64))[0].contiguous()
        rows = S * M
        res = {"steps": S, "members": M, "atoms": N, "features": D, "rows": rows, "components": k,
               "fp64_copy_bytes": rows * D * 8, "row_split": list(ops.covariance_row_split(rows, D, 0)),
               "workspace_bytes": int(ops._lib.load().mdnopca_covariance_workspace_bytes(S, M, D, 0))}
        ms, (aligned, rmsd) = timed(lambda: ops.superpose_frames(x, q), a.reps, a.warmup)
        res["superpose"] = spread_of(ms)
        flat = aligned.reshape(rows, D)
        ms, (total, bad) = timed(lambda: ops.feature_sums(flat), a.reps, a.warmup)
        res["feature_sums"] = spread_of(ms)
        mean = total / float(rows)
        ms, sums = timed(lambda: ops.feature_covariance(aligned.reshape(S, M, D), mean, 0), a.reps, a.warmup)
        res["covariance"] = spread_of(ms)
        res["covariance"]["fp64_tflops_full_product"] = 2.0 * rows * D * D / (statistics.median(ms) * 1e-3) / 1e12
        ms, lagged = timed(lambda: ops.feature_covariance(aligned.reshape(S, M, D), mean, 10), a.reps, a.warmup)
        res["covariance_lag_10"] = spread_of(ms)
        res["covariance_lag_10"]["fp64_tflops"] = 2.0 * M * (S - 10) * D * D / (statistics.median(ms) * 1e-3) / 1e12
        ms, P = timed(lambda: ops.project_features(flat, mean, V), a.reps, a.warmup)
        res["project"] = spread_of(ms)
        res["total_median_ms"] = sum(res[s]["median_ms"] for s in ("superpose", "feature_sums", "covariance", "project"))
        del lagged
        torch.cuda.empty_cache()
        if not a.skip_torch:
            torch.cuda.reset_peak_memory_stats()
            before = int(torch.cuda.memory_allocated())
            try:
                tms, t_al = timed(lambda: torch_superpose(x, q), a.torch_reps, 1)
                res["torch_superpose"] = spread_of(tms)
                res["aligned_max_abs_diff"] = float((t_al - aligned).abs().max())
                del t_al
                tms, (t_mean, t_sums, Xc) = timed(lambda: torch_covariance(aligned), a.torch_reps, 1)
                res["torch_mean_and_covariance"] = spread_of(tms)
                res["covariance_max_rel_diff"] = float((t_sums - sums).abs().max() / sums.abs().max())
                tms, t_P = timed(lambda: Xc @ V, a.torch_reps, 1)
                res["torch_project"] = spread_of(tms)
                res["project_max_abs_diff"] = float((t_P - P).abs().max())
                res["torch_total_median_ms"] = sum(res[s]["median_ms"] for s in ("torch_superpose", "torch_mean_and_covariance", "torch_project"))
                res["torch_over_kernels"] = res["torch_total_median_ms"] / res["total_median_ms"]
                del t_mean, t_sums, Xc, t_P
            except torch.cuda.OutOfMemoryError:
                res["torch_composition"] = "out of memory"
            res["torch_peak_temporary_bytes"] = int(torch.cuda.max_memory_allocated()) - before
        print(json.dumps(res), flush=True)
        del x, aligned, flat, sums, P
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
