"""Time the structural-coverage entry point (csrc/conformations.hip) against the torch composition of the same statistics on
the same device: the superposed RMSD of every frame of a synthetic run f32 [S, M, N, 3] against every one of Fb reference
frames, the nearest reference frame per frame and the nearest frame per member and reference frame; HIP events after
warm-up calls.  Two modes: matrix=False (the minima only) and with the f64 [S, M, Fb] matrix (8 S M Fb bytes: 512 MB at 64
members x 1,000 steps x 1,000 frames).  The yardstick is how one would write it without the kernel: centred frames in fp64,
a batched 3 x 3 covariance per pair (einsum), Horn's 4 x 4 matrix, torch.linalg.eigvalsh, min over rows and columns — over
chunks of steps, since the temporaries of all pairs at once (200 B per pair and more) do not fit.  Where the composition
would take too long it is timed on the first --torch-steps steps and scaled to S (it is linear in the pairs); the line says
so.  Prints ONE JSON line per M: the median, minimum and maximum of the repetitions, the fp64 TFLOP/s the median implies
against 18 N flop per pair (the nine sums alone), and the agreement of the two.

    python scripts/bench_cross_rmsd.py [--steps 1000] [--members 8 64] [--atoms 504] [--reference 1000] [--reps 50] [--warmup 3]
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


def torch_cross_rmsd(x, y, pairs_per_chunk=1 << 21):
    """The composition in fp64: (nearest [S, M], nearest_index, cover [M, Fb], cover_step), over chunks of steps."""
    S, M, N, _ = x.shape
    Fb = y.shape[0]
    b = y.double()
    b = b - b.mean(1, keepdim=True)
    gb = (b * b).sum((1, 2))
    near, near_i, cov, cov_s = [], [], None, None
    rows = max(1, pairs_per_chunk // max(1, M * Fb))
    for s0 in range(0, S, rows):
        a = x[s0:s0 + rows].double()
        a = a - a.mean(2, keepdim=True)
        ga = (a * a).sum((2, 3))
        c = torch.einsum("smkr,jkc->smjrc", a, b)
        K = torch.empty(c.shape[:3] + (4, 4), dtype=torch.float64, device=x.device)
        xx, xy, xz, yx, yy, yz, zx, zy, zz = (c[..., r, q] for r in range(3) for q in range(3))
        K[..., 0, 0], K[..., 1, 1], K[..., 2, 2], K[..., 3, 3] = xx + yy + zz, xx - yy - zz, yy - xx - zz, zz - xx - yy
        K[..., 0, 1] = K[..., 1, 0] = yz - zy
        K[..., 0, 2] = K[..., 2, 0] = zx - xz
        K[..., 0, 3] = K[..., 3, 0] = xy - yx
        K[..., 1, 2] = K[..., 2, 1] = xy + yx
        K[..., 1, 3] = K[..., 3, 1] = zx + xz
        K[..., 2, 3] = K[..., 3, 2] = yz + zy
        lam = torch.linalg.eigvalsh(K)[..., -1]
        r = (((ga[:, :, None] + gb[None, None, :]) - 2.0 * lam).clamp_min(0.0) / N).sqrt()
        v, i = r.min(2)
        near.append(v)
        near_i.append(i)
        cv, cs = r.min(0)
        cs = cs + s0
        if cov is None:
            cov, cov_s = cv, cs
        else:
            better = cv < cov
            cov, cov_s = torch.where(better, cv, cov), torch.where(better, cs, cov_s)
    return torch.cat(near), torch.cat(near_i), cov, cov_s


def spread_of(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--members", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--atoms", type=int, default=504)
    ap.add_argument("--reference", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=0, help="time the composition on this many steps and scale (0: all)")
    ap.add_argument("--skip-torch", action="store_true", help="time the kernel only")
    a = ap.parse_args()

    from molecular_dynamics_neural_operator_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("bench_cross_rmsd.py needs a GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    S, N, Fb = a.steps, a.atoms, a.reference
    for M in a.members:
        g = torch.Generator(device=dev).manual_seed(1)
        base = torch.rand((1, N, 3), generator=g, device=dev, dtype=torch.float64) * 17.1
        y = (base + torch.randn((Fb, N, 3), generator=g, device=dev, dtype=torch.float64) * 1.0).float()
        x = (y.double()[torch.randint(Fb, (S, M), generator=g, device=dev)] +
             torch.randn((S, M, N, 3), generator=g, device=dev, dtype=torch.float64) * 0.3).float()
        del base
        pairs = S * M * Fb
        res = {"steps": S, "members": M, "atoms": N, "reference": Fb, "pairs": pairs, "matrix_bytes": pairs * 8,
               "workspace_bytes": int(ops._lib.load().mdnoconf_cross_rmsd_workspace_bytes(S, M, N, Fb, 1))}
        out = None
        for key, want_matrix in (("cross_rmsd_minima", False), ("cross_rmsd_with_matrix", True)):
            ms, o = timed(lambda: ops.cross_rmsd(x, y, matrix=want_matrix), a.reps, a.warmup)
            res[key] = spread_of(ms)
            res[key]["fp64_tflops"] = 18.0 * N * pairs / (statistics.median(ms) * 1e-3) / 1e12
            if not want_matrix:
                out = [t.clone() for t in o[1:]]
            else:
                res["minima_equal_in_both_modes"] = all(bool(torch.equal(u.view(torch.int64), v.view(torch.int64)))
                                                        for u, v in zip(out, o[1:]))
            del o
        torch.cuda.empty_cache()
        if not a.skip_torch:
            torch.cuda.reset_peak_memory_stats()
            before = int(torch.cuda.memory_allocated())
            ts = a.torch_steps if 0 < a.torch_steps < S else S
            try:
                tms, ref = timed(lambda: torch_cross_rmsd(x[:ts], y), a.torch_reps, 1)
                scaled = statistics.median(tms) * S / ts
                res["torch_composition"] = dict(spread_of(tms), timed_steps=ts, median_ms_scaled_to_all_steps=scaled)
                res["torch_over_kernel"] = scaled / res["cross_rmsd_minima"]["median_ms"]
                res["nearest_index_agreement"] = float((ref[1] == out[1][:ts]).double().mean())
                res["nearest_max_abs_diff"] = float((ref[0] - out[0][:ts]).abs().max())
                del ref
            except torch.cuda.OutOfMemoryError:
                res["torch_composition"] = "out of memory"
            res["torch_peak_temporary_bytes"] = int(torch.cuda.max_memory_allocated()) - before
        print(json.dumps(res), flush=True)
        del x, y, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
