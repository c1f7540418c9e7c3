"""Time the Markov-model entry points (csrc/markov.hip) against the torch composition of the same statistics on the same
device, in fp64: nearest-centre assignment of a synthetic run's S x M feature rows (torch.cdist + argmin over chunks of rows),
10 Lloyd rounds (assignment, then index_add_ and bincount), k-centres seeding for k = 100 (a loop of direct distances and
argmax, no read-back) and the pooled transition counts at 29 lags (bincount of from * n + to); HIP events after warm-up calls,
medians of --reps calls (a stage that takes longer than --budget seconds for all its repetitions is repeated less often; the
JSON says how often).  Prints ONE JSON line per (M, D, k): the median, minimum and maximum per stage, the fp64 TFLOP/s the
assignment's median implies against 2 R k D flop and that as a fraction of the 77.4 TFLOP/s issue loop of
scripts/micro/mfma_f64_issue.hip, the kernels' workspace and the torch composition's peak temporaries.

    python scripts/bench_markov.py [--steps 1000] [--members 8 64] [--shapes 10x100 1512x100 1512x1000] [--reps 50]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

ISSUE_LOOP_TFLOPS = 77.4
CHUNK = 8192


def timed(fn, reps, warmup, budget):
    """(ms of every repetition after `warmup` calls, the last result); fewer repetitions (at least 3) where `reps` of them
    would take longer than `budget` seconds."""
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    once = time.perf_counter() - t0
    reps = max(3, min(reps, int(budget / max(once, 1e-6))))
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
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def torch_assign(x, c):
    cd = c.double()
    labels, dist2 = [], []
    for r0 in range(0, x.shape[0], CHUNK):
        d = torch.cdist(x[r0:r0 + CHUNK].double(), cd)
        v, i = d.min(1)
        labels.append(i)
        dist2.append(v * v)
    return torch.cat(labels), torch.cat(dist2)


def torch_lloyd(x, c, rounds):
    k, D = c.shape
    for _ in range(rounds):
        labels, _ = torch_assign(x, c)
        sums = torch.zeros((k, D), dtype=torch.float64, device=x.device)
        for r0 in range(0, x.shape[0], CHUNK):
            sums.index_add_(0, labels[r0:r0 + CHUNK], x[r0:r0 + CHUNK].double())
        counts = torch.bincount(labels, minlength=k)
        c = torch.where((counts > 0)[:, None], sums / counts[:, None], c.double()).to(x.dtype)
    return c


def torch_kcenters(x, k):
    xd = x.double()
    mind2 = torch.full((x.shape[0],), float("inf"), dtype=torch.float64, device=x.device)
    index = [torch.zeros((), dtype=torch.int64, device=x.device)]
    for _ in range(1, k):
        mind2 = torch.minimum(mind2, (xd - xd[index[-1]]).square_().sum(1))
        index.append(mind2.argmax())
    return torch.stack(index)


def torch_counts(labels, n, lags):
    S = labels.shape[0]
    out = []
    for lag in lags:
        a, b = labels[:S - lag].reshape(-1).long(), labels[lag:].reshape(-1).long()
        ok = (a >= 0) & (a < n) & (b >= 0) & (b < n)
        out.append(torch.bincount((a * n + b)[ok], minlength=n * n).reshape(n, n))
    return torch.stack(out)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--members", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--shapes", nargs="+", default=["10x100", "1512x100", "1512x1000"], help="D x k")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--budget", type=float, default=4.0, help="seconds per stage")
    ap.add_argument("--lloyd-rounds", type=int, default=10)
    ap.add_argument("--seed-centres", type=int, default=100)
    ap.add_argument("--lags", type=int, default=29)
    ap.add_argument("--skip-torch", action="store_true", help="time the kernels only")
    a = ap.parse_args()

    from molecular_dynamics_neural_operator_amd import forecast, ops

    if not torch.cuda.is_available():
        raise SystemExit("bench_markov.py needs a GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    lib = ops._lib.load()
    S = a.steps
    lags = list(range(1, a.lags + 1))
    for M in a.members:
        for shape in a.shapes:
            D, k = (int(v) for v in shape.split("x"))
            R = S * M
            g = torch.Generator(device=dev).manual_seed(1)
            base = torch.randn((k, D), generator=g, device=dev) * 3.0
            x = (base[torch.randint(0, k, (R,), generator=g, device=dev)] + torch.randn((R, D), generator=g, device=dev)).contiguous()
            c = (base + 0.1 * torch.randn((k, D), generator=g, device=dev)).contiguous()
            origin = c.double().mean(0)
            kc = min(a.seed_centres, k)
            res = {"steps": S, "members": M, "rows": R, "features": D, "states": k,
                   "assign_workspace_bytes": int(lib.mdnomsm_assign_workspace_bytes(R, k, D)),
                   "distance_matrix_bytes": R * k * 8, "fp64_copy_bytes": R * D * 8}
            ms, (labels, dist2) = timed(lambda: ops.assign_features(x, c, origin), a.reps, a.warmup, a.budget)
            res["assign"] = spread_of(ms)
            tf = 2.0 * R * k * D / (statistics.median(ms) * 1e-3) / 1e12
            res["assign"]["fp64_tflops"] = tf
            res["assign"]["fraction_of_issue_loop"] = tf / ISSUE_LOOP_TFLOPS
            ms, _ = timed(lambda: ops.centroid_sums(x, labels, k), a.reps, a.warmup, a.budget)
            res["centroid_sums"] = spread_of(ms)
            ms, _ = timed(lambda: forecast.kmeans(x, k, iters=a.lloyd_rounds, init=c), a.reps, 1, a.budget)
            res[f"lloyd_{a.lloyd_rounds}_rounds"] = spread_of(ms)
            ms, (index, radius) = timed(lambda: ops.kcenters(x, kc, 0), a.reps, 1, a.budget)
            res[f"kcenters_{kc}"] = spread_of(ms)
            steps = labels.reshape(S, M)
            ms, (counts, skipped) = timed(lambda: ops.transition_counts(steps, k, lags, pooled=True), a.reps, a.warmup, a.budget)
            res[f"counts_{len(lags)}_lags"] = spread_of(ms)
            if not a.skip_torch:
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = int(torch.cuda.memory_allocated())
                try:
                    tms, (t_labels, t_d2) = timed(lambda: torch_assign(x, c), a.reps, 1, a.budget)
                    res["torch_assign"] = spread_of(tms)
                    res["labels_differ"] = int((t_labels != labels).sum())
                    res["dist2_max_abs_diff"] = float((t_d2 - dist2).abs().max())
                    tms, _ = timed(lambda: torch_lloyd(x, c, a.lloyd_rounds), a.reps, 1, a.budget)
                    res[f"torch_lloyd_{a.lloyd_rounds}_rounds"] = spread_of(tms)
                    tms, t_index = timed(lambda: torch_kcenters(x, kc), a.reps, 1, a.budget)
                    res[f"torch_kcenters_{kc}"] = spread_of(tms)
                    res["kcenters_index_differ"] = int((t_index != index).sum())
                    tms, t_counts = timed(lambda: torch_counts(steps, k, lags), a.reps, 1, a.budget)
                    res[f"torch_counts_{len(lags)}_lags"] = spread_of(tms)
                    res["counts_differ"] = int((t_counts != counts[:, 0]).sum())
                    del t_labels, t_d2, t_index, t_counts
                except torch.cuda.OutOfMemoryError:
                    res["torch_composition"] = "out of memory"
                res["torch_peak_temporary_bytes"] = int(torch.cuda.max_memory_allocated()) - before
            print(json.dumps(res), flush=True)
            del x, c, labels, dist2, counts
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
