"""Time the pair-distance histogram and the radius of gyration on the device (HIP events; warm-up, repeats, median and
range) beside `score_forecast` on the same frames, which walks the same pairs without binning them.  Prints ONE JSON line.

    python scripts/bench_observe.py [--members 64] [--steps 100] [--atoms 504] [--big 50000] [--reps 10]

Frames: jittered copies of synthetic.periodic_box_frame (a liquid-like box of side ~17.1 A at 504 atoms), scored open and
in their box; one frame of --big atoms (synthetic.box_frame) in the tiled form.  An experimental build of the library
(scripts/micro/build_exp.sh) is timed by pointing MDNO_LIB at it."""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--atoms", type=int, default=504)
    ap.add_argument("--big", type=int, default=50000, help="atoms of the single large frame (0: skip)")
    ap.add_argument("--r-max", type=float, default=8.5)
    ap.add_argument("--bins", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()

    from molecular_dynamics_neural_operator_amd import ops, synthetic as syn
    if not torch.cuda.is_available():
        raise SystemExit("bench_observe.py needs a GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    S, M, N = a.steps, a.members, a.atoms
    base, L = syn.periodic_box_frame(N, 0.1, seed=1)
    rng = np.random.default_rng(2)
    frames = torch.from_numpy((base[None, None] + rng.normal(scale=0.3, size=(S, M, N, 3))).astype(np.float32)).to(dev)
    truth = frames[:, 0].contiguous()
    box = (L, L, L)
    r_max = min(a.r_max, L / 2)
    pairs = S * M * N * (N - 1) // 2
    out = {"lib": os.environ.get("MDNO_LIB", "in-tree"), "members": M, "steps": S, "atoms": N, "box": L, "r_max": r_max,
           "bins": a.bins, "pairs": pairs, "reps": a.reps}

    def rate(t, n):
        t["pairs_per_s"] = n / (t["median_ms"] * 1e-3)
        return t

    for name, bx in (("open", None), ("box", box)):
        for form in ("lds", "tiled"):
            out[f"hist_{name}_{form}"] = rate(timed(lambda: ops.pair_histogram(frames, r_max, a.bins, bx, form), a.reps), pairs)
        # the yardstick: the same pairs tested (forecast and truth: two tests per pair, plus mse and rmsd), not binned
        out[f"score_{name}"] = rate(timed(lambda: ops.forecast_score(frames, truth, r_max, box=bx), a.reps), pairs)
        h = ops.pair_histogram(frames, r_max, a.bins, bx)
        out[f"counted_fraction_{name}"] = float(h.sum()) / pairs
        assert torch.equal(h, ops.pair_histogram(frames, r_max, a.bins, bx, "tiled"))
    out["rg"] = timed(lambda: ops.radius_of_gyration(frames), a.reps)
    if a.big:
        big = torch.from_numpy(syn.box_frame(a.big, 0.1, seed=1)[None]).to(dev)
        n_big = a.big * (a.big - 1) // 2
        out["big_atoms"] = a.big
        out["hist_big_tiled"] = rate(timed(lambda: ops.pair_histogram(big, r_max, a.bins, None, "tiled"), a.reps), n_big)
        out["score_big"] = rate(timed(lambda: ops.forecast_score(big[None], big, r_max), max(2, a.reps // 3)), n_big)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
