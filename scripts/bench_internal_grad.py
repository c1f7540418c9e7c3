"""Time the differentiable internal coordinates (forecast.internal_coordinates under autograd: csrc/internal.hip forward,
csrc/internal_grad.hip backward) against the same computation composed from torch gathers in fp64 on the same device.
Shapes: 128 frames x 28 atoms with the full backbone set (a training batch), 8 frames x 504 atoms and `--steps` x 8 frames x
504 atoms with Featurizer.backbone(504, 3, 4).  Per shape ONE JSON line: the median of `--calls` calls (HIP events around one
call, after `--warmup` calls of that shape) of forward + backward of internal_coordinates(x).square().sum(), of the backward
kernel alone and of its global form; the same for the torch composition, with the peak of its temporaries
(torch.cuda.max_memory_allocated above what was held before the call) and the largest difference between the two gradients.
What uneven chains cost: at 504 atoms the backward alone is also timed with Featurizer.backbone(504, 3, 1), where every atom
is a hub (about 500 pairs each), against the stride-4 set, where every fourth atom is one (about 125 pairs, the others about
9 items): time per incidence of each (on at most `--hub-frames` frames: its g has 127,000 columns).

    python scripts/bench_internal_grad.py [--calls 50] [--warmup 3] [--steps 1000] [--hub-frames 256]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def torch_features(x, ft):
    """The default mode of include/mdno_internal.h composed from differentiable torch operations in fp64 (no clamp: the
    backward treats it as the identity) -> f64 [F, D]."""
    x = x.to(torch.float64)
    bond = lambda a, b: x[:, b.long()] - x[:, a.long()]
    p, t, q = ft.pairs, ft.triples, ft.quads
    cols = [bond(p[:, 0], p[:, 1]).norm(dim=-1)]
    u, w = bond(t[:, 1], t[:, 0]), bond(t[:, 1], t[:, 2])
    cols.append((u * w).sum(-1) / (u.norm(dim=-1) * w.norm(dim=-1)))
    b1, b2, b3 = bond(q[:, 0], q[:, 1]), bond(q[:, 1], q[:, 2]), bond(q[:, 2], q[:, 3])
    n1, n2 = torch.linalg.cross(b1, b2), torch.linalg.cross(b2, b3)
    xx, yy = (n1 * n2).sum(-1), b2.norm(dim=-1) * (b1 * n2).sum(-1)
    h = torch.sqrt(xx * xx + yy * yy)
    cols.append(torch.stack([xx / h, yy / h], -1).reshape(x.shape[0], -1))
    return torch.cat(cols, 1)


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
    ap.add_argument("--hub-frames", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_internal_grad.py needs a GPU (there is no CPU path)")
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    dev = torch.device("cuda:0")
    for n_frames, atoms, (min_sep, stride) in ((128, 28, (3, 1)), (8, 504, (3, 4)), (a.steps * 8, 504, (3, 4))):
        base = syn.box_frame(atoms, seed=1) if atoms > 128 else syn.chain_frame(atoms, seed=1)
        steps = -(-n_frames // 8)
        traj = torch.from_numpy(syn.ou_trajectory(base, steps, seed=2)).to(dev)                      # [S, N, 3]
        frames = traj[:, None] + 0.05 * torch.randn(steps, 8, atoms, 3, device=dev, generator=torch.Generator(dev).manual_seed(3))
        frames = frames.reshape(-1, atoms, 3)[:n_frames].to(torch.float32).contiguous()
        ft = forecast.Featurizer.backbone(atoms, min_sep, stride).to(dev)
        F, D = frames.shape[0], ft.dim()
        ptr, inc = ft.incidence(atoms, dev)
        out = {}

        def kernel_step():
            x = frames.detach().requires_grad_()
            forecast.internal_coordinates(x, ft).square().sum().backward()
            out["k"] = x.grad

        def torch_step():
            x = frames.detach().requires_grad_()
            torch_features(x, ft).square().sum().backward()
            out["t"] = x.grad

        k_ms = timed(kernel_step, a.calls, a.warmup)
        g = (2.0 * forecast.internal_coordinates(frames, ft)).contiguous()                           # what square().sum() hands back
        b_ms = timed(lambda: out.__setitem__("b", ops.internal_features_bwd(frames, g, ft.pairs, ft.triples, ft.quads, ptr, inc)),
                     a.calls, a.warmup)
        bg_ms = timed(lambda: out.__setitem__("bg", ops.internal_features_bwd(frames, g, ft.pairs, ft.triples, ft.quads, ptr, inc,
                                                                             form="global")), a.calls, a.warmup)
        f_ms = timed(lambda: forecast.internal_coordinates(frames, ft), a.calls, a.warmup)
        same = bool(torch.equal(out["b"].view(torch.int32), out["bg"].view(torch.int32)) and
                    torch.equal(out["b"].view(torch.int32), out["k"].view(torch.int32)))
        del g
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t_ms = timed(torch_step, a.calls, a.warmup)
        peak = torch.cuda.max_memory_allocated() - held
        scale = float(out["t"].abs().max())
        diff = float((out["k"].double() - out["t"].double()).abs().max())
        line = {"frames": F, "atoms": atoms, "features": D, "min_separation": min_sep, "stride": stride, "incidences": int(inc.numel()),
                "atom_chunk": ops.icg_atom_chunk(F, atoms), "workgroups": -(-F // ops.ic_frames_per_group(atoms)) * -(-atoms // ops.icg_atom_chunk(F, atoms)),
                "calls": a.calls, "fwd_bwd_ms_median": k_ms[0], "fwd_bwd_ms_min_max": k_ms[1:], "forward_kernel_ms_median": f_ms[0],
                "backward_kernel_ms_median": b_ms[0], "backward_kernel_ms_min_max": b_ms[1:], "backward_global_form_ms_median": bg_ms[0],
                "forms_and_autograd_bit_equal": same, "torch_fp64_fwd_bwd_ms_median": t_ms[0], "torch_fp64_fwd_bwd_ms_min_max": t_ms[1:],
                "torch_over_kernel": t_ms[0] / k_ms[0], "torch_peak_temporaries_bytes": peak, "gradient_bytes": F * atoms * 12,
                "max_abs_gradient": scale, "max_abs_difference": diff}
        del out
        torch.cuda.empty_cache()
        if atoms == 504:
            # every atom a hub against every fourth: the backward alone, per incidence
            Fh = min(F, a.hub_frames)
            hub = {}
            for name, s in (("stride_1", 1), ("stride_4", 4)):
                fh = forecast.Featurizer.backbone(atoms, min_sep, s).to(dev)
                hp, hi = fh.incidence(atoms, dev)
                gh = torch.randn(Fh, fh.dim(), device=dev, generator=torch.Generator(dev).manual_seed(5))
                ms = timed(lambda: ops.internal_features_bwd(frames[:Fh], gh, fh.pairs, fh.triples, fh.quads, hp, hi), a.calls, a.warmup)
                per = (hp[1:] - hp[:-1]).to(torch.float64)
                hub[name] = {"frames": Fh, "features": fh.dim(), "incidences": int(hi.numel()), "longest_chain": int(per.max()),
                             "mean_chain": float(per.mean()), "backward_kernel_ms_median": ms[0],
                             "ns_per_frame_incidence": ms[0] * 1e6 / (Fh * int(hi.numel()))}
                del gh
            hub["stride_4_over_stride_1_per_incidence"] = hub["stride_4"]["ns_per_frame_incidence"] / hub["stride_1"]["ns_per_frame_incidence"]
            line["uneven_chains"] = hub
        print(json.dumps(line), flush=True)
        del frames, traj
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
