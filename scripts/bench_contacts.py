"""Time the contact statistics (ops.pair_statistics, ops.contact_bits, ops.contact_correlation; csrc/contacts.hip) against the
same numbers composed from torch in fp64 on the same device, and against ops.pair_histogram on the same frames (the same pair
arithmetic once per pair and frame: what the fp64 pair stream costs).  Shapes: 1,000 steps x 504 atoms at 8 and at 64
members, and 1,000 steps x 64 members x 28 atoms.  Per shape ONE JSON line: the median of `--calls` calls of each (HIP events
around one call, after `--warmup` calls of that shape) of
    pair_statistics at block_len 64 with the moments and without, the bytes of maps each writes and the achieved bytes/s;
    contact_series + correlation at 29 lags for the native pairs of the first frame (ContactPairs.native);
    pair_histogram (200 bins) of the same frames;
    the torch compositions (cdist per chunk of steps, `<`, sums per block; gathers, `<`, shifted products per lag), their
    ratio to the kernels and the peak of their temporaries (torch.cuda.max_memory_allocated above what was held before);
and whether the torch counts equal the kernels' (the sums differ by torch's own summation order).

    python scripts/bench_contacts.py [--calls 50] [--warmup 3] [--steps 1000]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

BLOCK = 64
N_LAGS = 29


def torch_statistics(frames, threshold, moments):
    """count / sum_r / sum_r2 per block of BLOCK steps from torch.cdist in fp64, one block of steps at a time."""
    S, M, N = frames.shape[:3]
    counts, sr, sr2 = [], [], []
    for s0 in range(0, S, BLOCK):
        x = frames[s0:s0 + BLOCK].to(torch.float64)
        r = torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist")                      # [B, M, N, N]
        counts.append((r < threshold).sum(0, dtype=torch.int32))
        if moments:
            sr.append(r.sum(0))
            sr2.append((r * r).sum(0))
    return torch.stack(counts), (torch.stack(sr) if moments else None), (torch.stack(sr2) if moments else None)


def torch_series(frames, pairs, cut, lags):
    """bool series [S, M, P] by gathers, then origins / both per lag by shifted products."""
    x = frames.to(torch.float64)
    d = (x[:, :, pairs[:, 1].long()] - x[:, :, pairs[:, 0].long()]).norm(dim=-1)
    c = d < cut
    per_frame = c.sum(2, dtype=torch.int32)
    S = c.shape[0]
    origins = torch.stack([c[:S - l].sum(0, dtype=torch.int32) for l in lags], -1)
    both = torch.stack([(c[:S - l] & c[l:]).sum(0, dtype=torch.int32) for l in lags], -1)
    return c, per_frame, origins, both


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
    ap.add_argument("--torch-calls", type=int, default=5, help="calls of the torch compositions (they are the slow side)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_contacts.py needs a GPU (there is no CPU path)")
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    dev = torch.device("cuda:0")
    for members, atoms in ((8, 504), (64, 504), (64, 28)):
        base = syn.box_frame(atoms, seed=1) if atoms > 128 else syn.chain_frame(atoms, seed=1)
        traj = torch.from_numpy(syn.ou_trajectory(base, a.steps, seed=2)).to(dev)                  # [S, N, 3]
        frames = (traj[:, None] + 0.05 * torch.randn(a.steps, members, atoms, 3, device=dev, generator=torch.Generator(dev).manual_seed(3)))
        frames = frames.to(torch.float32).contiguous()
        S = a.steps
        Bk = -(-S // BLOCK)
        elems = Bk * members * atoms * atoms
        out = {}
        full_ms = timed(lambda: out.__setitem__("full", ops.pair_statistics(frames, 8.0, block_len=BLOCK)), a.calls, a.warmup)
        out.pop("full")
        count_ms = timed(lambda: out.__setitem__("count", ops.pair_statistics(frames, 8.0, block_len=BLOCK, moments=False)), a.calls, a.warmup)
        hist_ms = timed(lambda: ops.pair_histogram(frames, 8.0, 200), a.calls, a.warmup)
        native = forecast.ContactPairs.native(frames[0, 0], 8.0, min_separation=3).to(dev)
        lags = forecast.default_lags(S)[:N_LAGS]
        series_ms = timed(lambda: out.__setitem__("cs", forecast.contact_series(frames, native)), a.calls, a.warmup)
        corr_ms = timed(lambda: out.__setitem__("cc", out["cs"].correlation(lags)), a.calls, a.warmup)
        (tc_ms, tc_peak) = with_peak(lambda: out.__setitem__("tcount", torch_statistics(frames, 8.0, False)[0]), a.torch_calls, 1)
        counts_equal = bool(torch.equal(out.pop("tcount"), out["count"][0]))
        out.pop("count")
        (tf_ms, tf_peak) = with_peak(lambda: torch_statistics(frames, 8.0, True), a.torch_calls, 1)
        (ts_ms, ts_peak) = with_peak(lambda: out.__setitem__("ts", torch_series(frames, native.pairs, native.cut, lags)), a.torch_calls, 1)
        c, per_frame, origins, both = out["ts"]
        series_equal = bool(torch.equal(out["cs"].series(), c.permute(1, 2, 0)) and torch.equal(out["cs"].per_frame, per_frame)
                            and torch.equal(out["cc"].origins, origins) and torch.equal(out["cc"].both, both))
        pair_frames = S * members * atoms * (atoms + 1) // 2
        print(json.dumps({
            "members": members, "atoms": atoms, "steps": S, "block_len": BLOCK, "blocks": Bk, "calls": a.calls,
            "pair_statistics_ms_median": full_ms[0], "pair_statistics_ms_min_max": full_ms[1:], "pair_statistics_map_bytes": elems * 20,
            "pair_statistics_write_bytes_per_s": elems * 20 / (full_ms[0] * 1e-3),
            "pair_statistics_pair_frames_per_s": pair_frames / (full_ms[0] * 1e-3),
            "counts_only_ms_median": count_ms[0], "counts_only_ms_min_max": count_ms[1:], "counts_only_map_bytes": elems * 4,
            "counts_only_pair_frames_per_s": pair_frames / (count_ms[0] * 1e-3),
            "pair_histogram_200_bins_ms_median": hist_ms[0], "pair_statistics_over_pair_histogram": full_ms[0] / hist_ms[0],
            "native_pairs": len(native), "lags": len(lags), "contact_series_ms_median": series_ms[0],
            "contact_correlation_ms_median": corr_ms[0],
            "torch_fp64_statistics_ms_median": tf_ms[0], "torch_over_pair_statistics": tf_ms[0] / full_ms[0],
            "torch_fp64_statistics_peak_temporaries_bytes": tf_peak,
            "torch_fp64_counts_ms_median": tc_ms[0], "torch_over_counts_only": tc_ms[0] / count_ms[0],
            "torch_fp64_counts_peak_temporaries_bytes": tc_peak, "torch_counts_equal": counts_equal,
            "torch_fp64_series_and_correlation_ms_median": ts_ms[0],
            "torch_over_series_and_correlation": ts_ms[0] / (series_ms[0] + corr_ms[0]),
            "torch_fp64_series_peak_temporaries_bytes": ts_peak, "torch_series_equal": series_equal}), flush=True)
        del out, frames, traj
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
