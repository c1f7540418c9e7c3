"""A numpy fp64 restatement of THE RULE of include/mdno_ensemble.h (a helper module like dynamics_ref.py: no fixtures, no
settings).  The per-sample quantities are formed with an explicit ascending-j loop over the sorted members, vectorised over
the samples, so each of them has the rule's bits; the sum over a step's n = 3 N samples is taken exactly (math.fsum, rounded
once), and beside every sum stands the gate for ANY order of adding its n terms in fp64,

    gate = (n - 1) u / (1 - (n - 1) u) * sum |q|,   u = 2^-53

(the standard bound for recursive summation in any order, e.g. Higham, Accuracy and Stability of Numerical Algorithms,
section 4.2): derived, not measured.  Since the per-sample values must match exactly, no further slack is given.  (The
exact sum's own rounding, at most u |sum|, is not added to the gate.  It does not need to be: the device adds a tile's
terms as a tree, whose bound is depth * u * sum|q| with depth <= 2 at n = 3 and depth + 1 <= n - 1 from n = 6 on; at n = 3
both numbers are fp64 values within 1.5 ulp of each other, so at most one ulp apart, and one ulp of the sum is at most
2 u sum|q| — the gate — since the four terms are non-negative.  The smallest cases do come close: error / gate up to 0.98 at
n = 3 and 6.)"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -53


@dataclass
class Samples:
    """Per-sample values of frames [S, M, N, 3] against truth [S, N, 3]: q f64 [S, n, 4], rank i64 [S, n], tie and valid
    bool [S, n], n = 3 N."""
    q: np.ndarray
    rank: np.ndarray
    tie: np.ndarray
    valid: np.ndarray


@dataclass
class Score:
    sums: np.ndarray          # f64 [S, 4]; NaN for a step with an invalid sample
    gate: np.ndarray          # f64 [S, 4]
    rank_hist: np.ndarray     # i64 [S, M + 1]
    n_invalid: np.ndarray     # i64 [S]
    n_ties: np.ndarray        # i64 [S]
    members: int
    samples_per_step: int
    per_sample: Samples


def per_sample(frames: np.ndarray, truth: np.ndarray) -> Samples:
    frames = np.asarray(frames, dtype=np.float32)
    truth = np.asarray(truth, dtype=np.float32)
    S, M, N, _ = frames.shape
    assert truth.shape == (S, N, 3) and M >= 1
    n = 3 * N
    x = frames.reshape(S, M, n)
    y32 = truth.reshape(S, n)
    valid = np.isfinite(x).all(1) & np.isfinite(y32)
    with np.errstate(all="ignore"):
        xs = np.sort(x, axis=1)                               # fp32 compare; -0 == +0
        y = y32.astype(np.float64)
        d = [xs[:, j].astype(np.float64) - y for j in range(M)]
        total = np.zeros((S, n))
        q2 = np.zeros((S, n))
        q3 = np.zeros((S, n))
        for j in range(M):                                    # ascending j
            total = total + d[j]
            q2 = q2 + np.abs(d[j])
            q3 = q3 + float(2 * j - M + 1) * d[j]
        mean = total / float(M)
        q1 = np.zeros((S, n))
        for j in range(M):
            c = d[j] - mean
            q1 = q1 + c * c
        q1 = q1 / float(M - 1) if M >= 2 else np.zeros((S, n))
        q = np.stack([mean * mean, q1, q2, q3], axis=-1)
        rank = (x < y32[:, None]).sum(1).astype(np.int64)
        tie = (x == y32[:, None]).any(1)
    q[~valid] = np.nan
    return Samples(q, rank, tie & valid, valid)


def score(frames: np.ndarray, truth: np.ndarray) -> Score:
    ps = per_sample(frames, truth)
    S, M = frames.shape[0], frames.shape[1]
    n = ps.q.shape[1]
    sums = np.zeros((S, 4))
    gate = np.zeros((S, 4))
    hist = np.zeros((S, M + 1), dtype=np.int64)
    g = (n - 1) * U / (1.0 - (n - 1) * U) if n > 0 else 0.0
    for s in range(S):
        ok = ps.valid[s]
        if ok.all():
            for c in range(4):
                col = ps.q[s, :, c].tolist()
                sums[s, c] = math.fsum(col)
                gate[s, c] = g * math.fsum(abs(v) for v in col)
        else:
            sums[s] = np.nan
            gate[s] = np.nan
        hist[s] = np.bincount(ps.rank[s][ok], minlength=M + 1)
    return Score(sums, gate, hist, (~ps.valid).sum(1).astype(np.int64), ps.tie.sum(1).astype(np.int64), M, n, ps)


def pair_sum_brute(frames: np.ndarray) -> np.ndarray:
    """sum_{m<k} |x_m - x_k| per sample, term by term in fp64: f64 [S, n] (what q3 equals through the sort)."""
    S, M, N, _ = frames.shape
    x = np.asarray(frames, dtype=np.float32).reshape(S, M, 3 * N).astype(np.float64)
    out = np.zeros((S, 3 * N))
    for m in range(M):
        for k in range(m + 1, M):
            out += np.abs(x[:, m] - x[:, k])
    return out


# ------------------------------------------------------------------------------------------------ the derived quantities
def rmse(sc: Score):
    return np.sqrt(sc.sums[:, 0] / sc.samples_per_step)


def spread(sc: Score):
    return np.sqrt(sc.sums[:, 1] / sc.samples_per_step)


def pooled(sc: Score):
    """(spread-skill, CRPS, fair CRPS, rank histogram i64 [M + 1]) with every step pooled before the ratios."""
    M, n = sc.members, sc.samples_per_step * sc.sums.shape[0]
    t = sc.sums.sum(0)
    ss = math.sqrt((M + 1) / M) * math.sqrt(t[1] / n) / math.sqrt(t[0] / n)
    crps = t[2] / (M * n) - t[3] / (M * M * n)
    fair = t[2] / (M * n) - t[3] / (M * (M - 1) * n) if M >= 2 else float("nan")
    return ss, crps, fair, sc.rank_hist.sum(0)


def ensemble(S, M, N, seed=1, sigma=0.3, truth_sigma=0.3, box=17.1):
    """The input of the calibration checks and the GPU tests: base uniform in [0, box)^3, members base + N(0, sigma), the
    truth base + N(0, truth_sigma) drawn after them.  (frames f32 [S, M, N, 3], truth f32 [S, N, 3])"""
    rng = np.random.default_rng(seed)
    base = rng.random((S, 1, N, 3)) * box
    frames = (base + rng.normal(0.0, sigma, size=(S, M, N, 3))).astype(np.float32)
    truth = (base[:, 0] + rng.normal(0.0, truth_sigma, size=(S, N, 3))).astype(np.float32)
    return frames, truth
