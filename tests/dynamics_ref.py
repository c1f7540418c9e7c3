"""The rules of include/mdno_dynamics.h restated in numpy fp64, operation for operation (a helper module like
observe_ref.py: no fixtures, no settings): the same differences, the same parenthesisation of the sum of squares, np.sqrt,
the strict comparison, truncation to the bin, np.rint for the image count.  numpy evaluates every ufunc on its own, so
nothing is contracted into an FMA.  Only the ORDER of the sums differs from the kernels' (numpy adds pairwise), and with
`remove_com` the order inside the centroid's sum; `Stats.gate*` bound what that can change.  tests/test_dynamics_host.py
checks the properties the GPU tests lean on; tests/test_gpu_dynamics.py holds the kernels to these functions."""
from dataclasses import dataclass

import numpy as np

EPS = 2.0 ** -52


def as_trajectory(x):
    """f32 [S, M, N, 3] (a [S, N, 3] truth is M = 1)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x[:, None] if x.ndim == 3 else x


def n_origins(S, tau, stride=1, span=0):
    last = S - 1 - span - tau
    return 0 if last < 0 else last // stride + 1


def centroids(x):
    """c f64 [S, M, 3]: the fp64 sum of the coordinates over the atoms, divided by N."""
    x = as_trajectory(x).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return x.sum(2) / float(x.shape[2])


def centroid_error(x):
    """The bound on the difference of two fp64 centroids of the same frame taken in different orders, per component:
    (N + 2) * 2^-53 * max|x| (N - 1 adds, one division, the centroid's own rounding)."""
    x = as_trajectory(x)
    finite = np.abs(x[np.isfinite(x)].astype(np.float64))
    return (x.shape[2] + 2) * 2.0 ** -53 * (float(finite.max()) if finite.size else 0.0)


def _diff(x64, c, t0, t1, remove_com):
    with np.errstate(invalid="ignore", over="ignore"):
        d = x64[t1] - x64[t0]
        if remove_com:
            dc = c[t1] - c[t0]
            d = d - dc[:, :, None, :]
    return d


def origins(S, tau, stride=1, span=0):
    return np.arange(n_origins(S, tau, stride, span), dtype=np.int64) * stride


def displacement_terms(x, tau, stride=1, remove_com=False):
    """(s f64 [n_origins, M, N], d f64 [n_origins, M, N, 3]): the squared displacement of every sample of lag tau."""
    x = as_trajectory(x)
    x64 = x.astype(np.float64)
    t = origins(x.shape[0], tau, stride)
    d = _diff(x64, centroids(x) if remove_com else None, t, t + tau, remove_com)
    with np.errstate(invalid="ignore", over="ignore"):
        sq = [d[..., a] * d[..., a] for a in range(3)]
        s = (sq[0] + sq[1]) + sq[2]
    return s, d


def velocity_terms(x, tau, stride=1, remove_com=False):
    """(p f64 [n_origins, M, N], v, v'): p = (vx*vx' + vy*vy') + vz*vz' of every sample of lag tau."""
    x = as_trajectory(x)
    x64 = x.astype(np.float64)
    c = centroids(x) if remove_com else None
    t = origins(x.shape[0], tau, stride, 1)
    v = _diff(x64, c, t, t + 1, remove_com)
    w = _diff(x64, c, t + tau, t + tau + 1, remove_com)
    with np.errstate(invalid="ignore", over="ignore"):
        pr = [v[..., a] * w[..., a] for a in range(3)]
        p = (pr[0] + pr[1]) + pr[2]
    return p, v, w


def _bins(r, r_max, n_bins):
    inv_dr = float(n_bins) / float(r_max)
    with np.errstate(invalid="ignore"):
        keep = r < r_max
    b = (r[keep] * inv_dr).astype(np.int64)
    b[b == n_bins] = n_bins - 1
    assert b.size == 0 or (b.min() >= 0 and b.max() < n_bins)
    return np.bincount(b, minlength=n_bins).astype(np.int64)


def _margin(r, r_max, n_bins):
    """min |t - round(t)|, t = r * inv_dr, over the samples with 0 < r < r_max * (1 + 1e-9): the distance of the nearest
    sample from a bin edge (r == r_max is the edge t == n_bins), in bins; inf without such a sample."""
    with np.errstate(invalid="ignore"):
        r = r[(r > 0.0) & (r < r_max * (1.0 + 1e-9))]
    t = r * (float(n_bins) / float(r_max))
    m = np.abs(t - np.rint(t))
    return float(m.min()) if m.size else float("inf")


def _sum(a):
    """Sum over origins and atoms: [n_origins, M, N] -> [M]."""
    with np.errstate(invalid="ignore", over="ignore"):
        return a.sum(axis=(0, 2))


@dataclass
class Stats:
    sum2: np.ndarray          # f64 [M, L]
    sum4: np.ndarray          # f64 [M, L]
    counts: np.ndarray        # i64 [M, L, n_bins] (n_bins == 0: [M, L, 0])
    n_samples: np.ndarray     # i64 [L]
    gate2: np.ndarray         # f64 [M, L]: what a kernel's sum2 may differ by
    gate4: np.ndarray
    margin: float             # bins
    beyond: int               # samples with r >= r_max


def displacement_stats(x, lags, stride=1, remove_com=False, r_max=None, n_bins=0):
    """The rule of mdno_displacement_stats for frames f32 [S, M, N, 3].  The gates: without remove_com the terms are the
    same operations on the same bits as the kernel's, so only the order of the n adds differs: n * 2^-52 * sum|term|
    (twice the bound n * 2^-53 * sum|term| of one sum in any order).  With remove_com the kernel's centroids may differ
    from these by centroid_error(x) = e per component, a displacement component by 2 e, so to first order a term s by
    2 * (|dx| + |dy| + |dz|) * 2 e and a term s^2 by 2 s times that: those sums are added."""
    x = as_trajectory(x)
    S, M, N = x.shape[:3]
    L = len(lags)
    out = Stats(np.zeros((M, L)), np.zeros((M, L)), np.zeros((M, L, n_bins), np.int64), np.zeros(L, np.int64),
                np.zeros((M, L)), np.zeros((M, L)), float("inf"), 0)
    e = 2.0 * centroid_error(x) if remove_com else 0.0
    for l, tau in enumerate(lags):
        s, d = displacement_terms(x, tau, stride, remove_com)
        n = s.shape[0] * N
        out.n_samples[l] = n
        with np.errstate(invalid="ignore", over="ignore"):
            s2 = s * s
            out.sum2[:, l], out.sum4[:, l] = _sum(s), _sum(s2)
            ds = 2.0 * ((np.abs(d[..., 0]) + np.abs(d[..., 1])) + np.abs(d[..., 2])) * e
            out.gate2[:, l] = n * EPS * _sum(np.abs(s)) + _sum(ds)
            out.gate4[:, l] = n * EPS * _sum(s2) + _sum(2.0 * s * ds)
            if n_bins > 0:
                r = np.sqrt(s)
                for m in range(M):
                    out.counts[m, l] = _bins(r[:, m], r_max, n_bins)
                out.margin = min(out.margin, _margin(r, r_max, n_bins))
                out.beyond += int((r >= r_max).sum())
    return out


def velocity_autocorrelation(x, lags, stride=1, remove_com=False):
    """(corr f64 [M, L], gate f64 [M, L], n_samples i64 [L]) by the rule of mdno_velocity_autocorrelation; the gate as in
    displacement_stats, a term v . v' moving by (|v|_1 + |v'|_1) * 2 e under a centroid error e."""
    x = as_trajectory(x)
    S, M, N = x.shape[:3]
    L = len(lags)
    corr, gate, ns = np.zeros((M, L)), np.zeros((M, L)), np.zeros(L, np.int64)
    e = 2.0 * centroid_error(x) if remove_com else 0.0
    for l, tau in enumerate(lags):
        p, v, w = velocity_terms(x, tau, stride, remove_com)
        n = p.shape[0] * N
        ns[l] = n
        with np.errstate(invalid="ignore", over="ignore"):
            corr[:, l] = _sum(p)
            mag = [np.abs(v[..., a] * w[..., a]) for a in range(3)]
            l1 = sum(np.abs(v[..., a]) + np.abs(w[..., a]) for a in range(3))
            gate[:, l] = n * EPS * _sum((mag[0] + mag[1]) + mag[2]) + _sum(l1 * e)
    return corr, gate, ns


def unwrap(x, box):
    """The rule of mdno_unwrap_frames: x f32 [S, ..., 3] -> f32 of the same shape."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = x.copy()
    if x.shape[0] == 0:
        return out
    x64 = x.astype(np.float64)
    for a in range(3):
        L = float(box[a])
        if not L > 0.0:
            continue
        inv = 1.0 / L
        n = np.zeros(x.shape[1:-1], dtype=np.float64)
        u = x[0, ..., a].copy()
        with np.errstate(invalid="ignore", over="ignore"):
            for t in range(1, x.shape[0]):
                nl = n * L
                d = (x64[t, ..., a] - nl) - u.astype(np.float64)
                k = np.rint(d * inv)
                n = n + k
                nl = n * L
                u = (x64[t, ..., a] - nl).astype(np.float32)
                out[t, ..., a] = u
    return out


def wrap(x, box):
    """x (any float array [..., 3]) wrapped into [0, L) on every periodic axis, in fp64, as f32.  Exact (and undone bit for
    bit by `unwrap`) where x and L share a binary grid the f32 format holds."""
    y = np.asarray(x, dtype=np.float64).copy()
    for a in range(3):
        L = float(box[a])
        if L > 0.0:
            y[..., a] = y[..., a] - np.floor(y[..., a] / L) * L
    return y.astype(np.float32)
