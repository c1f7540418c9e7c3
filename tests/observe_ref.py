"""The rule of include/mdno_observe.h restated in numpy fp64, operation for operation (a helper module like
philox_ref.py: no fixtures, no settings): the same differences, np.rint for the minimum image, the same
parenthesisation of the sum of squares, np.sqrt, the strict comparison, truncation to the bin.  numpy evaluates every
ufunc on its own, so nothing is contracted into an FMA.  tests/test_observe_host.py checks the properties the GPU tests
lean on; tests/test_gpu_observe.py holds the kernels to `histogram` exactly."""
import numpy as np


def pair_distances(x, box=None):
    """r f64 [N, N] for a frame x f32 [N, 3]: r[i, j] is the distance of the rule for destination i and source j
    (d = x_j - x_i, reduced by rint(d * invL) * L on a periodic axis).  NaN / Inf coordinates propagate."""
    x = np.ascontiguousarray(x, dtype=np.float32).astype(np.float64)
    sq = []
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[None, :, :] - x[:, None, :]
        for a in range(3):
            da = d[..., a]
            L = 0.0 if box is None else float(box[a])
            if L > 0.0:
                inv = 1.0 / L
                k = np.rint(da * inv)
                da = da - k * L
            sq.append(da * da)
        s = (sq[0] + sq[1]) + sq[2]
        return np.sqrt(s)


def _upper(x, box):
    x = np.asarray(x)
    iu = np.triu_indices(x.shape[0], 1)
    return pair_distances(x, box)[iu]


def histogram(x, r_max, n_bins, box=None):
    """counts i64 [n_bins] of the unordered pairs i < j of one frame."""
    r = _upper(x, box)
    inv_dr = float(n_bins) / float(r_max)
    with np.errstate(invalid="ignore"):
        keep = r < r_max
    b = (r[keep] * inv_dr).astype(np.int64)
    b[b == n_bins] = n_bins - 1
    assert b.size == 0 or (b.min() >= 0 and b.max() < n_bins)
    return np.bincount(b, minlength=n_bins).astype(np.int64)


def histograms(frames, r_max, n_bins, box=None):
    """counts i64 [..., n_bins] for frames f32 [..., N, 3]."""
    frames = np.asarray(frames)
    flat = frames.reshape((-1,) + frames.shape[-2:])
    out = np.stack([histogram(f, r_max, n_bins, box) for f in flat]) if flat.shape[0] else np.zeros((0, n_bins), np.int64)
    return out.reshape(frames.shape[:-2] + (n_bins,))


def margin(x, r_max, n_bins, box=None, ignore_zero=False):
    """min |t - round(t)| with t = r * inv_dr over all pairs i < j of one frame with r < r_max * (1 + 1e-9): how far the
    nearest pair is from a bin edge (r == r_max is the edge t == n_bins), in bins.  A comparison of counts does not
    hinge on the last bit of a square root while this stays far above 1e-16 * n_bins.  `ignore_zero`: leave out pairs
    that sit on an edge exactly (the cases built from integer triples).  inf where there is no such pair."""
    r = _upper(x, box)
    with np.errstate(invalid="ignore"):
        r = r[r < r_max * (1.0 + 1e-9)]
    t = r * (float(n_bins) / float(r_max))
    m = np.abs(t - np.rint(t))
    if ignore_zero:
        m = m[m > 0.0]
    return float(m.min()) if m.size else float("inf")


def contact_count(x, threshold, box=None):
    """The "forecast" contact count of mdno_forecast_score on one frame: ordered pairs, diagonal included, r < threshold."""
    with np.errstate(invalid="ignore"):
        return int((pair_distances(x, box) < threshold).sum())


def radius_of_gyration(x):
    """sqrt(mean_i |x_i - c|^2), c the centroid, in fp64 (numpy's pairwise sums); NaN without atoms."""
    x = np.ascontiguousarray(x, dtype=np.float32).astype(np.float64)
    if x.shape[0] == 0:
        return float("nan")
    with np.errstate(invalid="ignore", over="ignore"):
        c = x.sum(0) / x.shape[0]
        d = x - c
        return float(np.sqrt((d * d).sum() / x.shape[0]))
