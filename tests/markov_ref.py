"""A numpy restatement of include/mdno_markov.h for tests/test_markov_host.py and tests/test_gpu_markov.py (a helper module
like essential_ref.py: no fixtures, no settings).  Every sum runs in np.longdouble, ties go to the lowest index, rows and
centres with a NaN or Inf are treated as the header says, and each function returns the first-order rounding bound of the
fp64 rule beside its value."""
import numpy as np

U53 = 2.0 ** -53
LD = np.longdouble


def finite_rows(X):
    X = np.asarray(X)
    return np.isfinite(X).all(axis=1) if X.shape[1] else np.ones(X.shape[0], bool)


def centred(X, origin=None):
    """x~ = (double)x - origin: ONE fp64 rounding, as the kernel does on the way into LDS."""
    X = np.asarray(X).astype(np.float64)
    return X if origin is None else X - np.asarray(origin, np.float64)[None]


def pair_d2(X, C, origin=None):
    """(d2 [R, k] in longdouble, bound [R, k]): d2 = max(0, n + m - 2 g) of the centred rows, and the header's first-order
    bound (D + 4) 2^-53 (n + m + 2 sum |x~| |c~|): D fused accumulations, the two norms and three final roundings."""
    D = np.asarray(X).shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        xt, ct = centred(X, origin).astype(LD), centred(C, origin).astype(LD)
        n, m = (xt * xt).sum(1), (ct * ct).sum(1)
        g = xt @ ct.T
        ag = np.abs(xt) @ np.abs(ct).T
        d2 = np.maximum(LD(0), n[:, None] + m[None] - 2 * g)
        bound = (D + 4) * U53 * (n[:, None] + m[None] + 2 * ag)
    return d2, bound


def assign(X, C, origin=None):
    """-> labels i32 [R], dist2 f64 [R], gap [R]: gap is (second best - best) / (bound of best + bound of second best) over
    the valid centres, inf where fewer than two are valid or the row is not finite."""
    X, C = np.asarray(X), np.asarray(C)
    R, k = X.shape[0], C.shape[0]
    labels = np.full(R, -1, np.int32)
    dist2 = np.full(R, np.nan)
    gap = np.full(R, np.inf)
    if R == 0 or k == 0:
        return labels, dist2, gap
    d2, bound = pair_d2(X, C, origin)
    ok_r, ok_c = finite_rows(X), finite_rows(C)
    d2 = np.where(ok_c[None], d2, LD(np.inf))
    d2 = np.where(np.isnan(d2), LD(np.inf), d2)
    for r in np.nonzero(ok_r)[0]:
        j = int(np.argmin(d2[r]))                                                  # (the first minimum: the lowest index)
        if not np.isfinite(d2[r, j]):
            continue
        labels[r], dist2[r] = j, float(d2[r, j])
        rest = d2[r].copy()
        rest[j] = np.inf
        j2 = int(np.argmin(rest))
        if np.isfinite(rest[j2]):
            both = bound[r, j] + bound[r, j2]
            gap[r] = float((rest[j2] - d2[r, j]) / both) if both > 0 else (np.inf if rest[j2] > d2[r, j] else 0.0)
    return labels, dist2, gap


def kcenters(X, k, first=0):
    """-> index i64 [k], radius f64 [k], gap [k]: per round (best - second best mind2) / (their two bounds
    (D + 2) 2^-53 mind2), inf where there is no second candidate (round 0: inf)."""
    X = np.asarray(X)
    R, D = X.shape
    ok = finite_rows(X)
    Xl = np.where(np.isfinite(X), X, 0).astype(np.float64).astype(LD)
    index = np.zeros(k, np.int64)
    radius = np.zeros(k)
    gap = np.full(k, np.inf)
    index[0], radius[0] = first, np.inf
    mind2 = np.full(R, np.inf, LD)
    for i in range(1, k):
        c = index[i - 1]
        if c >= 0 and ok[c]:
            e = ((Xl - Xl[c][None]) ** 2).sum(1)
            mind2 = np.minimum(mind2, e)
        cand = np.where(ok, mind2, LD(-1))
        if not ok.any():
            index[i], radius[i] = -1, np.nan
            continue
        j = int(np.argmax(cand))                                                   # (the first maximum: the lowest row)
        index[i], radius[i] = j, float(np.sqrt(cand[j]))
        rest = cand.copy()
        rest[j] = -1
        j2 = int(np.argmax(rest))
        if rest[j2] >= 0 and np.isfinite(cand[j]):
            both = (D + 2) * U53 * (cand[j] + rest[j2])
            gap[i] = float((cand[j] - rest[j2]) / both) if both > 0 else (np.inf if cand[j] > rest[j2] else 0.0)
    return index, radius, gap


def centroid_sums(X, labels, k):
    """-> sums f64 [k, D] (from longdouble), counts i64 [k], abs_sums [k, D] (the gate is count 2^-53 abs_sums)."""
    X, labels = np.asarray(X), np.asarray(labels)
    D = X.shape[1]
    sums, abs_sums, counts = np.zeros((k, D), LD), np.zeros((k, D), LD), np.zeros(k, np.int64)
    for j in range(k):
        rows = X[labels == j].astype(np.float64).astype(LD)
        counts[j] = rows.shape[0]
        sums[j], abs_sums[j] = rows.sum(0), np.abs(rows).sum(0)
    return sums.astype(np.float64), counts, abs_sums.astype(np.float64)


def transition_counts(labels, n, lags, pooled=False):
    """labels [S, M] -> counts i64 [L, M or 1, n, n], n_skipped i64 [L]."""
    labels = np.asarray(labels)
    if labels.ndim == 1:
        labels = labels[:, None]
    S, M = labels.shape
    counts = np.zeros((len(lags), 1 if pooled else M, n, n), np.int64)
    skipped = np.zeros(len(lags), np.int64)
    for l, lag in enumerate(lags):
        if lag >= S:
            continue
        a, b = labels[:S - lag], labels[lag:]
        ok = (a >= 0) & (a < n) & (b >= 0) & (b < n)
        skipped[l] = int((~ok).sum())
        for m in range(M):
            np.add.at(counts[l, 0 if pooled else m], (a[ok[:, m], m], b[ok[:, m], m]), 1)
    return counts, skipped


def features(R, D, seed, offset=20.0):
    """Per-column-scaled Gaussians about offsets up to +-offset, rounded to f32: [R, D]."""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.2, 3.0, D)
    shift = rng.uniform(-offset, offset, D)
    return (rng.normal(size=(R, D)) * scale + shift).astype(np.float32)


def perturbed_rows(X, k, seed, amount=0.3):
    """k centres: rows of X (cycled) plus Gaussian noise, rounded to f32."""
    rng = np.random.default_rng(seed)
    if X.shape[0] == 0:
        return np.zeros((k, X.shape[1]), np.float32)
    rows = X[rng.permutation(max(X.shape[0], k))[:k] % X.shape[0]]
    return (rows.astype(np.float64) + amount * rng.normal(size=rows.shape)).astype(np.float32)
