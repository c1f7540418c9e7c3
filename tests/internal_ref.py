"""numpy restatement of include/mdno_internal.h: the same fp64 operations in the same order (elementwise + - * / sqrt
rint on np.float64 arrays — no np.dot, np.linalg or np.cross, whose orders are not the header's), so the device result can
be held to it bit for bit.  Arrays run over the frames; the tuples are walked one by one."""
import numpy as np

NAN = np.float64("nan")


def _box(box):
    if box is None:
        return np.zeros(3), np.zeros(3)
    L = np.asarray(box, np.float64).reshape(3)
    inv = np.array([np.float64(1.0) / l if l > 0.0 else np.float64(0.0) for l in L])       # formed once, like the host does
    return L, inv


def bond(x, a, b, L, inv):
    """v(a->b) of frames x f32 [F, N, 3] -> three f64 [F] arrays."""
    v = []
    for c in range(3):
        d = x[:, b, c].astype(np.float64) - x[:, a, c].astype(np.float64)
        if L[c] > 0.0:
            d = d - np.rint(d * inv[c]) * L[c]
        v.append(d)
    return v


def dot(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


def cross(p, q):
    return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]


def clamp(c):
    """c > 1 ? 1 : (c < -1 ? -1 : c): a NaN fails both tests and stays."""
    with np.errstate(invalid="ignore"):
        return np.where(c > 1.0, 1.0, np.where(c < -1.0, -1.0, c))


def _ok(idx, N):
    return all(0 <= int(i) < N for i in idx)


def distance(x, i, j, L, inv):
    v = bond(x, i, j, L, inv)
    return np.sqrt(dot(v, v))


def angle_cos(x, i, j, k, L, inv):
    """The UNCLAMPED c of the header (clamp() of it is the feature)."""
    u, w = bond(x, j, i, L, inv), bond(x, j, k, L, inv)
    return dot(u, w) / (np.sqrt(dot(u, u)) * np.sqrt(dot(w, w)))


def dihedral_xyh(x, i, j, k, l, L, inv):
    b1, b2, b3 = bond(x, i, j, L, inv), bond(x, j, k, L, inv), bond(x, k, l, L, inv)
    n1, n2 = cross(b1, b2), cross(b2, b3)
    xx = dot(n1, n2)
    yy = np.sqrt(dot(b2, b2)) * dot(b1, n2)
    return xx, yy, np.sqrt(xx * xx + yy * yy)


def features(frames, pairs=(), triples=(), quads=(), box=None):
    """frames f32 [F, N, 3] -> f64 [F, P + A + 2 T], the default mode of mdnoic_features."""
    x = np.asarray(frames, np.float32)
    F, N = x.shape[0], x.shape[1]
    L, inv = _box(box)
    cols = []
    bad = np.full(F, NAN)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for p in pairs:
            cols.append(distance(x, *map(int, p), L, inv) if _ok(p, N) else bad)
        for t in triples:
            cols.append(clamp(angle_cos(x, *map(int, t), L, inv)) if _ok(t, N) else bad)
        for q in quads:
            if _ok(q, N):
                xx, yy, h = dihedral_xyh(x, *map(int, q), L, inv)
                cols += [clamp(xx / h), clamp(yy / h)]
            else:
                cols += [bad, bad]
    return np.stack(cols, 1).astype(np.float64) if cols else np.zeros((F, 0), np.float64)


def radians_longdouble(frames, pairs=(), triples=(), quads=(), box=None):
    """The radians mode with the last step in long double: distances as they are, acos of the restatement's own fp64
    clamp(c), atan2 of its own fp64 (y, x) -> longdouble [F, P + A + T]; NaN where h is not > 0 or an index is out of range."""
    x = np.asarray(frames, np.float32)
    F, N = x.shape[0], x.shape[1]
    L, inv = _box(box)
    cols = []
    bad = np.full(F, np.longdouble("nan"))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for p in pairs:
            cols.append(distance(x, *map(int, p), L, inv).astype(np.longdouble) if _ok(p, N) else bad)
        for t in triples:
            cols.append(np.arccos(clamp(angle_cos(x, *map(int, t), L, inv)).astype(np.longdouble)) if _ok(t, N) else bad)
        for q in quads:
            if _ok(q, N):
                xx, yy, h = dihedral_xyh(x, *map(int, q), L, inv)
                a = np.arctan2(yy.astype(np.longdouble), xx.astype(np.longdouble))
                cols.append(np.where(h > 0.0, a, np.longdouble("nan")))
            else:
                cols.append(bad)
    return np.stack(cols, 1) if cols else np.zeros((F, 0), np.longdouble)


def conditioning(frames, triples=(), quads=(), box=None):
    """(min over quads and frames of h / (|b1| |b2| |b3|), max over triples and frames of |c|): how far the input stays from the
    singular geometries (collinear atoms, straight or folded-back angles).  h = |b1| |b2|^2 |b3| sin sin, so the ratio is |b2|
    times the product of the two sines."""
    x = np.asarray(frames, np.float32)
    L, inv = _box(box)
    worst_h, worst_c = np.inf, 0.0
    for q in quads:
        i, j, k, l = map(int, q)
        b1, b2, b3 = bond(x, i, j, L, inv), bond(x, j, k, L, inv), bond(x, k, l, L, inv)
        _, _, h = dihedral_xyh(x, i, j, k, l, L, inv)
        worst_h = min(worst_h, float((h / (np.sqrt(dot(b1, b1)) * np.sqrt(dot(b2, b2)) * np.sqrt(dot(b3, b3)))).min()))
    for t in triples:
        worst_c = max(worst_c, float(np.abs(angle_cos(x, *map(int, t), L, inv)).max()))
    return worst_h, worst_c


def column_histogram(x, lo, hi, n_bins):
    """x [R, D] (f32 or f64) -> (counts i64 [D, n_bins + 2], n_nan i64 [D]) by the header's rule."""
    x = np.asarray(x)
    R, D = x.shape
    lo = np.broadcast_to(np.asarray(lo, np.float64).reshape(-1), (D,)) if np.size(lo) == 1 else np.asarray(lo, np.float64)
    hi = np.broadcast_to(np.asarray(hi, np.float64).reshape(-1), (D,)) if np.size(hi) == 1 else np.asarray(hi, np.float64)
    counts = np.zeros((D, n_bins + 2), np.int64)
    n_nan = np.zeros(D, np.int64)
    for a in range(D):
        v = x[:, a].astype(np.float64)
        inv_w = np.float64(n_bins) / (hi[a] - lo[a])
        nan = np.isnan(v)
        n_nan[a] = int(nan.sum())
        v = v[~nan]
        below, above = v < lo[a], v >= hi[a]
        mid = v[~below & ~above]
        b = ((mid - lo[a]) * inv_w).astype(np.int64)
        b = np.where(b >= n_bins, n_bins - 1, b)
        counts[a, 0] = int(below.sum())
        counts[a, n_bins + 1] = int(above.sum())
        counts[a, 1:n_bins + 1] = np.bincount(b, minlength=n_bins)
    return counts, n_nan
