"""The numpy fp64 restatement of THE RULE of include/mdno_surface.h (a helper module like contacts_ref.py: no fixtures, no
settings).  Every operation is an IEEE operation rounded once, in the header's order, so the counts are EQUAL to the
device's — and the restatement also reports how close any comparison came to its boundary (the margin), so that a test
can show that its inputs do not sit where one ulp of a libm would decide."""
import numpy as np


def golden_spiral(P):
    """The default table of forecast.Spheres, written out again: z = 1 - (2 k + 1) / P, rho = sqrt(1 - z z), phi = k pi (3 - sqrt 5)."""
    k = np.arange(P, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / float(P)
    rho = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)


def differences(x, i, box):
    """d [N, 3] of one frame x f32 [N, 3]: d[j] = x_j - x_i in fp64, reduced on the periodic axes."""
    xd = x.astype(np.float64)
    d = xd - xd[i]
    if box is not None:
        for a in range(3):
            L = float(box[a])
            if L > 0.0:
                d[:, a] = d[:, a] - np.rint(d[:, a] * (1.0 / L)) * L
    return d


def frame_counts(x, R, U, box=None):
    """One frame x f32 [N, 3], R f64 [N], U f64 [P, 3] -> (counts i32 [N], the smallest |t - R_j^2| / R_j^2 over all point
    and neighbour tests, the smallest |sqrt(s) - (R_i + R_j)| over the pairs); inf where there was no test."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    R = np.asarray(R, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    N, P = x.shape[0], U.shape[0]
    counts = np.zeros(N, dtype=np.int32)
    m_point, m_pair = np.inf, np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(N):
            if not np.isfinite(x[i]).all():
                counts[i] = -1
                continue
            d = differences(x, i, box)
            s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            r = np.sqrt(s)
            reach = R[i] + R
            nb = r < reach                      # NaN, Inf: False
            nb[i] = False
            gap = np.abs(r - reach)
            gap[i] = np.inf
            gap = gap[np.isfinite(gap)]
            if gap.size:
                m_pair = min(m_pair, float(gap.min()))
            q = R[i] * U                        # [P, 3]
            dn, r2 = d[nb], R[nb] * R[nb]
            if dn.shape[0] == 0:
                counts[i] = P
                continue
            e = q[:, None, :] - dn[None, :, :]  # [P, n, 3]
            t = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            buried = (t < r2[None, :]).any(1)
            counts[i] = P - int(buried.sum())
            m_point = min(m_point, float((np.abs(t - r2[None, :]) / r2[None, :]).min()))
    return counts, m_point, m_pair


def exposed_points(frames, R, U, box=None):
    """frames f32 [..., N, 3] -> (counts i32 [..., N], point margin, pair margin) over all frames."""
    frames = np.asarray(frames, dtype=np.float32)
    lead, N = frames.shape[:-2], frames.shape[-2]
    flat = frames.reshape((-1, N, 3))
    out = np.zeros((flat.shape[0], N), dtype=np.int32)
    m_point, m_pair = np.inf, np.inf
    for f in range(flat.shape[0]):
        out[f], a, b = frame_counts(flat[f], R, U, box)
        m_point, m_pair = min(m_point, a), min(m_pair, b)
    return out.reshape(lead + (N,)), m_point, m_pair


def cap_exposed_fraction(d, Ri, Rj):
    """The closed form for two spheres at distance d, |Ri - Rj| < d < Ri + Rj: the exposed fraction of sphere i,
    1 - h / (2 Ri) with h = Ri - (d^2 + Ri^2 - Rj^2) / (2 d)."""
    h = Ri - (d * d + Ri * Ri - Rj * Rj) / (2.0 * d)
    return 1.0 - h / (2.0 * Ri)
