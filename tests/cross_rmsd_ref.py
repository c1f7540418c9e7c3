"""numpy fp64 restatement of include/mdno_conformations.h for tests/test_conformations_host.py and
tests/test_gpu_cross_rmsd.py (a helper module like ensemble_ref.py: no fixtures, no settings).

Two routes that share no step after the centring:
  rmsd2_matrix      centre, einsum for the nine sums S_rc, Horn's 4 x 4 matrix, np.linalg.eigvalsh, max(0, G - 2 lambda) / N
  superpose_rmsd2   explicit Kabsch by SVD with the determinant correction, rotate, residual (restated from
                    tests/test_gpu_forecast.py)

THE GATE is the project's own for this quantity (test_rmsd_against_explicit_superposition):
    |matrix^2 - reference rmsd^2| <= 8 * 2^-52 * G,    G = g_p + g_q of that pair.
It holds for ANY order of the sums.  rmsd^2 = (G - 2 lambda) / N.  G and the nine S_rc are N-term (3 N-term) fp64 sums of
products of the centred coordinates; the any-order bound of such a sum is about N u relative to the sum of the absolute
terms (u = 2^-53), and by Cauchy-Schwarz sum_k |a_k[r] b_k[c]| <= sqrt(g_p g_q) <= G / 2, so every S_rc carries at most about
N u G / 2 and G about N u G.  lambda is a 1-Lipschitz function of Horn's matrix in the spectral norm, whose entries are sums
of up to three S_rc: the perturbation of 2 lambda stays below about 3 N u G.  The division by N takes the factor N back:
about (1 + 3) u G = 2 * 2^-52 G in the worst case for the accumulations (2.5 with the products' own roundings), whatever
their order.  The rest of the 8 is for the centring (a centroid off by N u |c| moves S only in second order, the centred
terms summing to zero) and the eigen-solve (Jacobi or LAPACK: a few u ||K|| <= a few u G, divided by N like the rest).
Measured on the host, the two routes above differ from each other by less than 2.2 * 2^-52 G over N in {1, 2, 3, 4, 5, 15,
16, 17, 28, 63, 64, 65, 129, 504}, noise 0 to 5, rotations and an offset of 1e3 (tests/test_conformations_host.py asserts
the gate on that set and prints the figure per N), so the reference alone stays inside the gate."""
import numpy as np

U52 = 2.0 ** -52
GATE = 8 * U52


def centre(frames):
    """frames [..., N, 3] (any float dtype) -> (centred f64 [..., N, 3], g [...], valid [...]).  N == 0: valid, g = 0."""
    x = np.asarray(frames).astype(np.float64)
    valid = np.isfinite(x).all(axis=(-1, -2))
    if x.shape[-2] == 0:
        return x, np.zeros(x.shape[:-2]), valid
    with np.errstate(invalid="ignore"):
        xc = x - x.mean(axis=-2, keepdims=True)
        return xc, (xc ** 2).sum(axis=(-1, -2)), valid


def horn(S):
    """Horn's symmetric 4 x 4 quaternion matrix of S [..., 3, 3]."""
    K = np.empty(S.shape[:-2] + (4, 4))
    xx, xy, xz = S[..., 0, 0], S[..., 0, 1], S[..., 0, 2]
    yx, yy, yz = S[..., 1, 0], S[..., 1, 1], S[..., 1, 2]
    zx, zy, zz = S[..., 2, 0], S[..., 2, 1], S[..., 2, 2]
    K[..., 0, 0], K[..., 1, 1], K[..., 2, 2], K[..., 3, 3] = xx + yy + zz, xx - yy - zz, yy - xx - zz, zz - xx - yy
    K[..., 0, 1] = K[..., 1, 0] = yz - zy
    K[..., 0, 2] = K[..., 2, 0] = zx - xz
    K[..., 0, 3] = K[..., 3, 0] = xy - yx
    K[..., 1, 2] = K[..., 2, 1] = xy + yx
    K[..., 1, 3] = K[..., 3, 1] = zx + xz
    K[..., 2, 3] = K[..., 3, 2] = yz + zy
    return K


def rmsd2_matrix(A, B):
    """A [Fa, N, 3], B [Fb, N, 3] -> (rmsd^2 f64 [Fa, Fb], G f64 [Fa, Fb]); NaN in rmsd^2 where either frame is invalid."""
    Fa, N = A.shape[0], A.shape[1]
    Fb = B.shape[0]
    a, ga, va = centre(A)
    b, gb, vb = centre(B)
    G = ga[:, None] + gb[None, :]
    ok = va[:, None] & vb[None, :]
    if N == 0:
        return np.zeros((Fa, Fb)), np.zeros((Fa, Fb))
    a, b = np.where(va[:, None, None], a, 0.0), np.where(vb[:, None, None], b, 0.0)
    S = np.einsum("ikr,jkc->ijrc", a, b)
    lam = np.linalg.eigvalsh(horn(S))[..., -1] if Fa * Fb else np.zeros((Fa, Fb))
    r2 = np.maximum(0.0, np.where(ok, G, 0.0) - 2.0 * lam) / N
    return np.where(ok, r2, np.nan), np.where(ok, G, np.nan)


def lowest_min(v, axis):
    """(minimum over the non-NaN entries along `axis`, the LOWEST index that attains it); NaN and -1 where there is none."""
    ok = ~np.isnan(v)
    if v.shape[axis] == 0:
        shape = tuple(s for i, s in enumerate(v.shape) if i != axis % v.ndim)
        return np.full(shape, np.nan), np.full(shape, -1, dtype=np.int64)
    w = np.where(ok, v, np.inf)
    idx = w.argmin(axis=axis)                       # numpy: the first occurrence
    val = np.take_along_axis(w, np.expand_dims(idx, axis), axis).squeeze(axis)
    none = ~ok.any(axis=axis)
    return np.where(none, np.nan, val), np.where(none, -1, idx).astype(np.int64)


class Result:
    def __init__(self, matrix2, G):
        self.matrix2, self.G = matrix2, G                       # [S, M, Fb]: rmsd^2 and the pair's G
        self.matrix = np.sqrt(matrix2)
        self.nearest, self.nearest_index = lowest_min(self.matrix, 2)           # [S, M]
        self.cover, self.cover_step = lowest_min(self.matrix, 0)                # [M, Fb]


def cross_rmsd(A, B):
    """A f32 [S, M, N, 3], B f32 [Fb, N, 3] -> Result by the rule of the header."""
    S, M, N = A.shape[:3]
    r2, G = rmsd2_matrix(A.reshape(S * M, N, 3), B)
    return Result(r2.reshape(S, M, B.shape[0]), G.reshape(S, M, B.shape[0]))


def superpose_rmsd2(P, Q):
    """rmsd^2 by explicit superposition in numpy fp64 (Kabsch): centre, SVD of the covariance, determinant correction,
    rotate, residual.  Also G = sum |p - mean p|^2 + sum |q - mean q|^2."""
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    Pc, Qc = P - P.mean(0), Q - Q.mean(0)
    U, _, Vt = np.linalg.svd(Pc.T @ Qc)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T
    res = Pc @ R.T - Qc
    return (res ** 2).sum() / P.shape[0], (Pc ** 2).sum() + (Qc ** 2).sum()


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


# ------------------------------------------------------------------------------------------------ inputs
KINDS = ("identical", "rigid copy", "mirror image", "noise", "rotated and translated", "planar", "collinear", "offset 1e3")


def grid_cloud(N, rng):
    """N atoms at the benchmark's density on the 1/64 grid (f32 holds them, their quarter turns and integer shifts)."""
    side = max((N / 0.1) ** (1.0 / 3.0), 6.0)
    return np.round((rng.random((N, 3)) - 0.5) * side * 64) / 64


def variant(kind, base, rng):
    """One frame of the family `kind` of tests/test_gpu_forecast.py's rmsd_cases(), about the grid cloud `base` (f64)."""
    N = base.shape[0]
    sigma = 10.0 ** rng.uniform(-6.0, np.log10(3.0))
    if kind == "identical":
        return base
    if kind == "rigid copy":                    # exact in f32: quarter turn + integer shift
        return np.stack([-base[:, 1], base[:, 0], base[:, 2]], axis=1) + np.array([5.0, -3.0, 7.0])
    if kind == "mirror image":
        return base * np.array([1.0, 1.0, -1.0])
    if kind == "noise":
        return base + rng.normal(scale=sigma, size=base.shape)
    if kind == "rotated and translated":
        return (base + rng.normal(scale=sigma, size=base.shape)) @ rotation(rng).T + rng.normal(size=3) * 20
    if kind == "planar":
        flat = base + rng.normal(scale=sigma, size=base.shape)
        flat[:, 2] = 0
        return flat @ rotation(rng).T
    if kind == "collinear":
        return np.outer(np.linspace(-30, 30, N) + rng.normal(scale=sigma, size=N), [1.0, 2.0, -0.5]) @ rotation(rng).T + 3
    if kind == "offset 1e3":
        return base + rng.normal(scale=0.5, size=base.shape) + 1e3
    raise ValueError(kind)


def stacked(S, M, N, Fb, seed):
    """(A f32 [S, M, N, 3], B f32 [Fb, N, 3], kinds of A's rows [S][M], kinds of B's frames [Fb]): every frame one of KINDS
    about ONE grid cloud, the random ones with their own draw, so that every (row, column) has its own expected value.
    Row (0, 0) and column 0 are "identical" (the cloud itself), column 1 (Fb >= 2) its exact rigid copy, column 2 its mirror
    image; the other frames walk the five random kinds from a seeded offset (a second rigid copy or mirror image would
    repeat a whole row or column of expected values)."""
    rng = np.random.default_rng(seed)
    base = grid_cloud(N, rng)
    kb = [KINDS[j] if j < 3 else KINDS[3 + (j + seed) % 5] for j in range(Fb)]
    ka = [[KINDS[0] if s == m == 0 else KINDS[3 + (s * M + m + seed) % 5] for m in range(M)] for s in range(S)]
    B = np.stack([variant(k, base, rng) for k in kb]).astype(np.float32) if Fb else np.zeros((0, N, 3), np.float32)
    A = np.stack([np.stack([variant(k, base, rng) for k in row]) for row in ka]).astype(np.float32) if S * M else \
        np.zeros((S, M, N, 3), np.float32)
    return A, B, ka, kb
