"""numpy restatement of include/mdno_essential.h for tests/test_essential_host.py and tests/test_gpu_essential.py (a helper
module like cross_rmsd_ref.py: no fixtures, no settings).

Covariance, column sums and projection accumulate in np.longdouble (80-bit extended where the platform has it: a 64-bit
significand, so the reference's own error is 2^-11 of an fp64 rounding per term and negligible beside the gates); the
centring x - mean is done in fp64 exactly as the header states it, so both sides multiply the SAME centred values.

THE GATES (first-order bounds for n rounded products summed in ANY order, u = 2^-53):
    covariance   |C - C_ref|[a, b] <= (K + 2) u sum_r |x~[r, a]| |x~[r', b]|
    column sums  |s - s_ref|[a]    <= R u sum_r |x[r, a]|
    projection   |P - P_ref|[r, c] <= (D + 2) u sum_a |x~[r, a]| |V[a, c]|
A sum of n terms carries at most (n - 1) roundings of partial sums, each at most u times the sum of the absolute terms, and
every product one more: n u sum |terms| to first order; the + 2 is room for the second-order terms at these sizes.

Superposition takes two routes that share no step after the centring and must agree: Horn's quaternion eigenvector
(np.linalg.eigh of the 4 x 4 matrix) and Kabsch by SVD with the determinant correction."""
import numpy as np

import cross_rmsd_ref as cref

U53 = 2.0 ** -53
LD = np.longdouble


# ------------------------------------------------------------------------------------------------ covariance
def centred_pairs(X, mean, lag):
    """X f32 [S, M, D], mean f64 [D] -> (A, B) f64 [K, D]: the centred rows t and t + lag of every member, K = M (S - lag)."""
    S, M, D = X.shape
    n = max(S - lag, 0)
    xc = X.astype(np.float64) - np.asarray(mean, dtype=np.float64)
    return xc[:n].reshape(n * M, D), xc[lag:lag + n].reshape(n * M, D)


def covariance_sums(X, mean, lag=0):
    """(C f64 [D, D] rounded once from the long-double sums, bound f64 [D, D] = sum |x~_a| |x~_b|, K)."""
    A, B = centred_pairs(X, mean, lag)
    C = A.astype(LD).T @ B.astype(LD)
    return C.astype(np.float64), np.abs(A).T @ np.abs(B), A.shape[0]


def feature_sums(X):
    """X f32 [R, D] -> (sum f64 [D], bound f64 [D] = sum |x|, number of rows with a non-finite value)."""
    bad = ~np.isfinite(X).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        s = X.astype(LD).sum(axis=0).astype(np.float64)
        s = np.where(np.isfinite(X).all(axis=0), s, np.nan)
        return s, np.abs(X.astype(np.float64)).sum(axis=0), int(bad.sum())


def project(X, mean, V):
    """X f32 [R, D], mean f64 [D], V f64 [D, k] -> (P f64 [R, k], bound f64 [R, k] = sum_a |x~_a| |V_ac|)."""
    xc = X.astype(np.float64) - np.asarray(mean, dtype=np.float64)
    return (xc.astype(LD) @ V.astype(LD)).astype(np.float64), np.abs(xc) @ np.abs(V)


def covariance(X, lag=0, mean=None):
    """The host-side estimate forecast.Covariance.matrix() gives: (matrix, mean, n)."""
    S, M, D = X.shape
    if mean is None:
        mean = (X.astype(LD).reshape(S * M, D).sum(axis=0) / (S * M)).astype(np.float64)
    C, _, K = covariance_sums(X, mean, lag)
    return C / (K - 1 if lag == 0 else K), mean, K


def pca(C, k):
    """(values descending [k], vectors [D, k]) of the symmetric C, every vector's largest-magnitude entry positive."""
    w, v = np.linalg.eigh(0.5 * (C + C.T))
    w, v = w[::-1][:k], v[:, ::-1][:, :k]
    return w, v * np.where(v[np.abs(v).argmax(axis=0), np.arange(v.shape[1])] < 0, -1.0, 1.0)


def tica(C0, Ct, k, eps=1e-10):
    """(values descending [k], vectors [D, k]): whiten with the eigenpairs of C0 above eps * lambda_max, eigh of the
    whitened symmetrised Ct."""
    w, u = np.linalg.eigh(0.5 * (C0 + C0.T))
    keep = w > eps * w[-1]
    W = u[:, keep] / np.sqrt(w[keep])
    lam, q = np.linalg.eigh(W.T @ (0.5 * (Ct + Ct.T)) @ W)
    return lam[::-1][:k], (W @ q[:, ::-1])[:, :k]


def rmsip(V, W):
    return float(np.sqrt(((V.T @ W) ** 2).sum() / V.shape[1]))


# ------------------------------------------------------------------------------------------------ superposition
def quaternion_rotation(q):
    q0, q1, q2, q3 = q / np.linalg.norm(q)
    return np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                     [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                     [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])


def superpose_horn(P, Q):
    """P, Q [N, 3] -> (aligned f64 [N, 3] = R (p - c_p) + c_q, rmsd^2 = max(0, G - 2 lambda) / N, G): the quaternion route."""
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    cp, cq = P.mean(0), Q.mean(0)
    a, b = P - cp, Q - cq
    G = (a ** 2).sum() + (b ** 2).sum()
    w, v = np.linalg.eigh(cref.horn((a.T @ b)[None])[0])
    return a @ quaternion_rotation(v[:, -1]).T + cq, max(0.0, G - 2.0 * w[-1]) / P.shape[0], G


def superpose_kabsch(P, Q):
    """The same three by SVD with the determinant correction (the rotation takes P onto Q)."""
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    cp, cq = P.mean(0), Q.mean(0)
    a, b = P - cp, Q - cq
    U, _, Vt = np.linalg.svd(a.T @ b)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T
    out = a @ R.T
    return out + cq, ((out - b) ** 2).sum() / P.shape[0], (a ** 2).sum() + (b ** 2).sum()


def pair_distances(x):
    """x [N, 3] -> the N (N - 1) / 2 pair distances, f64."""
    x = x.astype(np.float64)
    i, j = np.triu_indices(x.shape[0], 1)
    return np.sqrt(((x[i] - x[j]) ** 2).sum(1))


# ------------------------------------------------------------------------------------------------ inputs
def features(S, M, D, seed):
    """f32 [S, M, D]: a seeded random walk per member and column (so that a lag matters and C(lag) is far from symmetric:
    column b is driven by column b - 1's past) about a per-column offset of tens of Angstrom (so that centring matters)."""
    rng = np.random.default_rng(seed)
    offset = rng.uniform(-40.0, 40.0, size=D)
    scale = rng.uniform(0.5, 2.0, size=D)
    x = np.zeros((S, M, D))
    step = rng.normal(size=(S, M, D))
    for t in range(S):
        prev = x[t - 1] if t else np.zeros((M, D))
        x[t] = 0.5 * prev + step[t] + 0.4 * np.roll(prev, 1, axis=1)                   # (spectral radius 0.9: stationary)
    return (offset + scale * x).astype(np.float32)


def planted_modes(S, M, N, seed, amplitudes=(3.0, 1.5), noise=0.02):
    """A toy trajectory with two planted collective modes: frames f32 [S, M, N, 3] = a base structure + a_1(t) e_1 +
    a_2(t) e_2 + small noise, every frame under its own random rigid motion; also the base f32 [N, 3] and the unit mode
    vectors e f64 [2, 3 N].  The modes are orthogonal to each other and to the six rigid-body directions of the base (to
    first order a superposition removes nothing of them)."""
    rng = np.random.default_rng(seed)
    base = cref.grid_cloud(N, rng)
    base = base - base.mean(0)
    rigid = [np.tile(np.eye(3)[d], N) for d in range(3)] + [np.cross(np.eye(3)[d], base).reshape(-1) for d in range(3)]
    basis = []
    for v in rigid + [rng.normal(size=3 * N) for _ in range(2)]:
        for b in basis:
            v = v - (v @ b) * b
        basis.append(v / np.linalg.norm(v))
    e = np.stack(basis[6:])
    frames = np.empty((S, M, N, 3), np.float32)
    for s in range(S):
        for m in range(M):
            amp = rng.normal(size=2) * np.asarray(amplitudes)
            x = base + (amp @ e).reshape(N, 3) + rng.normal(scale=noise, size=(N, 3))
            frames[s, m] = x @ cref.rotation(rng).T + rng.normal(size=3) * 10
    return frames, base.astype(np.float32), e


def ar1(S, phi, seed, D=1):
    """x_{t+1} = phi x_t + noise, stationary start, f32 [S, D] (independent columns)."""
    rng = np.random.default_rng(seed)
    x = np.empty((S, D))
    x[0] = rng.normal(size=D) / np.sqrt(1.0 - phi * phi)
    for t in range(1, S):
        x[t] = phi * x[t - 1] + rng.normal(size=D)
    return x.astype(np.float32)
