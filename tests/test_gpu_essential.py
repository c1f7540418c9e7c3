"""Essential dynamics on the device (csrc/essential.hip through ops and forecast) against tests/essential_ref.py, the numpy
restatement of include/mdno_essential.h whose sums run in long double.

Gates (derived in the helper's docstring; first-order bounds for n rounded products summed in ANY order, u = 2^-53):
    covariance   |C - C_ref|[a, b] <= (K + 2) u sum |x~_a| |x~_b|     with the mean passed in (the same bits on both sides)
    column sums  |s - s_ref|[a]    <= R u sum |x[:, a]|
    projection   |P - P_ref|[r, c] <= (D + 2) u sum_a |x~_a| |V_ac|
    superposition  rmsd^2 inside the project's 8 * 2^-52 * G of the reference; the un-rotated RMS distance of `aligned` to
                 the reference at most rmsd_ref + 2 * 2^-24 * rms|aligned| (one fp32 rounding per coordinate; the factor 2
                 covers the fp64 rotation error); pair distances inside `aligned` those of the input to fp32 rounding,
                 4 * 2^-24 * max|aligned| (two endpoints, each off by at most sqrt(3) 2^-24 max|aligned|).
Every test prints its largest ratio.

Shapes: the smallest at which a kernel can go wrong — D at 1, 2, 3, 5 and around one and two tiles of 32, the reference's
84 (nine tiles at a lag, six at lag 0) and one case at the workload's 1,512; K at 1, 3, 4, 5 and at c - 1, c, c + 1, 2 c + 1
for the row chunk c of the header, and at 256 c - 1 and 256 c + 2 where the number of splits stops growing; lags 0, 1, S - 1,
S; one and three members.  Every (a, b) has its own expected value and C(lag > 0) is far from symmetric, so a transposed
tile, a swapped operand or the f32 lane map on the f64 MFMA fails everywhere."""
import functools

import numpy as np
import pytest
import torch

import cross_rmsd_ref as cref
import essential_ref as ref

pytestmark = pytest.mark.gpu

TILE, CHUNK, MAX_SPLITS, MAX_K = 32, 64, 256, 32           # test_header_constants holds them to ops (and the host test to the header)
U53 = 2.0 ** -53

# (S, M, D, lag): K = M (S - lag)
COV_SHAPES = [
    (1, 1, 1, 0), (2, 1, 2, 1), (1, 3, 3, 0), (4, 3, 5, 3), (4, 1, 31, 0), (6, 1, 32, 1),                  # K = 1, 1, 3, 3, 4, 5
    (21, 3, 33, 0), (22, 3, 65, 1), (64, 1, 84, 0), (65, 1, 84, 1), (66, 1, 65, 1), (65, 1, 33, 0),        # K = 63, 63, 64, 64, 65, 65
    (43, 3, 84, 0), (44, 3, 84, 1), (130, 1, 32, 129), (130, 1, 2, 1),                                     # K = 129, 129, 1, 129
    (5462, 3, 5, 1), (5463, 3, 3, 1), (16386, 1, 1, 0),                                                    # K = 256 c - 1, 256 c + 2
    (5, 3, 31, 5), (5, 3, 84, 7), (0, 3, 5, 0), (4, 0, 5, 0),                                              # lag >= S, no rows: zeros
    (33, 3, 1512, 0),                                                                                      # K = 99 at the workload's D
]


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def on(dev, x):
    return torch.from_numpy(np.array(x, order="C")).to(dev)                # (a copy: the shared inputs are read-only)


def bits(x):
    return x.contiguous().view(torch.int64) if x.dtype == torch.float64 else x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def test_header_constants():
    from molecular_dynamics_neural_operator_amd import ops
    assert (ops.PCA_TILE, ops.PCA_ROW_CHUNK, ops.PCA_MAX_SPLITS, ops.PCA_MAX_COMPONENTS) == (TILE, CHUNK, MAX_SPLITS, MAX_K)
    ks = {M * max(S - lag, 0) for S, M, D, lag in COV_SHAPES}
    assert {0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, MAX_SPLITS * CHUNK - 1, MAX_SPLITS * CHUNK + 2} <= ks
    assert {1, 2, 3, 5, 31, 32, 33, 65, 84, 1512} <= {s[2] for s in COV_SHAPES}
    assert ops.covariance_row_split(MAX_SPLITS * CHUNK - 1, 5, 1) == (CHUNK, MAX_SPLITS)
    assert ops.covariance_row_split(MAX_SPLITS * CHUNK + 2, 3, 1) == (2 * CHUNK, MAX_SPLITS // 2 + 1)


# ================================================================================================ 1. covariance
@functools.lru_cache(maxsize=None)
def cov_case(S, M, D, lag):
    """(X f32 [S, M, D], mean f64 [D], reference sums, bound, K): computed once, shared, never written to."""
    X = ref.features(S, M, D, seed=100000 * lag + 1000 * D + 10 * S + M)
    mean = X.astype(np.float64).reshape(-1, D).mean(axis=0) if S * M else np.zeros(D)
    C, bound, K = ref.covariance_sums(X, mean, lag)
    for a in (X, mean, C, bound):
        a.setflags(write=False)
    return X, mean, C, bound, K


@pytest.mark.parametrize("S,M,D,lag", COV_SHAPES)
def test_covariance_equals_the_restatement(dev, S, M, D, lag):
    from molecular_dynamics_neural_operator_amd import ops
    X, mean, want, bound, K = cov_case(S, M, D, lag)
    x, mu = on(dev, X), on(dev, mean)
    got_t = ops.feature_covariance(x, mu, lag)
    got = got_t.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (D, D)
    if K == 0:
        assert not got.any() and not np.signbit(got).any()
        return
    d = np.abs(got - want)
    ratio = float((d[bound > 0] / (U53 * bound[bound > 0])).max()) if (bound > 0).any() else 0.0
    L, splits = ops.covariance_row_split(K, D, lag)
    print(f"S={S} M={M} D={D} lag={lag}: K={K}, {splits} split(s) of {L} rows, largest |dC| / (2^-53 sum|x~||x~|) = {ratio:.3f} "
          f"(allowed {K + 2})")
    assert np.all(d <= (K + 2) * U53 * bound)
    # every (a, b) has its own value, and at a lag C is far from symmetric: a transposed tile cannot pass
    if D > 1 and K > 1:
        off = ~np.eye(D, dtype=bool)
        assert len(np.unique(want[np.triu(off)])) == D * (D - 1) // 2
        if lag > 0:
            asym = np.abs(want - want.T)[off]
            assert np.median(asym) > 1e6 * (K + 2) * U53 * np.median(bound[off])
    if lag == 0:
        assert same(got_t, got_t.T.contiguous())                                             # bitwise symmetric
        assert np.all(np.diag(got) >= 0)
    # the same bits on a second call, and whatever the workspace held before
    assert same(ops.feature_covariance(x, mu, lag), got_t)
    if D <= 84:
        from molecular_dynamics_neural_operator_amd import _lib
        lib = _lib.load()
        nbytes = lib.mdnopca_covariance_workspace_bytes(S, M, D, lag)
        for fill in (0xFF, 0x00, 0x7F):
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
            out = torch.full((D, D), float("nan"), dtype=torch.float64, device=dev)
            assert lib.mdnopca_covariance(_lib.ptr(x), S, M, D, _lib.ptr(mu), lag, _lib.ptr(out), _lib.ptr(ws), nbytes,
                                          _lib.stream_ptr(dev)) == 0
            assert same(out, got_t), fill


def test_covariance_of_a_plain_stack_and_of_frames(dev):
    """[F, D] is one member; forecast.covariance takes frames [S, M, N, 3] as D = 3 N features and forms the mean on the
    device: the sums stay inside the gate of the restatement fed the DEVICE's mean, and the mean inside its own gate."""
    from molecular_dynamics_neural_operator_amd import forecast, ops
    X, mean, want, bound, K = cov_case(44, 3, 84, 1)
    flat = np.ascontiguousarray(X[:, 0])
    got = ops.feature_covariance(on(dev, flat), on(dev, mean), 2)
    w2, b2, K2 = ref.covariance_sums(flat[:, None], mean, 2)
    assert K2 == 42 and np.all(np.abs(got.cpu().numpy() - w2) <= (K2 + 2) * U53 * b2)
    frames = on(dev, X.reshape(44, 3, 28, 3))
    for lag in (0, 1):
        c = forecast.covariance(frames, lag=lag)
        assert c.n == 3 * (44 - lag) and c.lag == lag and c.sums.shape == (84, 84) and c.mean.dtype == torch.float64
        s_ref, s_bound, _ = ref.feature_sums(X.reshape(-1, 84))
        assert np.all(np.abs(c.mean.cpu().numpy() * 132.0 - s_ref) <= (132 + 2) * U53 * s_bound)
        w, b, K = ref.covariance_sums(X, c.mean.cpu().numpy(), lag)
        assert np.all(np.abs(c.sums.cpu().numpy() - w) <= (K + 2) * U53 * b)
        assert same(c.sums, forecast.covariance(on(dev, X), c.mean, lag).sums)              # [S, M, D] is the same call
        assert same(c.matrix(), c.sums / float(K - 1 if lag == 0 else K))
    assert c.rmsf().shape == (28,) and same(forecast.covariance(frames[:, 0].contiguous(), lag=1).sums,
                                            forecast.covariance(on(dev, np.ascontiguousarray(X[:, 0])), lag=1).sums)


# ================================================================================================ 2. column sums
@pytest.mark.parametrize("R,D", [(1, 1), (15, 16), (16, 17), (17, 15), (63, 84), (64, 1), (65, 33), (1000, 84), (3, 1512), (0, 5)])
def test_feature_sums_equal_the_restatement(dev, R, D):
    from molecular_dynamics_neural_operator_amd import ops
    X = ref.features(R, 1, D, seed=7 * R + D)[:, 0]
    want, bound, n_bad = ref.feature_sums(X)
    x = on(dev, X)
    got_t, bad = ops.feature_sums(x)
    got = got_t.cpu().numpy()
    assert got.shape == (D,) and got.dtype == np.float64 and bad.dtype == torch.int64 and bad.tolist() == [0] == [n_bad]
    d = np.abs(got - want)
    ratio = float((d[bound > 0] / (U53 * bound[bound > 0])).max()) if (bound > 0).any() else 0.0
    print(f"R={R} D={D}: largest |d sum| / (2^-53 sum|x|) = {ratio:.3f} (allowed {R})")
    assert np.all(d <= R * U53 * bound)
    assert same(ops.feature_sums(x)[0], got_t)
    if R == 0:
        assert not got.any()


def test_feature_sums_count_the_invalid_rows(dev):
    from molecular_dynamics_neural_operator_amd import ops
    X = ref.features(70, 1, 40, seed=3)[:, 0].copy()
    X[3, 5], X[3, 17], X[40, 5], X[69, 39] = np.nan, np.inf, -np.inf, np.inf
    want, bound, n_bad = ref.feature_sums(X)
    got, bad = ops.feature_sums(on(dev, X))
    got = got.cpu().numpy()
    assert n_bad == 3 and bad.tolist() == [3]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.flatnonzero(np.isnan(got)).tolist() == [5, 17, 39]
    ok = ~np.isnan(want)
    assert np.all(np.abs(got - want)[ok] <= 70 * U53 * bound[ok])


# ================================================================================================ 3. projection
@pytest.mark.parametrize("R,D,k", [(1, 1, 1), (15, 63, 10), (16, 64, 16), (17, 65, 17), (100, 84, 32), (33, 1512, 10), (5, 3, 2)])
def test_projection_equals_the_restatement(dev, R, D, k):
    from molecular_dynamics_neural_operator_amd import ops
    X = ref.features(R, 1, D, seed=11 * R + D)[:, 0]
    rng = np.random.default_rng(R + D + k)
    mean, V = X.astype(np.float64).mean(axis=0), rng.normal(size=(D, k))
    want, bound = ref.project(X, mean, V)
    x, mu, v = on(dev, X), on(dev, mean), on(dev, V)
    got_t = ops.project_features(x, mu, v)
    got = got_t.cpu().numpy()
    assert got.shape == (R, k) and got.dtype == np.float64
    d = np.abs(got - want)
    ratio = float((d[bound > 0] / (U53 * bound[bound > 0])).max()) if (bound > 0).any() else 0.0
    print(f"R={R} D={D} k={k}: largest |dP| / (2^-53 sum|x~||V|) = {ratio:.3f} (allowed {D + 2})")
    assert np.all(d <= (D + 2) * U53 * bound)
    assert same(ops.project_features(x, mu, v), got_t)
    assert len(np.unique(want)) == R * k                                                     # every (r, c) has its own value


def test_projection_refusals_and_empty_shapes(dev):
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    x, mu = torch.zeros((4, 6), device=dev), torch.zeros(6, dtype=torch.float64, device=dev)
    for k in (0, MAX_K + 1):
        with pytest.raises(MdnoError, match="k ="):
            ops.project_features(x, mu, torch.zeros((6, k), dtype=torch.float64, device=dev))
    with pytest.raises(MdnoError, match="vectors"):
        ops.project_features(x, mu, torch.zeros((5, 2), dtype=torch.float64, device=dev))
    with pytest.raises(MdnoError, match="mean"):
        ops.project_features(x, mu[:5], torch.zeros((6, 2), dtype=torch.float64, device=dev))
    assert ops.project_features(x[:0], mu, torch.ones((6, 2), dtype=torch.float64, device=dev)).shape == (0, 2)
    p = ops.project_features(x[:, :0].contiguous(), mu[:0], torch.ones((0, 2), dtype=torch.float64, device=dev))
    assert p.shape == (4, 2) and not p.any()
    with pytest.raises(MdnoError, match="lag"):
        ops.feature_covariance(x, mu, -1)
    assert ops.feature_covariance(x[:, :0].contiguous(), mu[:0]).shape == (0, 0)


# ================================================================================================ 4. superposition
SUPERPOSE_SHAPES = [(1, 1, 1), (2, 1, 2), (3, 3, 3), (1, 2, 4), (43, 3, 5), (3, 3, 28), (2, 2, 63), (9, 1, 64), (4, 2, 65), (3, 2, 504)]


@functools.lru_cache(maxsize=None)
def superpose_case(S, M, N):
    """(frames f32 [F, N, 3] = the S M frames of cross_rmsd_ref.stacked followed by its three reference frames — the cloud
    itself, its exact rigid copy, its mirror image —, the kinds, reference f32 [N, 3] = the cloud, reference rmsd^2, G)."""
    A, B, ka, kb = cref.stacked(S, M, N, 3, seed=77 * N + S)
    frames = np.concatenate([A.reshape(S * M, N, 3), B])
    kinds = [k for row in ka for k in row] + list(kb)
    r2, G = cref.rmsd2_matrix(frames, B[:1])
    for a in (frames, r2, G):
        a.setflags(write=False)
    return frames, kinds, B[0], r2[:, 0], G[:, 0]


@pytest.mark.parametrize("S,M,N", SUPERPOSE_SHAPES)
def test_superposition_meets_its_bounds(dev, S, M, N):
    """S M + 3 frames: 4 (one wave), ..., 9 = two workgroups' worth + 1, 132 frames."""
    from molecular_dynamics_neural_operator_amd import forecast, ops
    frames, kinds, reference, r2_ref, G = superpose_case(S, M, N)
    F = frames.shape[0]
    f, q = on(dev, frames), on(dev, reference)
    aligned_t, rmsd_t = forecast.superpose(f, q)
    aligned, rmsd = aligned_t.cpu().numpy(), rmsd_t.cpu().numpy()
    assert aligned.shape == (F, 1, N, 3) and aligned.dtype == np.float32 and rmsd.shape == (F, 1) and rmsd.dtype == np.float64
    aligned, rmsd = aligned[:, 0], rmsd[:, 0]
    assert np.isfinite(aligned).all() and np.isfinite(rmsd).all()                            # degenerate frames included
    d = np.abs(rmsd ** 2 - r2_ref)
    assert np.all(d[G == 0] == 0)
    ratio = float((d[G > 0] / (cref.U52 * G[G > 0])).max()) if (G > 0).any() else 0.0
    assert np.all(d <= cref.GATE * G)
    al = aligned.astype(np.float64)
    dist = np.sqrt(((al - reference.astype(np.float64)) ** 2).sum(axis=(1, 2)) / N)
    slack = 2.0 * 2.0 ** -24 * np.sqrt((al ** 2).sum(axis=(1, 2)) / N)
    over = float(((dist - np.sqrt(r2_ref)) / np.where(slack > 0, slack, 1.0)).max())
    print(f"S={S} M={M} N={N}: largest |d rmsd^2| / (2^-52 G) = {ratio:.3f} (allowed 8); largest (RMS distance - rmsd_ref) / "
          f"(2^-24 rms|aligned|) = {2 * over:.3f} (allowed 2)")
    assert np.all(dist <= np.sqrt(r2_ref) + slack)
    # a rigid image of the input: pair distances to fp32 rounding (every frame up to 65 atoms, a dozen frames above)
    for i in range(F if N <= 65 else min(F, 12)):
        tol = 4.0 * 2.0 ** -24 * np.abs(al[i]).max()
        assert np.all(np.abs(ref.pair_distances(aligned[i]) - ref.pair_distances(frames[i])) <= tol), (i, kinds[i])
    # the cloud itself and its exact rigid copy come to rest on the reference; a mirror image does NOT
    assert kinds[-3:] == ["identical", "rigid copy", "mirror image"]
    for i in (F - 3, F - 2):
        assert rmsd[i] ** 2 <= cref.GATE * G[i] and np.abs(al[i] - reference).max() <= 2.0 * 2.0 ** -24 * max(np.abs(al[i]).max(), 1e-30)
    if N >= 5:
        assert rmsd[F - 1] ** 2 * N > 1e-2 * G[F - 1]
    # each output alone has the bits it has beside the other; a second call too; [S, M, N, 3] is the same frames
    assert same(ops.superpose_frames(f, q, aligned=True, rmsd=False)[0], aligned_t) and ops.superpose_frames(f, q, True, False)[1] is None
    assert same(ops.superpose_frames(f, q, aligned=False, rmsd=True)[1], rmsd_t)
    a4, r4 = forecast.superpose(on(dev, frames[:S * M].reshape(S, M, N, 3)), q)
    assert same(a4.reshape(S * M, 1, N, 3), aligned_t[:S * M]) and same(r4.reshape(S * M, 1), rmsd_t[:S * M])
    # a frame with a NaN, another with an Inf: NaN frames and NaN rmsd, every other frame's bits unchanged
    if F >= 4:
        dirty = frames.copy()
        dirty[1, N // 2, 1], dirty[F - 1, 0, 2] = np.nan, np.inf
        a2, r2 = forecast.superpose(on(dev, dirty), q)
        keep = [i for i in range(F) if i not in (1, F - 1)]
        assert torch.isnan(a2[[1, F - 1]]).all() and torch.isnan(r2[[1, F - 1]]).all()
        assert same(a2[keep], aligned_t[keep]) and same(r2[keep], rmsd_t[keep])


def test_superposition_edge_cases(dev):
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    frames, kinds, reference, r2_ref, G = superpose_case(3, 3, 28)
    f = on(dev, frames)
    for bad in (np.nan, np.inf):                                                             # a non-finite reference: NaN everywhere
        q = reference.copy()
        q[27, 2] = bad
        a, r = forecast.superpose(f, on(dev, q))
        assert torch.isnan(a).all() and torch.isnan(r).all()
    a, r = forecast.superpose(torch.zeros((4, 2, 0, 3), device=dev), torch.zeros((0, 3), device=dev))     # N == 0
    assert a.shape == (4, 2, 0, 3) and r.shape == (4, 2) and not r.any()
    a, r = forecast.superpose(torch.zeros((0, 2, 5, 3), device=dev), torch.zeros((5, 3), device=dev))
    assert a.shape == (0, 2, 5, 3) and r.shape == (0, 2)
    with pytest.raises(MdnoError, match="reference"):
        forecast.superpose(f, on(dev, reference[:27]))
    with pytest.raises(MdnoError, match="no output"):
        ops.superpose_frames(f, on(dev, reference), False, False)


# ================================================================================================ 5. end to end
def test_pca_recovers_two_planted_modes(dev):
    """100 steps x 3 members of a 10-atom structure moving along two planted orthogonal modes (amplitudes 3 and 1.5, noise
    0.02), every frame under its own random rigid motion: superpose + covariance + pca on the device against the numpy
    restatement of the same pipeline (Kabsch in fp64, rounded once to fp32 like the device's frames)."""
    from molecular_dynamics_neural_operator_amd import forecast
    S, M, N = 100, 3, 10
    frames, base, e = ref.planted_modes(S, M, N, seed=5)
    aligned, rmsd = forecast.superpose(on(dev, frames), on(dev, base))
    cov = forecast.covariance(aligned)
    comp = forecast.pca(cov, 2)
    want_al = np.stack([ref.superpose_kabsch(p, base)[0] for p in frames.reshape(-1, N, 3)]).astype(np.float32)
    assert np.abs(aligned.cpu().numpy().reshape(-1, N, 3) - want_al).max() <= 2.0 * 2.0 ** -24 * np.abs(want_al).max()
    C, mean, K = ref.covariance(aligned.cpu().numpy().reshape(S, M, 3 * N))
    w, v = ref.pca(C, 2)
    cos = (comp.vectors.cpu().numpy() * v).sum(axis=0)                                       # signed: the same sign convention
    rel = np.abs(comp.values.cpu().numpy() - w) / w
    print(f"planted modes: 1 - cos = {1 - cos}, relative eigenvalue error = {rel}, explained = {comp.explained_ratio().tolist()}")
    assert np.all(cos >= 1 - 1e-9) and np.all(rel <= 1e-9)
    # and they ARE the planted directions, up to the sampling error of 300 frames: the angle between an estimated and a
    # true principal axis is about sqrt(l1 l2) / ((l1 - l2) sqrt(K)) = 4.5 / 6.75 / 17 = 0.04 rad, cos 0.999: 0.99 leaves room
    planted = np.abs(comp.vectors.cpu().numpy().T @ e.T)
    assert planted[0, 0] >= 0.99 and planted[1, 1] >= 0.99 and float(comp.explained_ratio().sum()) > 0.95
    # projections: the restatement on the same components; their variances are the eigenvalues
    P = forecast.project(aligned, comp)
    assert P.shape == (S, M, 2) and P.dtype == torch.float64
    pw, pb = ref.project(aligned.cpu().numpy().reshape(S * M, 3 * N), comp.mean.cpu().numpy(), comp.vectors.cpu().numpy())
    assert np.all(np.abs(P.cpu().numpy().reshape(-1, 2) - pw) <= (3 * N + 2) * U53 * pb)
    assert np.allclose(P.reshape(-1, 2).var(0, unbiased=True).cpu().numpy(), comp.values.cpu().numpy(), rtol=1e-9)
    F, counts, edges = forecast.free_energy(P, bins=8)
    assert int(counts.sum()) == S * M and counts.device == P.device and float(F.min()) == 0.0
    Fh, ch, eh = forecast.free_energy(P.cpu(), bins=8, range=((float(edges[0, 0]), float(edges[0, -1])), (float(edges[1, 0]), float(edges[1, -1]))))
    assert torch.equal(ch, counts.cpu()) and float(forecast.histogram_total_variation(counts, counts)) == 0.0
    # TICA on the same frames runs through the rank deficiency the superposition leaves (six rigid-body directions)
    t = forecast.tica(cov, forecast.covariance(aligned, cov.mean, lag=1), 2)
    tw, tv = ref.tica(C, ref.covariance(aligned.cpu().numpy().reshape(S, M, 3 * N), 1, mean)[0], 2)
    assert torch.isfinite(t.vectors).all() and np.allclose(t.values.cpu().numpy(), tw, rtol=0, atol=1e-7)


def _engine_inputs(M):
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    N, W = 28, 3
    base = syn.chain_frame(N, seed=1)
    traj = syn.ou_trajectory(base, W + 6, seed=2)
    wins = syn.ensemble_windows(traj[:W], M, sigma=0.1, seed0=100)              # [M, W, N, 3]
    reference = torch.from_numpy(np.ascontiguousarray(traj[W]).astype(np.float32))
    return torch.from_numpy(np.ascontiguousarray(wins.transpose(1, 0, 2, 3))), torch.from_numpy(syn.amino_acids(N, seed=1)), reference


def _model(dev):
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    model = KernelNN(64, 128, 2, 6, 7, 3, 20, 4)
    model.load_state_dict(near_identity_state_dict(64, 128, seed=0, kernel_gain=1e-3, feature_gain=0.1))
    return model.eval().to(dev)


def test_engines_equal_their_stated_composition(dev):
    """A noisy 4-step, 8-member, N = 28 run: both engines' superpose and covariance equal the forecast composition on
    produced(...) bit for bit, also from a non-zero first step, at a lag and with the mean passed in; the trajectory buffer
    is unchanged."""
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine, RolloutEngine
    wins, aa, reference = _engine_inputs(8)
    reference = reference.to(dev)
    model = _model(dev)
    for cls in (RolloutEngine, GroupedRolloutEngine):
        eng = cls(model, 8, 28, 3, 8.0, max_steps=4, device=dev, noise_sigma=0.05, noise_seed=7)
        eng.run(wins, aa, 4)
        before = eng.frames().clone()
        if cls is GroupedRolloutEngine:
            assert len(eng.engines) == 2
        for first, steps, lag in ((0, None, 0), (0, None, 1), (1, 2, 0), (1, 3, 2)):
            n = 4 - first if steps is None else steps
            produced = eng.produced(first, n).contiguous()
            wa, wr = forecast.superpose(produced, reference)
            a, r = eng.superpose(reference, first, steps)
            assert same(a, wa) and same(r, wr) and a.shape == (n, 8, 28, 3), (cls.__name__, first, steps)
            want = forecast.covariance(wa, None, lag)
            got = eng.covariance(reference, lag=lag, first_step=first, steps=steps)
            assert same(got.sums, want.sums) and same(got.mean, want.mean) and (got.n, got.lag) == (want.n, lag) == (8 * (n - lag), lag)
            given = eng.covariance(reference, mean=want.mean, lag=lag, first_step=first, steps=steps)
            assert same(given.sums, want.sums)
        assert bool(torch.isfinite(got.sums).all()) and torch.equal(eng.frames(), before)
        eng.close()


# ================================================================================================ 6. guard bands
def _run_guarded(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import ops
    res = []
    with Guard(fill, record_calls=False) as G:
        for S, M, D, lag in ((44, 3, 84, 1), (43, 3, 84, 0), (22, 3, 65, 1), (1, 1, 1, 0), (65, 1, 33, 0)):
            X, mean = cov_case(S, M, D, lag)[:2]
            x, mu = G.place(on(dev, X)), G.place(on(dev, mean))
            res.append(ops.feature_covariance(x, mu, lag).clone())
            res.append(ops.feature_sums(x.reshape(S * M, D))[0].clone())
            v = G.place(on(dev, np.random.default_rng(D).normal(size=(D, min(D, 17)))))
            res.append(ops.project_features(x.reshape(S * M, D), mu, v).clone())
        for S, M, N in ((3, 3, 28), (4, 2, 65), (1, 1, 1)):
            frames, kinds, reference = superpose_case(S, M, N)[:3]
            res.extend(t.clone() for t in ops.superpose_frames(G.place(on(dev, frames)), G.place(on(dev, reference))))
        G.verify()
    return res


def test_essential_entry_points_stay_inside_their_buffers(dev):
    """Every input, output and workspace inside guard bands under both fill bytes: every band intact and every result
    identical under 0x00 and 0xFF (nothing unset is read)."""
    from guarded import FILLS
    a, b = (_run_guarded(dev, fill) for fill in FILLS)
    assert len(a) == len(b) == 5 * 3 + 3 * 2
    for i, (u, v) in enumerate(zip(a, b)):
        assert not torch.isnan(u.double()).any() and same(u, v), i
