"""Essential dynamics without a GPU: what is particular to include/mdno_essential.h and its ctypes table (that header,
table and exports agree is tests/test_cabi_tables.py's); every refusal of the header comes back before any device work; the workspace size is
monotone and independent of the row count; the row-split rule of ops.covariance_row_split obeys the header's bounds; and
forecast.Covariance, pca, tica, rmsip and free_energy hold on closed-form toys fed from the numpy restatement
(tests/essential_ref.py) on CPU tensors."""
import math
import re

import numpy as np
import pytest
import torch

import cross_rmsd_ref as cref
import essential_ref as ref
from cabi import CSRC, INCLUDE, lib  # noqa: F401  (lib: the fixture)

HEADER = INCLUDE / "mdno_essential.h"
NAMES = {"mdnopca_superpose", "mdnopca_feature_sums", "mdnopca_covariance_workspace_bytes", "mdnopca_covariance", "mdnopca_project"}
FAKE = 0x10000          # a made-up address: nothing may dereference it
BIG = 1 << 62
IMAX = (1 << 31) - 1


def test_essential_header_table_and_exports_agree(lib):
    """What is particular to this header; that header, table and exports agree is tests/test_cabi_tables.py's."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    assert set(_lib.ESSENTIAL_SIGNATURES) == NAMES
    assert lib.mdno_abi_version() == 15 == _lib.ABI_VERSION and lib.mdno_train_abi_version() == 1 == _lib.TRAIN_ABI_VERSION
    assert (CSRC / "essential.hip").exists()                                              # inside the library's content hash
    text = HEADER.read_text()
    for name, value in (("TILE", ops.PCA_TILE), ("ROW_PASS", ops.PCA_ROW_PASS), ("ROW_CHUNK", ops.PCA_ROW_CHUNK),
                        ("TARGET_WORKGROUPS", ops.PCA_TARGET_WORKGROUPS), ("MAX_SPLITS", ops.PCA_MAX_SPLITS),
                        ("SUM_PARTIALS", ops.PCA_SUM_PARTIALS), ("MAX_COMPONENTS", ops.PCA_MAX_COMPONENTS)):
        assert int(re.search(rf"#define MDNO_PCA_{name} (\d+)", text).group(1)) == value, name
    assert ops.PCA_MAX_COMPONENTS >= 16 and ops.PCA_ROW_CHUNK % ops.PCA_ROW_PASS == 0
    assert "mdnopca_" in text and "prefix" in text.lower()                                # the header says why the names differ


def test_the_rotation_solve_sits_beside_the_eigenvalue_solve():
    """rotation_from_moments is the second function of csrc/superpose.h; essential.hip includes it and defines none."""
    holders = [f.name for f in sorted(CSRC.iterdir()) if f.suffix in (".hip", ".h")
               and re.search(r"double\s+rotation_from_moments\s*\(", f.read_text())]
    assert holders == ["superpose.h"]
    text = (CSRC / "essential.hip").read_text()
    assert '#include "superpose.h"' in text and "rotation_from_moments(" in text
    assert "mfma_f64_16x16x4f64" in text and "atomicAdd(" not in re.sub(r"atomicAdd\(n_invalid", "", text)   # no float atomics


def superpose(lib, frames=FAKE, S=3, M=2, N=4, reference=FAKE, aligned=FAKE, rmsd=FAKE):
    return lib.mdnopca_superpose(frames, S, M, N, reference, aligned, rmsd, None)


def sums(lib, x=FAKE, R=5, D=4, total=FAKE, n_invalid=FAKE):
    return lib.mdnopca_feature_sums(x, R, D, total, n_invalid, None)


def cov(lib, x=FAKE, S=6, M=2, D=5, mean=FAKE, lag=1, c=FAKE, ws=FAKE, ws_bytes=BIG):
    return lib.mdnopca_covariance(x, S, M, D, mean, lag, c, ws, ws_bytes, None)


def proj(lib, x=FAKE, R=5, D=4, mean=FAKE, v=FAKE, k=2, p=FAKE):
    return lib.mdnopca_project(x, R, D, mean, v, k, p, None)


def test_entry_points_refuse_before_device_work(lib):
    """No pointer below is a device pointer: a call that got as far as a launch would fault, not return a code."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    E, U = _lib.EINVAL, _lib.EUNSUPPORTED
    err = lib.mdno_last_error
    # superpose
    for kw in ({"S": -1}, {"M": -1}, {"N": -1}):
        assert superpose(lib, **kw) == E, kw
    assert superpose(lib, aligned=None, rmsd=None) == E and b"no output" in err()
    for kw in ({"frames": None}, {"reference": None}):
        assert superpose(lib, **kw) == E and b"null pointer" in err(), kw
    assert superpose(lib, S=IMAX, M=IMAX) == U and b"grid" in err()
    assert superpose(lib, S=IMAX, M=IMAX, aligned=None, rmsd=None) == E                    # (the argument checks come first)
    assert superpose(lib, S=0, frames=None, reference=None) == 0 and superpose(lib, M=0, frames=None, reference=None) == 0
    # feature_sums
    for kw in ({"R": -1}, {"D": -1}):
        assert sums(lib, **kw) == E, kw
    for kw in ({"x": None}, {"total": None}, {"n_invalid": None}, {"n_invalid": None, "R": 0, "D": 0}):
        assert sums(lib, **kw) == E and b"null pointer" in err(), kw
    # covariance
    for kw in ({"S": -1}, {"M": -1}, {"D": -1}, {"lag": -1}):
        assert cov(lib, **kw) == E, kw
    for kw in ({"x": None}, {"mean": None}, {"c": None}, {"c": None, "S": 0}):
        assert cov(lib, **kw) == E and b"null pointer" in err(), kw
    for lag in (0, 1):
        need = lib.mdnopca_covariance_workspace_bytes(6, 2, 5, lag)
        assert need >= 8 * ops.PCA_TILE ** 2
        assert cov(lib, lag=lag, ws_bytes=need - 1) == E and b"workspace" in err()
        assert cov(lib, lag=lag, ws=None) == E and b"workspace" in err()
        assert cov(lib, lag=lag, ws_bytes=0) == E
    assert cov(lib, S=IMAX, M=IMAX, D=IMAX) == U and b"grid" in err()                       # 2^52 tiles
    assert cov(lib, S=IMAX, M=IMAX, D=IMAX, lag=0) == U and b"grid" in err()
    assert cov(lib, S=IMAX, M=IMAX, D=IMAX, lag=-1) == E                                   # (the argument checks come first)
    assert cov(lib, D=0, x=None, mean=None, c=None, ws=None, ws_bytes=0) == 0               # C is empty: nothing to write
    # project
    for kw in ({"R": -1}, {"D": -1}, {"k": 0}, {"k": -1}, {"k": ops.PCA_MAX_COMPONENTS + 1}):
        assert proj(lib, **kw) == E, kw
    assert proj(lib, k=0) == E and b"outside" in err()
    for kw in ({"x": None}, {"mean": None}, {"v": None}, {"p": None}):
        assert proj(lib, **kw) == E and b"null pointer" in err(), kw
    assert proj(lib, R=16 * (1 << 31)) == U and b"grid" in err()
    assert proj(lib, R=0, x=None, mean=None, v=None, p=None) == 0


def test_workspace_bytes_are_monotone_and_independent_of_the_rows(lib):
    from molecular_dynamics_neural_operator_amd import ops
    f = lib.mdnopca_covariance_workspace_bytes
    tile = 8 * ops.PCA_TILE ** 2
    base = dict(S=100, M=8, D=84)
    for lag in (0, 1, 7, 100, 101):
        b0 = f(*base.values(), lag)
        for key in base:
            prev = 0
            for scale in (1, 2, 3, 7, 40, 128):
                args = dict(base)
                args[key] = base[key] * scale
                cur = f(*args.values(), lag)
                assert cur >= prev and cur >= b0, (key, scale)
                prev = cur
        assert f(1, 1, 84, lag) == b0 == f(IMAX, IMAX, 84, lag)                             # the bound does not depend on K
    prev = 0
    for D in list(range(0, 200)) + [504, 1511, 1512, 1513, 4096, 1 << 20, IMAX]:
        cur = f(100, 8, D, 0)
        assert cur >= prev, D
        prev = cur
        # whatever K is, tiles x splits partial tiles fit
        for lag in (0, 1):
            for K in (1, 63, 64, 65, 129, 1000, 64000, 10 ** 9):
                L, splits = ops.covariance_row_split(K, D, lag)
                T = -(-D // ops.PCA_TILE)
                tiles = T * (T + 1) // 2 if lag == 0 else T * T
                assert tiles * splits * tile <= cur or cur == (1 << 64) - 1, (D, lag, K)
                if D:
                    assert L % ops.PCA_ROW_CHUNK == 0 and (splits - 1) * L < K <= splits * L and splits <= ops.PCA_MAX_SPLITS
    assert f(-1, 8, 84, 0) == 0 and f(100, -1, 84, 0) == 0 and f(100, 8, -1, 0) == 0 and f(100, 8, 84, -1) == 0
    assert f(100, 8, 0, 0) == 0 and f(100, 8, 1, 0) > 0
    # the workload: 64 members x 1,000 steps x 1,512 coordinates stays far below the 774 MB fp64 copy it replaces
    assert f(1000, 64, 1512, 0) < 64 * 1024 * 1024
    # the reference's N = 28: nine tiles at a lag, six at lag 0, and the rows ARE split
    assert ops.covariance_row_split(64000, 84, 1)[1] > 100 and ops.covariance_row_split(64000, 84, 0)[1] > 100
    assert ops.covariance_row_split(129, 84, 1) == (64, 3) and ops.covariance_row_split(64, 84, 1) == (64, 1)


def test_python_arguments_are_checked_without_a_device():
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    x, y = torch.zeros(6, 4, 5, 3), torch.zeros(5, 3)
    feats, mean, vec = torch.zeros(6, 4, 15), torch.zeros(15, dtype=torch.float64), torch.zeros(15, 2, dtype=torch.float64)
    comps = forecast.Components(torch.ones(2, dtype=torch.float64), vec, mean, 1.0)
    for fn in (lambda: ops.superpose_frames(x, y), lambda: forecast.superpose(x, y), lambda: ops.feature_sums(feats[0]),
               lambda: ops.feature_covariance(feats, mean), lambda: forecast.covariance(x), lambda: forecast.covariance(feats, lag=1),
               lambda: ops.project_features(feats[0], mean, vec), lambda: forecast.project(x, comps)):
        with pytest.raises(MdnoError, match="CPU tensor"):
            fn()
    with pytest.raises(MdnoError, match="torch tensor"):
        ops.superpose_frames(x.numpy(), y)
    with pytest.raises(MdnoError, match="expected"):
        forecast.covariance(torch.zeros(2, 3, 4, 5, 3))


def cov_of(X, lag=0, mean=None):
    """forecast.Covariance fed from the numpy restatement (CPU tensors)."""
    from molecular_dynamics_neural_operator_amd.forecast import Covariance
    if mean is None:
        mean = ref.covariance(X)[1]
    sums, _, K = ref.covariance_sums(X, mean, lag)
    return Covariance(torch.from_numpy(mean), torch.from_numpy(sums), K, lag)


def test_covariance_arithmetic_on_a_diagonal_toy():
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    # three independent columns with variances 9, 4, 1 exactly: +-3, +-2, +-1 in all eight sign patterns, twice (M = 2)
    rows = np.array([[sx * 3.0, sy * 2.0, sz * 1.0] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)
    X = np.stack([rows + np.float32(10.0), rows[::-1] + np.float32(10.0)], axis=1)          # [8, 2, 3] about an offset
    c = cov_of(X)
    assert c.n == 16 and c.lag == 0 and c.mean.tolist() == [10.0, 10.0, 10.0]
    assert torch.equal(c.sums, torch.diag(torch.tensor([144.0, 64.0, 16.0], dtype=torch.float64)))
    assert torch.equal(c.matrix(), c.sums / 15.0) and torch.equal(c.symmetrized(), c.matrix())
    assert torch.allclose(c.rmsf(), torch.tensor([math.sqrt(224.0 / 15.0)], dtype=torch.float64), rtol=1e-15)
    lagged = cov_of(X, lag=1)
    assert lagged.n == 14 and torch.equal(lagged.matrix(), lagged.sums / 14.0)
    assert torch.equal(lagged.symmetrized(), 0.5 * (lagged.matrix() + lagged.matrix().T))
    p = forecast.pca(c, 3)
    assert torch.allclose(p.values, torch.tensor([144.0, 64.0, 16.0], dtype=torch.float64) / 15.0, rtol=1e-14)
    assert torch.equal(p.vectors.abs().round(), torch.eye(3, dtype=torch.float64)) and (p.vectors.diagonal() > 0).all()
    assert torch.allclose(p.explained_ratio(), torch.tensor([144.0, 64.0, 16.0], dtype=torch.float64) / 224.0, rtol=1e-14)
    assert p.mean is c.mean and p.cpu().vectors.shape == (3, 2 + 1)
    two = forecast.pca(c, 2)
    assert two.vectors.shape == (3, 2) and abs(float(two.explained_ratio().sum()) - 208.0 / 224.0) < 1e-14
    with pytest.raises(MdnoError, match="D = 3 N"):
        cov_of(X[:, :, :2]).rmsf()
    with pytest.raises(MdnoError, match="lag-0"):
        forecast.pca(lagged, 1)
    for k in (0, 4, True, 1.0):
        with pytest.raises(MdnoError, match="k ="):
            forecast.pca(c, k)
    with pytest.raises(MdnoError, match="no lag"):
        p.timescales()


def test_rmsip_of_identical_and_orthogonal_subspaces():
    from molecular_dynamics_neural_operator_amd.forecast import Components
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    q, _ = np.linalg.qr(np.random.default_rng(5).normal(size=(12, 12)))
    mean = torch.zeros(12, dtype=torch.float64)
    mk = lambda cols: Components(torch.ones(len(cols), dtype=torch.float64), torch.from_numpy(np.ascontiguousarray(q[:, cols])), mean, 1.0)
    a = mk([0, 1, 2])
    assert abs(a.rmsip(a) - 1.0) < 1e-14
    rot = np.linalg.qr(np.random.default_rng(6).normal(size=(3, 3)))[0]                      # the same subspace, another basis
    same = Components(a.values, torch.from_numpy(q[:, :3] @ rot), mean, 1.0)
    assert abs(a.rmsip(same) - 1.0) < 1e-14
    assert a.rmsip(mk([3, 4, 5])) < 1e-14                                                    # orthogonal subspaces
    assert abs(a.rmsip(mk([0, 1, 7])) - math.sqrt(2.0 / 3.0)) < 1e-14                        # two of three shared
    assert abs(a.rmsip(mk([0, 1, 7])) - ref.rmsip(q[:, [0, 1, 2]], q[:, [0, 1, 7]])) < 1e-15
    with pytest.raises(MdnoError, match="rmsip"):
        a.rmsip(mk([0, 1]))


def test_sign_convention_and_its_ties():
    from molecular_dynamics_neural_operator_amd import forecast
    # C = [[2, -1], [-1, 2]]: eigenvectors (1, -1) / sqrt 2 (value 3) and (1, 1) / sqrt 2 (value 1): both entries tie in
    # magnitude, so the LOWEST index decides: entry 0 is made positive
    c = forecast.Covariance(torch.zeros(2, dtype=torch.float64), torch.tensor([[2.0, -1.0], [-1.0, 2.0]], dtype=torch.float64), 2, 0)
    p = forecast.pca(c, 2)
    assert torch.allclose(p.values, torch.tensor([3.0, 1.0], dtype=torch.float64), rtol=1e-14)
    assert (p.vectors[0] > 0).all() and p.vectors[1, 0] < 0 and p.vectors[1, 1] > 0
    v = torch.tensor([[0.5, -0.5, 0.1], [-0.5, 0.5, -0.9], [0.5, 0.5, 0.2], [-0.5, -0.5, 0.3]], dtype=torch.float64)
    fixed = forecast._fix_signs(v.clone())
    assert torch.equal(fixed[:, 0], v[:, 0]) and torch.equal(fixed[:, 1], -v[:, 1]) and torch.equal(fixed[:, 2], -v[:, 2])
    # and the restatement follows the same rule
    w, vec = ref.pca(c.matrix().numpy(), 2)
    assert np.allclose(vec, p.vectors.numpy(), atol=1e-15) and np.allclose(w, p.values.numpy())


def test_tica_recovers_the_ar1_autocorrelation():
    """x_{t+1} = phi x_t + noise: the TICA eigenvalue at lag tau is phi^tau up to the sampling error of the seeded series.
    The tolerance comes from the restatement on the SAME series: forecast.tica must agree with it to rounding, and the
    restatement's own distance from phi^tau is bounded by 4 standard errors of a lag-tau autocorrelation estimate,
    sqrt((1 + phi^2tau) / n) at most (Bartlett), over n = 20,000 samples."""
    from molecular_dynamics_neural_operator_amd import forecast
    S, tau = 20000, 3
    phis = (0.95, 0.6)
    X = np.stack([ref.ar1(S, phis[0], 11)[:, 0], ref.ar1(S, phis[1], 12)[:, 0]], axis=1)[:, None] * np.float32([2.0, 0.5]) + np.float32(30.0)
    X = X.astype(np.float32)                                                                 # [S, 1, 2]
    c0, ct = cov_of(X), cov_of(X, lag=tau)
    t = forecast.tica(c0, ct, 2)
    want, vec = ref.tica(ref.covariance(X)[0], ref.covariance(X, tau, c0.mean.numpy())[0], 2)
    assert np.allclose(t.values.numpy(), want, rtol=0, atol=1e-12)
    for c in range(2):
        got = t.vectors[:, c].numpy()
        assert abs(abs(vec[:, c] @ got) / (np.linalg.norm(vec[:, c]) * np.linalg.norm(got)) - 1.0) < 1e-9
    for value, phi in zip(t.values.tolist(), phis):
        tol = 4.0 * math.sqrt((1.0 + phi ** (2 * tau)) / (1.0 - phi * phi) / S)             # inflated by the series' memory
        print(f"phi={phi}: TICA eigenvalue {value:.5f}, phi^tau {phi ** tau:.5f}, allowed {tol:.5f}")
        assert abs(value - phi ** tau) <= tol
    ts = t.timescales()
    assert t.lag == tau and torch.allclose(ts, -tau / torch.log(t.values.abs()))
    assert abs(float(ts[0]) - (-1.0 / math.log(phis[0]))) < 0.25 * (-1.0 / math.log(phis[0]))
    # C(0)-orthonormal vectors
    g = t.vectors.T @ c0.symmetrized() @ t.vectors
    assert torch.allclose(g, torch.eye(2, dtype=torch.float64), atol=1e-10)


def test_tica_on_a_rank_deficient_covariance_does_not_blow_up():
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    S = 4000
    x = np.stack([ref.ar1(S, 0.9, 21)[:, 0], ref.ar1(S, 0.3, 22)[:, 0]], axis=1).astype(np.float64)
    mix = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [2.0, -1.0], [0.0, 0.0]]).T          # five columns of rank two
    X = (x @ mix).astype(np.float32)[:, None]
    c0, ct = cov_of(X), cov_of(X, lag=2)
    assert np.linalg.matrix_rank(c0.matrix().numpy(), tol=1e-6) == 2
    t = forecast.tica(c0, ct, 2, eps=1e-6)
    assert torch.isfinite(t.values).all() and torch.isfinite(t.vectors).all() and t.total == 2.0
    assert (t.values.abs() <= 1.0 + 1e-9).all() and float(t.vectors.abs().max()) < 1e3
    assert abs(float(t.values[0]) - 0.9 ** 2) < 0.1 and abs(float(t.values[1]) - 0.3 ** 2) < 0.1
    with pytest.raises(MdnoError, match="k ="):
        forecast.tica(c0, ct, 3, eps=1e-6)                                                   # only two dimensions are kept
    with pytest.raises(MdnoError, match="lags"):
        forecast.tica(ct, ct, 1)


def test_free_energy_bins_exactly():
    from molecular_dynamics_neural_operator_amd import forecast
    # points on bin edges and inside: range [0, 4] x [0, 2], 4 x 4 bins of 1.0 x 0.5
    P = torch.tensor([[0.0, 0.0, 9.0], [1.0, 0.5, 9.0], [0.999999, 0.49999, 9.0], [4.0, 2.0, 9.0], [3.5, 1.75, 9.0], [3.5, 1.75, 9.0],
                      [4.0000001, 1.0, 9.0], [2.0, float("nan"), 9.0], [-1e-9, 0.0, 9.0]], dtype=torch.float64)
    F, counts, edges = forecast.free_energy(P, 0, 1, bins=4, range=((0.0, 4.0), (0.0, 2.0)))
    want = torch.zeros(4, 4, dtype=torch.int64)
    want[0, 0], want[1, 1], want[3, 3] = 2, 1, 3
    assert counts.dtype == torch.int64 and torch.equal(counts, want)
    assert edges.shape == (2, 5) and edges[0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and edges[1].tolist() == [0.0, 0.5, 1.0, 1.5, 2.0]
    assert F[3, 3] == 0.0 and abs(float(F[0, 0]) - math.log(1.5)) < 1e-15 and abs(float(F[1, 1]) - math.log(3.0)) < 1e-15
    assert torch.isinf(F[0, 1]) and F[0, 1] > 0
    # the data's own extent by default; the other component pair; leading dimensions are flattened
    F2, counts2, edges2 = forecast.free_energy(P[:6].reshape(2, 3, 3), 1, 0, bins=2)
    assert int(counts2.sum()) == 6 and edges2[0].tolist() == [0.0, 1.0, 2.0] and edges2[1].tolist() == [0.0, 2.0, 4.0]
    assert counts2.tolist() == [[3, 0], [0, 3]]
    tv = forecast.histogram_total_variation
    assert float(tv(counts, counts)) == 0.0 and float(tv(counts, 7 * counts)) == 0.0
    other = torch.zeros_like(counts)
    other[2, 0] = 5
    assert float(tv(counts, other)) == 1.0
    half = counts.clone()
    half[2, 0] = 6
    assert abs(float(tv(counts, half)) - 0.5) < 1e-15


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 28, 63, 64, 65, 504])
def test_the_two_superposition_routes_agree(N):
    """Horn's eigenvector against Kabsch by SVD on the stacked families: rmsd^2 inside the project's gate of each other, and
    where the optimum is unique (no degenerate family) the aligned coordinates too."""
    A, B, ka, kb = cref.stacked(3, 2, N, 3, seed=N)
    Q = B[0]
    worst = 0.0
    for s in range(3):
        for m in range(2):
            a1, r1, G = ref.superpose_horn(A[s, m], Q)
            a2, r2, _ = ref.superpose_kabsch(A[s, m], Q)
            assert abs(r1 - r2) <= cref.GATE * G, (N, ka[s][m])
            worst = max(worst, abs(r1 - r2) / G if G > 0 else 0.0)
            for al in (a1, a2):                                                              # both are rigid images of the frame
                assert np.allclose(ref.pair_distances(al), ref.pair_distances(A[s, m]), rtol=1e-12, atol=1e-12)
                res = ((al - Q.astype(np.float64)) ** 2).sum() / N
                assert abs(res - r1) <= 1e-9 * max(G, 1.0) / N + 1e-6 * r1                   # the residual IS the rmsd^2
            if N >= 5 and ka[s][m] in ("noise", "rotated and translated", "offset 1e3", "identical"):
                assert np.allclose(a1, a2, atol=1e-6 * max(1.0, np.abs(a1).max())), (N, ka[s][m])
    print(f"N={N}: Horn against Kabsch, largest |d rmsd^2| / (2^-52 G) = {worst / cref.U52:.3f} (allowed 8)")
