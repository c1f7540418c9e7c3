"""Markov state models without a GPU: what is particular to include/mdno_markov.h and its ctypes table (that header,
table and exports agree is tests/test_cabi_tables.py's); every refusal of the header comes back before any device work; the workspace sizes are
monotone; forecast.MarkovModel holds on closed-form chains; and the bookkeeping of the transition counts is checked on
the numpy restatement (tests/markov_ref.py) fed through forecast.TransitionCounts on CPU tensors."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import markov_ref as ref
from cabi import CSRC, INCLUDE, lib  # noqa: F401  (lib: the fixture)

HEADER = INCLUDE / "mdno_markov.h"
NAMES = {"mdnomsm_assign_workspace_bytes", "mdnomsm_assign", "mdnomsm_kcenters_workspace_bytes", "mdnomsm_kcenters",
         "mdnomsm_centroid_sums", "mdnomsm_transition_counts"}
FAKE = 0x10000          # a made-up address: nothing may dereference it
BIG = 1 << 62
IMAX = (1 << 31) - 1
SIZE_MAX = (1 << 64) - 1


def test_markov_header_table_and_exports_agree(lib):
    """What is particular to this header; that header, table and exports agree is tests/test_cabi_tables.py's."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    assert set(_lib.MARKOV_SIGNATURES) == NAMES
    assert lib.mdno_abi_version() == 15 == _lib.ABI_VERSION and lib.mdno_train_abi_version() == 1 == _lib.TRAIN_ABI_VERSION
    assert (CSRC / "markov.hip").exists()                                                     # inside the library's content hash
    text = HEADER.read_text()
    for name, value in (("MAX_STATES", ops.MSM_MAX_STATES), ("ROW_TILE", ops.MSM_ROW_TILE), ("CENTRE_TILE", ops.MSM_CENTRE_TILE),
                        ("FEATURE_PASS", ops.MSM_FEATURE_PASS), ("ARGMAX_TILE", ops.MSM_ARGMAX_TILE),
                        ("SUM_PARTIALS", ops.MSM_SUM_PARTIALS), ("SUM_FEATURES", ops.MSM_SUM_FEATURES),
                        ("SUM_STATES", ops.MSM_SUM_STATES), ("LDS_STATES", ops.MSM_LDS_STATES), ("MAX_LAGS", ops.MSM_MAX_LAGS)):
        assert int(re.search(rf"#define MDNO_MSM_{name} (\d+)", text).group(1)) == value, name
    assert ops.MSM_MAX_STATES >= 1024 and ops.MSM_MAX_LAGS == ops.MAX_LAGS == 1024
    assert _lib.MARKOV_DTYPES == {"float32": int(re.search(r"#define MDNO_MSM_F32 (\d+)", text).group(1)),
                                  "float64": int(re.search(r"#define MDNO_MSM_F64 (\d+)", text).group(1))}
    assert "mdnomsm_" in text and "prefix" in text.lower()                                    # the header says why the names differ
    src = (CSRC / "markov.hip").read_text()
    assert '#include "../../include/mdno_markov.h"' in src and "mfma_f64_16x16x4f64" in src
    assert not re.search(r"atomicAdd\([^;]*\b(double|float)\b", src)                          # integer atomics only


def assign(lib, x=FAKE, R=5, D=4, dtype=0, centres=FAKE, k=3, origin=FAKE, label=FAKE, dist2=FAKE, ws=FAKE, ws_bytes=BIG):
    return lib.mdnomsm_assign(x, R, D, dtype, centres, k, origin, label, dist2, ws, ws_bytes, None)


def kcen(lib, x=FAKE, R=9, D=4, dtype=0, k=3, first=0, index=FAKE, radius=FAKE, ws=FAKE, ws_bytes=BIG):
    return lib.mdnomsm_kcenters(x, R, D, dtype, k, first, index, radius, ws, ws_bytes, None)


def csum(lib, x=FAKE, R=9, D=4, dtype=0, label=FAKE, k=3, sums=FAKE, counts=FAKE):
    return lib.mdnomsm_centroid_sums(x, R, D, dtype, label, k, sums, counts, None)


def trans(lib, label=FAKE, S=9, M=2, n=3, lags=(1, 2), L=None, pooled=0, counts=FAKE, skipped=FAKE):
    arr = None if lags is None else (C.c_int32 * max(len(lags), 1))(*lags)
    return lib.mdnomsm_transition_counts(label, S, M, n, arr, len(lags) if L is None else L, pooled, counts, skipped, None)


def test_entry_points_refuse_before_device_work(lib):
    """No device pointer below is a device pointer: a call that got as far as a launch would fault, not return a code."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    E, U = _lib.EINVAL, _lib.EUNSUPPORTED
    err = lib.mdno_last_error
    top = ops.MSM_MAX_STATES
    # assign
    for kw in ({"R": -1}, {"D": -1}, {"k": -1}, {"dtype": 2}, {"dtype": -1}, {"k": top + 1}):
        assert assign(lib, **kw) == E, kw
    assert assign(lib, dtype=7) == E and b"dtype" in err()
    assert assign(lib, label=None, dist2=None) == E and b"no output" in err()
    for kw in ({"x": None}, {"centres": None}):
        assert assign(lib, **kw) == E and b"null pointer" in err(), kw
    need = lib.mdnomsm_assign_workspace_bytes(5, 3, 4)
    assert need >= 5 * 12
    for kw in ({"ws": None}, {"ws_bytes": need - 1}, {"ws_bytes": 0}):
        assert assign(lib, **kw) == E and b"workspace" in err(), kw
    assert assign(lib, R=ops.MSM_ROW_TILE * (1 << 31)) == U and b"grid" in err()
    assert assign(lib, R=ops.MSM_ROW_TILE * (1 << 31), dtype=3) == E                         # (the argument checks come first)
    assert assign(lib, R=0, x=None, centres=None, ws=None, ws_bytes=0) == 0                   # R == 0 touches nothing
    # kcenters
    for kw in ({"R": -1}, {"D": -1}, {"dtype": 2}, {"k": 0}, {"k": -1}, {"k": top + 1, "R": top + 5}, {"k": 10}, {"first": -1},
               {"first": 9}, {"R": 0, "k": 1}):
        assert kcen(lib, **kw) == E, kw
    assert kcen(lib, k=10) == E and b"centres of" in err()
    assert kcen(lib, first=9) == E and b"first" in err()
    for kw in ({"x": None}, {"index": None}, {"radius": None}):
        assert kcen(lib, **kw) == E and b"null pointer" in err(), kw
    need = lib.mdnomsm_kcenters_workspace_bytes(9, 4)
    assert need >= 9 * 8 + 16
    for kw in ({"ws": None}, {"ws_bytes": need - 1}):
        assert kcen(lib, **kw) == E and b"workspace" in err(), kw
    assert kcen(lib, R=ops.MSM_ARGMAX_TILE * (1 << 31)) == U and b"grid" in err()
    # centroid_sums
    for kw in ({"R": -1}, {"D": -1}, {"dtype": 5}, {"k": 0}, {"k": top + 1}):
        assert csum(lib, **kw) == E, kw
    for kw in ({"x": None}, {"label": None}, {"sums": None}, {"counts": None}):
        assert csum(lib, **kw) == E and b"null pointer" in err(), kw
    # transition_counts
    for kw in ({"S": -1}, {"M": -1}, {"n": 0}, {"n": top + 1}, {"L": 0}, {"L": ops.MAX_LAGS + 1}, {"lags": (1, 0)}, {"lags": (-3,)},
               {"lags": None, "L": 1}):
        assert trans(lib, **kw) == E, kw
    assert trans(lib, lags=(2, 0)) == E and b"below 1" in err()
    for kw in ({"label": None}, {"counts": None}, {"skipped": None}):
        assert trans(lib, **kw) == E and b"null pointer" in err(), kw
    assert trans(lib, M=65536) == U and b"grid" in err()


def test_workspace_bytes_are_monotone(lib):
    from molecular_dynamics_neural_operator_amd import ops
    f, g = lib.mdnomsm_assign_workspace_bytes, lib.mdnomsm_kcenters_workspace_bytes
    prev = 0
    for R in (0, 1, 63, 64, 65, 1000, 64000, 10 ** 9):
        inner = 0
        for k in (0, 1, 63, 64, 65, 100, 1000, ops.MSM_MAX_STATES):
            cur = f(R, k, 10)
            assert cur >= inner and cur == f(R, k, 1512) == f(R, k, 0), (R, k)       # independent of D
            tiles = -(-k // ops.MSM_CENTRE_TILE)
            assert cur >= tiles * R * 12 and cur <= tiles * R * 12 + 512
            inner = cur
        assert inner >= prev
        prev = inner
        assert g(R, 10) == g(R, 1512) >= (R * 8 if R else 0)
    assert [g(R, 3) for R in (0, 1, 255, 256, 257, 10 ** 6)] == sorted(g(R, 3) for R in (0, 1, 255, 256, 257, 10 ** 6))
    assert f(-1, 3, 4) == 0 and f(5, -1, 4) == 0 and f(5, 3, -1) == 0 and f(5, ops.MSM_MAX_STATES + 1, 4) == 0
    assert g(-1, 4) == 0 and g(5, -1) == 0
    assert f(1 << 62, ops.MSM_MAX_STATES, 4) == SIZE_MAX
    # the workload: 64 members x 1,000 steps against 1,000 centres stays far below the 512 MB distance matrix it replaces
    assert f(64000, 1000, 1512) < 16 * 1024 * 1024


def test_python_arguments_are_checked_without_a_device():
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    x, c = torch.zeros(6, 4), torch.zeros(3, 4)
    frames = torch.zeros(6, 2, 5, 3)
    lab = torch.zeros(6, dtype=torch.int32)
    for fn in (lambda: ops.assign_features(x, c), lambda: forecast.assign(frames, torch.zeros(3, 15)), lambda: ops.kcenters(x, 2),
               lambda: forecast.kcenters(frames, 2), lambda: forecast.kmeans(x, 2), lambda: ops.centroid_sums(x, lab, 3),
               lambda: ops.transition_counts(lab, 3, [1]), lambda: forecast.transition_counts(lab.reshape(3, 2), 3, [1]),
               lambda: forecast.discretize(frames, 2)):
        with pytest.raises(MdnoError, match="CPU tensor"):
            fn()
    with pytest.raises(MdnoError, match="torch tensor"):
        ops.assign_features(x.numpy(), c)
    with pytest.raises(MdnoError, match="method"):
        forecast.discretize(frames, 2, method="dbscan")
    for lags in ([], [0], [1.5], list(range(1, ops.MAX_LAGS + 2))):
        with pytest.raises(MdnoError, match="lag"):
            ops.check_msm_lags(lags)
    assert ops.check_msm_lags(torch.tensor([1, 5])) == [1, 5]


def counts_of(labels, n, lags, pooled=False):
    """forecast.TransitionCounts fed from the numpy restatement (CPU tensors)."""
    from molecular_dynamics_neural_operator_amd.forecast import TransitionCounts
    counts, skipped = ref.transition_counts(labels, n, lags, pooled)
    return TransitionCounts(torch.from_numpy(counts), torch.from_numpy(skipped), tuple(lags))


def from_matrix(c, lag=1, more=()):
    from molecular_dynamics_neural_operator_amd.forecast import TransitionCounts
    mats = [np.asarray(c, np.int64)] + [np.asarray(m, np.int64) for _, m in more]
    return TransitionCounts(torch.from_numpy(np.stack(mats)[:, None]), torch.zeros(len(mats), dtype=torch.int64),
                            (lag,) + tuple(l for l, _ in more))


def test_two_state_chain_in_closed_form():
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    tc = from_matrix([[90, 10], [20, 80]], lag=5)
    m = forecast.markov_model(tc, reversible=False)
    assert m.lag == 5 and m.active.tolist() == [0, 1] and not m.reversible
    assert torch.allclose(m.T, torch.tensor([[0.9, 0.1], [0.2, 0.8]], dtype=torch.float64), rtol=0, atol=1e-16)
    assert torch.allclose(m.stationary(), torch.tensor([2.0 / 3.0, 1.0 / 3.0], dtype=torch.float64), atol=1e-14)
    assert abs(complex(m.eigenvalues[0]) - 1.0) < 1e-14 and abs(complex(m.eigenvalues[1]) - 0.7) < 1e-14
    ts = m.timescales(1)
    assert ts.shape == (1,) and abs(float(ts[0]) - (-5.0 / math.log(0.7))) < 1e-12
    assert torch.allclose(m.free_energies(), torch.tensor([0.0, math.log(2.0)], dtype=torch.float64), atol=1e-14)
    # the reversible estimate of the same counts: (C + C^T) = [[180, 30], [30, 160]]
    r = forecast.markov_model(tc)
    assert r.reversible and torch.allclose(r.T, torch.tensor([[180 / 210, 30 / 210], [30 / 190, 160 / 190]], dtype=torch.float64), atol=1e-16)
    assert torch.allclose(r.pi, torch.tensor([210 / 400, 190 / 400], dtype=torch.float64), atol=1e-16)
    lam2 = 180 / 210 + 160 / 190 - 1.0                                             # trace - 1
    assert r.eigenvalues.dtype == torch.float64 and abs(float(r.eigenvalues[0]) - 1.0) < 1e-14 and abs(float(r.eigenvalues[1]) - lam2) < 1e-14
    assert torch.allclose(r.pi @ r.T, r.pi, atol=1e-15)                            # stationary, and detailed balance:
    flux = r.pi[:, None] * r.T
    assert torch.allclose(flux, flux.T, atol=1e-16)
    # the limits of the timescales: lambda = 1 -> inf, lambda = 0 -> 0
    edge = forecast.MarkovModel(3, 3, torch.arange(3), torch.eye(3, dtype=torch.float64), torch.tensor([1.0, 1.0, 0.0], dtype=torch.float64),
                                torch.full((3,), 1 / 3, dtype=torch.float64), True)
    assert edge.timescales().tolist() == [float("inf"), 0.0]
    with pytest.raises(MdnoError, match="k ="):
        m.timescales(2)
    with pytest.raises(MdnoError, match="lag_index"):
        forecast.markov_model(tc, lag_index=1)


def test_three_cycle_is_not_reversible_and_symmetrising_makes_it_real():
    from molecular_dynamics_neural_operator_amd import forecast
    tc = from_matrix([[0, 30, 0], [0, 0, 30], [30, 0, 0]])
    m = forecast.markov_model(tc, reversible=False)
    assert m.active.tolist() == [0, 1, 2] and m.eigenvalues.is_complex()
    lam = sorted(m.eigenvalues.tolist(), key=lambda z: z.imag)
    roots = [complex(-0.5, -math.sqrt(3) / 2), complex(1.0, 0.0), complex(-0.5, math.sqrt(3) / 2)]
    assert all(abs(a - b) < 1e-12 for a, b in zip(lam, roots))                     # the cube roots of unity: all |lambda| = 1
    assert (m.timescales() > 1e12).all()                                           # (|lambda| = 1 up to rounding: never decays)
    assert torch.allclose(m.stationary(), torch.full((3,), 1 / 3, dtype=torch.float64), atol=1e-14)
    r = forecast.markov_model(tc)
    assert not r.eigenvalues.is_complex()
    assert torch.allclose(r.T, torch.tensor([[0, .5, .5], [.5, 0, .5], [.5, .5, 0]], dtype=torch.float64), atol=1e-16)
    assert torch.allclose(r.eigenvalues, torch.tensor([1.0, -0.5, -0.5], dtype=torch.float64), atol=1e-14)
    assert torch.allclose(r.timescales(), torch.full((2,), -1.0 / math.log(0.5), dtype=torch.float64), rtol=1e-12)


def test_active_set_and_its_tie_rule():
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    # states {1, 4} and {2, 5} form two disconnected blocks of the same size, 0 is never visited, 3 is only entered (from 2)
    c = np.zeros((6, 6), np.int64)
    c[1, 4], c[4, 1], c[1, 1], c[4, 4] = 5, 5, 10, 10
    c[2, 5], c[5, 2], c[2, 2], c[5, 5] = 7, 7, 3, 3
    c[2, 3] = 1
    m = forecast.markov_model(from_matrix(c))
    assert m.active.tolist() == [1, 4] and m.n_states == 6                         # the tie goes to the set with the lowest state
    assert m.stationary().tolist() == [0.0, 0.5, 0.0, 0.0, 0.5, 0.0]
    c[5, 3], c[3, 5] = 1, 1                                                        # now 3 joins {2, 5}: the larger set wins
    m2 = forecast.markov_model(from_matrix(c))
    assert m2.active.tolist() == [2, 3, 5]
    assert forecast._largest_connected_set(torch.from_numpy(c)) == [2, 3, 5]
    one_way = np.zeros((3, 3), np.int64)
    one_way[0, 1], one_way[1, 2] = 4, 4                                            # a chain that is only walked down: singletons
    assert forecast.markov_model(from_matrix(one_way), reversible=False).active.tolist() == [0]
    with pytest.raises(MdnoError, match="no transition"):
        forecast.markov_model(from_matrix(np.zeros((3, 3), np.int64)))
    # populations compared over the union of the active sets
    assert float(m.population_total_variation(m)) == 0.0
    assert abs(float(m.population_total_variation(m2)) - 1.0) < 1e-15
    half = np.zeros((6, 6), np.int64)
    half[1, 1], half[1, 2], half[2, 1], half[2, 2] = 10, 5, 5, 10                  # shares state 1 (weight 1/2 in both)
    assert abs(float(m.population_total_variation(forecast.markov_model(from_matrix(half)))) - 0.5) < 1e-15


def test_chapman_kolmogorov_is_zero_for_counts_built_from_the_square():
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    # T = [[3/4, 1/4], [1/4, 3/4]] and T^2 = [[5/8, 3/8], [3/8, 5/8]]: 64 origins per state, every figure a dyadic rational
    tc = from_matrix([[48, 16], [16, 48]], lag=2, more=((4, [[40, 24], [24, 40]]), (6, [[36, 28], [28, 36]]), (5, [[1, 0], [0, 1]])))
    for reversible in (True, False):
        m = forecast.markov_model(tc, reversible=reversible)
        assert m.chapman_kolmogorov(tc, 1).tolist() == [0.0, 0.0]
        assert m.chapman_kolmogorov(tc, 0).tolist() == [0.0, 0.0]                  # n = 1: the model itself
        # T^3 = [[9/16, 7/16], [7/16, 9/16]] = 36/64, 28/64
        assert m.chapman_kolmogorov(tc, 2).tolist() == [0.0, 0.0]
        with pytest.raises(MdnoError, match="multiple"):
            m.chapman_kolmogorov(tc, 3)
    off = from_matrix([[48, 16], [16, 48]], lag=2, more=((4, [[48, 16], [16, 48]]),))   # too slow at the double lag
    assert forecast.markov_model(off).chapman_kolmogorov(off, 1).tolist() == [0.125, 0.125]


@pytest.mark.parametrize("S,M", [(1, 1), (2, 3), (7, 1), (8, 3), (40, 4)])
def test_transition_count_bookkeeping(S, M):
    from molecular_dynamics_neural_operator_amd import forecast
    rng = np.random.default_rng(S * 10 + M)
    n = 4
    labels = rng.integers(-1, n + 1, size=(S, M)).astype(np.int32)                  # -1 and n are out of range
    lags = [1, 2, 7, 8, 50]
    per, pooled = counts_of(labels, n, lags), counts_of(labels, n, lags, pooled=True)
    assert per.counts.shape == (5, M, n, n) and pooled.counts.shape == (5, 1, n, n)
    for l, lag in enumerate(lags):
        assert int(per.counts[l].sum()) + int(per.n_skipped[l]) == M * max(S - lag, 0), lag
        if lag >= S:
            assert int(per.counts[l].sum()) == 0 and int(per.n_skipped[l]) == 0
    assert torch.equal(per.sum_members().counts, pooled.counts) and torch.equal(per.n_skipped, pooled.n_skipped)
    if M > 1:
        parts = [counts_of(labels[:, :1], n, lags), counts_of(labels[:, 1:], n, lags)]
        joined = forecast.TransitionCounts.cat(parts)
        assert torch.equal(joined.counts, per.counts) and torch.equal(joined.n_skipped, per.n_skipped)
    # by hand at lag 1 for member 0
    want = np.zeros((n, n), np.int64)
    for t in range(S - 1):
        a, b = labels[t, 0], labels[t + 1, 0]
        if 0 <= a < n and 0 <= b < n:
            want[a, b] += 1
    assert np.array_equal(per.counts[0, 0].numpy(), want)


def test_assignment_scores_on_cpu_tensors():
    from molecular_dynamics_neural_operator_amd.forecast import Assignment
    labels = torch.tensor([[0, 1], [0, -1], [2, 1], [0, 1]], dtype=torch.int32)
    dist2 = torch.tensor([[1.0, 4.0], [9.0, float("nan")], [0.25, 4.0], [4.0, 16.0]], dtype=torch.float64)
    a = Assignment(labels, dist2)
    assert a.outside(2.0).tolist() == [0.25, 0.5]                                  # (a frame without a label is outside)
    assert a.outside(torch.tensor(0.5, dtype=torch.float64)).tolist() == [0.75, 1.0]
    assert a.populations(3).tolist() == [[0.75, 0.0, 0.25], [0.0, 1.0, 0.0]]
    flat = Assignment(labels[:, 0], dist2[:, 0])
    assert float(flat.outside(2.0)) == 0.25 and flat.populations(3).tolist() == [0.75, 0.0, 0.25]
    both = Assignment.cat([Assignment(labels[:, :1], dist2[:, :1]), Assignment(labels[:, 1:], dist2[:, 1:])])
    assert torch.equal(both.labels, labels) and both.cpu().dist2.shape == (4, 2)


def test_the_restatement_follows_the_header_on_small_cases():
    X = np.array([[0.0, 0.0], [3.0, 4.0], [np.nan, 1.0], [1.0, 0.0]], np.float32)
    Cn = np.array([[3.0, 4.0], [0.0, 0.0], [0.0, 0.0], [np.inf, 0.0]], np.float32)
    labels, dist2, _ = ref.assign(X, Cn)
    assert labels.tolist() == [1, 0, -1, 1] and dist2[[0, 1, 3]].tolist() == [0.0, 0.0, 1.0] and np.isnan(dist2[2])
    assert ref.assign(X, Cn[3:])[0].tolist() == [-1, -1, -1, -1] and ref.assign(X, Cn[:0])[0].tolist() == [-1] * 4
    from molecular_dynamics_neural_operator_amd.forecast import Assignment
    a = Assignment(torch.from_numpy(labels), torch.from_numpy(dist2))             # what forecast.assign would hand back
    assert a.populations(2).tolist() == [1.0 / 3.0, 2.0 / 3.0] and float(a.outside(0.5)) == 0.5
    index, radius, _ = ref.kcenters(X, 3, first=3)
    assert index.tolist() == [3, 1, 0] and radius[0] == np.inf and abs(radius[1] - math.sqrt(20.0)) < 1e-15 and radius[2] == 1.0
    sums, counts, _ = ref.centroid_sums(X[[0, 1, 3]], np.array([1, 1, 5]), 3)
    assert counts.tolist() == [0, 2, 0] and sums.tolist() == [[0.0, 0.0], [3.0, 4.0], [0.0, 0.0]]
