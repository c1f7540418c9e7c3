"""Ensemble verification without a GPU: what is particular to include/mdno_ensemble.h and its ctypes table (that header,
table and exports agree is tests/test_cabi_tables.py's); every refusal of the header comes back before any device work; the workspace size is
monotone; the arithmetic of forecast.EnsembleScore holds against closed forms; and the numpy restatement of the rule
(tests/ensemble_ref.py) has the properties the GPU tests lean on — q3 is the brute-force pair sum, and the three diagnostics
read a calibrated and an under-dispersed ensemble correctly."""
import math
import re

import numpy as np
import pytest
import torch

import ensemble_ref as ref
from cabi import CSRC, INCLUDE, lib  # noqa: F401  (lib: the fixture)

HEADER = INCLUDE / "mdno_ensemble.h"
NAMES = {"mdnoens_score_workspace_bytes", "mdnoens_score"}
FAKE = 0x10000          # a made-up address: nothing may dereference it
BIG = 1 << 62


def test_ensemble_header_table_and_exports_agree(lib):
    """What is particular to this header; that header, table and exports agree is tests/test_cabi_tables.py's."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    assert set(_lib.ENSEMBLE_SIGNATURES) == NAMES
    assert lib.mdno_abi_version() == 15 == _lib.ABI_VERSION and lib.mdno_train_abi_version() == 1          # additive: both stay
    assert (CSRC / "ensemble.hip").exists()                                              # inside the library's content hash
    text = HEADER.read_text()
    assert int(re.search(r"#define MDNO_ENS_SAMPLE_TILE (\d+)", text).group(1)) == ops.ENSEMBLE_SAMPLE_TILE
    assert int(re.search(r"#define MDNO_ENS_MAX_MEMBERS (\d+)", text).group(1)) == ops.MAX_ENSEMBLE_MEMBERS == 1024
    assert int(re.search(r"#define MDNO_ENS_MAX_REGISTER_MEMBERS (\d+)", text).group(1)) == ops.MAX_REGISTER_MEMBERS == 64
    assert "mdnoens_" in text and "prefix" in text.lower()                               # the header says why the names differ: ABI
    assert _lib.ENSEMBLE_FORMS == {"auto": 0, "registers": 1, "lds": 2}


def score(lib, frames=FAKE, truth=FAKE, S=3, M=8, N=5, sums=FAKE, hist=FAKE, inv=FAKE, ties=FAKE, form=0, ws=FAKE, ws_bytes=BIG):
    return lib.mdnoens_score(frames, truth, S, M, N, sums, hist, inv, ties, form, ws, ws_bytes, None)


def test_entry_point_refuses_before_device_work(lib):
    """No pointer below is a device pointer: a call that got as far as a launch would fault, not return a code."""
    from molecular_dynamics_neural_operator_amd import _lib
    E, U = _lib.EINVAL, _lib.EUNSUPPORTED
    err = lib.mdno_last_error
    assert score(lib, S=-1) == E and score(lib, M=-1) == E and score(lib, N=-1) == E
    for M in (0, 1025, 1 << 20):
        assert score(lib, M=M) == E and b"M=" in err(), M
    for form in (-1, 3, 99):
        assert score(lib, form=form) == E and b"form" in err(), form
    for kw in ({"frames": None}, {"truth": None}, {"sums": None}, {"hist": None}, {"inv": None}, {"ties": None}):
        assert score(lib, **kw) == E and b"null pointer" in err(), kw
    need = lib.mdnoens_score_workspace_bytes(3, 8, 5)
    assert need >= 3 * 4 * 8
    assert score(lib, ws_bytes=need - 1) == E and b"workspace" in err()
    assert score(lib, ws=None) == E and b"workspace" in err()
    assert score(lib, ws_bytes=0) == E
    # the register form holds 64 members
    assert score(lib, M=65, form=1) == U and b"register" in err()
    assert score(lib, M=1024, form=1) == U
    assert score(lib, M=1025, form=1) == E                                               # (the range comes first)
    # S times the tiles of a step beyond the launch grid
    assert score(lib, S=1 << 20, N=1 << 20) == U and b"grid" in err()
    assert score(lib, S=(1 << 31) - 1, N=86) == U and b"grid" in err()
    # nothing to do: returns 0 and looks at nothing, whatever the pointers (the sizes and the form are still checked)
    assert score(lib, S=0) == 0
    assert score(lib, S=0, M=5000, frames=None, truth=None, sums=None, hist=None, inv=None, ties=None, ws=None, ws_bytes=0) == 0
    assert score(lib, S=0, form=3) == E and score(lib, S=0, N=-1) == E


def test_workspace_bytes_are_monotone(lib):
    from molecular_dynamics_neural_operator_amd import ops
    f = lib.mdnoens_score_workspace_bytes
    base = dict(S=100, M=8, N=300)
    b0 = f(*base.values())
    tiles = -(-3 * 300 // ops.ENSEMBLE_SAMPLE_TILE)
    assert b0 >= 100 * tiles * 4 * 8                                  # four partials per (step, tile)
    for key in base:
        prev = 0
        for scale in (1, 2, 3, 7, 40, 128):
            args = dict(base)
            args[key] = base[key] * scale
            cur = f(*args.values())
            assert cur >= prev and cur >= b0, (key, scale)
            prev = cur
    assert f(0, 8, 300) == 0 and f(-1, 8, 300) == 0 and f(100, 8, 0) > 0
    assert f(1000, 64, 504) >= 1000 * 6 * 32


def test_python_arguments_are_checked_without_a_device():
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    x, y = torch.zeros(6, 4, 5, 3), torch.zeros(6, 5, 3)
    for call in (lambda: ops.ensemble_score(x, y), lambda: forecast.ensemble_score(x, y),
                 lambda: forecast.ensemble_score(x, y, form="lds")):
        with pytest.raises(MdnoError, match="CPU tensor"):
            call()
    with pytest.raises(MdnoError, match="torch tensor"):
        ops.ensemble_score(x.numpy(), y)
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine, RolloutEngine
    assert callable(RolloutEngine.ensemble_score) and callable(GroupedRolloutEngine.ensemble_score)
    assert "cannot be merged" in GroupedRolloutEngine.ensemble_score.__doc__


# ------------------------------------------------------------------------------------------------ EnsembleScore
def close(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool((np.abs(a - b) <= rel * np.abs(b)).all())


def as_score(sc):
    from molecular_dynamics_neural_operator_amd.forecast import EnsembleScore
    return EnsembleScore(torch.from_numpy(sc.sums), torch.from_numpy(sc.rank_hist), torch.from_numpy(sc.n_invalid),
                         torch.from_numpy(sc.n_ties), sc.members, sc.samples_per_step)


def grid_ensemble(S, M, N, c, seed=3):
    """Members y + (m - c) on the integer grid (shuffled along m): every quantity of the rule is exact."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 64, size=(S, N, 3)).astype(np.float32)
    off = np.arange(M, dtype=np.float32) - c
    x = y[:, None] + rng.permuted(np.broadcast_to(off[None, :, None, None], (S, M, N, 3)), axis=1)
    return x.astype(np.float32), y


@pytest.mark.parametrize("M", [2, 5, 8, 64])
def test_ensemble_score_arithmetic_on_the_integer_grid(M):
    """d_j = j - c: mean (M - 1) / 2 - c, unbiased variance M (M + 1) / 12, sum |d_j|, and sum_{m<k} (k - m) = M (M^2 - 1) / 6,
    all exact in fp64; the truth's rank is c."""
    S, N, c = 3, 7, 1
    n = 3 * N
    x, y = grid_ensemble(S, M, N, c)
    sc = ref.score(x, y)
    mean = (M - 1) / 2.0 - c
    absd = float(sum(abs(j - c) for j in range(M)))
    assert (sc.sums[:, 0] == n * mean * mean).all() and (sc.sums[:, 2] == n * absd).all()
    assert (sc.sums[:, 3] == n * (M * (M * M - 1) / 6.0)).all()
    assert close(sc.sums[:, 1], n * (M * (M + 1) / 12.0), 1e-15 * n)
    assert (sc.rank_hist[:, c] == n).all() and sc.rank_hist.sum() == S * n and (sc.n_ties == n).all() and not sc.n_invalid.any()
    e = as_score(sc)
    assert e.rmse().dtype == torch.float64 and close(e.rmse(), abs(mean)) and close(e.spread(), math.sqrt(M * (M + 1) / 12.0))
    assert close(e.spread_skill(), math.sqrt((M + 1) / M) * math.sqrt(M * (M + 1) / 12.0) / abs(mean))
    assert close(e.crps(), absd / M - (M * M - 1) / (6.0 * M))
    assert close(e.crps(fair=True), absd / M - (M + 1) / 6.0)
    h = e.rank_histogram()
    assert h.shape == (S, M + 1) and (h[:, c] == 1.0).all() and float(h.sum()) == S
    assert close(e.rank_flatness(), 1.0 - 1.0 / (M + 1))


def test_ensemble_score_one_member_cat_sum_cpu_and_empty_steps():
    from molecular_dynamics_neural_operator_amd.forecast import EnsembleScore
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    x, y = ref.ensemble(4, 1, 9)
    sc = ref.score(x, y)
    e = as_score(sc)
    assert not e.spread().any() and not sc.sums[:, 1].any() and not sc.sums[:, 3].any()
    mae = np.abs(x[:, 0].astype(np.float64) - y).reshape(4, -1).mean(1)
    assert close(e.crps(), mae) and torch.isnan(e.crps(fair=True)).all()
    assert close(e.rmse(), np.sqrt(((x[:, 0].astype(np.float64) - y) ** 2).reshape(4, -1).mean(1)))
    assert not e.spread_skill().any() and e.rank_hist.shape == (4, 2) and (e.rank_hist.sum(1) == 27).all()
    # cat along the steps, sum pools before the ratios, cpu keeps everything
    x8, y8 = ref.ensemble(5, 8, 9)
    a, b = as_score(ref.score(x8[:2], y8[:2])), as_score(ref.score(x8[2:], y8[2:]))
    whole = as_score(ref.score(x8, y8))
    both = EnsembleScore.cat([a, b])
    for name in ("sums", "rank_hist", "n_invalid", "n_ties"):
        assert torch.equal(getattr(both, name), getattr(whole, name)), name
    assert (both.members, both.samples_per_step, both.n_steps) == (8, 27, 1)
    with pytest.raises(MdnoError, match="same members"):
        EnsembleScore.cat([a, e])
    p = whole.sum()
    assert p.sums.shape == (1, 4) and p.rank_hist.shape == (1, 9) and p.n_steps == 5 and int(p.rank_hist.sum()) == 5 * 27
    assert close(p.rmse(), math.sqrt(float(whole.sums[:, 0].sum()) / (5 * 27)))
    assert close(p.crps(), float(whole.sums[:, 2].sum()) / (8 * 135) - float(whole.sums[:, 3].sum()) / (64 * 135))
    part = whole.sum(slice(1, 3))
    assert part.n_steps == 2 and torch.equal(part.sums[0], whole.sums[1:3].sum(0))
    assert whole.sum([0, 4]).n_steps == 2 and whole.sum(2).n_steps == 1 and torch.equal(whole.sum(2).sums[0], whole.sums[2])
    assert close(whole.sum(2).spread(), whole.spread()[2])
    k = whole.cpu()
    assert torch.equal(k.sums, whole.sums) and torch.equal(k.rank_hist, whole.rank_hist) and k.members == 8
    # a step without valid samples: NaN everywhere, no exception
    z = EnsembleScore(torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 9, dtype=torch.int64), torch.zeros(2, dtype=torch.int64),
                      torch.zeros(2, dtype=torch.int64), 8, 0)
    for v in (z.rmse(), z.spread(), z.spread_skill(), z.crps(), z.crps(True), z.rank_flatness()):
        assert v.shape == (2,) and torch.isnan(v).all()
    assert torch.isnan(z.rank_histogram()).all()
    bad = x8.copy()
    bad[1, 3, 2, 0] = np.nan
    nb = as_score(ref.score(bad, y8))
    assert torch.isnan(nb.rmse()).tolist() == [False, True, False, False, False] and nb.n_invalid.tolist() == [0, 1, 0, 0, 0]
    assert int(nb.rank_hist[1].sum()) == 26 and close(nb.rank_histogram().sum(-1), 1.0)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("M", [1, 2, 3, 8, 33, 64])
def test_q3_is_the_pair_sum(M):
    x, y = ref.ensemble(2, M, 41, seed=7)
    ps = ref.per_sample(x, y)
    brute = ref.pair_sum_brute(x)
    rel = np.abs(ps.q[..., 3] - brute) / np.maximum(brute, 1e-300)
    print(f"M={M}: q3 against the brute-force pair sum, largest relative difference {rel.max():.3g}")
    assert (rel <= 1e-14).all() if M > 1 else not ps.q[..., 3].any()
    # the order of the members does not enter
    perm = np.random.default_rng(0).permutation(M)
    again = ref.per_sample(x[:, perm], y)
    assert np.array_equal(ps.q, again.q) and np.array_equal(ps.rank, again.rank)
    # and EnsembleScore's CRPS is the textbook one: mean_m |x_m - y| - sum_{m,k} |x_m - x_k| / (2 M^2), per step
    n = ps.q.shape[1]
    want = ps.q[..., 2].sum(1) / (M * n) - brute.sum(1) / (M * M * n)
    assert close(as_score(ref.score(x, y)).crps(), want, 1e-13)


def chi2_z(hist):
    M = hist.size - 1
    expect = hist.sum() / (M + 1)
    return (float(((hist - expect) ** 2 / expect).sum()) - M) / math.sqrt(2 * M)


@pytest.mark.parametrize("M", [8, 16, 64])
def test_calibration_reads_correctly_on_the_restatement(M):
    """Members and truth drawn alike (sigma 0.3, S = 8, N = 513: n = 12,312 samples): spread-skill and the fair CRPS over
    its Gaussian value sigma / sqrt(pi) within 3 % of 1 (about four standard errors), a flat rank histogram (chi^2 z-score
    <= 4).  The members' sigma halved: spread-skill below 0.7 and a U-shaped histogram."""
    S, N, sigma = 8, 513, 0.3
    x, y = ref.ensemble(S, M, N, seed=1, sigma=sigma, truth_sigma=sigma)
    sc = ref.score(x, y)
    assert not sc.n_invalid.any()
    ss, crps, fair, hist = ref.pooled(sc)
    ratio = fair / (sigma / math.sqrt(math.pi))
    z = chi2_z(hist)
    print(f"M={M}: spread-skill {ss:.3f}, fair CRPS / (sigma / sqrt(pi)) {ratio:.3f}, rank-histogram z {z:.2f}")
    assert abs(ss - 1.0) <= 0.03 and abs(ratio - 1.0) <= 0.03 and z <= 4.0
    assert crps > fair                                                       # the plain estimator is biased upwards
    e = as_score(sc).sum()
    assert close(e.spread_skill(), ss) and close(e.crps(fair=True), fair) and float(e.rank_flatness()) < 0.05
    x2, y2 = ref.ensemble(S, M, N, seed=1, sigma=sigma / 2, truth_sigma=sigma)
    under = ref.score(x2, y2)
    ss2, _, _, hist2 = ref.pooled(under)
    share = hist2.sum() / (M + 1)
    print(f"M={M}, members' sigma halved: spread-skill {ss2:.3f}, end bins {hist2[0] / share:.2f} and {hist2[-1] / share:.2f} x uniform")
    assert ss2 < 0.7 and hist2[0] > share and hist2[-1] > share
    assert float(as_score(under).sum().rank_flatness()) > float(e.rank_flatness())
