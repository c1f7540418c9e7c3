"""Displacement statistics, the velocity autocorrelation and unwrapping on the device (include/mdno_dynamics.h,
csrc/dynamics.hip) against the numpy fp64 restatement of the rules (tests/dynamics_ref.py): counts as exact integers, the
fp64 sums within a gate derived from the number of terms (and, with the centroid removed, from the centroid's rounding),
the cases that are exact by construction, the identities with mdno_forecast_score and between the two statistics,
non-finite coordinates, the same bits on every run and for every M, the engines' entry points, unwrapping bit for bit, and
guard bands around every buffer the new entry points write."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dynamics_ref as ref

pytestmark = pytest.mark.gpu

L0 = 17.1
SEED = 1
M0 = 3
R_MAX, N_BINS = 4.0, 64
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 300, 513]
SHAPES = {"S2": (2, (0, 1)), "S40": (40, (0, 1, 2, 7, 39)), "S130": (130, (1, 5, 64, 65, 129))}
STRIDES = (1, 3)
# origin counts of DYNAMICS_ORIGIN_CHUNK - 1, the chunk itself and + 1 (64): at stride 1 in the first three, at stride 3 in
# the last (192 // 3 + 1 = 65, 189 // 3 + 1 = 64, 186 // 3 + 1 = 63; at stride 1 it has four chunks with a ragged last)
CHUNK_SHAPES = {"S64": (64, (0, 1, 2)), "S65": (65, (0, 1, 2)), "S66": (66, (0, 1, 2)), "S193": (193, (0, 3, 6))}
CHUNK_SIZES = (65, 257)
ALL_SHAPES = {**SHAPES, **CHUNK_SHAPES}
C_INT32 = ctypes.c_int32


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def walk(S, N, M=M0, seed=SEED):
    """f32 [S, M, N, 3]: positions uniform in [0, 17.1)^3, then Gaussian steps of sigma 0.3 plus a drift of
    (0.05, -0.02, 0.01) per frame, accumulated in fp64, stored as fp32."""
    rng = np.random.default_rng(seed)
    x0 = rng.random((M, N, 3)) * L0
    steps = rng.normal(0.0, 0.3, size=(S - 1, M, N, 3)) + np.array([0.05, -0.02, 0.01])
    x = np.concatenate([x0[None], x0[None] + np.cumsum(steps, axis=0)]).astype(np.float32)
    x.setflags(write=False)
    return x


def vlags(S, lags):
    """The lags of a shape for the velocities: capped at S - 2."""
    return tuple(sorted({min(t, S - 2) for t in lags}))


@functools.lru_cache(maxsize=None)
def expected(N, key, stride, com):
    """The restatement's (Stats, (corr, gate, n_samples)) of walk(S, N), with the condition the comparison of counts rests
    on."""
    S, lags = ALL_SHAPES[key]
    x = walk(S, N)
    st = ref.displacement_stats(x, lags, stride, com, R_MAX, N_BINS)
    assert st.margin >= 1e-9, f"N={N} {key} stride={stride} com={com}: a sample lies {st.margin} bins from an edge; choose another seed"
    return st, ref.velocity_autocorrelation(x, vlags(S, lags), stride, com)


def on(dev, x):
    return torch.tensor(np.ascontiguousarray(x)).to(dev)


def device_stats(dev, x, lags, stride, com, r_max=R_MAX, n_bins=N_BINS):
    from molecular_dynamics_neural_operator_amd import ops
    s2, s4, c = ops.displacement_stats(on(dev, x), list(lags), stride, com, r_max, n_bins)
    assert s2.dtype == s4.dtype == torch.float64 and s2.is_cuda and (c is None or c.dtype == torch.int64)
    return s2.cpu().numpy(), s4.cpu().numpy(), None if c is None else c.cpu().numpy()


def device_corr(dev, x, lags, stride, com):
    from molecular_dynamics_neural_operator_amd import ops
    c = ops.velocity_autocorrelation(on(dev, x), list(lags), stride, com)
    assert c.dtype == torch.float64 and c.is_cuda
    return c.cpu().numpy()


def ratio(got, want, gate):
    """max |got - want| / gate; 0 where both the difference and the gate are 0 (exact cases), inf where only the gate is."""
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / gate)
    return float(q.max()) if q.size else 0.0


def compare(dev, N, key):
    S, lags = ALL_SHAPES[key]
    x = walk(S, N)
    worst = 0.0
    for stride in STRIDES:
        for com in (False, True):
            st, (corr, cgate, _) = expected(N, key, stride, com)
            s2, s4, counts = device_stats(dev, x, lags, stride, com)
            assert counts.shape == (M0, len(lags), N_BINS)
            assert np.array_equal(counts, st.counts), (stride, com, int(np.abs(counts - st.counts).sum()))
            r2, r4 = ratio(s2, st.sum2, st.gate2), ratio(s4, st.sum4, st.gate4)
            got = device_corr(dev, x, vlags(S, lags), stride, com) if S >= 2 else corr
            rc = ratio(got, corr, cgate)
            worst = max(worst, r2, r4, rc)
            print(f"N={N} {key} stride={stride} com={com}: error / gate sum2 {r2:.3g} sum4 {r4:.3g} corr {rc:.3g}; margin "
                  f"{st.margin:.3g} bins, {st.beyond} samples beyond r_max")
            assert r2 <= 1.0 and r4 <= 1.0 and rc <= 1.0, (stride, com, r2, r4, rc)
    return worst


# ================================================================================================ 1. the restatement
@pytest.mark.parametrize("key", sorted(SHAPES))
@pytest.mark.parametrize("N", SIZES)
def test_statistics_equal_the_restatement(dev, N, key):
    """Strides 1 and 3, the centroid removed or not: counts as exact integers, sum2 / sum4 / corr within the derived gate.
    One, two and three atom tiles with ragged last ones (257, 300, 513), one origin (lag S - 1) to three chunks (S = 130)."""
    worst = compare(dev, N, key)
    print(f"N={N} {key}: largest error / gate {worst:.3g}")


@pytest.mark.parametrize("key", sorted(CHUNK_SHAPES))
@pytest.mark.parametrize("N", CHUNK_SIZES)
def test_origin_counts_around_the_chunk(dev, N, key):
    from molecular_dynamics_neural_operator_amd import ops
    assert ops.DYNAMICS_ORIGIN_CHUNK == 64
    compare(dev, N, key)


# ================================================================================================ 2. exact by construction
@pytest.mark.parametrize("N", [1, 65, 300])
def test_lag_zero(dev, N):
    x = walk(40, N)
    for com in (False, True):
        s2, s4, counts = device_stats(dev, x, (0, 0), 3, com)
        n = ref.n_origins(40, 0, 3) * N
        assert not s2.any() and not s4.any() and (counts[:, :, 0] == n).all() and not counts[:, :, 1:].any()


@pytest.mark.parametrize("N", [8, 64, 512])
def test_rigid_integer_translation_is_exact(dev, N):
    """Integer coordinates moved by the integer vector (1, -2, 3) per frame: every term is tau^2 * 14 exactly, in a known
    bin, and with the centroid removed (N a power of two: the centroid is exact) exactly zero."""
    S, lags = 70, (0, 1, 3, 4, 69)
    x0 = np.random.default_rng(3).integers(0, 32, size=(1, 2, N, 3))
    x = (x0 + np.arange(S)[:, None, None, None] * np.array([1, -2, 3])).astype(np.float32)
    for stride in STRIDES:
        s2, s4, counts = device_stats(dev, x, lags, stride, False, 16.0, 16)
        zs2, zs4, zcounts = device_stats(dev, x, lags, stride, True, 16.0, 16)
        for l, tau in enumerate(lags):
            n = ref.n_origins(S, tau, stride) * N
            r2 = tau * tau * 14
            assert (s2[:, l] == n * r2).all() and (s4[:, l] == n * r2 * r2).all(), (stride, tau)
            want = np.zeros(16, np.int64)
            if r2 < 256:
                want[int(np.sqrt(r2))] = n                                     # tau = 0, 1, 3, 4: r = 0, 3.74, 11.2, 14.97
            assert (counts[:, l] == want).all()
            assert (zcounts[:, l, 0] == n).all() and not zcounts[:, l, 1:].any()
        assert not zs2.any() and not zs4.any()
        assert not device_corr(dev, x, (0, 5, 68), stride, True).any()
        c = device_corr(dev, x, (0, 5, 68), stride, False)
        assert (c == np.array([ref.n_origins(S, t, stride, 1) * N * 14 for t in (0, 5, 68)], dtype=np.float64)).all()


def test_one_atom_without_its_centroid_does_not_move(dev):
    x = walk(40, 1)
    s2, s4, counts = device_stats(dev, x, (1, 7, 39), 1, True)
    assert not s2.any() and not s4.any() and (counts[:, :, 0] == [39, 33, 1]).all()
    assert not device_corr(dev, x, (0, 1, 38), 1, True).any()


@pytest.mark.parametrize("N", [65, 300])
def test_every_sample_is_counted_below_a_large_r_max(dev, N):
    S, lags = 130, (1, 5, 64, 65, 129)
    x = walk(S, N)
    for stride in STRIDES:
        st = ref.displacement_stats(x, lags, stride, False, 1000.0, 4096)
        assert st.beyond == 0
        counts = device_stats(dev, x, lags, stride, False, 1000.0, 4096)[2]
        assert (counts.sum(-1) == st.n_samples[None]).all()
        assert np.array_equal(counts, st.counts) or st.margin < 1e-9


# ================================================================================================ 3. identities
@pytest.mark.parametrize("N", [65, 300])
def test_one_origin_is_three_times_the_mse(dev, N):
    """origin_stride >= S leaves the origin t = 0: sum2 / N is 3 * mse of score_forecast(frames[tau], frames[0]).  Both are
    fp64 sums of the same 3 N squares in different orders: relative difference at most 3 N * 2^-52 (+ one division)."""
    from molecular_dynamics_neural_operator_amd import forecast, ops
    S, lags = 40, [1, 2, 7, 39]
    xd = on(dev, walk(S, N))
    s2 = ops.displacement_stats(xd, lags, S, False)[0]
    truth = xd[0:1].expand(len(lags), M0, N, 3).contiguous()
    mse = forecast.score_forecast(xd[lags].contiguous(), truth).mse                   # [L, M]
    a, b = (s2 / N).cpu().numpy(), (3.0 * mse.T).cpu().numpy()
    rel = np.abs(a - b) / b
    print(f"N={N}: sum2 / N against 3 * mse, largest relative difference {rel.max():.3g}")
    assert (rel <= (3 * N + 4) * 2.0 ** -52).all()


@pytest.mark.parametrize("N", [65, 300])
def test_correlation_at_lag_zero_is_sum2_at_lag_one(dev, N):
    S = 130
    x = walk(S, N)
    for com in (False, True):
        st = ref.displacement_stats(x, (1,), 1, com)
        corr = device_corr(dev, x, (0,), 1, com)
        s2 = device_stats(dev, x, (1,), 1, com, None, 0)[0]
        assert ratio(corr, s2, 2.0 * st.gate2) <= 1.0                                  # (each within the gate of the restatement)
        assert np.array_equal(corr.view(np.int64), s2.view(np.int64))                 # the same terms in the same order


# ================================================================================================ 4. other properties
@pytest.mark.parametrize("com", [False, True])
def test_a_nan_atom_spoils_exactly_what_touches_it(dev, com):
    """NaN in frame 7 of member 1 (stride 3: origins 0, 3, 6, ...): the lags with an origin t or t + tau == 7 go
    non-finite in member 1 only, the other members keep their bits, and the counts lose exactly the samples that touch the
    atom (with the centroid removed: the frame)."""
    S, N, lags = 40, 65, (0, 1, 2, 7, 39)
    x = walk(S, N)
    bad = x.copy()
    bad[7, 1, 3, 0] = np.nan
    touched = [any(t == 7 or t + tau == 7 for t in ref.origins(S, tau, 3)) for tau in lags]
    assert touched == [False, True, False, True, False]
    clean = device_stats(dev, x, lags, 3, com)
    got = device_stats(dev, bad, lags, 3, com)
    want = ref.displacement_stats(bad, lags, 3, com, R_MAX, N_BINS)
    for k in (0, 1):
        assert (~np.isfinite(got[k][1])).tolist() == touched
        assert np.array_equal(got[k][[0, 2]].view(np.int64), clean[k][[0, 2]].view(np.int64))
        assert np.array_equal(got[k][1][~np.array(touched)].view(np.int64), clean[k][1][~np.array(touched)].view(np.int64))
    assert np.array_equal(got[2], want.counts) and np.array_equal(got[2][[0, 2]], clean[2][[0, 2]])
    lost = clean[2][1].sum(-1) - got[2][1].sum(-1)
    inside = clean[2][1].sum(-1)
    if com:      # every atom of the frame: what the clean run counted of these origins
        assert (lost[~np.array(touched)] == 0).all() and (lost[np.array(touched)] > 1).all() and (lost <= N).all()
    else:
        assert lost.tolist() == [0, 1, 0, 1, 0] and (inside > 0).all()
    vl = (0, 1, 6, 38)
    vtouch = [any(7 in (t, t + 1, t + tau, t + tau + 1) for t in ref.origins(S, tau, 3, 1)) for tau in vl]
    c = device_corr(dev, bad, vl, 3, com)
    c0 = device_corr(dev, x, vl, 3, com)
    assert (~np.isfinite(c[1])).tolist() == vtouch and any(vtouch) and not all(vtouch)
    assert np.array_equal(c[[0, 2]].view(np.int64), c0[[0, 2]].view(np.int64))


def test_same_bits_on_every_call_and_for_every_m(dev):
    S, N, lags = 130, 300, (1, 5, 64, 65, 129)
    x = walk(S, N)
    for com in (False, True):
        a = device_stats(dev, x, lags, 1, com)
        b = device_stats(dev, x, lags, 1, com)
        one = device_stats(dev, x[:, 1:2], lags, 1, com)
        for u, v, w in zip(a, b, one):
            assert np.array_equal(u.view(np.int64), v.view(np.int64))
            assert np.array_equal(u[1:2].view(np.int64), w.view(np.int64))
        ca, cb = device_corr(dev, x, lags[:-1], 1, com), device_corr(dev, x, lags[:-1], 1, com)
        assert np.array_equal(ca.view(np.int64), cb.view(np.int64))
        assert np.array_equal(ca[1:2].view(np.int64), device_corr(dev, x[:, 1:2], lags[:-1], 1, com).view(np.int64))


def test_truth_shape_default_lags_and_the_dataclass(dev):
    from molecular_dynamics_neural_operator_amd import forecast
    S, N = 130, 65
    x = walk(S, N)
    xd = on(dev, x)
    t = forecast.displacement_stats(xd[:, 0].contiguous(), r_max=R_MAX, n_bins=N_BINS)           # a [S, N, 3] truth: M = 1
    lags = forecast.default_lags(S)
    assert t.sum2.shape == (1, len(lags)) and t.counts.shape == (1, len(lags), N_BINS) and t.lags.tolist() == lags
    assert t.lags.device == t.sum2.device == t.n_samples.device == xd.device and lags[-1] == 64
    assert t.n_samples.tolist() == [(S - tau) * N for tau in lags] and (t.r_max, t.n_bins) == (R_MAX, N_BINS)
    full = forecast.displacement_stats(xd, lags, r_max=R_MAX, n_bins=N_BINS)
    assert torch.equal(full.sum2[0:1], t.sum2) and torch.equal(full.counts[0:1], t.counts)
    st = ref.displacement_stats(x, lags, 1, False, R_MAX, N_BINS)
    assert np.allclose(full.msd().cpu().numpy(), st.sum2 / st.n_samples[None], rtol=1e-12, atol=0)
    # a random walk of sigma 0.3 per component and frame plus a drift: MSD = 3 * 0.09 * tau + |drift|^2 tau^2
    msd = full.msd().cpu().numpy()
    model = 0.27 * np.array(lags) + 0.003 * np.array(lags) ** 2
    assert (np.abs(msd[:, 1:] - model[1:]) < 0.2 * model[1:]).all()
    tv = full.total_variation(t)
    assert tv.shape == (M0, len(lags)) and not tv[0].any() and (tv[1:, 1:] > 0).all() and (tv <= 1).all()
    d = full.diffusion_coefficient(1.0, first=1)
    assert d.shape == (M0,) and (d > 0.04).all() and (d < 0.12).all()
    assert abs(float(full.non_gaussian()[:, 1:].abs().max())) < 0.2                     # Gaussian steps
    g = full.van_hove()
    assert g.shape == (M0, len(lags), N_BINS) and float((g[:, 1] * (R_MAX / N_BINS)).sum(-1).min()) > 0.999
    c, cl = forecast.velocity_autocorrelation(xd, normalized=True)
    assert cl.tolist() == forecast.default_lags(S, 1) and c.shape == (M0, len(cl)) and (c[:, 0] == 1.0).all()
    assert float(c[:, 1:].abs().max()) < 0.2                                          # independent steps decorrelate at once
    raw, _ = forecast.velocity_autocorrelation(xd, [0, 3])
    want, _, ns = ref.velocity_autocorrelation(x, [0, 3])
    assert np.allclose(raw.cpu().numpy(), want / ns[None], rtol=1e-12, atol=1e-15)
    # no frames, no members, no atoms
    from molecular_dynamics_neural_operator_amd import ops
    s2, s4, cn = ops.displacement_stats(xd[:0], [0, 3], 1, False, R_MAX, 8)
    assert s2.shape == (M0, 2) and not s2.any() and not s4.any() and cn.shape == (M0, 2, 8) and not cn.any()
    s2, s4, cn = ops.displacement_stats(xd[:, :, :0].contiguous(), [0, 3], 1, True, R_MAX, 8)
    assert s2.shape == (M0, 2) and not s2.any() and not s4.any() and not cn.any()
    assert not ops.velocity_autocorrelation(xd[:, :, :0].contiguous(), [0, 3]).any()
    assert ops.displacement_stats(xd[:, :0].contiguous(), [0, 3])[0].shape == (0, 2)
    assert ops.unwrap_frames(xd[:0], (L0, L0, L0)).shape == (0, M0, N, 3)


def test_1024_lags_in_four_batches(dev):
    """More lags than one launch carries (256): every batch lands in its own rows."""
    S, N = 40, 5
    x = walk(S, N)
    lags = [(7 * k) % S for k in range(1024)]
    s2, s4, counts = device_stats(dev, x, lags, 1, False, R_MAX, 4)
    base = device_stats(dev, x, list(range(S)), 1, False, R_MAX, 4)
    for u, v in zip((s2, s4, counts), base):
        assert np.array_equal(u, v[:, lags])
    vl = [t % (S - 1) for t in lags[:300]]
    assert np.array_equal(device_corr(dev, x, vl, 1, True), device_corr(dev, x, list(range(S - 1)), 1, True)[:, vl])


def _engine_inputs():
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    M, N, W = 2, 28, 3
    base = syn.chain_frame(N, seed=1)
    traj = syn.ou_trajectory(base, W, seed=2)
    wins = syn.ensemble_windows(traj[:W], M, sigma=0.1, seed0=100)                   # [M, W, N, 3]
    return torch.from_numpy(np.ascontiguousarray(wins.transpose(1, 0, 2, 3))), torch.from_numpy(syn.amino_acids(N, seed=1))


def test_engines_score_their_own_frames(dev):
    """RolloutEngine / GroupedRolloutEngine on a 5-step, 2-member, N = 28 run equal forecast.* on eng.produced(...) bit for
    bit, also from a non-zero first step (a view into the trajectory buffer)."""
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine, RolloutEngine
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    wins, aa = _engine_inputs()
    model = KernelNN(64, 128, 2, 6, 7, 3, 20, 4)
    model.load_state_dict(near_identity_state_dict(64, 128, seed=0, kernel_gain=1e-3, feature_gain=0.1))
    model.eval().to(dev)
    for cls in (RolloutEngine, GroupedRolloutEngine):
        eng = cls(model, 2, 28, 3, 8.0, max_steps=5, device=dev)
        eng.run(wins, aa, 5)
        for first, steps in ((0, None), (1, 4), (2, 2)):
            n = 5 - first if steps is None else steps
            fr = eng.produced(first, n).clone()
            lags = [0, 1, n - 1]
            d = eng.displacement_stats(lags, 1, True, 2.0, 16, first_step=first, steps=steps)
            w = forecast.displacement_stats(fr, lags, 1, True, 2.0, 16)
            assert d.sum2.shape == (2, 3) and d.counts.shape == (2, 3, 16)
            for name in ("sum2", "sum4", "counts", "lags", "n_samples"):
                assert torch.equal(getattr(d, name), getattr(w, name)), (cls.__name__, first, name)
            assert d.n_samples.tolist() == [n * 28, (n - 1) * 28, 28] and int(d.counts.sum()) > 0
            c, cl = eng.velocity_autocorrelation([0, n - 2], first_step=first, steps=steps)
            wc, wl = forecast.velocity_autocorrelation(fr, [0, n - 2])
            assert torch.equal(c, wc) and torch.equal(cl, wl) and c.shape == (2, 2)
        dflt = eng.displacement_stats()
        assert dflt.lags.tolist() == forecast.default_lags(5) and dflt.counts is None and dflt.sum2.shape == (2, 3)
        eng.close()


# ================================================================================================ 5. unwrap
@pytest.mark.parametrize("box", [(L0, L0, L0), (L0, L0, 0.0), (0.0, 0.0, 0.0), (5.0, 40.0, L0)])
def test_unwrap_equals_the_restatement(dev, box):
    """A walk that leaves its cell many times, wrapped in fp64 and stored as f32 (M = 3, N = 300: two blocks of threads and
    a ragged one), against the restatement bit for bit; [S, N, 3] as well."""
    from molecular_dynamics_neural_operator_amd import forecast
    x = walk(130, 300)
    w = ref.wrap(x.astype(np.float64) * 3.0 - 20.0, box)                   # steps up to ~4.5: above L / 2 on the 5.0 axis too
    want = ref.unwrap(w, box)
    got = forecast.unwrap(on(dev, w), box)
    assert got.dtype == torch.float32 and got.shape == w.shape
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    if any(L > 0 for L in box):
        assert (want != w).any()
    else:
        assert np.array_equal(want.view(np.int32), w.view(np.int32))                 # every axis open: a copy
    one = forecast.unwrap(on(dev, w[:, 1]), box)
    assert one.shape == (130, 300, 3) and np.array_equal(one.cpu().numpy().view(np.int32), want[:, 1].view(np.int32))


def test_unwrap_returns_a_wrapped_grid_walk_and_leaves_an_unwrapped_one(dev):
    """The walk on the grid 2^-10 of tests/test_dynamics_host.py: wrapped exactly, unwrapped to the input bits; a trajectory
    that never wrapped comes back unchanged; MSD of the unwrapped frames is the walk's."""
    from molecular_dynamics_neural_operator_amd import forecast, ops
    rng = np.random.default_rng(5)
    S, M, N, L = 200, 2, 65, 16.0
    x0 = rng.integers(0, 16 * 1024, size=(M, N, 3))
    steps = np.clip(np.rint(rng.normal(0, 1.5, size=(S - 1, M, N, 3)) * 1024), -7 * 1024, 7 * 1024).astype(np.int64)
    grid = np.concatenate([x0[None], x0[None] + np.cumsum(steps, 0)])
    wk = (grid / 1024.0).astype(np.float32)
    box = (L, L, L)
    w = ref.wrap(wk, box)
    assert (w != wk).any()
    back = forecast.unwrap(on(dev, w), box)
    assert np.array_equal(back.cpu().numpy().view(np.int32), wk.view(np.int32))
    a = ops.displacement_stats(back, [1, 10, 99])[0]
    b = ops.displacement_stats(on(dev, wk), [1, 10, 99])[0]
    assert torch.equal(a, b) and not torch.equal(a, ops.displacement_stats(on(dev, w), [1, 10, 99])[0])
    inside = (wk[:50] * 0.01 + 8.0).astype(np.float32)
    same = forecast.unwrap(on(dev, inside), box)
    assert np.array_equal(same.cpu().numpy().view(np.int32), inside.view(np.int32))


# ================================================================================================ 6. guard bands
def _run_guarded(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import _lib, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError, ptr, stream_ptr
    lib = _lib.load()
    res = []
    with Guard(fill, record_calls=False) as G:
        for N in (65, 257):
            x = G.place(on(dev, walk(130, N)))
            for com in (False, True):
                for stride in STRIDES:
                    res.extend(t.clone() for t in ops.displacement_stats(x, [1, 5, 64, 65, 129], stride, com, R_MAX, 7))
                    res.append(ops.velocity_autocorrelation(x, [0, 5, 128], stride, com).clone())
            s2, s4, c = ops.displacement_stats(x, [0, 129], 1, True)               # n_bins == 0: no counts at all
            assert c is None
            res.extend([s2.clone(), s4.clone()])
            res.append(ops.unwrap_frames(x, (L0, 5.0, 0.0)).clone())
        G.verify()
        # rows past the stated shapes stay untouched: outputs of 5 lags given to a call over 3
        x = G.place(on(dev, walk(40, 65)))
        lags3 = (C_INT32 * 3)(0, 1, 39)
        s2 = torch.empty((M0 + 1, 3), dtype=torch.float64, device=dev)
        s4 = torch.empty((M0 + 1, 3), dtype=torch.float64, device=dev)
        cn = torch.empty((M0 + 1, 3, 7), dtype=torch.int64, device=dev)
        co = torch.empty((M0 + 1, 3), dtype=torch.float64, device=dev)
        out = torch.empty((41, M0, 65, 3), dtype=torch.float32, device=dev)
        nbytes = lib.mdno_displacement_stats_workspace_bytes(40, M0, 65, 3, 7)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)                       # exactly the stated size
        assert lib.mdno_displacement_stats(ptr(x), 40, M0, 65, lags3, 3, 1, 1, R_MAX, 7, ptr(s2), ptr(s4), ptr(cn), ptr(ws),
                                           nbytes, stream_ptr(dev)) == 0
        vbytes = lib.mdno_velocity_autocorrelation_workspace_bytes(40, M0, 65, 3)
        vws = torch.empty(vbytes, dtype=torch.uint8, device=dev)
        lagsv = (C_INT32 * 3)(0, 1, 38)
        assert lib.mdno_velocity_autocorrelation(ptr(x), 40, M0, 65, lagsv, 3, 1, 1, ptr(co), ptr(vws), vbytes,
                                                 stream_ptr(dev)) == 0
        assert lib.mdno_unwrap_frames(ptr(x), 40, M0, 65, ops.box_arg((L0, L0, L0)), ptr(out), stream_ptr(dev)) == 0
        G.verify()
        for t in (s2, s4, co):
            assert (t[M0].cpu().view(torch.uint8) == fill).all() and bool(torch.isfinite(t[:M0]).all())
        assert (cn[M0].cpu().view(torch.uint8) == fill).all() and int(cn[:M0].sum()) > 0
        assert (out[40].cpu().view(torch.uint8) == fill).all()
        res.extend([s2[:M0].clone(), s4[:M0].clone(), cn[:M0].clone(), co[:M0].clone(), out[:40].clone()])
        # n_bins == 0 with counts == NULL writes nothing but the sums; refused calls write nothing at all
        since = len(G.records)
        t2 = torch.empty((M0, 3), dtype=torch.float64, device=dev)
        t4 = torch.empty((M0, 3), dtype=torch.float64, device=dev)
        tc = torch.empty((M0, 3, 7), dtype=torch.int64, device=dev)
        tw = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert lib.mdno_displacement_stats(ptr(x), 40, M0, 65, lags3, 3, 1, 0, 0.0, 0, ptr(s2), ptr(s4), None, ptr(ws), nbytes,
                                           stream_ptr(dev)) == 0
        bad_lag = (C_INT32 * 3)(0, 1, 40)
        for args in ((lags3, 3, 0, R_MAX, 7, nbytes), (bad_lag, 3, 1, R_MAX, 7, nbytes), (lags3, 3, 1, 0.0, 7, nbytes),
                     (lags3, 3, 1, R_MAX, 4097, nbytes), (lags3, 3, 1, R_MAX, 7, nbytes - 1), (lags3, 0, 1, R_MAX, 7, nbytes)):
            lg, nl, stride, r_max, n_bins, wb = args
            rc = lib.mdno_displacement_stats(ptr(x), 40, M0, 65, lg, nl, stride, 1, r_max, n_bins, ptr(t2), ptr(t4), ptr(tc),
                                             ptr(tw), wb, stream_ptr(dev))
            assert rc == _lib.EINVAL, args[1:]
        assert lib.mdno_velocity_autocorrelation(ptr(x), 40, M0, 65, lags3, 3, 1, 1, ptr(t2), ptr(tw), nbytes,
                                                 stream_ptr(dev)) == _lib.EINVAL               # lag 39 > S - 2
        tout = torch.empty((40, M0, 65, 3), dtype=torch.float32, device=dev)
        assert lib.mdno_unwrap_frames(ptr(x), 40, M0, 65, ops.box_arg((-1.0, L0, L0)), ptr(tout), stream_ptr(dev)) == _lib.EINVAL
        with pytest.raises(MdnoError):
            ops.displacement_stats(x, [0, 40], 1, True, R_MAX, 7)
        G.untouched(since)
        G.verify()
        res.extend([s2[:M0].clone(), s4[:M0].clone()])
    return res


def test_dynamics_entry_points_stay_inside_their_buffers(dev):
    """Every buffer the new entry points write (sum2, sum4, counts, corr, out, the workspace) inside guard bands under both
    fill bytes: every band intact, every result identical under 0x00 and 0xFF (nothing unset is read: the zeroing of counts
    covers exactly its rows, a workgroup beyond its lag's chunks leaves no partial that is read), rows past the stated shapes
    untouched, and a refused call leaves its buffers untouched."""
    from pathlib import Path
    from guarded import FILLS, header_functions, writes_memory
    header = Path(__file__).resolve().parents[1] / "include" / "mdno_dynamics.h"
    writing = {n for n, params in header_functions(header).items() if writes_memory(params)}
    assert writing == {"mdno_displacement_stats", "mdno_velocity_autocorrelation", "mdno_unwrap_frames"}, writing
    a, b = (_run_guarded(dev, fill) for fill in FILLS)
    assert len(a) == len(b) == 2 * (4 * 4 + 3) + 5 + 2
    for i, (u, v) in enumerate(zip(a, b)):
        assert not torch.isnan(u.double()).any() and torch.equal(u, v), i
    want = ref.displacement_stats(walk(130, 65), [1, 5, 64, 65, 129], 1, False, R_MAX, 7)
    assert np.array_equal(a[2].cpu().numpy(), want.counts)
