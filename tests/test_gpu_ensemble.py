"""Ensemble verification on the device (include/mdno_ensemble.h, csrc/ensemble.hip) against the numpy fp64 restatement of
the rule (tests/ensemble_ref.py): the rank histogram and the two counters as exact integers, the four fp64 sums within the
gate derived from the number of terms, the cases that are exact by construction, the invariance under the order of the
members, the two kernel forms bit for bit, step independence, constructed ties, non-finite input, a huge finite value beside
the padding, the engines' entry points, and guard bands around every buffer the entry point writes."""
import functools

import numpy as np
import pytest
import torch

import ensemble_ref as ref

pytestmark = pytest.mark.gpu

MEMBERS = [1, 2, 3, 5, 8, 31, 32, 33, 63, 64, 65, 100, 257, 1024]
ATOMS = [1, 2, 85, 86, 171]          # 3 N = 3, 6, 255 | 258 (one sample tile of 256 and the first of two), 513 (three tiles)
ATOMS_WIDE = [1, 86, 171]            # M > 64
STEPS = [1, 3]
NAMES = ("sums", "rank_hist", "n_invalid", "n_ties")


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def forms_of(M):
    return ("registers", "lds") if M <= 64 else ("lds",)


def atoms_of(M):
    return ATOMS if M <= 64 else ATOMS_WIDE


@functools.lru_cache(maxsize=None)
def case(S, M, N):
    """(frames, truth, the restatement's Score) of the GPU tests' input: base uniform in [0, 17.1)^3 plus N(0, 0.3) per
    member, the truth drawn likewise, from the first seed of the case's own range at which no member equals the truth in fp32
    (at 1,024 members x 513 samples about two such coincidences are expected per draw; ties have their own test)."""
    first = 100000 * M + 1000 * N + 100 * S
    for seed in range(first, first + 100):
        x, y = ref.ensemble(S, M, N, seed=seed)
        if not (x == y[:, None]).any():
            break
    x.setflags(write=False)
    y.setflags(write=False)
    sc = ref.score(x, y)
    assert not sc.n_ties.any() and not sc.n_invalid.any(), (S, M, N)
    return x, y, sc


def on(dev, x):
    return torch.tensor(np.ascontiguousarray(x)).to(dev)


def device_score(dev, x, y, form="auto"):
    from molecular_dynamics_neural_operator_amd import ops
    out = ops.ensemble_score(on(dev, x), on(dev, y), form)
    S, M = x.shape[0], x.shape[1]
    assert out[0].dtype == torch.float64 and all(t.dtype == torch.int64 for t in out[1:]) and all(t.is_cuda for t in out)
    assert [tuple(t.shape) for t in out] == [(S, 4), (S, M + 1), (S,), (S,)]
    return tuple(t.cpu().numpy() for t in out)


def ratio(got, want, gate):
    """max |got - want| / gate; 0 where the difference is 0 (exact cases), inf where only the gate is."""
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / gate)
    return float(q.max()) if q.size else 0.0


def same(a, b):
    """Every output equal: the integers exactly, the sums numerically bit for bit (the sign of a zero aside; NaN == NaN)."""
    return all(np.array_equal(u, v, equal_nan=u.dtype == np.float64) for u, v in zip(a, b))


def check_against(got, sc, what):
    assert np.array_equal(got[1], sc.rank_hist), what
    assert np.array_equal(got[2], sc.n_invalid) and np.array_equal(got[3], sc.n_ties), what
    r = ratio(got[0], sc.sums, sc.gate)
    assert r <= 1.0, (what, r)
    return r


# ================================================================================================ 1. the restatement
@pytest.mark.parametrize("M", MEMBERS)
def test_scores_equal_the_restatement_in_both_forms(dev, M):
    """Every N and S of the list, registers and LDS where both exist: integers exact, sums within the derived gate, the two
    forms and auto the same bits."""
    worst = 0.0
    for N in atoms_of(M):
        for S in STEPS:
            x, y, sc = case(S, M, N)
            outs = {form: device_score(dev, x, y, form) for form in forms_of(M) + ("auto",)}
            for form, got in outs.items():
                r = check_against(got, sc, (M, N, S, form))
                worst = max(worst, r)
                print(f"M={M} N={N} S={S} {form}: error / gate {r:.3g}")
            first = outs["auto"]
            for form, got in outs.items():
                assert same(first, got), (M, N, S, form)
    print(f"M={M}: largest error / gate {worst:.3g}")


@pytest.mark.parametrize("M", [1, 2, 3, 5, 8, 33, 63, 64, 65, 100, 257, 1024])
def test_integer_offsets_on_a_grid_are_exact(dev, M):
    """The truth on the grid 2^-10, the members at the truth + (m - c), shuffled: every term is exact in fp64, so sums 0, 2
    and 3 equal the restatement and the closed forms bit for bit — n ((M - 1) / 2 - c)^2, n sum_j |j - c|, n M (M^2 - 1) / 6
    — and so does the variance n M (M + 1) / 12 where that number is a dyadic fraction (otherwise: within the gate); the
    truth's rank is c and every sample is a tie."""
    rng = np.random.default_rng(M)
    c = M // 3
    for N in (86, 171):
        S, n = 2, 3 * N
        y = (rng.integers(0, 16 * 1024, size=(S, N, 3)) / 1024.0).astype(np.float32)
        off = np.broadcast_to((np.arange(M, dtype=np.float64) - c)[None, :, None, None], (S, M, N, 3))
        x = (y[:, None].astype(np.float64) + rng.permuted(off, axis=1)).astype(np.float32)
        sc = ref.score(x, y)
        mean = (M - 1) / 2.0 - c
        closed = [n * mean * mean, n * (M * (M + 1) / 12.0), n * float(sum(abs(j - c) for j in range(M))), n * (M * (M * M - 1) / 6.0)]
        for form in forms_of(M):
            got = device_score(dev, x, y, form)
            assert np.array_equal(got[1], sc.rank_hist) and (got[1][:, c] == n).all() and (got[3] == n).all() and not got[2].any()
            for k in (0, 2, 3):
                assert (got[0][:, k] == sc.sums[:, k]).all() and (got[0][:, k] == closed[k]).all(), (form, N, k)
            if M * (M + 1) % 6 == 0:
                assert (got[0][:, 1] == sc.sums[:, 1]).all() and (got[0][:, 1] == closed[1]).all(), (form, N)
            assert ratio(got[0], sc.sums, sc.gate) <= 1.0


# ================================================================================================ 2. invariances
@pytest.mark.parametrize("M", [2, 5, 33, 64, 100, 1024])
def test_the_order_of_the_members_does_not_enter(dev, M):
    N = 171 if M <= 100 else 86
    x, y, _ = case(3, M, N)
    perm = np.roll(np.random.default_rng(M).permutation(M), 1)
    if (perm == np.arange(M)).all():
        perm = perm[::-1]
    assert (perm != np.arange(M)).any()
    for form in forms_of(M):
        assert same(device_score(dev, x, y, form), device_score(dev, x[:, perm], y, form)), form


@pytest.mark.parametrize("M", [8, 64, 257])
def test_same_bits_on_every_call_and_a_step_depends_on_nothing_but_itself(dev, M):
    x, y, _ = case(3, M, 171)
    for form in forms_of(M):
        a, b = device_score(dev, x, y, form), device_score(dev, x, y, form)
        assert same(a, b)
        for s in range(3):
            one = device_score(dev, x[s:s + 1], y[s:s + 1], form)
            assert same(tuple(t[s:s + 1] for t in a), one), (form, s)
        back = device_score(dev, x[::-1], y[::-1], form)
        assert same(tuple(t[::-1] for t in a), back)


# ================================================================================================ 3. ties, non-finite, large
@pytest.mark.parametrize("M", [3, 64, 100])
def test_constructed_ties(dev, M):
    """Members set equal to the truth at chosen samples (one member, two members, all members): each such sample counts
    once in n_ties and its rank is the number of members strictly below the truth."""
    x, y, _ = case(3, M, 86)
    x = x.copy()
    x[0, 1, 4, 2] = y[0, 4, 2]
    x[1, 0, 0, 0] = x[1, M - 1, 0, 0] = y[1, 0, 0]
    x[1, :, 85, 1] = y[1, 85, 1]
    x[1, 2, 7, 0] = -0.0
    yy = y.copy()
    yy[1, 7, 0] = 0.0                                      # -0 == +0: a tie
    sc = ref.score(x, yy)
    assert sc.n_ties.tolist() == [1, 3, 0]
    assert sc.per_sample.rank[1, 85 * 3 + 1] == 0                       # every member equal: none strictly below
    for form in forms_of(M):
        got = device_score(dev, x, yy, form)
        check_against(got, sc, form)
        assert got[3].tolist() == [1, 3, 0] and (got[1].sum(1) == 258).all()


@pytest.mark.parametrize("M", [5, 64, 100])
def test_non_finite_values_spoil_exactly_their_step(dev, M):
    """NaN in one member and Inf in the truth at another sample, both in step 1 of 3: that step's four sums are not finite,
    its histogram loses exactly those two samples, n_invalid counts them; steps 0 and 2 keep their bits."""
    x, y, clean = case(3, M, 86)
    x, y = x.copy(), y.copy()
    x[1, M // 2, 10, 1] = np.nan
    y[1, 60, 2] = np.inf
    sc = ref.score(x, y)
    assert sc.n_invalid.tolist() == [0, 2, 0]
    for form in forms_of(M):
        ok = device_score(dev, case(3, M, 86)[0], case(3, M, 86)[1], form)
        got = device_score(dev, x, y, form)
        assert (~np.isfinite(got[0])).all(1).tolist() == [False, True, False]
        assert np.array_equal(got[0][[0, 2]], ok[0][[0, 2]]) and np.array_equal(got[1][[0, 2]], ok[1][[0, 2]])
        assert got[2].tolist() == [0, 2, 0] and got[3].tolist() == [0, 0, 0]
        assert np.array_equal(got[1], sc.rank_hist) and got[1].sum(1).tolist() == [258, 256, 258]
        lost = ok[1][1] - got[1][1]
        want = np.zeros(M + 1, dtype=np.int64)
        for e in (10 * 3 + 1, 60 * 3 + 2):
            want[clean.per_sample.rank[1, e]] += 1
        assert np.array_equal(lost, want)


def test_a_huge_finite_value_sorts_beside_the_padding(dev):
    """M = 5 is padded to a network of 8 wires by COUNT: a member at 3e38 (finite, legal) is the largest of the five, not
    confused with the padding; -3e38 likewise at the bottom."""
    x, y, _ = case(3, 5, 86)
    x = x.copy()
    x[0, 2, 3, 0] = 3e38
    x[1, 4, 9, 1] = -3e38
    x[2, 0, 80, 2] = 3e38
    x[2, 3, 80, 2] = -3e38
    sc = ref.score(x, y)
    assert not sc.n_invalid.any() and np.isfinite(sc.sums).all() and sc.sums[0, 3] > 1e38
    for form in ("registers", "lds"):
        got = device_score(dev, x, y, form)
        r = check_against(got, sc, form)
        print(f"3e38 among 5 members, {form}: error / gate {r:.3g}")


def test_empty_shapes(dev):
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    x, y, _ = case(3, 8, 86)
    xd, yd = on(dev, x), on(dev, y)
    out = ops.ensemble_score(xd[:0], yd[:0])
    assert [tuple(t.shape) for t in out] == [(0, 4), (0, 9), (0,), (0,)]
    out = ops.ensemble_score(xd[:, :, :0].contiguous(), yd[:, :0].contiguous())               # no atoms: rows of zeros
    assert all(not t.any() for t in out) and out[1].shape == (3, 9)
    e = forecast.ensemble_score(xd[:, :, :0].contiguous(), yd[:, :0].contiguous())
    assert torch.isnan(e.rmse()).all() and torch.isnan(e.rank_flatness()).all() and e.samples_per_step == 0
    for bad in (lambda: ops.ensemble_score(xd, yd[:2]), lambda: ops.ensemble_score(xd, yd[:, :5]),
                lambda: ops.ensemble_score(xd, xd), lambda: ops.ensemble_score(xd[0], yd), lambda: ops.ensemble_score(xd, yd, "tiled"),
                lambda: ops.ensemble_score(xd[:, :0], yd), lambda: ops.ensemble_score(xd[:, :1].expand(3, 1025, 86, 3), yd),
                lambda: ops.ensemble_score(xd[:, :1].expand(3, 65, 86, 3), yd, "registers")):
        with pytest.raises(MdnoError):
            bad()


# ================================================================================================ 4. the engines
def _engine_inputs(M, same_members):
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    N, W = 28, 3
    base = syn.chain_frame(N, seed=1)
    traj = syn.ou_trajectory(base, W + 4, seed=2)
    wins = syn.ensemble_windows(traj[:W], M, sigma=0.0 if same_members else 0.1, seed0=100)            # [M, W, N, 3]
    if same_members:
        wins = np.repeat(wins[:1], M, axis=0)
    truth = torch.from_numpy(np.ascontiguousarray(traj[W:W + 4]).astype(np.float32))
    return (torch.from_numpy(np.ascontiguousarray(wins.transpose(1, 0, 2, 3))), torch.from_numpy(syn.amino_acids(N, seed=1)), truth)


def _model(dev):
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    model = KernelNN(64, 128, 2, 6, 7, 3, 20, 4)
    model.load_state_dict(near_identity_state_dict(64, 128, seed=0, kernel_gain=1e-3, feature_gain=0.1))
    return model.eval().to(dev)


def test_engines_score_their_own_frames(dev):
    """A noisy 4-step, 8-member, N = 28 run: RolloutEngine.ensemble_score equals forecast.ensemble_score(eng.frames(), truth)
    bit for bit, also from a non-zero first step; GroupedRolloutEngine scores its groups' concatenated frames once."""
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine, RolloutEngine
    wins, aa, truth = _engine_inputs(8, False)
    truth = truth.to(dev)
    model = _model(dev)
    for cls in (RolloutEngine, GroupedRolloutEngine):
        eng = cls(model, 8, 28, 3, 8.0, max_steps=4, device=dev, noise_sigma=0.05, noise_seed=7)
        eng.run(wins, aa, 4)
        e = eng.ensemble_score(truth)
        w = forecast.ensemble_score(eng.frames().contiguous(), truth)
        for name in NAMES:
            assert torch.equal(getattr(e, name), getattr(w, name)), (cls.__name__, name)
        assert (e.members, e.samples_per_step, e.n_steps) == (8, 84, 1) and e.sums.shape == (4, 4)
        assert bool((e.spread() > 0).all()) and bool(torch.isfinite(e.spread_skill()).all()) and int(e.rank_hist.sum()) == 4 * 84
        if cls is GroupedRolloutEngine:
            cat = torch.cat([g.frames() for g in eng.engines], dim=1)
            assert len(eng.engines) == 2 and torch.equal(cat, eng.frames())
            assert torch.equal(forecast.ensemble_score(cat, truth).sums, e.sums)
        part = eng.ensemble_score(truth[1:3], first_step=1, steps=2)
        assert torch.equal(part.sums, e.sums[1:3]) and torch.equal(part.rank_hist, e.rank_hist[1:3])
        eng.close()


def test_without_noise_the_members_coincide(dev):
    """noise_sigma = 0 and one window for every member: the members stay equal bit for bit, so the spread and the pair sum
    are exactly 0 and the CRPS is the mean absolute error."""
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    wins, aa, truth = _engine_inputs(8, True)
    truth = truth.to(dev)
    eng = RolloutEngine(_model(dev), 8, 28, 3, 8.0, max_steps=4, device=dev, noise_sigma=0.0)
    eng.run(wins, aa, 4)
    e = eng.ensemble_score(truth)
    assert not e.sums[:, 1].any() and not e.sums[:, 3].any() and not e.spread().any() and not e.spread_skill().any()
    mae = (eng.frames()[:, 0].double() - truth.double()).abs().reshape(4, -1).mean(1)
    assert torch.allclose(e.crps(), mae, rtol=1e-12, atol=0) and bool((e.rmse() > 0).all())
    eng.close()


# ================================================================================================ 5. guard bands
def _run_guarded(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import _lib, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError, ptr, stream_ptr
    lib = _lib.load()
    res = []
    with Guard(fill, record_calls=False) as G:
        for M, N in ((8, 86), (64, 171), (100, 86), (1024, 2)):
            x, y, _ = case(3, M, N)
            xd, yd = G.place(on(dev, x)), G.place(on(dev, y))
            for form in forms_of(M):
                res.extend(t.clone() for t in ops.ensemble_score(xd, yd, form))
        G.verify()
        # rows past the stated shapes stay untouched: outputs of 4 steps given to a call over 3, the workspace exactly as stated
        x, y, _ = case(3, 8, 86)
        xd, yd = G.place(on(dev, x)), G.place(on(dev, y))
        for form in (1, 2):
            sums = torch.empty((4, 4), dtype=torch.float64, device=dev)
            hist = torch.empty((4, 9), dtype=torch.int64, device=dev)
            inv = torch.empty((4,), dtype=torch.int64, device=dev)
            ties = torch.empty((4,), dtype=torch.int64, device=dev)
            nbytes = lib.mdnoens_score_workspace_bytes(3, 8, 86)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            assert lib.mdnoens_score(ptr(xd), ptr(yd), 3, 8, 86, ptr(sums), ptr(hist), ptr(inv), ptr(ties), form, ptr(ws), nbytes,
                                     stream_ptr(dev)) == 0
            G.verify()
            for t in (sums, hist, inv, ties):
                assert (t[3].cpu().reshape(-1).view(torch.uint8) == fill).all()
            assert bool(torch.isfinite(sums[:3]).all()) and hist[:3].sum(1).tolist() == [258] * 3
            res.extend([sums[:3].clone(), hist[:3].clone(), inv[:3].clone(), ties[:3].clone()])
        # a refused call writes nothing
        since = len(G.records)
        t_sums = torch.empty((3, 4), dtype=torch.float64, device=dev)
        t_hist = torch.empty((3, 9), dtype=torch.int64, device=dev)
        t_inv = torch.empty((3,), dtype=torch.int64, device=dev)
        t_ties = torch.empty((3,), dtype=torch.int64, device=dev)
        t_ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        for M, form, wb, code in ((8, 3, nbytes, _lib.EINVAL), (8, 0, nbytes - 1, _lib.EINVAL), (0, 0, nbytes, _lib.EINVAL),
                                  (1025, 0, nbytes, _lib.EINVAL), (65, 1, nbytes, _lib.EUNSUPPORTED)):
            rc = lib.mdnoens_score(ptr(xd), ptr(yd), 3, M, 86, ptr(t_sums), ptr(t_hist), ptr(t_inv), ptr(t_ties), form, ptr(t_ws),
                                   wb, stream_ptr(dev))
            assert rc == code, (M, form, wb)
        with pytest.raises(MdnoError):
            ops.ensemble_score(xd, yd[:2])
        G.untouched(since)
        G.verify()
    return res


def test_ensemble_entry_point_stays_inside_its_buffers(dev):
    """sums, rank_hist, n_invalid, n_ties and the workspace inside guard bands under both fill bytes, both forms, one to
    three sample tiles, 8 to 1,024 members: every band intact, every result identical under 0x00 and 0xFF (nothing unset is
    read: the zeroing covers exactly the integer rows), rows past the stated shapes untouched, a refused call writes
    nothing."""
    from pathlib import Path
    from guarded import FILLS
    import re
    header = Path(__file__).resolve().parents[1] / "include" / "mdno_ensemble.h"
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    assert re.findall(r"^int\s+(mdnoens_\w+)\s*\(", text, flags=re.M) == ["mdnoens_score"]            # the one that writes
    a, b = (_run_guarded(dev, fill) for fill in FILLS)
    assert len(a) == len(b) == 4 * (2 + 2 + 1 + 1) + 8
    for i, (u, v) in enumerate(zip(a, b)):
        assert not torch.isnan(u.double()).any() and torch.equal(u, v), i
    assert np.array_equal(a[1].cpu().numpy(), case(3, 8, 86)[2].rank_hist)
