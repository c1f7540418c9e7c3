"""Pair-distance histograms and the radius of gyration on the device (include/mdno_observe.h, csrc/observe.hip) against
the numpy fp64 restatement of the rule (tests/observe_ref.py): counts as exact integers in both kernel forms, the cases
whose bins are known by construction, the identity with the contact counts of mdno_forecast_score, non-finite
coordinates, leading dimensions, the engines' entry points, the radius of gyration against fp64, and guard bands around
every buffer the new entry points write."""
import functools

import numpy as np
import pytest
import torch

import observe_ref as ref

pytestmark = pytest.mark.gpu

L0 = 17.1
SEED = 1
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 300, 513]
# (n_bins, r_max, box)
COMBOS = {"one_bin": (1, 8.0, None), "seven": (7, 8.0, None), "cubic": (64, 8.5, (17.1, 17.1, 17.1)),
          "slab_half_box": (4096, 8.55, (17.1, 17.1, 0.0)), "open_200": (200, 12.0, None)}
FORMS = ("lds", "tiled")


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def random_frames(N, F=3, seed=SEED):
    """f32 [F, N, 3], uniform in [-0.2 L, 1.3 L)^3: frames need not lie inside the box."""
    rng = np.random.default_rng(seed)
    x = ((rng.random((F, N, 3)) * 1.5 - 0.2) * L0).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def expected(N, combo):
    """The restatement's counts i64 [3, n_bins] of random_frames(N), with the condition the comparison rests on."""
    n_bins, r_max, box = COMBOS[combo]
    x = random_frames(N)
    m = min(ref.margin(f, r_max, n_bins, box) for f in x)
    assert m >= 1e-9, f"N={N} {combo}: a pair lies {m} bins from an edge; choose another seed"
    want = ref.histograms(x, r_max, n_bins, box)
    want.setflags(write=False)
    return want, m


def device_counts(dev, x, r_max, n_bins, box=None, form="auto"):
    from molecular_dynamics_neural_operator_amd import ops
    c = ops.pair_histogram(torch.tensor(x).to(dev), r_max, n_bins, box, form)
    assert c.dtype == torch.int64 and c.is_cuda
    return c.cpu().numpy()


# ================================================================================================ 1. exact equality
@pytest.mark.parametrize("combo", sorted(COMBOS))
@pytest.mark.parametrize("N", SIZES)
def test_counts_equal_the_restatement(dev, N, combo):
    """Both forms, F = 1 and F = 3: wave and tile edges, an odd N for the row pairing, two and three pair tiles with a
    ragged last one (300, 513), r_max == L / 2 exactly on a slab, 1 and 4,096 bins."""
    n_bins, r_max, box = COMBOS[combo]
    want, m = expected(N, combo)
    x = random_frames(N)
    print(f"N={N} {combo}: margin {m:.3g} bins, {int(want.sum())} pairs counted of {3 * N * (N - 1) // 2}")
    for form in FORMS:
        for F in (1, 3):
            got = device_counts(dev, x[:F], r_max, n_bins, box, form)
            assert got.shape == (F, n_bins)
            assert np.array_equal(got, want[:F]), (form, F, int(np.abs(got - want[:F]).sum()))
    assert np.array_equal(device_counts(dev, x, r_max, n_bins, box, "auto"), want)
    if N >= 63:
        assert want.sum() > 0 and all(int(w.sum()) < N * (N - 1) // 2 for w in want)      # r_max cuts the frame


# ================================================================================================ 2. exact by construction
def triple_atoms():
    """Integer coordinates whose distances are known exactly: 3-4-5 and 5-12-13 triples from the origin, one pair at
    r == r_max == 13, two atoms at the same place."""
    return np.array([[0, 0, 0], [3, 4, 0], [5, 12, 0], [0, 0, 0], [0, 13, 0], [40, 40, 40]], dtype=np.float32)


@pytest.mark.parametrize("form", FORMS)
def test_exact_bins_by_construction(dev, form):
    x = triple_atoms()
    r = ref.pair_distances(x)
    assert r[0, 1] == 5.0 and r[0, 2] == 13.0 and r[0, 4] == 13.0 and r[0, 3] == 0.0
    want = ref.histogram(x, 13.0, 13)
    assert ref.margin(x, 13.0, 13, ignore_zero=True) >= 1e-3          # every other pair is well inside its bin
    got = device_counts(dev, x[None], 13.0, 13, None, form)[0]
    assert np.array_equal(got, want)
    # by hand: pairs among atoms 0..4 (atom 5 is far from all).  0-3 coincide: bin 0.  0-1 and 3-1 at exactly 5: bin 5.
    # 0-2, 3-2, 0-4, 3-4 at exactly 13 == r_max: not counted.  1-2 = sqrt(4 + 64) = 8.246: bin 8.  1-4 = sqrt(9 + 81)
    # = 9.487: bin 9.  2-4 = sqrt(25 + 1) = 5.099: bin 5.
    hand = np.zeros(13, dtype=np.int64)
    hand[0], hand[5], hand[8], hand[9] = 1, 3, 1, 1
    assert np.array_equal(got, hand)


@pytest.mark.parametrize("form", FORMS)
def test_whole_box_vectors_leave_the_histogram_unchanged(dev, form):
    """L = 32 and coordinates that are multiples of 2^-4: moving atoms by whole box vectors is exact in fp32 and in
    the fp64 differences, so every minimum-image distance keeps its bits."""
    L, r_max, n_bins = 32.0, 13.0, 13
    box = (L, L, L)
    rng = np.random.default_rng(7)
    base = np.concatenate([triple_atoms()[:5], rng.integers(0, 32 * 16, size=(60, 3)) / 16.0]).astype(np.float32)
    moved = (base.astype(np.float64) + rng.integers(-3, 4, size=base.shape) * L).astype(np.float32)
    assert np.array_equal(moved.astype(np.float64) - base.astype(np.float64), np.rint((moved - base) / L) * L)
    assert (moved != base).any()
    want = ref.histogram(base, r_max, n_bins, box)
    assert np.array_equal(ref.histogram(moved, r_max, n_bins, box), want)
    assert want[5] >= 2 and want[0] >= 1
    a = device_counts(dev, base[None], r_max, n_bins, box, form)[0]
    b = device_counts(dev, moved[None], r_max, n_bins, box, form)[0]
    assert np.array_equal(a, want) and np.array_equal(b, want)


# ================================================================================================ 3. further cases
@pytest.mark.parametrize("N", [300, 513])
@pytest.mark.parametrize("box", [None, (17.1, 17.1, 0.0)])
def test_contact_identity(dev, N, box):
    """2 * counts.sum() + N is the forecast contact count of ops.forecast_score on the same frames (ordered pairs,
    diagonal included): the new kernels tied to an existing one, in exact integers."""
    from molecular_dynamics_neural_operator_amd import ops
    x = torch.tensor(random_frames(N)).to(dev)
    thr = 8.0
    contacts = ops.forecast_score(x[:, None].contiguous(), x, thr, box=box)[2][:, 0, 0]
    for form in FORMS:
        counts = ops.pair_histogram(x, thr, 31, box, form)
        assert torch.equal(2 * counts.sum(-1) + N, contacts), form
    assert int(contacts.min()) > N


@pytest.mark.parametrize("form", FORMS)
def test_non_finite_atoms_are_in_no_pair(dev, form):
    from molecular_dynamics_neural_operator_amd import ops
    N, n_bins, r_max = 65, 7, 8.0
    x = random_frames(N).copy()
    x[1, 5, 1] = np.nan
    x[1, 40, 2] = np.inf
    keep = np.ones(N, bool)
    keep[[5, 40]] = False
    for box in (None, (17.1, 17.1, 17.1)):
        want = ref.histograms(x, r_max, n_bins, box)
        assert np.array_equal(want[1], ref.histogram(x[1][keep], r_max, n_bins, box))      # the others are counted
        assert np.array_equal(device_counts(dev, x, r_max, n_bins, box, form), want)
    rg = ops.radius_of_gyration(torch.from_numpy(x).to(dev)).cpu().numpy()
    assert np.isnan(rg[1]) and np.isfinite(rg[[0, 2]]).all()


@pytest.mark.parametrize("form", FORMS)
def test_a_box_nothing_wraps_in_is_the_open_result(dev, form):
    x = random_frames(257)
    opn = device_counts(dev, x, 12.0, 200, None, form)
    assert np.array_equal(device_counts(dev, x, 12.0, 200, (1e6, 1e6, 1e6), form), opn)
    assert np.array_equal(device_counts(dev, x, 12.0, 200, (0.0, 0.0, 0.0), form), opn)
    assert not np.array_equal(device_counts(dev, x, 8.5, 200, (17.1, 17.1, 17.1), form),
                              device_counts(dev, x, 8.5, 200, None, form))


def test_leading_dimensions(dev):
    from molecular_dynamics_neural_operator_amd import forecast, ops
    x = np.stack([random_frames(65, 3, seed=s) for s in (1, 2)], axis=1)          # [S, M, N, 3] = [3, 2, 65, 3]
    xd = torch.from_numpy(x).to(dev)
    flat = ops.pair_histogram(xd.reshape(6, 65, 3), 8.0, 7)
    h = forecast.pair_histogram(xd, 8.0, 7)
    assert h.counts.shape == (3, 2, 7) and torch.equal(h.counts.reshape(6, 7), flat)
    assert h.n_atoms == 65 and h.n_frames == 1 and h.box is None
    assert np.array_equal(h.counts.cpu().numpy(), ref.histograms(x, 8.0, 7))
    s = h.sum((0,))
    assert s.counts.shape == (2, 7) and s.n_frames == 3 and torch.equal(s.counts, h.counts.sum(0))
    assert ops.pair_histogram(xd[0, 0], 8.0, 7).shape == (7,)
    rg = forecast.radius_of_gyration(xd)
    assert rg.shape == (3, 2) and torch.equal(rg.reshape(6), ops.radius_of_gyration(xd.reshape(6, 65, 3)))
    # no frames, no atoms, one atom
    assert ops.pair_histogram(xd[:0], 8.0, 7).shape == (0, 2, 7)
    for form in ("auto",) + FORMS:
        assert not ops.pair_histogram(xd[:, :, :1].contiguous(), 8.0, 7, form=form).any()
        assert not ops.pair_histogram(xd[:, :, :0].contiguous(), 8.0, 7, form=form).any()
    assert torch.isnan(ops.radius_of_gyration(xd[:, :, :0].contiguous())).all()


def _engine_inputs():
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    M, N, W = 2, 28, 3
    base = syn.chain_frame(N, seed=1)
    traj = syn.ou_trajectory(base, W, seed=2)
    wins = syn.ensemble_windows(traj[:W], M, sigma=0.1, seed0=100)                   # [M, W, N, 3]
    return torch.from_numpy(np.ascontiguousarray(wins.transpose(1, 0, 2, 3))), torch.from_numpy(syn.amino_acids(N, seed=1))


@pytest.mark.parametrize("box", [None, (40.0, 40.0, 0.0)])
def test_engines_observe_their_own_frames(dev, box):
    """RolloutEngine.pair_histogram / radius_of_gyration on a 3-step, 2-member, N = 28 run equal the ops on
    eng.frames() in the engine's own box; the grouped engine equals the single one."""
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine, RolloutEngine
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    wins, aa = _engine_inputs()
    model = KernelNN(64, 128, 2, 6, 7, 3, 20, 4)
    model.load_state_dict(near_identity_state_dict(64, 128, seed=0, kernel_gain=1e-3, feature_gain=0.1))
    model.eval().to(dev)
    got = []
    for cls in (RolloutEngine, GroupedRolloutEngine):
        eng = cls(model, 2, 28, 3, 8.0, max_steps=3, device=dev, box=box)
        fr = eng.run(wins, aa, 3).clone()
        h = eng.pair_histogram(12.0, 50)
        assert h.counts.shape == (3, 2, 50) and h.box == eng.box and h.n_atoms == 28
        assert torch.equal(h.counts, ops.pair_histogram(fr, 12.0, 50, box=eng.box))
        assert int(h.counts.sum()) > 0
        assert torch.equal(eng.pair_histogram(12.0, 50, first_step=1, steps=2).counts, h.counts[1:])
        rg = eng.radius_of_gyration()
        assert rg.shape == (3, 2) and torch.equal(rg, ops.radius_of_gyration(fr))
        assert torch.equal(eng.radius_of_gyration(2), rg[2:])
        got.append((fr, h.counts, rg))
        eng.close()
    if torch.equal(got[0][0], got[1][0]):          # (the groups' frames are the single engine's for like members)
        assert torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][2], got[1][2])
    else:
        assert torch.equal(got[1][1], ops.pair_histogram(got[1][0], 12.0, 50, box=box))


# ================================================================================================ 4. radius of gyration
@pytest.mark.parametrize("N", [1, 2, 65, 2049])
def test_radius_of_gyration_against_fp64(dev, N):
    """|x| <= 32, relative gate 1e-9: the kernel and numpy differ in summation order and in the centroid's rounding only,
    bounded by about N * 2^-52 * max|x|^2 / rg^2 = 5e-10 at N = 2,049.  Worst relative difference seen on an MI355X:
    0 at all four sizes (the coordinate sums of f32 values are exact in fp64, and the rest rounded alike for these frames)."""
    from molecular_dynamics_neural_operator_amd import ops
    rng = np.random.default_rng(N)
    x = ((rng.random((3, N, 3)) * 2.0 - 1.0) * 32.0).astype(np.float32)
    want = np.array([ref.radius_of_gyration(f) for f in x])
    got = ops.radius_of_gyration(torch.from_numpy(x).to(dev))
    assert got.dtype == torch.float64 and got.shape == (3,)
    got = got.cpu().numpy()
    err = np.abs(got - want) / np.where(want > 0, want, 1.0)
    print(f"N={N}: rg {want}, worst relative difference {err.max():.3g}")
    assert (np.abs(got - want) <= 1e-9 * want).all()
    again = ops.radius_of_gyration(torch.from_numpy(x).to(dev)).cpu().numpy()
    assert np.array_equal(got.view(np.int64), again.view(np.int64))          # fixed order: the same bits


# ================================================================================================ 5. guard bands
def _run_guarded(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import _lib, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError, ptr, stream_ptr
    lib = _lib.load()
    res = []
    with Guard(fill, record_calls=False) as G:
        for N in (65, 257):
            x = G.place(torch.tensor(random_frames(N)).to(dev))
            for form in FORMS:
                for box in (None, (17.1, 17.1, 17.1)):
                    res.append(ops.pair_histogram(x, 8.0, 7, box, form).clone())
            res.append(ops.radius_of_gyration(x).clone())
        G.verify()
        # refused calls write nothing: the C entry point with real buffers and a bad argument
        since = len(G.records)
        x = G.place(torch.tensor(random_frames(65)).to(dev))
        counts = torch.empty((3, 7), dtype=torch.int64, device=dev)
        bad_box = ops.box_arg((15.9, 17.1, 17.1))
        for n_bins, r_max, box, form, code in ((0, 8.0, None, 0, _lib.EINVAL), (7, 0.0, None, 2, _lib.EINVAL),
                                               (7, 8.0, bad_box, 2, _lib.EINVAL), (7, 8.0, None, 3, _lib.EINVAL)):
            rc = lib.mdno_pair_histogram(ptr(x), 3, 65, r_max, n_bins, box, ptr(counts), form, None, 0, stream_ptr(dev))
            assert rc == code, (n_bins, r_max, form, rc)
        with pytest.raises(MdnoError):
            ops.pair_histogram(x, 8.0, 7, (15.9, 17.1, 17.1), "tiled")
        G.untouched(since)
        G.verify()
    return res


def test_observe_entry_points_stay_inside_their_buffers(dev):
    """Both forms of the histogram and the radius of gyration at N = 65 and 257 with 7 bins inside guard bands under both
    fill bytes: every band intact, every result identical under 0x00 and 0xFF (the tiled form's zeroing covers exactly
    its rows, nothing unset is read), and a refused call leaves its buffers untouched."""
    from pathlib import Path
    from guarded import FILLS, header_functions, writes_memory
    header = Path(__file__).resolve().parents[1] / "include" / "mdno_observe.h"
    writing = {n for n, params in header_functions(header).items() if writes_memory(params)}
    assert writing == {"mdno_pair_histogram", "mdno_radius_of_gyration"}, writing
    a, b = (_run_guarded(dev, fill) for fill in FILLS)
    assert len(a) == len(b) == 10
    for i, (u, v) in enumerate(zip(a, b)):
        assert not torch.isnan(u.double()).any() and torch.equal(u, v), i
    want = ref.histograms(random_frames(65), 8.0, 7)
    assert np.array_equal(a[0].cpu().numpy(), want) and np.array_equal(a[2].cpu().numpy(), want)
