"""Distance-constraint projection on the device (include/mdno_constrain.h, csrc/constrain.hip)
against the numpy fp64 restatement of the header's rule (tests/constrain_ref.py).  Every operation of the rule is an IEEE
operation rounded once and the order is fixed, so there is no tolerance anywhere in this file: the projected frames equal the
restatement's fp64 state rounded once to fp32 bit for bit, the sweep counts are equal and viol_in / viol_out are bit-equal
doubles.  Then the engine: a constrained rollout is the step-by-step composition of a plain engine and the stand-alone
projection, with graph replay and with plain launches, after the noise, in groups, and not at all when switched off."""
import functools

import numpy as np
import pytest
import torch

import constrain_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def device_project(dev, frames, table, weights=None, box=None, iterations=8, tol=0.0, in_place=False):
    """ops.project_constraints on the restatement's own coloured table -> numpy (out, sweeps, viol_in, viol_out)."""
    from molecular_dynamics_neural_operator_amd import ops
    pairs, lo, hi, ptr = table[:4]
    x = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32)).to(dev)
    keep = x.clone()
    w = None if weights is None else torch.from_numpy(np.asarray(weights, dtype=np.float32)).to(dev)
    out, sweeps, vin, vout = ops.project_constraints(
        x, torch.from_numpy(pairs).to(dev), torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev), torch.from_numpy(ptr).to(dev),
        w, box=box, iterations=iterations, tol=tol, out=x if in_place else None)
    if in_place:
        assert out.data_ptr() == x.data_ptr()
    else:
        assert torch.equal(x.view(torch.int32), keep.view(torch.int32))          # the input is left alone
    return out.cpu().numpy(), sweeps.cpu().numpy(), vin.cpu().numpy(), vout.cpu().numpy()


def check(dev, frames, table, **kw):
    """Device = restatement, bit for bit, out of place and in place; returns the restatement's (out, sweeps, vin, vout)."""
    want = R.project(frames, *table[:4], **kw)[:4]
    for in_place in (False, True):
        got = device_project(dev, frames, table, in_place=in_place, **kw)
        assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
        assert np.array_equal(got[1], want[1]), ("sweeps", in_place, got[1], want[1])
        assert np.array_equal(bits64(got[2]), bits64(want[2])), ("viol_in", in_place)
        assert np.array_equal(bits64(got[3]), bits64(want[3])), ("viol_out", in_place)
        assert np.array_equal(bits32(got[0]), bits32(want[0])), ("frames", in_place)
    return want


def noisy_frames(n, n_frames, seed, sigma=0.3, band=0.05, second=True):
    """Noisy copies of one random-walk chain of n atoms and the table of its chain (+ (i, i + 2)) bands."""
    clean, _ = R.random_walk_chain(n, 3.8, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    pairs = R.chain_pairs(n, second)
    d = R.lengths(clean, pairs) if len(pairs) else np.zeros(0)
    frames = (clean[None] + rng.normal(scale=sigma, size=(n_frames,) + clean.shape)).astype(np.float32)
    return frames, R.colour_table(pairs, d - band, d + band)


# ================================================================================================ 1. the rule, bit for bit
@pytest.mark.parametrize("N,F", [(1, 3), (2, 1), (3, 3), (28, 130), (65, 3), (257, 3)])
def test_projection_equals_the_restatement_at_every_size(dev, N, F):
    """No constraint at all (N = 1), one (N = 2), two colours (N = 3), chain + (i, i + 2) at 28 atoms over 130 frames (nine
    workgroups of 16 frames, the last with two), and the wave and workgroup tails (65, 257)."""
    frames, table = noisy_frames(N, F, seed=N)
    assert table[3].shape[0] - 1 == {1: 0, 2: 1, 3: 3}.get(N, 4)
    _, sweeps, vin, vout = check(dev, frames, table)
    if N > 1:          # (a short chain can land inside its bands exactly, and then stops: tol = 0)
        assert (sweeps == 8).all() if N >= 28 else (sweeps >= 1).all()
        assert (vout < vin).all()
    else:
        assert not sweeps.any() and not vin.any() and not vout.any()


def test_three_atom_chain_has_two_colours(dev):
    frames, table = noisy_frames(3, 3, seed=3, second=False)
    assert table[3].tolist() == [0, 1, 2]
    check(dev, frames, table)


def test_early_exit_is_per_frame(dev):
    """130 frames of 28 atoms with noise from 0 to 0.5 A against tol = 1e-3 and 40 sweeps: the frames of one workgroup stop
    after different numbers of sweeps (a clean frame after none), and each equals the restatement's."""
    clean, _ = R.random_walk_chain(28, 3.8, seed=5)
    rng = np.random.default_rng(55)
    pairs = R.chain_pairs(28)
    d = R.lengths(clean, pairs)
    table = R.colour_table(pairs, d - 0.05, d + 0.05)
    sig = np.linspace(0.0, 0.5, 130)[:, None, None]
    frames = (clean[None] + sig * rng.normal(size=(130,) + clean.shape)).astype(np.float32)
    out, sweeps, vin, vout = check(dev, frames, table, iterations=40, tol=1e-3)
    assert sweeps[0] == 0 and np.array_equal(bits32(out[0]), bits32(frames[0]))
    assert len(set(sweeps[:16].tolist())) > 2 and len(set(sweeps.tolist())) > 5 and sweeps.max() <= 40
    done = sweeps < 40
    assert done.sum() > 60 and (vout[done] <= 1e-3).all()
    # iterations = 0 measures only: the frames' own bits, viol_out = viol_in
    out0, sweeps0, vin0, vout0 = check(dev, frames, table, iterations=0)
    assert np.array_equal(bits32(out0), bits32(frames)) and not sweeps0.any() and np.array_equal(bits64(vin0), bits64(vin))
    assert np.array_equal(bits64(vout0), bits64(vin0))


def test_colours_of_1_256_and_257_constraints(dev):
    """514 atoms: 257 disjoint pairs (2k, 2k + 1) share colour 0, the 256 pairs (2k + 1, 2k + 2) colour 1, and (0, 2), whose
    atoms hold both, is alone in colour 2: one constraint, a full workgroup, and a workgroup and one."""
    n = 514
    k = np.arange(257)
    pairs = np.concatenate([np.stack([2 * k, 2 * k + 1], 1), np.stack([2 * k[:256] + 1, 2 * k[:256] + 2], 1), [[0, 2]]])
    clean, _ = R.random_walk_chain(n, 3.8, seed=8)
    d = R.lengths(clean, pairs)
    table = R.colour_table(pairs, d - 0.02, d + 0.02)
    assert np.diff(table[3]).tolist() == [257, 256, 1]
    frames = (clean[None] + np.random.default_rng(8).normal(scale=0.2, size=(3,) + clean.shape)).astype(np.float32)
    check(dev, frames, table)


def test_hub_atom_in_70_constraints(dev):
    n = 71
    pairs = np.stack([np.zeros(70, dtype=np.int64), np.arange(1, 71)], 1)
    x = np.random.default_rng(9).normal(scale=4.0, size=(3, n, 3)).astype(np.float32)
    table = R.colour_table(pairs, 5.0, 6.0)
    assert table[3].shape[0] - 1 == 70 and np.diff(table[3]).max() == 1
    _, sweeps, vin, vout = check(dev, x, table)
    assert (sweeps > 0).all() and (vout < vin).all()


def test_largest_frame_and_one_above(dev):
    from molecular_dynamics_neural_operator_amd import forecast as F, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    n = ops.CST_MAX_ATOMS
    frames, table = noisy_frames(n, 2, seed=11, second=False)
    _, sweeps, vin, vout = check(dev, frames, table, iterations=3)
    assert (sweeps == 3).all() and (vout < vin).all()
    big = torch.zeros((1, n + 1, 3), device=dev)
    with pytest.raises(MdnoError, match="at most"):
        F.project_constraints(big, F.DistanceConstraints.chain(n + 1, 3.7, 3.9))
    with pytest.raises(MdnoError, match="at most"):
        ops.project_constraints(big, *(torch.from_numpy(t).to(dev) for t in table[:4]))


def test_weights_pin_atoms(dev):
    """Atom 9 pinned, atoms 20 and 21 (a bond: its constraint is skipped) pinned, one heavy and one light atom."""
    frames, table = noisy_frames(28, 3, seed=12)
    w = np.ones(28, dtype=np.float32)
    w[[9, 20, 21]] = 0.0
    w[3], w[15] = 0.25, 7.0
    out, sweeps, _, _ = check(dev, frames, table, weights=w)
    assert np.array_equal(bits32(out[:, [9, 20, 21]]), bits32(frames[:, [9, 20, 21]])) and (sweeps == 8).all()
    assert not np.array_equal(out[:, 10], frames[:, 10])


def test_coincident_nan_inf_atoms_and_out_of_range_indices(dev):
    frames, _ = noisy_frames(28, 4, seed=13)
    frames[0, 5] = frames[0, 4]                           # len == 0: skipped (and the pair (3, 5), (4, 6) go on)
    frames[1, 7, 1] = np.nan
    frames[2, 19, 0] = np.inf
    frames[3, 2, 2] = -np.inf
    pairs = np.concatenate([R.chain_pairs(28), [[-1, 3], [4, 28], [2 ** 31 - 1, 0], [-2 ** 31, 5], [28, 29]]])
    table = R.colour_table(pairs, 3.7, 3.9)
    table = (table[0], np.where(table[0][:, 0] + 2 == table[0][:, 1], 5.0, table[1]), np.where(table[0][:, 0] + 2 == table[0][:, 1], 7.0, table[2]),
             table[3])
    out, sweeps, vin, vout = check(dev, frames, table)
    assert np.isfinite(vin).all() and np.isfinite(vout).all() and (sweeps == 8).all()
    bad = ~np.isfinite(out).all(2)
    assert bad.sum() == 3 and bad[1, 7] and bad[2, 19] and bad[3, 2]
    for f, a in ((1, 7), (2, 19), (3, 2)):
        assert np.array_equal(bits32(out[f, a]), bits32(frames[f, a]))
    # with a box the difference of an Inf and a finite coordinate becomes NaN through the image: still confined
    check(dev, frames, table, box=(40.0, 40.0, 40.0))


def test_one_sided_and_equality_bands(dev):
    frames, _ = noisy_frames(28, 3, seed=14, sigma=0.5)
    pairs = R.chain_pairs(28)
    n_bonds = 27
    lo = np.where(np.arange(len(pairs)) < n_bonds, 3.8, 6.0)          # bonds: lo == hi; (i, i + 2): a lower bound only
    hi = np.where(np.arange(len(pairs)) < n_bonds, 3.8, np.inf)
    table = R.colour_table(pairs, lo, hi)
    out, sweeps, vin, vout = check(dev, frames, table, iterations=30, tol=1e-7)
    assert (vout < vin).all()
    far = np.full(len(pairs), 100.0)                                    # hi = inf and nothing below lo = 0: nothing to do
    out, sweeps, vin, vout = check(dev, frames, R.colour_table(pairs, 0.0, np.inf))
    assert np.array_equal(bits32(out), bits32(frames)) and not sweeps.any() and not vin.any()
    check(dev, frames, R.colour_table(pairs, far, far), iterations=2)  # and everything far outside


def test_periodic_boxes(dev):
    """A cubic box with pairs across the boundary (k != 0 in the minimum image) and a slab (z open)."""
    L = 12.0
    rng = np.random.default_rng(15)
    frames = (rng.random((3, 40, 3)) * L).astype(np.float32)
    frames[:, 0, 0], frames[:, 1, 0] = 0.4, L - 0.5                     # 0.9 apart through the x boundary
    pairs = R.chain_pairs(40)
    table = R.colour_table(pairs, 2.0, 3.0)
    cubic = check(dev, frames, table, box=(L, L, L))
    slab = check(dev, frames, table, box=(L, L, 0.0))
    open_ = check(dev, frames, table)
    assert not np.array_equal(cubic[0], slab[0]) and not np.array_equal(slab[0], open_[0])
    check(dev, frames, table, box=(L, 0.0, 2.5 * L), iterations=3)
    two = np.array([[[0.4, 1.0, 2.0], [L - 0.5, 1.0, 2.0]]], dtype=np.float32)
    out, sweeps, vin, vout = check(dev, two, R.colour_table([[0, 1]], 2.0, 3.0), box=(L, L, L))
    assert abs(vin[0] - 1.1) < 1e-6 and sweeps[0] >= 1                  # 0.9 apart through the x boundary, not 11.1
    assert out[0, 0, 0] > 0.4 and out[0, 1, 0] < L - 0.5                # pushed apart THROUGH the boundary, never wrapped
    assert abs((out[0, 0, 0] - 0.4) - 0.55) < 1e-5 and abs((L - 0.5 - out[0, 1, 0]) - 0.55) < 1e-5


def test_two_calls_and_every_batch_give_the_same_bits(dev):
    frames, table = noisy_frames(28, 130, seed=16)
    a = device_project(dev, frames, table)
    b = device_project(dev, frames, table)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    for sl in (slice(0, 1), slice(5, 8), slice(17, 130)):               # F = 1, 3, 113: other groups, the same frames
        c = device_project(dev, frames[sl], table)
        assert np.array_equal(bits32(c[0]), bits32(a[0][sl])) and np.array_equal(c[1], a[1][sl])
        assert np.array_equal(bits64(c[3]), bits64(a[3][sl]))


def test_python_layer_shapes_and_from_frames(dev):
    """forecast.project_constraints on [S, M, N, 3] = the restatement on the package's own coloured table; from_frames takes
    the truth's per-pair range, inside which the truth comes back untouched."""
    from molecular_dynamics_neural_operator_amd import forecast as F
    frames, _ = noisy_frames(28, 12, seed=17, sigma=0.1)
    truth = torch.from_numpy(frames).to(dev).view(4, 3, 28, 3)
    ft = F.Featurizer.backbone(28, 3, 4)
    dc = F.DistanceConstraints.from_frames(truth, ft, margin=0.0)
    d = F.internal_coordinates(truth, F.Featurizer.of(pairs=ft.pairs), dtype=torch.float64).reshape(12, -1)
    assert len(dc) == ft.pairs.shape[0] and torch.equal(dc.lo, d.amin(0).cpu()) and torch.equal(dc.hi, d.amax(0).cpu())
    same, rep = F.project_constraints(truth, dc)
    assert torch.equal(same.view(torch.int32), truth.view(torch.int32)) and rep.sweeps.shape == (4, 3) and not bool(rep.sweeps.any())
    assert not bool(rep.viol_in.any()) and rep.viol_in.dtype == torch.float64 and rep.sweeps.dtype == torch.int32
    wide = F.DistanceConstraints.from_frames(truth, ft.pairs, margin=0.25)
    assert torch.equal(wide.lo, (dc.lo - 0.25).clamp_min(0.0)) and torch.equal(wide.hi, dc.hi + 0.25)
    noisy = truth + 0.3 * torch.randn(truth.shape, device=dev, generator=torch.Generator(dev).manual_seed(1))
    got, rep = F.project_constraints(noisy, dc, iterations=5)
    t = dc.coloured(dev)
    want = R.project(noisy.cpu().numpy().reshape(12, 28, 3), t.pairs.cpu().numpy(), t.lo.cpu().numpy(), t.hi.cpu().numpy(),
                     t.colour_ptr.cpu().numpy(), iterations=5)
    assert np.array_equal(bits32(got.cpu().numpy().reshape(12, 28, 3)), bits32(want[0]))
    assert np.array_equal(rep.sweeps.cpu().numpy().reshape(-1), want[1])
    assert np.array_equal(bits64(rep.viol_out.cpu().numpy().reshape(-1)), bits64(want[3]))
    assert bool((rep.viol_out < rep.viol_in).all())


# ================================================================================================ 2. the engine
W, STEPS = 3, 6


@functools.lru_cache(maxsize=None)
def rollout_inputs(n_atoms=28, members=2, boxed=False):
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    first = syn.box_frame(n_atoms, seed=3) if boxed else syn.chain_frame(n_atoms, seed=3)
    base = syn.jitter_window(first, W, seed=3)
    wins = torch.from_numpy(syn.ensemble_windows(base, members, sigma=0.1)).permute(1, 0, 2, 3).contiguous()   # [W,M,N,3]
    aa = torch.from_numpy(syn.amino_acids(n_atoms, seed=3))
    model = KernelNN(64, 128, 2, 6, 7, 3, 20, 4)
    model.load_state_dict(near_identity_state_dict(64, 128, seed=1, kernel_gain=1e-2, feature_gain=1e-1, kernel_to_coords=1.0))
    return wins, aa, model.eval().to("cuda:0")


def equality_constraints(wins, second=True):
    """Every chain (and (i, i + 2)) distance held at its mean over the window: any frame the model produces violates them."""
    from molecular_dynamics_neural_operator_amd.forecast import DistanceConstraints
    n = wins.shape[2]
    pairs = R.chain_pairs(n, second)
    x = wins.numpy().astype(np.float64).reshape(-1, n, 3)
    d = np.stack([R.lengths(f, pairs) for f in x]).mean(0)
    return DistanceConstraints.of(pairs, d, d, n_atoms=n)


def run_engine(dev, wins, aa, model, steps=STEPS, cls=None, max_steps=None, **kw):
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    eng = (cls or RolloutEngine)(model, wins.shape[1], wins.shape[2], W, 8.0, max_steps=max_steps or steps, device=dev, **kw)
    eng.reset(wins, aa)
    eng.step(steps)
    eng.synchronize()
    out = eng.frames().clone()
    rep = eng.constraint_report() if kw.get("constraints") is not None else None
    if rep is not None:
        rep = tuple(t.clone() for t in (rep.sweeps, rep.viol_in, rep.viol_out))
    eng.close()
    return out, rep


def composed(dev, wins, aa, model, cons, steps, use_graph, box=None, iterations=8, tol=0.0):
    """An unconstrained engine run ONE step from the window, forecast.project_constraints on its frame, the window slid by
    hand: what the constrained engine must equal."""
    from molecular_dynamics_neural_operator_amd.forecast import project_constraints
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    eng = RolloutEngine(model, wins.shape[1], wins.shape[2], W, 8.0, max_steps=1, device=dev, use_graph=use_graph, box=box)
    window = wins.to(dev).clone()
    frames, reps = [], []
    for _ in range(steps):
        eng.reset(window, aa)
        eng.step(1)
        eng.synchronize()
        p, rep = project_constraints(eng.frames().clone(), cons, box=box, iterations=iterations, tol=tol)
        frames.append(p[0])
        reps.append((rep.sweeps[0], rep.viol_in[0], rep.viol_out[0]))
        window = torch.cat([window[1:], p], 0)
    eng.close()
    return torch.stack(frames), tuple(torch.stack([r[k] for r in reps]) for k in range(3))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("use_graph", [True, False])
def test_constrained_rollout_is_the_step_by_step_composition(dev, use_graph):
    wins, aa, model = rollout_inputs()
    cons = equality_constraints(wins)
    want, want_rep = composed(dev, wins, aa, model, cons, STEPS, use_graph, iterations=4, tol=1e-4)
    got, rep = run_engine(dev, wins, aa, model, use_graph=use_graph, constraints=cons, constraint_iterations=4, constraint_tol=1e-4)
    assert same_bits(got, want)
    for g, w_ in zip(rep, want_rep):
        assert g.shape == (STEPS, 2) and same_bits(g, w_)
    assert bool((rep[0] > 0).all()) and bool((rep[2] < rep[1]).all())          # the constraints were at work in every step
    plain, _ = run_engine(dev, wins, aa, model, use_graph=use_graph)
    assert not torch.equal(plain, got) and bool(torch.isfinite(got).all())


def test_graph_replay_equals_plain_launches_at_eight_steps_per_launch(dev):
    wins, aa, model = rollout_inputs()
    cons = equality_constraints(wins)
    a, ra = run_engine(dev, wins, aa, model, steps=9, max_steps=16, use_graph=True, constraints=cons)
    b, rb = run_engine(dev, wins, aa, model, steps=9, max_steps=16, use_graph=False, constraints=cons)
    assert same_bits(a, b) and all(same_bits(u, v) for u, v in zip(ra, rb)) and bool((ra[0] > 0).all())


def test_projection_comes_after_the_noise(dev):
    from molecular_dynamics_neural_operator_amd.forecast import project_constraints
    wins, aa, model = rollout_inputs()
    cons = equality_constraints(wins)
    kw = dict(noise_sigma=0.05, noise_seed=0x5EED0123456789AB, member_ids=(11, 4))
    noisy, _ = run_engine(dev, wins, aa, model, steps=1, **kw)
    both, rep = run_engine(dev, wins, aa, model, steps=1, constraints=cons, **kw)
    want, want_rep = project_constraints(noisy, cons)
    assert same_bits(both, want) and same_bits(rep[0], want_rep.sweeps) and same_bits(rep[2], want_rep.viol_out)
    clean, _ = run_engine(dev, wins, aa, model, steps=1, constraints=cons)
    assert not torch.equal(clean, both)


@pytest.mark.parametrize("use_graph", [True, False])
def test_constraints_switched_off_before_the_first_step(dev, use_graph):
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    wins, aa, model = rollout_inputs()
    cons = equality_constraints(wins)
    plain, _ = run_engine(dev, wins, aa, model, use_graph=use_graph)
    eng = RolloutEngine(model, 2, 28, W, 8.0, max_steps=STEPS, device=dev, use_graph=use_graph, constraints=cons)
    eng.reset(wins, aa)
    eng.set_constraints(None)
    eng.step(STEPS)
    eng.synchronize()
    assert same_bits(eng.frames(), plain)
    with pytest.raises(MdnoError):
        eng.constraint_report()
    with pytest.raises(MdnoError, match="before the first step"):
        eng.set_constraints(cons)
    eng.reset(wins, aa)                                     # and switched on again: the constrained frames
    eng.set_constraints(cons)
    eng.step(STEPS)
    eng.synchronize()
    want, _ = run_engine(dev, wins, aa, model, use_graph=use_graph, constraints=cons)
    assert same_bits(eng.frames(), want) and not torch.equal(want, plain)
    eng.close()


def test_grouped_engine_equals_the_ungrouped(dev):
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine
    wins, aa, model = rollout_inputs()
    cons = equality_constraints(wins)
    one, rep1 = run_engine(dev, wins, aa, model, constraints=cons)
    two, rep2 = run_engine(dev, wins, aa, model, cls=GroupedRolloutEngine, groups=2, constraints=cons)
    assert same_bits(one, two) and all(same_bits(u, v) for u, v in zip(rep1, rep2))


def test_first_step_from_sample_is_projected_like_any_other(dev):
    """Step 0 on the sample's own edge list runs outside the plan: its frame is the projection of the unconstrained one, its
    report row is that projection's, and the plan's step 1 goes on from the projected frame."""
    from molecular_dynamics_neural_operator_amd.forecast import project_constraints
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    from oracle import graph_kernel_oracle as O
    wins, aa, model = rollout_inputs()
    cons = equality_constraints(wins)
    win = wins[:, 1].contiguous()
    s0 = O.construct_pairdata(win[:1].numpy(), aa, 8.0)                    # graph of the window's FIRST frame
    out = {}
    for name, c in (("plain", None), ("constrained", cons)):
        eng = RolloutEngine(model, 1, 28, W, 8.0, max_steps=2, device=dev, constraints=c)
        eng.reset(win, aa)
        eng.first_step_from_sample(s0["edge_index"], s0["edge_attr"])
        eng.step(1)
        eng.synchronize()
        out[name] = eng.frames().clone()
        if c is not None:
            rep = eng.constraint_report()
            rep = (rep.sweeps.clone(), rep.viol_in.clone(), rep.viol_out.clone())
        eng.close()
    want, want_rep = project_constraints(out["plain"][:1], cons)
    assert same_bits(out["constrained"][:1], want) and not torch.equal(want, out["plain"][:1])
    assert same_bits(rep[0][:1], want_rep.sweeps) and same_bits(rep[1][:1], want_rep.viol_in) and same_bits(rep[2][:1], want_rep.viol_out)
    cont, cont_rep = run_engine(dev, torch.cat([win[1:].to(dev), want[0]]).unsqueeze(1).cpu(), aa, model, steps=1, constraints=cons)
    assert same_bits(out["constrained"][1:], cont) and same_bits(rep[0][1:], cont_rep[0]) and bool((rep[0] > 0).all())


def test_box_stand_in_at_504_atoms(dev):
    """One member of 504 atoms (the uniform box stand-in) with the chain's equality constraints, 3 steps: the composition."""
    wins, aa, model = rollout_inputs(504, 1, True)
    cons = equality_constraints(wins, second=False)
    want, want_rep = composed(dev, wins, aa, model, cons, 3, True)
    got, rep = run_engine(dev, wins, aa, model, steps=3, constraints=cons)
    assert same_bits(got, want) and all(same_bits(u, v) for u, v in zip(rep, want_rep)) and bool((rep[0] == 8).all())


# ================================================================================================ 3. guard bands
COVERED = {"mdnocst_project", "mdnocst_rollout_plan_set_constraints"}


def _run_guarded(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    wins, aa, model = rollout_inputs()
    cons = equality_constraints(wins)
    res = []
    with Guard(fill, record_calls=False) as G:
        for n, f in ((1, 3), (2, 1), (28, 17), (65, 3), (257, 2)):      # rows of 3 N floats: tails, part-filled groups
            frames, table = noisy_frames(n, f, seed=n)
            x = G.place(torch.from_numpy(frames).to(dev))
            tab = [G.place(torch.from_numpy(t).to(dev)) for t in table[:4]]
            w = G.place(torch.linspace(0.0, 2.0, n, device=dev))
            out = ops.project_constraints(x, *tab, weights=w, iterations=3)          # out, sweeps, viol_in, viol_out: guarded
            res += [t.clone() for t in out]
            ops.project_constraints(x, *tab, weights=w, iterations=3, out=x)         # in place: the input's own bands
            res.append(x.clone())
        for use_graph in (True, False):
            eng = RolloutEngine(model, 2, 28, W, 8.0, max_steps=3, device=dev, use_graph=use_graph, constraints=cons)
            res.append(eng.run(wins, aa, 3).clone())                                 # traj, workspace, reports: all guarded
            rep = eng.constraint_report()
            res += [rep.sweeps.clone(), rep.viol_in.clone(), rep.viol_out.clone(), eng.traj[:W].clone()]
            eng.close()
        G.verify()
    return res


def test_constrain_entry_points_stay_inside_their_buffers(dev):
    """The two entry points of include/mdno_constrain.h inside guard bands under both fill bytes: every band intact, and every
    output bitwise equal under both fills (nothing unset is read, no value written twice)."""
    import re
    from pathlib import Path
    from guarded import FILLS
    text = re.sub(r"/\*.*?\*/", "", (Path(__file__).resolve().parents[1] / "include" / "mdno_constrain.h").read_text(), flags=re.S)
    writing = {m.group(1) for m in re.finditer(r"^int\s+(mdnocst_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S | re.M)
               if re.search(r"(?<!const )\b(?:float|double|int32_t)\s*\*", m.group(2))}
    assert writing == COVERED, writing ^ COVERED
    wins, _, _ = rollout_inputs()
    a, b = (_run_guarded(dev, fill) for fill in FILLS)
    assert len(a) == len(b) == 5 * 5 + 2 * 5
    for i, (u, v) in enumerate(zip(a, b)):
        assert same_bits(u, v), i
    assert same_bits(a[25], a[30]) and all(same_bits(a[26 + k], a[31 + k]) for k in range(3))    # graph replay = plain launches
    assert torch.equal(a[29], wins.to(dev))                                                      # the window is untouched
