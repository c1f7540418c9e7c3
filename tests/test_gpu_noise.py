"""Seeded Gaussian noise on the device (include/mdno_noise.h, csrc/philox.h, csrc/noise.hip):
the raw generator against the numpy restatement (tests/philox_ref.py), stochastic rollouts and their invariances,
noisy training windows, guard bands around the three entry points."""
import functools

import numpy as np
import pytest
import torch

import philox_ref as P

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB          # a 64-bit seed: both key words in use
IDS = (0, 5, 2 ** 31 - 1)


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ================================================================================================ 1. raw generator
@pytest.mark.parametrize("purpose", ["rollout", "train_window"])
@pytest.mark.parametrize("index", [0, 1, 2 ** 40])
@pytest.mark.parametrize("n_atoms", [1, 5, 70])
def test_raw_generator_against_the_restatement(dev, n_atoms, index, purpose):
    """Words bitwise; z within 1e-5 absolute of the fp64 restatement (|z| < 6 and three fp32 library calls of a few
    ulp each: ~1e-6); twice the same bits; sigma = 0 exact zeros.  3 N = 3, 15, 210 values: every tail of the 4-wide
    block (rows of 3 and 15 floats also put the second and third stream at unaligned addresses)."""
    from molecular_dynamics_neural_operator_amd import ops
    z, words = ops.noise_fill(SEED, IDS, index, n_atoms, purpose=purpose, sigma=1.0, device=dev, with_words=True)
    want = P.noise_words(SEED, IDS, index, 3 * n_atoms, {"rollout": 0, "train_window": 1}[purpose])
    assert z.shape == (3, 3 * n_atoms) and words.shape == (3, 3 * n_atoms, 2)
    assert np.array_equal(words.cpu().numpy().astype(np.uint32), want)
    err = float(np.abs(z.cpu().numpy().astype(np.float64) - P.normals(want)).max())
    print("max |z - fp64|", err)
    assert err < 1e-5
    z2, words2 = ops.noise_fill(SEED, IDS, index, n_atoms, purpose=purpose, sigma=1.0, device=dev, with_words=True)
    assert torch.equal(z, z2) and torch.equal(words, words2)
    assert torch.equal(ops.noise_fill(SEED, IDS, index, n_atoms, purpose=purpose, sigma=1.0, device=dev), z)   # no words
    half = ops.noise_fill(SEED, IDS, index, n_atoms, purpose=purpose, sigma=0.5, device=dev)
    assert torch.equal(half, z * 0.5)
    zero = ops.noise_fill(SEED, IDS, index, n_atoms, purpose=purpose, sigma=0.0, device=dev)
    assert torch.equal(zero, torch.zeros_like(zero))
    # a window of 2 frames is the same stream, twice as long
    two = ops.noise_fill(SEED, IDS, index, n_atoms, frames=2, purpose=purpose, device=dev)
    assert torch.equal(two[:, :3 * n_atoms], z)


def test_raw_generator_moments(dev):
    """3 x 70 x 3 values at each of 200 indices: mean within 5 standard errors of 0 (5 / sqrt(n)) and variance within
    5 of 1 (5 sqrt(2 / n)) — first for the CPU restatement at this seed, so that the reference alone passes."""
    from molecular_dynamics_neural_operator_amd import ops
    n = 3 * 210 * 200
    ref = np.stack([P.normals(P.noise_words(SEED, IDS, i, 210, 0)) for i in range(200)])
    got = torch.stack([ops.noise_fill(SEED, IDS, i, 70, device=dev) for i in range(200)]).cpu().numpy().astype(np.float64)
    for name, v in (("restatement", ref), ("device", got)):
        print(name, "mean", v.mean(), "var", v.var())
        assert v.size == n and abs(v.mean()) < 5.0 / np.sqrt(n), name
        assert abs(v.var() - 1.0) < 5.0 * np.sqrt(2.0 / n), name
    assert np.abs(got - ref).max() < 1e-5


# ================================================================================================ rollouts
N_ROLL, W, STEPS, SIGMA = 37, 3, 6, 0.05
MEMBERS = (11, 4, 2 ** 31 - 1, 0)          # global member ids, not in order


@functools.lru_cache(maxsize=None)
def rollout_inputs(n_atoms=N_ROLL, members=4, depth=2):
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    base = syn.jitter_window(syn.chain_frame(n_atoms, seed=3), W, seed=3)
    wins = torch.from_numpy(syn.ensemble_windows(base, members, sigma=0.1)).permute(1, 0, 2, 3).contiguous()   # [W,M,N,3]
    aa = torch.from_numpy(syn.amino_acids(n_atoms, seed=3))
    model = KernelNN(64, 128, depth, 6, 7, 3, 20, 4)
    model.load_state_dict(near_identity_state_dict(64, 128, seed=1, kernel_gain=1e-2, feature_gain=1e-1, kernel_to_coords=1.0))
    return wins, aa, model.eval().to("cuda:0")


def run_engine(dev, wins, aa, model, pieces=(STEPS,), cls=None, **kw):
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    cls = cls or RolloutEngine
    eng = cls(model, wins.shape[1], wins.shape[2], W, 8.0, max_steps=sum(pieces), device=dev, **kw)
    eng.reset(wins, aa)
    for n in pieces:
        eng.step(n)
    eng.synchronize()
    out = eng.frames().clone()
    eng.close()
    return out, eng


@pytest.mark.parametrize("use_graph", [True, False])
def test_rollout_sigma_zero_is_the_plain_rollout(dev, use_graph):
    wins, aa, model = rollout_inputs()
    plain, _ = run_engine(dev, wins, aa, model, use_graph=use_graph)
    zero, eng = run_engine(dev, wins, aa, model, use_graph=use_graph, noise_sigma=0.0, noise_seed=SEED, member_ids=MEMBERS)
    assert torch.equal(plain, zero) and eng._member_ids_dev is None
    assert bool(torch.isfinite(plain).all())


def test_rollout_first_step_is_clean_plus_the_generators_values(dev):
    """frames_noisy[0] = fl(frames_clean[0] + sigma * z), element by element, z from ops.noise_fill at step 0."""
    from molecular_dynamics_neural_operator_amd import ops
    wins, aa, model = rollout_inputs()
    clean, _ = run_engine(dev, wins, aa, model, pieces=(1,))
    noisy, _ = run_engine(dev, wins, aa, model, pieces=(1,), noise_sigma=SIGMA, noise_seed=SEED, member_ids=MEMBERS)
    sz = ops.noise_fill(SEED, MEMBERS, 0, N_ROLL, sigma=SIGMA, device=dev).view(4, N_ROLL, 3)
    assert float(sz.abs().max()) > 0.05 and not torch.equal(noisy, clean)
    assert torch.equal(noisy[0] - clean[0], (clean[0] + sz) - clean[0])
    assert torch.equal(noisy[0], clean[0] + sz)


@functools.lru_cache(maxsize=None)
def noisy_reference():
    """Variant a: one call of 6 steps, graph replay."""
    wins, aa, model = rollout_inputs()
    out, eng = run_engine(torch.device("cuda:0"), wins, aa, model, noise_sigma=SIGMA, noise_seed=SEED, member_ids=MEMBERS)
    return out, eng.edges_per_step.cpu().clone(), eng.steps_per_launch


def test_rollout_noise_enters_every_later_step(dev):
    """Step k's frame is NOT clean + noise of step k alone: the noisy frame is what the next window and graph read."""
    from molecular_dynamics_neural_operator_amd import ops
    wins, aa, model = rollout_inputs()
    ref, _, _ = noisy_reference()
    clean, _ = run_engine(dev, wins, aa, model)
    assert bool(torch.isfinite(ref).all())
    sz1 = ops.noise_fill(SEED, MEMBERS, 1, N_ROLL, sigma=SIGMA, device=dev).view(4, N_ROLL, 3)
    assert not torch.equal(ref[1], clean[1] + sz1)
    # the frame stored for step 0 is the one step 1 started from: a rollout continued from it reproduces step 1
    wins1 = torch.cat([wins[1:].to(dev), ref[0:1]])
    cont, _ = run_engine(dev, wins1, aa, model, pieces=(1,))
    assert torch.equal(cont[0] + sz1, ref[1])


@pytest.mark.parametrize("variant", ["split_1_2_3", "plain_launches", "members_alone", "two_groups", "regrown"])
def test_rollout_invariances(dev, variant):
    """6 steps, M = 4, N = 37, sigma = 0.05: bitwise the frames of one graph-replayed call of 6 steps."""
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine, RolloutEngine
    wins, aa, model = rollout_inputs()
    ref, eps, _ = noisy_reference()
    noise = dict(noise_sigma=SIGMA, noise_seed=SEED)
    if variant == "split_1_2_3":
        got, _ = run_engine(dev, wins, aa, model, pieces=(1, 2, 3), member_ids=MEMBERS, **noise)
    elif variant == "plain_launches":
        got, eng = run_engine(dev, wins, aa, model, use_graph=False, member_ids=MEMBERS, **noise)
    elif variant == "members_alone":
        got = torch.cat([run_engine(dev, wins[:, m:m + 1].contiguous(), aa, model, member_ids=[MEMBERS[m]], **noise)[0]
                         for m in range(4)], dim=1)
    elif variant == "two_groups":
        got, eng = run_engine(dev, wins, aa, model, cls=GroupedRolloutEngine, groups=2, member_ids=MEMBERS, **noise)
        assert [e.member_ids for e in eng.engines] == [list(MEMBERS[:2]), list(MEMBERS[2:])]
    else:
        # a capacity one edge short of the fullest step's graph, treated as a fitted one (the fit itself only applies
        # from N > 256 on): one growth, the steps from the first truncated one on run again and redraw the same noise
        cap0 = int(eps.max()) - 1
        eng = RolloutEngine(model, 4, N_ROLL, W, 8.0, max_steps=STEPS, edge_cap=cap0, device=dev, member_ids=MEMBERS, **noise)
        eng.reset(wins, aa)
        eng._fit_cap = True
        eng.step(STEPS)
        eng.synchronize()
        print("regrown", eng.regrown, "edges per step", eps.tolist())
        assert len(eng.regrown) == 1 and eng.regrown[0][1] == cap0 and eng.edge_cap == min(4 * N_ROLL * N_ROLL, 4 * cap0)
        assert eng.edges_per_step.cpu().tolist() == eps.tolist()
        got = eng.frames().clone()
        eng.close()
    assert got.shape == ref.shape == (STEPS, 4, N_ROLL, 3)
    assert torch.equal(got, ref)


def test_rollout_seed_and_member_ids_matter(dev):
    from molecular_dynamics_neural_operator_amd import ops
    wins, aa, model = rollout_inputs()
    ref, _, _ = noisy_reference()
    other_seed, _ = run_engine(dev, wins, aa, model, noise_sigma=SIGMA, noise_seed=SEED + 1, member_ids=MEMBERS)
    permuted, _ = run_engine(dev, wins, aa, model, noise_sigma=SIGMA, noise_seed=SEED, member_ids=MEMBERS[::-1])
    default_ids, _ = run_engine(dev, wins, aa, model, noise_sigma=SIGMA, noise_seed=SEED)
    for m in range(4):
        assert not torch.equal(other_seed[:, m], ref[:, m]) and not torch.equal(permuted[:, m], ref[:, m])
    # default ids are 0 .. M-1: its member 0 and the reference's member 3 (global id 0) draw the same values
    clean, _ = run_engine(dev, wins, aa, model, pieces=(1,))
    sz0 = ops.noise_fill(SEED, [0], 0, N_ROLL, sigma=SIGMA, device=dev).view(N_ROLL, 3)
    assert torch.equal(default_ids[0, 0], clean[0, 0] + sz0) and torch.equal(ref[0, 3], clean[0, 3] + sz0)


def test_first_step_from_sample_gets_the_noise_of_step_zero(dev):
    """Step 0 on the sample's own edge list runs outside the plan: its frame is the clean one plus the generator's
    step-0 values, and the plan's steps go on from the noisy frame with the noise of steps 1, 2."""
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    from oracle import graph_kernel_oracle as O
    wins, aa, model = rollout_inputs()
    win = wins[:, 2].contiguous()
    s0 = O.construct_pairdata(win[:1].numpy(), aa, 8.0)                    # graph of the window's FIRST frame
    out = {}
    for sigma in (0.0, SIGMA):
        eng = RolloutEngine(model, 1, N_ROLL, W, 8.0, max_steps=3, device=dev, noise_sigma=sigma, noise_seed=SEED,
                            member_ids=[MEMBERS[2]])
        eng.reset(win, aa)
        eng.first_step_from_sample(s0["edge_index"], s0["edge_attr"])
        eng.step(2)
        eng.synchronize()
        out[sigma] = eng.frames().clone()
        eng.close()
    sz = [ops.noise_fill(SEED, [MEMBERS[2]], k, N_ROLL, sigma=SIGMA, device=dev).view(N_ROLL, 3) for k in range(3)]
    assert torch.equal(out[SIGMA][0, 0], out[0.0][0, 0] + sz[0]) and float(sz[0].abs().max()) > 0
    cont, _ = run_engine(dev, torch.cat([win[1:].to(dev), out[SIGMA][0]]).unsqueeze(1), aa, model, pieces=(1,))
    assert torch.equal(out[SIGMA][1, 0], cont[0, 0] + sz[1]) and not torch.equal(out[SIGMA][1], out[0.0][1])


def test_unknown_purpose_is_an_mdno_error(dev):
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    for bad in ("training", 256, -1, 1.5):
        with pytest.raises(MdnoError, match="purpose"):
            ops.noise_fill(SEED, IDS, 0, 5, purpose=bad, device=dev)
    assert torch.equal(ops.noise_fill(SEED, IDS, 0, 5, purpose=1, device=dev),
                       ops.noise_fill(SEED, IDS, 0, 5, purpose="train_window", device=dev))


def test_rollout_eight_steps_per_launch(dev):
    """A short chain (M N <= 128 rows) replays 8 steps per graph launch: 9 steps (8 + 1) = 9 plain launches = 4 + 5."""
    wins, aa, model = rollout_inputs(28, 2, 1)
    noise = dict(noise_sigma=SIGMA, noise_seed=SEED, member_ids=(7, 1))
    a, eng = run_engine(dev, wins, aa, model, pieces=(9,), **noise)
    b, _ = run_engine(dev, wins, aa, model, pieces=(9,), use_graph=False, **noise)
    c, _ = run_engine(dev, wins, aa, model, pieces=(4, 5), **noise)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and torch.equal(a, c)


def test_engine_arguments_are_checked(dev):
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    wins, aa, model = rollout_inputs()
    for bad in (dict(noise_sigma=-1.0), dict(noise_sigma=float("nan")), dict(member_ids=[0, 1, 2]), dict(member_ids=[0, 1, 2, -1]),
                dict(noise_seed=2 ** 64)):
        with pytest.raises(MdnoError):
            RolloutEngine(model, 4, N_ROLL, W, 8.0, max_steps=2, device=dev, **bad)


# ================================================================================================ training windows
N_TRAIN = 20


@functools.lru_cache(maxsize=None)
def device_trajectory():
    import tempfile
    from pathlib import Path
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.dataset import ContactMapDataset, write_trajectory_npz
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory
    traj = syn.ou_trajectory(syn.chain_frame(N_TRAIN, seed=5), 16, sigma=0.15, theta=0.2, seed=2)
    with tempfile.TemporaryDirectory() as d:
        path = Path(d) / "chain.npz"
        write_trajectory_npz(path, traj, [syn.contact_map(f, 8.0) for f in traj], syn.amino_acids(N_TRAIN, seed=0))
        dset = ContactMapDataset(str(path), window_size=W, horizon=1)
        return DeviceTrajectory(dset, torch.device("cuda:0"))


def test_noisy_windows_touch_x_position_only(dev):
    from molecular_dynamics_neural_operator_amd import ops
    dtraj = device_trajectory()
    assert len(dtraj) >= 10
    idx, s = [3, 7, 9], 0.02
    clean = dtraj.batch(idx)
    noisy = dtraj.batch(idx, noise_std=s, noise_seed=SEED, epoch=4)
    for k in ("y", "edge_attr", "edge_index", "x_aminoacid"):
        assert torch.equal(getattr(clean, k), getattr(noisy, k)), k
    sz = ops.noise_fill(SEED, idx, 4, N_TRAIN, frames=W, purpose="train_window", sigma=s, device=dev)      # [B, W*N*3]
    sz = sz.view(3, W, N_TRAIN, 3).permute(1, 0, 2, 3).reshape(W, 3 * N_TRAIN, 3)
    assert float(sz.abs().max()) > s and noisy.x_position.shape == clean.x_position.shape
    assert torch.equal(noisy.x_position - clean.x_position, (clean.x_position + sz) - clean.x_position)
    assert torch.equal(noisy.x_position, clean.x_position + sz)
    # noise_std = 0 is batch(idx); the epoch and the seed change the noise
    zero = dtraj.batch(idx, noise_std=0.0, noise_seed=SEED, epoch=4)
    assert all(torch.equal(getattr(clean, k), getattr(zero, k)) for k in clean._FIELDS)
    assert not torch.equal(dtraj.batch(idx, noise_std=s, noise_seed=SEED, epoch=5).x_position, noisy.x_position)
    assert not torch.equal(dtraj.batch(idx, noise_std=s, noise_seed=SEED + 1, epoch=4).x_position, noisy.x_position)
    assert torch.equal(dtraj.batch(idx, noise_std=s, noise_seed=SEED, epoch=4).x_position, noisy.x_position)


def test_a_samples_noise_does_not_depend_on_its_batch(dev):
    dtraj = device_trajectory()
    kw = dict(noise_std=0.02, noise_seed=SEED, epoch=1)
    alone = dtraj.batch([7], **kw).x_position
    assert torch.equal(dtraj.batch([3, 7, 9], **kw).x_position[:, N_TRAIN:2 * N_TRAIN], alone)
    assert torch.equal(dtraj.batch([9, 7], **kw).x_position[:, N_TRAIN:], alone)
    assert not torch.equal(dtraj.batch([9, 7], **kw).x_position[:, :N_TRAIN], alone)


def _train_once(dev, noise_std):
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN, LpLoss
    from molecular_dynamics_neural_operator_amd.training import Adam, train_epoch
    dtraj = device_trajectory()
    torch.manual_seed(3)
    model = KernelNN(64, 128, 1, 6, 7, 3, 20, 4)
    with torch.no_grad():
        for p_ in model.conv1.net.layers[4].parameters():
            p_.mul_(0.2)
    model = model.to(dev)
    before = {n: p_.detach().clone() for n, p_ in model.named_parameters()}
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=0.0)
    batches = [dtraj.batch(range(0, 4)), dtraj.batch(range(4, 8))]
    clean_x = [b.x_position.clone() for b in batches]
    loss, _ = train_epoch(model, batches, opt, LpLoss(size_average=False), noise_std=noise_std, noise_seed=SEED, epoch=2)
    assert all(torch.equal(b.x_position, x) for b, x in zip(batches, clean_x))          # the caller's batches stay clean
    grads = {n: p_.grad.detach().clone() for n, p_ in model.named_parameters()}
    after = {n: p_.detach().clone() for n, p_ in model.named_parameters()}
    return loss, before, grads, after


def test_train_epoch_on_noisy_windows(dev):
    loss, before, grads, after = _train_once(dev, 0.02)
    assert np.isfinite(loss)
    for n in before:
        assert bool(torch.isfinite(grads[n]).all()), n
        assert not torch.equal(before[n], after[n]), n
    loss2, _, grads2, after2 = _train_once(dev, 0.02)
    assert loss == loss2
    for n in before:
        assert torch.equal(grads[n], grads2[n]) and torch.equal(after[n], after2[n]), n
    loss0, _, _, after0 = _train_once(dev, 0.0)
    assert loss0 != loss and any(not torch.equal(after0[n], after[n]) for n in after)


def test_host_collated_batches_are_refused(dev):
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    from molecular_dynamics_neural_operator_amd.training import add_window_noise
    b = device_trajectory().batch([0, 1])
    bare = PairData(b.x_aminoacid, b.x_position, b.y, b.edge_attr, b.edge_index)
    with pytest.raises(MdnoError, match="DeviceTrajectory"):
        add_window_noise(bare, 0.02)


# ================================================================================================ 6. guard bands
COVERED = {"mdno_noise_fill", "mdno_noise_add_window", "mdno_rollout_plan_set_noise"}


def _run_guarded(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    wins, aa, model = rollout_inputs()
    dtraj = device_trajectory()
    with Guard(fill, record_calls=False) as G:
        res = []
        for n_atoms in (1, 5, 70):                       # 3, 15, 210 floats per stream: tails and unaligned rows
            z, words = ops.noise_fill(SEED, IDS, 2 ** 40, n_atoms, sigma=1.0, device=dev, with_words=True)
            res += [z.clone(), words.clone()]
        noisy = dtraj.batch([9, 0, 7], noise_std=0.02, noise_seed=SEED, epoch=3)          # rows of 60 floats per frame
        res.append(noisy.x_position.clone())
        for use_graph in (True, False):
            eng = RolloutEngine(model, 4, N_ROLL, W, 8.0, max_steps=3, device=dev, use_graph=use_graph, noise_sigma=SIGMA,
                                noise_seed=SEED, member_ids=MEMBERS)          # traj, workspace, counters: all guarded
            res.append(eng.run(wins, aa, 3).clone())
            res.append(eng.traj[:W].clone())
            eng.close()
        G.verify()
    return res


def test_noise_entry_points_stay_inside_their_buffers(dev):
    """The three entry points of include/mdno_noise.h inside guard bands under both fill bytes: every band intact, and
    every output bitwise equal under both fills (nothing unset is read, no value written twice)."""
    from pathlib import Path
    from guarded import FILLS, header_functions, writes_memory
    header = Path(__file__).resolve().parents[1] / "include" / "mdno_noise.h"
    writing = {n for n, params in header_functions(header).items() if writes_memory(params)}
    assert writing == COVERED, writing ^ COVERED
    wins, _, _ = rollout_inputs()
    a, b = (_run_guarded(dev, fill) for fill in FILLS)
    assert len(a) == len(b) == 11
    for i, (u, v) in enumerate(zip(a, b)):
        assert not torch.isnan(u.float()).any() and torch.equal(u, v), i
    assert torch.equal(a[7], a[9]) and torch.equal(a[8], wins.to(dev))          # graph replay = plain launches; window untouched
