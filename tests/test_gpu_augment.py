"""Random rigid motions of training samples on the device (include/mdno_augment.h, csrc/rigid_rule.h, csrc/augment.hip;
DESIGN.md section 4.23) against the numpy restatement (tests/rigid_ref.py), bit for bit: the motions, apply and inverse,
augmented batches and what they do to training, the equivariance score, guard bands around the three entry points.

Bitwise comparisons treat NaN as NaN: where the rule makes a NaN (a non-finite input) both sides must have one in the
same place, every other element must agree in every bit (the sign and payload of a NaN are not part of the rule)."""
import functools

import numpy as np
import pytest
import torch

import philox_ref as P
import rigid_ref as RR

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB          # a 64-bit seed: both key words in use
BIG_EPOCH = 2 ** 40 + 5


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def same_bits(got, want):
    """got (tensor or array) and want (array) of one dtype: NaN exactly where want has NaN, equal bits elsewhere."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    nan = np.isnan(want)
    view = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(view)[~nan], want.view(view)[~nan])


def same_motions(got, want):
    return all(same_bits(g, want[k]) for g, k in zip(got, ("quaternion", "pivot", "shift", "attempts")))


def sample_ids(B):
    ids = (np.arange(B, dtype=np.int64) * 7 + 3) % 1000
    ids[-1] = 2 ** 31 - 1
    return ids


def frames_of(B, N, F=1, seed=0, scale=10.0, offset=(30.0, -12.0, 5.0)):
    rng = np.random.default_rng(1000 * N + B + seed)
    return (rng.standard_normal((F, B * N, 3)) * scale + np.asarray(offset)).astype(np.float32)


# ================================================================================================ 1. motions
@pytest.mark.parametrize("N", [1, 2, 3, 28, 63, 64, 65, 257, 1025])
def test_motions_against_the_restatement(dev, N):
    """quaternion, pivot, shift, attempts of B = 1, 3, 64 samples, epochs 0 and 2^40 + 5, rotation on and off, translate
    0 and 2.5, both pivots: every bit.  N covers the centroid order: fewer rows than lanes, exactly 64, one more, many
    rounds with a tail."""
    from molecular_dynamics_neural_operator_amd import ops
    for B in (1, 3, 64):
        ids = sample_ids(B)
        frame = frames_of(B, N)[0]
        frame_d = torch.from_numpy(frame).to(dev)
        for epoch in (0, BIG_EPOCH):
            for rotate in (True, False):
                for translate in (0.0, 2.5):
                    for pivot in ("centroid", "origin"):
                        kw = dict(rotate=rotate, translate=translate)
                        got = ops.rigid_motions(SEED, ids, epoch, device=dev, n_atoms=N,
                                                first_frame=frame_d if pivot == "centroid" else None, **kw)
                        want = RR.motions(SEED, ids, epoch, n_atoms=N, first_frame=frame if pivot == "centroid" else None, **kw)
                        assert same_motions(got, want), (B, epoch, rotate, translate, pivot)
                        if not rotate:
                            assert (got[3] == -1).all() and (got[0] == torch.tensor([1.0, 0, 0, 0], device=dev, dtype=torch.float64)).all()
                        if translate == 0.0:
                            assert (got[2] == 0).all()
                        if pivot == "origin":
                            assert (got[1] == 0).all()
    # twice the same bits; a tensor of ids is the list
    a = ops.rigid_motions(SEED, ids, 3, translate=1.0, first_frame=frame_d, n_atoms=N)
    b = ops.rigid_motions(SEED, torch.from_numpy(ids), 3, translate=1.0, first_frame=frame_d, n_atoms=N)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_short_rejection_loop_falls_back_on_the_restatements_samples(dev):
    """last_element = 3 at seed 2024, epoch 0, samples 0..63: the identity on exactly the samples the restatement says,
    attempts -1 for what was not found; 65 never falls back."""
    from molecular_dynamics_neural_operator_amd import ops
    ids = np.arange(64)
    full, short = RR.motions(2024, ids, 0), RR.motions(2024, ids, 0, last_element=3)
    fell = short["attempts"][:, 1] < 0
    assert fell.any() and not fell.all() and (full["attempts"] >= 2).all()
    got = ops.rigid_motions(2024, ids, 0, last_element=3, device=dev)
    assert same_motions(got, short)
    assert np.array_equal((got[3][:, 1] < 0).cpu().numpy(), fell)
    assert (got[0][torch.from_numpy(fell).to(dev)] == torch.tensor([1.0, 0, 0, 0], device=dev, dtype=torch.float64)).all()
    assert same_motions(ops.rigid_motions(2024, ids, 0, device=dev), full)
    for last in (2, 4, 7, 64):
        assert same_motions(ops.rigid_motions(2024, ids, 0, last_element=last, device=dev), RR.motions(2024, ids, 0, last_element=last))


def test_the_words_of_the_third_purpose(dev):
    """The raw generator, as it is, at purpose 2: N = 22, one frame = 66 elements, the restatement's words."""
    from molecular_dynamics_neural_operator_amd import ops
    ids = sample_ids(3)
    for epoch in (0, BIG_EPOCH):
        _, words = ops.noise_fill(SEED, ids, epoch, 22, frames=1, purpose=2, device=dev, with_words=True)
        want = P.noise_words(SEED, ids, epoch, 66, RR.TRAIN_MOTION)
        assert words.shape == (3, 66, 2) and np.array_equal(words.cpu().numpy().astype(np.uint32), want)
        _, named = ops.noise_fill(SEED, ids, epoch, 22, purpose="train_motion", device=dev, with_words=True)
        assert torch.equal(named, words)
        _, other = ops.noise_fill(SEED, ids, epoch, 22, purpose="train_window", device=dev, with_words=True)
        assert not torch.equal(other, words)


# ================================================================================================ 2. apply, inverse
def _apply_case(name):
    """(frames f32 [F, B*N, 3] per F in (1, 10), B, N) of one named case."""
    if name == "single_atom":
        B, N = 3, 1
        make = lambda F: frames_of(B, N, F)
    elif name == "nan_atom":
        B, N = 3, 28

        def make(F):
            x = frames_of(B, N, F)
            x[0, N + 5, 1] = np.nan                       # sample 1, first frame: reaches its centroid
            x[-1, 2 * N + 7, 2] = np.nan                  # sample 2, last frame (for F = 1 also the first)
            return x
    elif name == "inf_atom":
        B, N = 3, 28

        def make(F):
            x = frames_of(B, N, F)
            x[0, 3, 0] = np.inf                           # sample 0
            x[-1, 2 * N + 1, 1] = -np.inf
            return x
    elif name == "far":
        B, N = 2, 65
        make = lambda F: frames_of(B, N, F, offset=(1000.0, -990.0, 1003.5))
    else:
        B, N = 5, 257
        make = lambda F: frames_of(B, N, F)
    return make, B, N


@pytest.mark.parametrize("pivot", ["centroid", "origin"])
@pytest.mark.parametrize("case", ["single_atom", "nan_atom", "inf_atom", "far", "plain"])
def test_apply_and_inverse_against_the_restatement(dev, case, pivot):
    from molecular_dynamics_neural_operator_amd import ops
    make, B, N = _apply_case(case)
    ids = sample_ids(B)
    for F in (1, 10):
        x = make(F)
        first = x[0] if pivot == "centroid" else None
        want_m = RR.motions(SEED, ids, 7, translate=2.5, first_frame=first, n_atoms=N)
        q, c, t, att = ops.rigid_motions(SEED, ids, 7, translate=2.5, n_atoms=N, device=dev,
                                         first_frame=None if first is None else torch.from_numpy(first).to(dev))
        assert same_motions((q, c, t, att), want_m), F
        x_d = torch.from_numpy(x).to(dev)
        moved = ops.rigid_apply(q, c, t, N, x_d)
        want = RR.apply(want_m, x, N)
        assert same_bits(moved, want), F
        assert same_bits(x_d, x)                                           # out of place: the input stays
        back = ops.rigid_apply(q, c, t, N, moved, inverse=True)
        want_back = RR.apply(want_m, want, N, inverse=True)
        assert same_bits(back, want_back), F
        # in place, both directions
        y_d = x_d.clone()
        assert ops.rigid_apply(q, c, t, N, y_d, out=y_d) is y_d and same_bits(y_d, want), F
        ops.rigid_apply(q, c, t, N, y_d, inverse=True, out=y_d)
        assert same_bits(y_d, want_back), F
        # a single frame without the leading dimension
        assert same_bits(ops.rigid_apply(q, c, t, N, x_d[0]), want[0])
        finite = np.isfinite(x).all(axis=(0, 2)).reshape(B, N)
        if case == "single_atom" and pivot == "centroid":                 # d = 0: p' = (float)(c + t)
            assert same_bits(moved[0], (want_m["pivot"] + want_m["shift"]).astype(np.float32))
        if case in ("nan_atom", "inf_atom"):
            bad = ~np.isfinite(want).all(axis=(0, 2)).reshape(B, N)
            if pivot == "origin":                                         # a non-finite coordinate stays on its own atom
                assert np.array_equal(bad, ~finite), F
            else:                                                         # through the centroid: every row of the sample
                hit = ~np.isfinite(x[0]).all(axis=1).reshape(B, N).all(axis=1)
                assert hit.any() and not hit.all()
                assert bad[hit].all() and np.array_equal(bad[~hit], ~finite[~hit]), F
        if case in ("far", "plain"):                                      # the round trip is the input within the two
            err = np.abs(back.cpu().numpy().astype(np.float64) - x).max()      # fp32 roundings of |p| <= ~1100 A
            print(case, pivot, F, "round trip max |error|", err)
            assert err <= 2 * 2.0 ** -24 * 2048


@pytest.mark.parametrize("pivot", ["centroid", "origin"])
def test_no_rotation_no_translation_returns_the_input_bits(dev, pivot):
    from molecular_dynamics_neural_operator_amd import ops
    B, N = 3, 65
    x = frames_of(B, N, 10)
    x_d = torch.from_numpy(x).to(dev)
    q, c, t, att = ops.rigid_motions(SEED, sample_ids(B), 1, rotate=False, translate=0.0, n_atoms=N, device=dev,
                                     first_frame=x_d[0] if pivot == "centroid" else None)
    assert torch.equal(ops.rigid_apply(q, c, t, N, x_d), x_d)
    assert torch.equal(ops.rigid_apply(q, c, t, N, x_d, inverse=True), x_d)


# ================================================================================================ batches
N_TRAIN, W_TRAIN = 28, 10


@functools.lru_cache(maxsize=None)
def device_trajectory():
    import tempfile
    from pathlib import Path
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.dataset import ContactMapDataset, write_trajectory_npz
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory
    traj = syn.ou_trajectory(syn.chain_frame(N_TRAIN, seed=5), 30, sigma=0.15, theta=0.2, seed=2)
    with tempfile.TemporaryDirectory() as d:
        path = Path(d) / "chain.npz"
        write_trajectory_npz(path, traj, [syn.contact_map(f, 8.0) for f in traj], syn.amino_acids(N_TRAIN, seed=0))
        dset = ContactMapDataset(str(path), window_size=W_TRAIN, horizon=1)
        return DeviceTrajectory(dset, torch.device("cuda:0"))


def small_model(dev, seed=3):
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    torch.manual_seed(seed)
    model = KernelNN(64, 128, 1, 6, 7, 3, 20, 4)
    with torch.no_grad():
        for p_ in model.conv1.net.layers[4].parameters():
            p_.mul_(0.2)
    return model.to(dev)


def batches_equal(a, b):
    for k in ("x_position", "y", "y_unroll", "edge_attr", "edge_index", "x_aminoacid"):
        if not torch.equal(getattr(a, k), getattr(b, k)):
            return False
    return a.num_graphs == b.num_graphs and np.array_equal(a.sample_ids, b.sample_ids) and a.rows_per_sample == b.rows_per_sample


@pytest.mark.parametrize("unroll", [1, 3])
@pytest.mark.parametrize("B", [1, 5])
def test_augment_batch_moves_everything_a_sample_has(dev, B, unroll):
    from molecular_dynamics_neural_operator_amd.training import RigidAugment, augment_batch
    dtraj = device_trajectory()
    idx = [11, 0, 7, 3, 12][:B]
    aug = RigidAugment(seed=SEED, translate=1.5)
    clean = dtraj.batch(idx, unroll=unroll)
    kept = {k: getattr(clean, k).clone() for k in ("x_position", "y", "y_unroll", "edge_attr", "edge_index", "x_aminoacid")}
    out = augment_batch(clean, aug, 4)
    m = out.motions
    assert all(torch.equal(getattr(clean, k), v) for k, v in kept.items())            # the caller's batch is untouched
    assert len(m) == B and m.n_atoms == N_TRAIN and out.num_graphs == B and out.rows_per_sample == N_TRAIN
    assert np.array_equal(out.sample_ids, np.asarray(idx))
    want_m = RR.motions(SEED, idx, 4, translate=1.5, first_frame=kept["x_position"][0].cpu().numpy(), n_atoms=N_TRAIN)
    assert same_motions((m.quaternion, m.pivot, m.shift, m.attempts), want_m)
    assert torch.equal(out.x_position, m.apply(clean.x_position)) and not torch.equal(out.x_position, clean.x_position)
    assert torch.equal(out.y, m.apply(clean.y)) and torch.equal(out.y_unroll, m.apply(clean.y_unroll))
    assert out.y_unroll.shape == (unroll, B * N_TRAIN, 3) and torch.equal(out.y_unroll[0], out.y)
    assert same_bits(out.x_position, RR.apply(want_m, kept["x_position"].cpu().numpy(), N_TRAIN))
    ei = out.edge_index
    assert torch.equal(ei, clean.edge_index) and torch.equal(out.x_aminoacid, clean.x_aminoacid) and ei.shape[1] > 0
    assert torch.equal(out.edge_attr[:, :3], out.x_position[0][ei[0]]) and torch.equal(out.edge_attr[:, 3:], out.x_position[0][ei[1]])
    assert torch.equal(clean.edge_attr[:, :3], clean.x_position[0][ei[0]])            # (what the gather restates)
    # the batch that asks for it = the batch augmented afterwards
    direct = dtraj.batch(idx, unroll=unroll, augment=aug, epoch=4)
    assert batches_equal(direct, out) and torch.equal(direct.motions.quaternion, m.quaternion)
    # the moved sample is rigid: pair distances of the first frame are the clean ones within fp32 rounding of ~50 A
    d0 = torch.cdist(clean.x_position[0, :N_TRAIN].double(), clean.x_position[0, :N_TRAIN].double())
    d1 = torch.cdist(out.x_position[0, :N_TRAIN].double(), out.x_position[0, :N_TRAIN].double())
    assert float((d0 - d1).abs().max()) < 1e-4


def test_a_samples_motion_does_not_depend_on_its_batch(dev):
    from molecular_dynamics_neural_operator_amd.training import RigidAugment
    dtraj = device_trajectory()
    aug = RigidAugment(seed=SEED, translate=0.5)
    N = N_TRAIN
    big = dtraj.batch([2, 9, 5, 0, 13, 7], augment=aug, epoch=2)
    small = dtraj.batch([7, 5], augment=aug, epoch=2)
    alone = dtraj.batch([5], augment=aug, epoch=2)
    rows = lambda b, k: b.x_position[:, k * N:(k + 1) * N]
    assert torch.equal(rows(big, 2), rows(small, 1)) and torch.equal(rows(big, 2), rows(alone, 0))
    assert torch.equal(rows(big, 5), rows(small, 0))
    assert torch.equal(big.y[2 * N:3 * N], alone.y) and torch.equal(big.motions.quaternion[2], alone.motions.quaternion[0])
    for other in (dtraj.batch([5], augment=aug, epoch=3), dtraj.batch([5], augment=RigidAugment(seed=SEED + 1, translate=0.5), epoch=2)):
        assert not torch.equal(other.x_position, alone.x_position)
        assert not torch.equal(other.motions.quaternion, alone.motions.quaternion)
        assert not torch.equal(other.motions.shift, alone.motions.shift)
    assert not torch.equal(rows(big, 0), rows(dtraj.batch([2]), 0))


def test_noise_is_added_after_the_motion_with_its_own_values(dev):
    from molecular_dynamics_neural_operator_amd.training import RigidAugment, add_window_noise
    dtraj = device_trajectory()
    aug = RigidAugment(seed=SEED, translate=0.5)
    idx = [4, 1, 9]
    moved = dtraj.batch(idx, augment=aug, epoch=6)
    both = dtraj.batch(idx, noise_std=0.02, noise_seed=SEED, epoch=6, augment=aug)
    assert torch.equal(both.x_position, add_window_noise(moved, 0.02, SEED, 6))
    assert torch.equal(both.y, moved.y) and torch.equal(both.edge_attr, moved.edge_attr)
    # the noise values are the ones the clean batch gets: keyed as before
    clean = dtraj.batch(idx)
    noisy = dtraj.batch(idx, noise_std=0.02, noise_seed=SEED, epoch=6)
    z_clean, z_moved = noisy.x_position - clean.x_position, both.x_position - moved.x_position
    # each difference carries the one fp32 rounding of its sum: half an ulp <= 2^-23 max|x| each, two of them
    tol = 2.0 ** -22 * float(torch.maximum(noisy.x_position.abs().max(), both.x_position.abs().max()))
    print("max |z_clean - z_moved|", float((z_clean - z_moved).abs().max()), "bound", tol)
    assert float((z_clean - z_moved).abs().max()) <= tol and float(z_clean.abs().max()) > 0.02


def _train(dev, batches, **kw):
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import Adam, train_epoch
    model = small_model(dev)
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=0.0)
    loss = train_epoch(model, batches, opt, LpLoss(size_average=False), **kw)
    return loss, {n: p_.detach().clone() for n, p_ in model.named_parameters()}


def test_train_epoch_augments_as_augment_batch_does(dev):
    """Two steps: parameters bit-equal to training on batches augmented beforehand; augment=None is the call without the
    argument; the caller's batches stay as they are; periodic batches and host-collated lists are refused."""
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.training import RigidAugment, augment_batch
    dtraj = device_trajectory()
    aug = RigidAugment(seed=SEED, translate=1.0)
    batches = [dtraj.batch(range(0, 4)), dtraj.batch(range(4, 8))]
    kept = [b.x_position.clone() for b in batches]
    loss_a, after_a = _train(dev, batches, augment=aug, epoch=2)
    assert all(torch.equal(b.x_position, x) for b, x in zip(batches, kept))
    loss_b, after_b = _train(dev, [augment_batch(b, aug, 2) for b in batches])
    assert loss_a == loss_b and np.isfinite(loss_a[0])
    assert all(torch.equal(after_a[n], after_b[n]) for n in after_a)
    loss_0, after_0 = _train(dev, batches)
    loss_n, after_n = _train(dev, batches, augment=None)
    assert loss_0 == loss_n and all(torch.equal(after_0[n], after_n[n]) for n in after_0)
    assert loss_0 != loss_a and any(not torch.equal(after_0[n], after_a[n]) for n in after_0)
    # with unrolled steps and noise
    unrolled = [dtraj.batch(range(0, 4), unroll=2)]
    loss_u, after_u = _train(dev, unrolled, augment=aug, epoch=2, unroll=2, noise_std=0.01, noise_seed=SEED)
    loss_v, after_v = _train(dev, [augment_batch(unrolled[0], aug, 2)], epoch=2, unroll=2, noise_std=0.01, noise_seed=SEED)
    assert loss_u == loss_v and all(torch.equal(after_u[n], after_v[n]) for n in after_u)
    with pytest.raises(MdnoError, match="DeviceTrajectory.batch"):
        _train(dev, [[dtraj.batch([0])]], augment=aug)                    # a list of samples: host-collated
    with pytest.raises(MdnoError, match="RigidAugment"):
        _train(dev, batches, augment=True)


def test_periodic_batches_refuse_augmentation(dev):
    import tempfile
    from pathlib import Path
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.dataset import ContactMapDataset, write_trajectory_npz
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory, RigidAugment, augment_batch
    traj = syn.ou_trajectory(syn.chain_frame(12, seed=5), 8, sigma=0.15, theta=0.2, seed=2)
    with tempfile.TemporaryDirectory() as d:
        path = Path(d) / "chain.npz"
        write_trajectory_npz(path, traj, [syn.contact_map(f, 8.0) for f in traj], syn.amino_acids(12, seed=0))
        dset = ContactMapDataset(str(path), window_size=3, horizon=1)
        periodic = DeviceTrajectory(dset, dev, box=(40.0, 40.0, 40.0), cutoff=8.0)
    aug = RigidAugment(seed=1)
    with pytest.raises(MdnoError, match="periodic"):
        periodic.batch([0, 1], augment=aug)
    plain = periodic.batch([0, 1])
    with pytest.raises(MdnoError, match="periodic"):
        augment_batch(plain, aug, 0)
    with pytest.raises(MdnoError, match="periodic"):
        _train(dev, [plain], augment=aug)


# ================================================================================================ equivariance score
def test_equivariance_error(dev):
    """Identity motions: exactly 0.  Seeded motions: the score composed by hand — two inference forwards, the moved batch
    put together from motions.apply and torch indexing, the reduction in numpy fp64 — within 1e-12 relative (the order
    of an fp64 sum of 3 N = 84 squares: 84 x 2^-53 ~ 1e-14)."""
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    from molecular_dynamics_neural_operator_amd.training import (EquivarianceError, RigidAugment, RigidMotions, draw_motions,
                                                                 equivariance_error)
    dtraj = device_trajectory()
    model = small_model(dev).train()
    batch = dtraj.batch([3, 10, 6])
    B, N = 3, N_TRAIN
    zero = equivariance_error(model, batch, RigidMotions.identity(B, N, dev))
    assert isinstance(zero, EquivarianceError) and zero.rms.dtype == torch.float64 and zero.rms.shape == (B,)
    assert (zero.rms == 0).all() and (zero.step_rms > 0).all() and (zero.relative() == 0).all()
    assert model.training                                                  # the mode it came with is put back
    aug = RigidAugment(seed=SEED, translate=2.0)
    got = equivariance_error(model, batch, aug, epoch=5)
    m = draw_motions(batch, aug, 5)
    by_motions = equivariance_error(model, batch, m)
    assert torch.equal(got.rms, by_motions.rms) and torch.equal(got.step_rms, by_motions.step_rms)
    model.eval()
    with torch.no_grad():
        out = model(batch)
        xp = m.apply(batch.x_position)
        moved = PairData(batch.x_aminoacid, xp, m.apply(batch.y), torch.cat([xp[0][batch.edge_index[0]], xp[0][batch.edge_index[1]]], 1),
                         batch.edge_index)
        moved.num_graphs = B
        out_g = model(moved)
        g_out = m.apply(out)
    diff = (out_g.cpu().numpy().astype(np.float64) - g_out.cpu().numpy().astype(np.float64)).reshape(B, N, 3)
    want = np.sqrt((diff ** 2).sum(axis=(1, 2)) / N)
    step = (out.cpu().numpy().astype(np.float64) - batch.x_position[-1].cpu().numpy().astype(np.float64)).reshape(B, N, 3)
    want_step = np.sqrt((step ** 2).sum(axis=(1, 2)) / N)
    print("rms", got.rms.tolist(), "step", got.step_rms.tolist(), "relative", got.relative().tolist())
    assert np.allclose(got.rms.cpu().numpy(), want, rtol=1e-12, atol=0) and (want > 0).all() and np.isfinite(want).all()
    assert np.allclose(got.step_rms.cpu().numpy(), want_step, rtol=1e-12, atol=0)
    assert np.allclose(got.relative().cpu().numpy(), want / want_step, rtol=1e-12, atol=0)
    assert same_bits(zero.step_rms, got.step_rms.cpu().numpy())          # the clean forward is the same one


# ================================================================================================ engine layout
def test_round_trip_on_the_engines_frame_layout(dev):
    """frames [S, M*N, 3] as an engine stores them, M members = M samples: apply then inverse equals the restatement's
    round trip in every bit, and the start windows [W, M, N, 3] move through the same call as their flat view."""
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd.training import RigidMotions
    S, M, N, W = 6, 4, 37, 3
    frames = frames_of(M, N, S, seed=9)
    ids = [11, 4, 2 ** 31 - 1, 0]
    want_m = RR.motions(SEED, ids, 0, translate=1.0, first_frame=frames[0], n_atoms=N)
    f_d = torch.from_numpy(frames).to(dev)
    m = RigidMotions(*ops.rigid_motions(SEED, ids, 0, translate=1.0, first_frame=f_d[0], n_atoms=N), N)
    there = m.apply(f_d)
    back = m.apply(there, inverse=True)
    want_there = RR.apply(want_m, frames, N)
    assert same_bits(there, want_there) and same_bits(back, RR.apply(want_m, want_there, N, inverse=True))
    wins = f_d[:W].view(W, M, N, 3)
    assert torch.equal(m.apply(wins.reshape(W, M * N, 3)).view(W, M, N, 3), there[:W].view(W, M, N, 3))


# ================================================================================================ guard bands
def _run_guarded(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd.training import RigidAugment
    dtraj = device_trajectory()
    res = []
    with Guard(fill, record_calls=False) as G:
        for B, N in ((1, 1), (3, 28), (5, 65)):
            x = G.place(torch.from_numpy(frames_of(B, N, 3)).to(dev))
            q, c, t, att = ops.rigid_motions(SEED, sample_ids(B), BIG_EPOCH, translate=2.5, first_frame=x[0], n_atoms=N)
            moved = ops.rigid_apply(q, c, t, N, x)
            ops.rigid_apply(q, c, t, N, x, inverse=True, out=x)                              # in place, inside its arena
            R = B * N
            ei = torch.randint(0, R, (2, 4 * R + 3), generator=torch.Generator().manual_seed(R)).to(dev)
            ei[0, 1], ei[1, 2], ei[0, -1] = R, -1, 2 ** 40                                   # outside the frame
            attr = ops.edge_attr_gather(moved[0], G.place(ei))
            assert bool(torch.isnan(attr[[1, 2, -1]]).all()) and not bool(torch.isnan(attr[3:-1]).any())
            assert torch.equal(attr[0, :3], moved[0][ei[0, 0]]) and torch.equal(attr[0, 3:], moved[0][ei[1, 0]])
            empty = ops.edge_attr_gather(moved[0], torch.empty((2, 0), dtype=torch.long, device=dev))
            assert empty.shape == (0, 6)
            res += [q.clone(), c.clone(), t.clone(), att.clone(), moved.clone(), x.clone(), attr.clone()]
        origin = ops.rigid_motions(SEED, sample_ids(4), 0, device=dev)
        res += [o.clone() for o in origin]
        b = dtraj.batch([9, 0, 7], augment=RigidAugment(seed=SEED, translate=1.0), epoch=3, unroll=2)
        res += [b.x_position.clone(), b.y.clone(), b.y_unroll.clone(), b.edge_attr.clone()]
        G.verify()
    return res


def test_augment_entry_points_stay_inside_their_buffers(dev):
    """The three entry points of include/mdno_augment.h inside guard bands under both fill bytes: every band intact, every
    output equal under both fills (nothing unset is read), NaN only in the rows of the out-of-frame edges."""
    from guarded import FILLS
    from molecular_dynamics_neural_operator_amd import _lib
    assert set(_lib.AUGMENT_SIGNATURES) == {"mdnoaug_motions", "mdnoaug_apply", "mdnoaug_edge_attr"}
    a, b = (_run_guarded(dev, fill) for fill in FILLS)
    assert len(a) == len(b) == 29
    for i, (u, v) in enumerate(zip(a, b)):
        assert same_bits(u, v.cpu().numpy()), i
        if i % 7 != 6 or i >= 21:
            assert not torch.isnan(u.double()).any(), i
