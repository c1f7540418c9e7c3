"""Contact statistics on the device (include/mdno_contacts.h, csrc/contacts.hip) against the numpy fp64
restatement of the header's rule (tests/contacts_ref.py).  Every operation of the rule is an IEEE operation rounded once and
every sum is one chain in step order, so there is no tolerance anywhere in this file: the counts, the bits, per_frame, origins
and both are EQUAL, sum_r and sum_r2 are bit-equal doubles per block and so is `.total()`."""
import numpy as np
import pytest
import torch

import contacts_ref as R

pytestmark = pytest.mark.gpu

T = 64          # MDNOCM_TILE


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    assert _lib.CONTACTS_TILE == T
    return torch.device("cuda:0")


def on(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    """Two tensors of one dtype and shape with the same bits."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return bool(torch.equal(a, b))


def cloud(S, M, N, seed, scale=6.0):
    """Gaussian clouds: at scale 6 about a sixth of the pairs lie inside 8."""
    return (np.random.default_rng(seed).normal(size=(S, M, N, 3)) * scale).astype(np.float32)


def device_statistics(dev, frames, threshold=8.0, box=None, block_len=64, moments=True):
    from molecular_dynamics_neural_operator_amd import forecast
    st = forecast.pair_statistics(on(dev, frames), threshold, box=box, block_len=block_len, moments=moments)
    S, M, N = frames.shape[:3]
    Bk = -(-S // block_len)
    assert st.count.shape == (Bk, M, N, N) and st.count.dtype == torch.int32 and st.n_frames.dtype == torch.int64
    if moments:
        assert st.sum_r.shape == st.sum_r2.shape == (Bk, M, N, N) and st.sum_r.dtype == st.sum_r2.dtype == torch.float64
    else:
        assert st.sum_r is None and st.sum_r2 is None
    return st


def check_statistics(st, want, members=slice(None)):
    count, sum_r, sum_r2, n_frames = want
    assert np.array_equal(st.n_frames.cpu().numpy(), n_frames)
    assert np.array_equal(st.count.cpu().numpy(), count[:, members]), "count"
    if st.sum_r is not None:
        assert np.array_equal(bits64(st.sum_r.cpu().numpy()), bits64(sum_r[:, members])), "sum_r"
        assert np.array_equal(bits64(st.sum_r2.cpu().numpy()), bits64(sum_r2[:, members])), "sum_r2"


# ================================================================================================ 1. statistics
@pytest.mark.parametrize("S", [1, 5, 63, 64, 65, 129])
@pytest.mark.parametrize("N", [1, 2, 3, T - 1, T, T + 1, 2 * T + 1])
def test_statistics_equal_the_restatement_at_every_size(dev, N, S):
    """Three members; block_len 1, 5, 64, S and S + 3 (one short block, whole blocks, a short last block); with and without
    the moments; and one member alone, whose maps are those of member 0 of the three.  N up to two tiles and one atom: a
    diagonal tile, a full off-diagonal tile with its mirror, and a one-atom tile row and column."""
    frames = cloud(S, 3, N, 1000 * N + S)
    r, sq = R.frame_distances(frames), R.frame_squares(frames)
    for block_len in sorted({1, 5, 64, S, S + 3}):
        want = R.block_statistics(r, sq, 8.0, block_len)
        st = device_statistics(dev, frames, block_len=block_len)
        check_statistics(st, want)
        tot = st.total()
        assert np.array_equal(tot.count.cpu().numpy(), R.total(want[0])) and int(tot.n_frames) == S
        assert np.array_equal(bits64(tot.sum_r.cpu().numpy()), bits64(R.total(want[1])))
        assert np.array_equal(bits64(tot.sum_r2.cpu().numpy()), bits64(R.total(want[2])))
        check_statistics(device_statistics(dev, frames, block_len=block_len, moments=False), want)
        for moments in (True, False):
            check_statistics(device_statistics(dev, frames[:, :1], block_len=block_len, moments=moments), want, slice(0, 1))


def test_either_sum_alone(dev):
    """ops level: sum_r without sum_r2 and the reverse are what the C ABI allows; the wrapper asks for both or neither, so the
    two pointers are passed by hand."""
    from molecular_dynamics_neural_operator_amd import _lib
    from molecular_dynamics_neural_operator_amd.ops import ptr, stream_ptr
    lib = _lib.load()
    frames = cloud(70, 2, T + 1, 5)
    want = R.pair_statistics(frames, 8.0, None, 64)
    x = on(dev, frames)
    for which in (1, 2):
        count = torch.empty((2, 2, T + 1, T + 1), dtype=torch.int32, device=dev)
        acc = torch.empty((2, 2, T + 1, T + 1), dtype=torch.float64, device=dev)
        _lib.check(lib.mdnocm_pair_statistics(ptr(x), 70, 2, T + 1, 8.0, None, 64, ptr(count), ptr(acc) if which == 1 else None,
                                              ptr(acc) if which == 2 else None, stream_ptr(dev)))
        assert np.array_equal(count.cpu().numpy(), want[0]) and np.array_equal(bits64(acc.cpu().numpy()), bits64(want[which]))


def test_a_pair_exactly_on_the_threshold_is_not_in_contact(dev):
    """Integer triples: (3, 4, 0), (6, 8, 0), (5, 12, 0), (2, 3, 6) and (1, 4, 8) put a pair at r == 5, 10, 13, 7 and 9 exactly;
    with that threshold it is out (strict), a float step of the threshold more and it is in.  Then one atom a float step
    inside the threshold on an axis and one a float step outside."""
    for off, thr in (((3, 4, 0), 5.0), ((6, 8, 0), 10.0), ((5, 12, 0), 13.0), ((2, 3, 6), 7.0), ((1, 4, 8), 9.0)):
        frames = np.zeros((3, 1, 2, 3), np.float32)
        frames[:, 0, 0] = (7.0, -2.0, 1.0)
        frames[:, 0, 1] = np.array((7.0, -2.0, 1.0), np.float32) + np.array(off, np.float32)
        for moments in (True, False):
            st = device_statistics(dev, frames, thr, block_len=2, moments=moments)
            assert st.count.cpu().tolist() == [[[[2, 0], [0, 2]]], [[[1, 0], [0, 1]]]], (off, moments)
            up = device_statistics(dev, frames, float(np.nextafter(thr, np.inf)), block_len=2, moments=moments)
            assert up.count.cpu().tolist() == [[[[2, 2], [2, 2]]], [[[1, 1], [1, 1]]]], (off, moments)
        check_statistics(st, R.pair_statistics(frames, thr, None, 2))
        st = device_statistics(dev, frames, thr, block_len=2)
        assert st.sum_r[0, 0, 0, 1].item() == 2 * thr and st.sum_r2[1, 0, 0, 1].item() == thr * thr
    thr = np.float32(8.0)
    frames = np.zeros((1, 1, 3, 3), np.float32)
    frames[0, 0, 1, 0] = np.nextafter(thr, np.float32(0))          # sqrt(x * x) == x for an fp32 x: r is the coordinate
    frames[0, 0, 2, 1] = -np.nextafter(thr, np.float32(np.inf))
    for moments in (True, False):
        st = device_statistics(dev, frames, 8.0, moments=moments)
        assert st.count[0, 0].cpu().tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 1]]
    check_statistics(device_statistics(dev, frames), R.pair_statistics(frames, 8.0))


def test_a_nan_and_an_inf_atom_mark_their_pairs_and_nothing_else(dev):
    S, M, N = 5, 3, 6
    clean = cloud(S, M, N, 9, scale=4.0)
    frames = clean.copy()
    frames[2, 1, 3, 0] = np.nan
    frames[2, 1, 4, 1] = np.inf
    want, want_clean = R.pair_statistics(frames, 8.0, None, 2), R.pair_statistics(clean, 8.0, None, 2)
    for moments in (True, False):
        st = device_statistics(dev, frames, block_len=2, moments=moments)
        count = st.count.cpu().numpy()
        assert np.array_equal(count, want[0])
        hit = np.zeros((3, M, N, N), bool)
        hit[1, 1, [3, 4], :] = hit[1, 1, :, [3, 4]] = True
        assert np.array_equal(count[~hit], want_clean[0][~hit])
        # a marked pair is not counted in the marked step: one frame less than the clean run where that frame was in contact
        assert (count[hit] <= want_clean[0][hit]).all() and (count[1, 1, 3, :] <= 1).all() and count[1, 1, 4, 4] == 1
        if moments:
            for got, ref, ref_clean in ((st.sum_r.cpu().numpy(), want[1], want_clean[1]), (st.sum_r2.cpu().numpy(), want[2], want_clean[2])):
                assert not np.isfinite(got[hit]).any() and np.isfinite(got[~hit]).all()
                assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
                assert np.array_equal(bits64(got[~hit]), bits64(ref_clean[~hit]))          # every other member and pair: its bits
                assert np.isnan(got[1, 1, 3, :]).all() and np.isposinf(got[1, 1, 4, 0]) and np.isnan(got[1, 1, 4, 4])


@pytest.mark.parametrize("box", [(20.0, 0.0, 0.0), (0.0, 17.5, 16.0), (16.0, 23.0, 19.0)])
def test_periodic_boxes_with_atoms_many_box_lengths_apart(dev, box):
    """One, two and three periodic axes; coordinates of scale 100 along them (5 along an open axis), so the images are 5 and
    more box lengths away."""
    from molecular_dynamics_neural_operator_amd import forecast, ops
    frames = cloud(9, 2, T + 3, 11, scale=100.0)
    for a in range(3):
        if box[a] == 0.0:
            frames[..., a] *= np.float32(0.05)
    want = R.pair_statistics(frames, 8.0, box, 4)
    assert want[0].sum() > 2 * 9 * 2 * (T + 3)           # as many contacts beyond the diagonal as on it: the minimum image is at work
    assert not np.array_equal(want[0], R.pair_statistics(frames, 8.0, None, 4)[0])
    check_statistics(device_statistics(dev, frames, box=box, block_len=4), want)
    check_statistics(device_statistics(dev, frames, box=box, block_len=4, moments=False), want)
    pairs = np.stack(np.triu_indices(T + 3, 1), 1)[::7]
    cut = np.random.default_rng(3).uniform(2.0, 8.0, size=len(pairs))
    c = R.contact_series(frames, pairs, cut, 8.0, box)
    assert c.any()
    bits, per_frame = ops.contact_bits(on(dev, frames), on(dev, pairs.astype(np.int32)), on(dev, cut), 8.0, box=box)
    assert np.array_equal(bits.cpu().numpy(), R.pack_bits(c)) and np.array_equal(per_frame.cpu().numpy(), R.per_frame(c))
    with pytest.raises(forecast.MdnoError, match="2 \\* cutoff"):
        forecast.pair_statistics(on(dev, frames), 8.01, box=(16.0, 23.0, 19.0))


# ================================================================================================ 2. series
def pair_list(P, N, seed):
    """P pairs of atoms 0 .. N - 1 with repeats, i == j pairs and indices outside the frame among them, and their cutoffs."""
    rng = np.random.default_rng(seed)
    pairs = rng.integers(0, N, size=(P, 2))
    cut = rng.uniform(3.0, 12.0, size=P)
    if P > 1:
        pairs[1] = pairs[0]                       # a repeated pair, with another cutoff
    if P >= 63:
        pairs[2] = pairs[0][::-1]
        pairs[5] = (3, 3)                         # i == j: r = 0
        pairs[7] = (N, 0)                         # outside the frame
        pairs[11] = (2, -1)
        pairs[13] = (2 ** 31 - 1, -2 ** 31)
        pairs[P - 1] = (N - 1, N + 5)
        cut[17] = 0.0                             # never in contact (r < 0 is false), i == j included
        pairs[17] = (4, 4)
    return pairs.astype(np.int32), cut


@pytest.mark.parametrize("S", [1, 64, 65, 130])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257])
def test_series_equal_the_restatement(dev, P, S):
    from molecular_dynamics_neural_operator_amd import ops
    N, M = 29, 3
    frames = cloud(S, M, N, 7 * P + S)
    pairs, cut = pair_list(P, N, P)
    c = R.contact_series(frames, pairs, cut, 10.5)
    bits, per_frame = ops.contact_bits(on(dev, frames), on(dev, pairs), on(dev, cut), 10.5)
    assert bits.shape == (M, P, -(-S // 64)) and bits.dtype == torch.int64 and per_frame.shape == (S, M) and per_frame.dtype == torch.int32
    assert np.array_equal(bits.cpu().numpy(), R.pack_bits(c))          # the bits from S on are 0 in both
    assert np.array_equal(per_frame.cpu().numpy(), R.per_frame(c))
    if P >= 63:
        assert c[:, 5].all() and not c[:, [7, 11, 13, 17, P - 1]].any()
        assert c.sum() > P * S // 20


def test_series_through_the_classes(dev):
    """ContactPairs.native -> contact_series -> fraction / series / correlation, against the restatement; an empty list."""
    from molecular_dynamics_neural_operator_amd import forecast
    S, M, N = 70, 2, 40
    frames = cloud(S, M, N, 21, scale=5.0)
    native = forecast.ContactPairs.native(frames[0, 0], 8.0, min_separation=3, factor=1.2)
    assert 40 < len(native) < N * N // 2
    cs = forecast.contact_series(on(dev, frames), native)
    c = R.contact_series(frames, native.pairs.numpy(), native.cut.numpy(), native.cut_max)
    assert np.array_equal(cs.series().cpu().numpy(), c) and cs.n_steps == S
    assert np.array_equal(cs.fraction().cpu().numpy(), R.per_frame(c).astype(np.float64) / len(native))
    assert bool((cs.fraction()[0, 0] == 1.0).all())                  # the native frame holds every native contact (factor > 1)
    cc = cs.correlation()
    lags = forecast.default_lags(S)
    origins, both = R.correlation(c, lags)
    assert cc.lags.tolist() == lags and np.array_equal(cc.origins.cpu().numpy(), origins) and np.array_equal(cc.both.cpu().numpy(), both)
    surv = both.sum(1) / origins.sum(1)
    assert np.array_equal(cc.survival().cpu().numpy(), surv) and bool((cc.survival()[:, 0] == 1.0).all())
    empty = forecast.contact_series(on(dev, frames), forecast.ContactPairs.of(None, []))
    assert empty.bits.shape == (M, 0, 2) and not empty.per_frame.any() and torch.isnan(empty.fraction()).all()
    assert empty.correlation([0, 3]).origins.shape == (M, 0, 2)
    st = forecast.pair_statistics(on(dev, frames[:, :1]), 8.0)
    listed = forecast.ContactPairs.from_statistics(st, 0.25, 3)
    p = R.total(R.pair_statistics(frames[:, :1], 8.0)[0])[0] / S
    i, j = np.triu_indices(N, 3)
    assert listed.pairs.tolist() == np.stack([i, j], 1)[p[i, j] >= 0.25].tolist() and listed.pairs.device.type == "cpu"
    assert 50 < len(listed) < len(i) - 50


# ================================================================================================ 3. correlation
@pytest.mark.parametrize("S", [1, 64, 65, 130])
def test_correlation_equals_the_restatement(dev, S):
    """Lags 0, 1, 63, 64, 65 and S - 1 (those below S) on dense random series (half the bits set, runs of set bits, an
    all-set and an all-clear row), then every lag twice: 2 S lags, more than one launch's worth at S = 130."""
    from molecular_dynamics_neural_operator_amd import ops
    rng = np.random.default_rng(S)
    M, P = 2, 37
    c = rng.random((M, P, S)) < 0.5
    c[0, 1] = True
    c[0, 2] = False
    c[1, 3:9] = np.repeat(rng.random((6, -(-S // 8))) < 0.6, 8, axis=1)[:, :S]
    bits = on(dev, R.pack_bits(c))
    for lags in (sorted({l for l in (0, 1, 63, 64, 65, S - 1) if 0 <= l < S}), list(range(S)) * 2, [S - 1] * 300):
        origins, both = ops.contact_correlation(bits, S, lags)
        want_o, want_b = R.correlation(c, lags)
        assert origins.shape == (M, P, len(lags)) and origins.dtype == both.dtype == torch.int32
        assert np.array_equal(origins.cpu().numpy(), want_o) and np.array_equal(both.cpu().numpy(), want_b)
    high = c.copy()
    wide = R.pack_bits(high).copy()
    if S % 64:
        wide[..., -1] |= np.int64(-1) << np.int64(S % 64)            # set bits from S on: they are never looked at
    origins, both = ops.contact_correlation(on(dev, wide), S, [0, S - 1])
    want_o, want_b = R.correlation(c, [0, S - 1])
    assert np.array_equal(origins.cpu().numpy(), want_o) and np.array_equal(both.cpu().numpy(), want_b)
    assert ops.contact_correlation(bits, S, [])[0].shape == (M, P, 0)
    with pytest.raises(ops.MdnoError, match="lag"):
        ops.contact_correlation(bits, S, [S])


# ================================================================================================ 4. identities
def test_identities_with_the_kernels_the_tree_already_has(dev):
    from molecular_dynamics_neural_operator_amd import forecast
    S, M, N = 21, 2, T + 9
    for box in (None, (30.0, 0.0, 28.0)):
        frames = cloud(S, M, N, 31, scale=6.0 if box is None else 40.0)
        x = on(dev, frames)
        st = forecast.pair_statistics(x, 8.0, box=box, block_len=S + 1, moments=False)
        maps = forecast.contact_maps(x, 8.0, box=box)
        assert torch.equal(st.count[0].to(torch.int64), maps.sum(0, dtype=torch.int64))
        blocks = forecast.pair_statistics(x, 8.0, box=box, block_len=4)
        upper = torch.triu(torch.ones((N, N), dtype=torch.bool, device=dev), 1)
        hist = forecast.pair_histogram(x, 8.0, 50, box=box).counts                   # [S, M, 50], unordered pairs
        assert torch.equal((blocks.count.to(torch.int64) * upper).sum((0, 2, 3)), hist.sum((0, 2)))
        assert torch.equal(blocks.total().count, st.count[0])
        pairs = np.stack(np.triu_indices(N, 1), 1)[::5]
        cut = np.random.default_rng(5).uniform(3.0, 9.0, size=len(pairs))
        cs = forecast.contact_series(x, forecast.ContactPairs.of(pairs, cut, N), box=box)
        d = forecast.internal_coordinates(x, forecast.Featurizer.distances(pairs, N), box=box, dtype=torch.float64)          # [S, M, P]
        assert torch.equal(cs.series(), (d < on(dev, cut)).permute(1, 2, 0))
        assert torch.equal(cs.per_frame.to(torch.int64), (d < on(dev, cut)).sum(2))


# ================================================================================================ 5. determinism
def test_a_blocks_bits_depend_on_its_frames_alone(dev):
    frames = cloud(129, 3, T + 1, 41)
    a = device_statistics(dev, frames)
    b = device_statistics(dev, frames)
    assert same(a.count, b.count) and same(a.sum_r, b.sum_r) and same(a.sum_r2, b.sum_r2)
    short = device_statistics(dev, frames[:100])                       # another S: block 0 whole, block 1 cut short
    assert same(short.count[0], a.count[0]) and same(short.sum_r[0], a.sum_r[0]) and same(short.sum_r2[0], a.sum_r2[0])
    assert not same(short.sum_r[1], a.sum_r[1])
    late = device_statistics(dev, frames[64:])                         # the same frames as another block index
    assert same(late.sum_r[0], a.sum_r[1]) and same(late.sum_r2[1], a.sum_r2[2]) and same(late.count, a.count[1:])
    other = frames.copy()
    other[:, [0, 2]] = cloud(129, 2, T + 1, 42, scale=50.0)            # the other members change, and their number
    moved = device_statistics(dev, other)
    alone = device_statistics(dev, frames[:, 1:2])
    for st, m in ((moved, 1), (alone, 0)):
        assert same(st.count[:, m], a.count[:, 1]) and same(st.sum_r[:, m], a.sum_r[:, 1]) and same(st.sum_r2[:, m], a.sum_r2[:, 1])
    assert same(a.sum_r, a.sum_r.transpose(2, 3).contiguous()) and same(a.sum_r2, a.sum_r2.transpose(2, 3).contiguous())
    assert same(a.count, a.count.transpose(2, 3).contiguous())


# ================================================================================================ 6. engines
def test_engines_equal_the_free_functions(dev):
    """A noisy 4-step, 8-member, N = 28 run without a box and under one that folds the chain onto itself: both engines'
    pair_statistics and contact_series equal the stand-alone calls on the produced(...) frames bit for bit, at the engine's own
    threshold and in the engine's own box; the trajectory buffer is unchanged."""
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine, RolloutEngine
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    traj = syn.ou_trajectory(syn.chain_frame(28, seed=1), 3 + 6, seed=2)
    wins = torch.from_numpy(np.ascontiguousarray(syn.ensemble_windows(traj[:3], 8, sigma=0.1, seed0=100).transpose(1, 0, 2, 3)))
    aa = torch.from_numpy(syn.amino_acids(28, seed=1))
    model = KernelNN(64, 128, 2, 6, 7, 3, 20, 4)
    model.load_state_dict(near_identity_state_dict(64, 128, seed=0, kernel_gain=1e-3, feature_gain=0.1))
    model = model.eval().to(dev)
    native = forecast.ContactPairs.native(torch.from_numpy(traj[0]), 8.0, min_separation=3)
    assert len(native) > 10 and native.cut_max == 8.0
    results = {}
    for box in (None, (16.0, 16.0, 0.0)):
        for cls in (RolloutEngine, GroupedRolloutEngine):
            eng = cls(model, 8, 28, 3, 8.0, max_steps=4, device=dev, noise_sigma=0.05, noise_seed=7, box=box)
            eng.run(wins, aa, 4)
            before = eng.frames().clone()
            for first, steps in ((0, None), (1, 2)):
                n = 4 - first if steps is None else steps
                produced = eng.produced(first, n).contiguous()
                for moments in (True, False):
                    want = forecast.pair_statistics(produced, 8.0, box=box, block_len=3, moments=moments)
                    got = eng.pair_statistics(block_len=3, moments=moments, first_step=first, steps=steps)
                    assert got.count.shape == (-(-n // 3), 8, 28, 28) and same(got.count, want.count) and got.box == box
                    assert got.threshold == 8.0 and torch.equal(got.n_frames, want.n_frames)
                    assert (got.sum_r is None and got.sum_r2 is None) if not moments else \
                        (same(got.sum_r, want.sum_r) and same(got.sum_r2, want.sum_r2))
                want = forecast.contact_series(produced, native, box=box)
                got = eng.contact_series(native, first_step=first, steps=steps)
                assert got.bits.shape == (8, len(native), 1) and same(got.bits, want.bits) and same(got.per_frame, want.per_frame)
                assert got.n_steps == n
            wide = eng.pair_statistics(threshold=7.0, block_len=64)
            assert same(wide.count, forecast.pair_statistics(eng.produced(0, 4).contiguous(), 7.0, box=box).count)
            results[(box, cls.__name__)] = (eng.produced(0, 4).contiguous(), eng.pair_statistics(), eng.contact_series(native))
            assert torch.equal(eng.frames(), before)
            eng.close()
    for box in (None, (16.0, 16.0, 0.0)):
        (fu, su, cu), (fg, sg, cg) = results[(box, "RolloutEngine")], results[(box, "GroupedRolloutEngine")]
        assert torch.equal(fu, fg)                  # (perturbed copies of one system: the groups' frames are the one engine's)
        assert same(su.count, sg.count) and same(su.sum_r, sg.sum_r) and same(su.sum_r2, sg.sum_r2)
        assert same(cu.bits, cg.bits) and same(cu.per_frame, cg.per_frame)
    open_frames, open_stats, _ = results[(None, "RolloutEngine")]
    boxed = forecast.pair_statistics(open_frames, 8.0, box=(16.0, 16.0, 0.0))
    assert not same(boxed.count, open_stats.count)                # the box matters on this chain, so "its own box" is a statement


# ================================================================================================ 7. guard bands
COVERED = {"mdnocm_pair_statistics", "mdnocm_contact_bits", "mdnocm_contact_correlation"}


def _run_guarded(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import ops
    res = []
    with Guard(fill, record_calls=False) as G:
        for N, S, M, block_len in ((1, 3, 2, 2), (3, 65, 1, 64), (T + 1, 5, 2, 3), (2 * T + 1, 2, 1, 5)):
            x = G.place(on(dev, cloud(S, M, N, N + S)))
            for box in (None, (40.0, 0.0, 40.0)):
                for moments in (True, False):
                    out = ops.pair_statistics(x, 8.0, box=box, block_len=block_len, moments=moments)          # outputs: guarded
                    res += [t.clone() for t in out if t is not None]
            for P in (1, 65, 257):
                pairs, cut = pair_list(P, N, P)
                bits, per_frame = ops.contact_bits(x, G.place(on(dev, pairs)), G.place(on(dev, cut)), 10.5)
                lags = sorted({0, 1, S - 1})
                origins, both = ops.contact_correlation(bits, S, lags)
                res += [bits.clone(), per_frame.clone(), origins.clone(), both.clone()]
        G.verify()
    return res


def test_contact_entry_points_stay_inside_their_buffers(dev):
    """The three entry points of include/mdno_contacts.h inside guard bands under both fill bytes: every band intact, and every
    output bitwise equal under both fills (nothing unset is read, every element is written)."""
    import re
    from pathlib import Path
    from guarded import FILLS
    text = re.sub(r"/\*.*?\*/", "", (Path(__file__).resolve().parents[1] / "include" / "mdno_contacts.h").read_text(), flags=re.S)
    writing = {m.group(1) for m in re.finditer(r"^int\s+(mdnocm_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S | re.M)
               if re.search(r"(?<!const )\b(?:double|int32_t|uint64_t)\s*\*", m.group(2))}
    assert writing == COVERED, writing ^ COVERED
    a, b = (_run_guarded(dev, fill) for fill in FILLS)
    assert len(a) == len(b) == 4 * (2 * (3 + 1) + 3 * 4)
    for i, (u, v) in enumerate(zip(a, b)):
        assert same(u, v), i
