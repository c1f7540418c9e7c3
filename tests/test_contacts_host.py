"""Contact statistics without a GPU: the numpy restatement of include/mdno_contacts.h (tests/contacts_ref.py) against
brute-force loops at tiny sizes, the arithmetic of the Python classes of forecast.py on CPU tensors built by hand, and every
refusal that happens before any device work."""
import math

import numpy as np
import pytest
import torch

import contacts_ref as R
from molecular_dynamics_neural_operator_amd import forecast as F
from molecular_dynamics_neural_operator_amd import ops
from molecular_dynamics_neural_operator_amd._lib import MdnoError


def frames_of(S, M, N, seed, scale=6.0):
    return (np.random.default_rng(seed).normal(size=(S, M, N, 3)) * scale).astype(np.float32)


def brute_distance(xi, xj, box):
    d = []
    for a in range(3):
        da = float(np.float64(xj[a]) - np.float64(xi[a]))
        L = 0.0 if box is None else box[a]
        if L > 0.0:
            da = da - float(np.rint(da * (1.0 / L))) * L
        d.append(da)
    s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return math.sqrt(s), s


# ================================================================================================ the restatement
@pytest.mark.parametrize("box", [None, (20.0, 0.0, 0.0), (20.0, 18.0, 0.0), (20.0, 18.0, 17.0)])
def test_pair_statistics_restatement_equals_brute_force_loops(box):
    S, M, N, block_len, cut = 7, 2, 5, 3, 8.0
    x = frames_of(S, M, N, 1, scale=15.0)
    count, sum_r, sum_r2, n_frames = R.pair_statistics(x, cut, box, block_len)
    assert count.shape == (3, M, N, N) and n_frames.tolist() == [3, 3, 1]
    for b in range(3):
        for m in range(M):
            for i in range(N):
                for j in range(N):
                    c, ar, as_ = 0, 0.0, 0.0
                    for s in range(b * block_len, min(S, (b + 1) * block_len)):
                        r, sq = brute_distance(x[s, m, i], x[s, m, j], box)
                        c += r < cut
                        ar = ar + r
                        as_ = as_ + sq
                    assert count[b, m, i, j] == c
                    assert sum_r[b, m, i, j].tobytes() == np.float64(ar).tobytes()
                    assert sum_r2[b, m, i, j].tobytes() == np.float64(as_).tobytes()
    assert np.array_equal(count, count.transpose(0, 1, 3, 2))
    assert np.array_equal(sum_r.view(np.int64), sum_r.transpose(0, 1, 3, 2).view(np.int64))
    assert (count[:, :, np.arange(N), np.arange(N)] == n_frames[:, None, None]).all()          # r = 0 on the diagonal
    assert R.total(sum_r).tobytes() == ((sum_r[0] + sum_r[1]) + sum_r[2]).tobytes()


def test_series_and_correlation_restatement_equal_brute_force_loops():
    S, M, N = 9, 2, 4
    x = frames_of(S, M, N, 2)
    pairs = np.array([[0, 1], [1, 0], [2, 2], [0, 3], [0, 3], [1, 7], [-1, 2]])
    cut = np.array([8.0, 8.0, 1.0, 5.0, 9.5, 8.0, 8.0])
    c = R.contact_series(x, pairs, cut, 9.0)
    assert c.shape == (M, 7, S)
    for m in range(M):
        for p, (i, j) in enumerate(pairs):
            for s in range(S):
                want = False
                if 0 <= i < N and 0 <= j < N:
                    r, _ = brute_distance(x[s, m, i], x[s, m, j], None)
                    want = r < cut[p] and r < 9.0
                assert c[m, p, s] == want
    assert c[:, 2].all() and not c[:, 5:].any() and np.array_equal(c[:, 0], c[:, 1])
    assert np.array_equal(R.per_frame(c), np.array([[c[m, :, s].sum() for m in range(M)] for s in range(S)]))
    lags = [0, 1, 4, 8]
    origins, both = R.correlation(c, lags)
    for m in range(M):
        for p in range(7):
            for l, lag in enumerate(lags):
                ts = [t for t in range(S - lag) if c[m, p, t]]
                assert origins[m, p, l] == len(ts) and both[m, p, l] == sum(bool(c[m, p, t + lag]) for t in ts)
    assert np.array_equal(origins[..., 0], both[..., 0])


def test_pack_bits_puts_step_s_into_bit_s_mod_64_of_word_s_div_64():
    c = np.zeros((1, 2, 130), bool)
    c[0, 0, [0, 63, 64, 129]] = True
    c[0, 1, :] = True
    w = R.pack_bits(c).view(np.uint64)
    assert w.shape == (1, 2, 3)
    assert w[0, 0].tolist() == [1 | (1 << 63), 1, 2] and w[0, 1].tolist() == [2 ** 64 - 1, 2 ** 64 - 1, 3]
    series = F.ContactSeries(torch.from_numpy(w.view(np.int64)), torch.zeros((130, 1), dtype=torch.int32), 130,
                             F.ContactPairs.of([[0, 1], [0, 2]], 8.0))
    assert np.array_equal(series.series().numpy(), c)


# ================================================================================================ the classes, by hand
def hand_statistics():
    count = torch.tensor([[[[4, 2], [2, 4]]], [[[2, 0], [0, 2]]], [[[0, 0], [0, 0]]]], dtype=torch.int32)          # [3, 1, 2, 2]
    sum_r = torch.tensor([[[[0.0, 8.0], [8.0, 0.0]]], [[[0.0, 20.0], [20.0, 0.0]]], [[[0.0, 0.0], [0.0, 0.0]]]], dtype=torch.float64)
    sum_r2 = torch.tensor([[[[0.0, 20.0], [20.0, 0.0]]], [[[0.0, 208.0], [208.0, 0.0]]], [[[0.0, 0.0], [0.0, 0.0]]]], dtype=torch.float64)
    return F.PairStatistics(count, sum_r, sum_r2, torch.tensor([4, 2, 0]), 8.0)


def test_probability_mean_and_std_per_block_and_in_total():
    st = hand_statistics()
    p = st.probability()
    assert p.shape == (3, 1, 2, 2) and p[0, 0].tolist() == [[1.0, 0.5], [0.5, 1.0]] and p[1, 0].tolist() == [[1.0, 0.0], [0.0, 1.0]]
    assert torch.isnan(p[2]).all() and torch.isnan(st.mean_distance()[2]).all() and torch.isnan(st.distance_std()[2]).all()
    assert st.mean_distance()[0, 0, 0, 1] == 2.0 and st.mean_distance()[1, 0, 0, 1] == 10.0
    assert st.distance_std()[0, 0, 0, 1] == 1.0 and st.distance_std()[1, 0, 0, 1] == 2.0          # 20/4 - 4 = 1; 208/2 - 100 = 4
    tot = st.total()
    assert tot.count.shape == (1, 2, 2) and int(tot.n_frames) == 6
    assert tot.count[0].tolist() == [[6, 2], [2, 6]] and tot.sum_r[0, 0, 1] == 28.0 and tot.sum_r2[0, 0, 1] == 228.0
    assert tot.probability()[0, 0, 1] == 2.0 / 6.0 and tot.total() is tot
    assert (st.distance_std()[:2, 0, 0, 0] == 0.0).all()
    bare = F.PairStatistics(st.count, None, None, st.n_frames, 8.0)
    assert bare.total().sum_r is None and bare.total().count[0].tolist() == [[6, 2], [2, 6]]
    with pytest.raises(MdnoError, match="without the moments"):
        bare.mean_distance()
    empty = F.PairStatistics(torch.zeros((0, 2, 3, 3), dtype=torch.int32), torch.zeros((0, 2, 3, 3), dtype=torch.float64),
                             torch.zeros((0, 2, 3, 3), dtype=torch.float64), torch.zeros(0, dtype=torch.int64), 8.0).total()
    assert empty.count.shape == (2, 3, 3) and torch.isnan(empty.probability()).all() and torch.isnan(empty.mean_distance()).all()


def test_total_adds_the_blocks_in_ascending_order():
    rng = np.random.default_rng(3)
    blocks = rng.normal(size=(5, 1, 3, 3)) * 10.0 ** rng.integers(-8, 8, size=(5, 1, 3, 3))
    st = F.PairStatistics(torch.zeros((5, 1, 3, 3), dtype=torch.int32), torch.from_numpy(blocks), torch.from_numpy(blocks[::-1].copy()),
                          torch.ones(5, dtype=torch.int64), 8.0).total()
    assert st.sum_r.numpy().tobytes() == R.total(blocks).tobytes() and st.sum_r2.numpy().tobytes() == R.total(blocks[::-1]).tobytes()


def test_difference_and_map_error_broadcast_one_truth_member():
    n = 4
    run = torch.zeros((2, n, n), dtype=torch.int32)
    run[0] = 10
    run[1] = torch.tensor([[10, 10, 5, 0], [10, 10, 10, 5], [5, 10, 10, 10], [0, 5, 10, 10]])
    truth = torch.full((1, n, n), 10, dtype=torch.int32)
    a = F.PairStatistics(run, None, None, torch.tensor(10), 8.0)
    b = F.PairStatistics(truth, None, None, torch.tensor(10), 8.0)
    d = a.difference(b)
    assert d.shape == (2, n, n) and not d[0].any() and d[1, 0, 3] == -1.0 and d[1, 0, 2] == -0.5
    assert a.map_error(b).tolist() == [0.0, (4 * 0.5 + 2 * 1.0) / 16]
    assert a.map_error(b, 2).tolist() == [0.0, (4 * 0.5 + 2 * 1.0) / 6]
    assert a.map_error(b, 3).tolist() == [0.0, 1.0] and torch.isnan(a.map_error(b, 4)).all()
    both = F.PairStatistics.cat([a, a])
    assert both.count.shape == (4, n, n) and both.cpu().map_error(b).tolist() == a.map_error(b).tolist() * 2
    with pytest.raises(MdnoError, match="maps of shape"):
        a.difference(F.PairStatistics(torch.zeros((1, 3, 3), dtype=torch.int32), None, None, torch.tensor(10), 8.0))
    with pytest.raises(MdnoError, match="min_separation"):
        a.map_error(b, -1)


def test_survival_per_pair_lifetime_and_total_variation():
    origins = torch.tensor([[[4, 3, 2], [0, 0, 0]], [[4, 4, 4], [4, 4, 4]]], dtype=torch.int32)           # [M=2, P=2, L=3]
    both = torch.tensor([[[4, 2, 1], [0, 0, 0]], [[4, 4, 4], [4, 0, 0]]], dtype=torch.int32)
    cc = F.ContactCorrelation(origins, both, torch.tensor([0, 1, 3]))
    s = cc.survival()
    assert s.tolist() == [[1.0, 2.0 / 3.0, 0.5], [1.0, 0.5, 0.5]]
    pp = cc.per_pair()
    assert pp[0, 0].tolist() == [1.0, 2.0 / 3.0, 0.5] and torch.isnan(pp[0, 1]).all() and pp[1, 1].tolist() == [1.0, 0.0, 0.0]
    want0 = 0.5 * (1.0 + 2.0 / 3.0) * 1 + 0.5 * (2.0 / 3.0 + 0.5) * 2
    assert cc.lifetime().tolist() == [want0, 0.75 + 1.0] and cc.lifetime(0.5).tolist() == [0.5 * want0, 0.5 * 1.75]
    one = F.ContactCorrelation(origins[1:], both[1:], torch.tensor([0, 1, 3]))
    tv = cc.total_variation(one)
    assert tv.shape == (2, 3) and tv[1].tolist() == [0.0, 0.0, 0.0] and tv[0].tolist() == [0.0, 2.0 / 3.0 - 0.5, 0.0]
    with pytest.raises(MdnoError, match="same lags"):
        cc.total_variation(F.ContactCorrelation(origins, both, torch.tensor([0, 1, 2])))
    never = F.ContactCorrelation(torch.zeros((1, 2, 3), dtype=torch.int32), torch.zeros((1, 2, 3), dtype=torch.int32), torch.tensor([0, 1, 3]))
    assert torch.isnan(never.survival()).all() and torch.isnan(never.lifetime()).all()
    nothing = F.ContactCorrelation(torch.zeros((2, 0, 1), dtype=torch.int32), torch.zeros((2, 0, 1), dtype=torch.int32), torch.tensor([0]))
    assert torch.isnan(nothing.survival()).all() and nothing.lifetime().tolist() == [0.0, 0.0]
    joined = F.ContactCorrelation.cat([cc, one])
    assert joined.origins.shape == (3, 2, 3) and joined.cpu().survival()[2].tolist() == s[1].tolist()


def test_fraction_is_per_frame_over_the_number_of_pairs_and_nan_without_pairs():
    pairs = F.ContactPairs.of([[0, 1], [0, 2], [1, 3], [2, 3]], 8.0)
    cs = F.ContactSeries(torch.zeros((2, 4, 1), dtype=torch.int64), torch.tensor([[4, 0], [1, 2], [3, 3]], dtype=torch.int32), 3, pairs)
    assert cs.fraction().tolist() == [[1.0, 0.0], [0.25, 0.5], [0.75, 0.75]]
    none = F.ContactSeries(torch.zeros((2, 0, 1), dtype=torch.int64), torch.zeros((3, 2), dtype=torch.int32), 3, F.ContactPairs.of(None, []))
    assert none.fraction().shape == (3, 2) and torch.isnan(none.fraction()).all()
    two = F.ContactSeries.cat([cs, cs])
    assert two.bits.shape == (4, 4, 1) and two.per_frame.shape == (3, 4)


def test_native_pairs_of_one_frame():
    x = torch.tensor([[0.0, 0, 0], [3.0, 0, 0], [6.0, 0, 0], [6.0, 4.0, 0], [0.0, 4.0, 0], [30.0, 0, 0]])
    nat = F.ContactPairs.native(x, threshold=8.0, min_separation=2)
    # j - i >= 2 and d0 < 8: (0,2) 6, (0,3) sqrt 52, (0,4) 4, (1,3) 5, (1,4) 5, (2,4) sqrt 52; atom 5 is far from all
    assert nat.pairs.tolist() == [[0, 2], [0, 3], [0, 4], [1, 3], [1, 4], [2, 4]] and nat.pairs.dtype == torch.int32
    assert nat.cut.tolist() == [8.0] * 6 and nat.cut_max == 8.0 and nat.n_atoms == 6 and len(nat) == 6
    tight = F.ContactPairs.native(x, threshold=8.0, min_separation=2, factor=1.2)
    assert tight.pairs.tolist() == nat.pairs.tolist()
    assert tight.cut.tolist() == [1.2 * 6.0, 1.2 * math.sqrt(52.0), 1.2 * 4.0, 1.2 * 5.0, 1.2 * 5.0, 1.2 * math.sqrt(52.0)]
    assert tight.cut_max == 1.2 * math.sqrt(52.0)
    assert F.ContactPairs.native(x, 8.0, min_separation=4).pairs.tolist() == [[0, 4]]
    assert F.ContactPairs.native(x, 5.0, min_separation=1).pairs.tolist() == [[0, 1], [0, 4], [1, 2], [2, 3]]          # strict: 5 is out
    wrapped = F.ContactPairs.native(x, 8.0, min_separation=1, box=(33.0, 0.0, 0.0))
    assert [0, 5] in wrapped.pairs.tolist() and [1, 5] in wrapped.pairs.tolist()               # 30 -> -3 by the minimum image
    assert len(F.ContactPairs.native(x[:1], 8.0)) == 0 and F.ContactPairs.native(x[:1], 8.0).cut_max == 0.0
    for bad in (dict(threshold=0.0), dict(threshold=float("nan")), dict(factor=0.0), dict(min_separation=-1), dict(box=(15.0, 0, 0))):
        with pytest.raises(MdnoError):
            F.ContactPairs.native(x, **{"threshold": 8.0, **bad})
    with pytest.raises(MdnoError, match="ONE frame"):
        F.ContactPairs.native(x[None])
    nat.check_frames(6)
    with pytest.raises(MdnoError, match="built for frames of 6"):
        nat.check_frames(7)


def test_pairs_of_and_from_statistics():
    cp = F.ContactPairs.of([[0, 1], [2, 2], [0, 1]], [7.0, 0.0, 9.0])
    assert cp.cut_max == 9.0 and cp.top == 2 and cp.n_atoms is None and cp.cut.dtype == torch.float64
    cp.check_frames(3)
    with pytest.raises(MdnoError):
        cp.check_frames(2)
    assert F.ContactPairs.of([[0, 1]], 8).to("cpu").cut.tolist() == [8.0]
    for pairs, cut, kw in (([[0, 1]], [1.0, 2.0], {}), ([[0, -1]], 8.0, {}), ([[0, 5]], 8.0, dict(n_atoms=5)), ([[0, 1]], float("nan"), {}),
                           ([[0, 1]], -1.0, {}), ([[0, 1]], 0.0, {}), ([[0, 1, 2]], 8.0, {}), ([[0.5, 1.0]], 8.0, {})):
        with pytest.raises(MdnoError):
            F.ContactPairs.of(pairs, cut, **kw)
    n = 5
    count = torch.zeros((2, 1, n, n), dtype=torch.int32)          # two blocks of 4 frames: the total decides
    count[0, 0, 0, 3] = count[0, 0, 3, 0] = 4
    count[1, 0, 0, 4] = count[1, 0, 4, 0] = 3
    count[:, 0, 1, 4] = count[:, 0, 4, 1] = 2
    count[:, 0, 0, 2] = count[:, 0, 2, 0] = 4
    st = F.PairStatistics(count, None, None, torch.tensor([4, 4]), 7.5)
    got = F.ContactPairs.from_statistics(st)
    assert got.pairs.tolist() == [[0, 3], [1, 4]] and got.cut.tolist() == [7.5, 7.5] and got.n_atoms == n          # (0, 2) is too near
    assert F.ContactPairs.from_statistics(st, 0.375, 2).pairs.tolist() == [[0, 2], [0, 3], [0, 4], [1, 4]]
    assert len(F.ContactPairs.from_statistics(st, 1.01)) == 0
    with pytest.raises(MdnoError, match="expected one"):
        F.ContactPairs.from_statistics(F.PairStatistics.cat([st, st]))


# ================================================================================================ refusals, no device work
def test_every_refusal_happens_on_the_host():
    x = torch.zeros((4, 2, 3, 3))
    with pytest.raises(MdnoError, match="CPU tensor"):
        F.pair_statistics(x)
    with pytest.raises(MdnoError, match="CPU tensor"):
        ops.pair_statistics(x, 8.0)
    pairs = F.ContactPairs.of([[0, 1]], 8.0)
    with pytest.raises(MdnoError, match="CPU tensor"):
        F.contact_series(x, pairs)
    with pytest.raises(MdnoError, match="CPU tensor"):
        ops.contact_bits(x, pairs.pairs, pairs.cut, 8.0)
    with pytest.raises(MdnoError, match="CPU tensor"):
        ops.contact_correlation(torch.zeros((2, 1, 1), dtype=torch.int64), 4, [0])
    for bad in (x[0], x[..., :2], x[None]):                       # wrong ranks and a last axis that is not 3
        with pytest.raises(MdnoError):
            ops.pair_statistics(bad, 8.0)
        with pytest.raises(MdnoError):
            F.contact_series(bad, pairs)
    for block_len in (0, -1, 1.5, True):
        with pytest.raises(MdnoError, match="block_len"):
            F.pair_statistics(x, block_len=block_len)
    for threshold in (0.0, -1.0, float("inf"), float("nan"), "a"):
        with pytest.raises(MdnoError, match="threshold"):
            F.pair_statistics(x, threshold)
    with pytest.raises(MdnoError, match="2 \\* cutoff"):
        F.pair_statistics(x, 8.0, box=(15.9, 0.0, 0.0))
    with pytest.raises(MdnoError, match="2 \\* cutoff"):
        ops.contact_bits(x, pairs.pairs, pairs.cut, 9.0, box=(17.0, 0.0, 0.0))          # the box is held to cut_max
    with pytest.raises(MdnoError, match="contact_pairs is a"):
        F.contact_series(x, [[0, 1]])
    with pytest.raises(MdnoError, match="built for frames"):
        F.contact_series(x, F.ContactPairs.of([[0, 3]], 8.0))
    cs = F.ContactSeries(torch.zeros((2, 1, 1), dtype=torch.int64), torch.zeros((4, 2), dtype=torch.int32), 4, pairs)
    for lags in ([4], [-1], [0, 5], [0.5], list(range(4)) * 300):
        with pytest.raises(MdnoError, match="lag"):
            cs.correlation(lags)
        with pytest.raises(MdnoError, match="lag"):
            ops.check_contact_lags(lags, 4)
    assert ops.check_contact_lags(torch.tensor([0, 3]), 4) == [0, 3] and ops.check_contact_lags([], 4) == []
    with pytest.raises(MdnoError, match="CPU tensor"):
        cs.correlation()                                          # default lags pass, then the bits are on the host
    assert ops.check_contact_args(8, (16.0, 0.0, 0.0), 64) == (8.0, (16.0, 0.0, 0.0), 64)
    assert ops.check_contact_args(8.0, (0.0, 0.0, 0.0)) == (8.0, None, 1)
