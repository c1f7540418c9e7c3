"""Dynamical scoring without a GPU: what is particular to include/mdno_dynamics.h and its ctypes table (that header,
table and exports agree is tests/test_cabi_tables.py's); every refusal of the header comes back as MDNO_EINVAL, or is raised as MdnoError,
before any device work; the workspace sizes are monotone; the numpy restatement of the rules (tests/dynamics_ref.py) has
the properties the GPU tests lean on; and the arithmetic of forecast.DisplacementStats holds against closed forms."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import dynamics_ref as ref
from cabi import CSRC, INCLUDE, lib  # noqa: F401  (lib: the fixture)

HEADER = INCLUDE / "mdno_dynamics.h"
NAMES = {"mdno_displacement_stats_workspace_bytes", "mdno_displacement_stats", "mdno_velocity_autocorrelation_workspace_bytes",
         "mdno_velocity_autocorrelation", "mdno_unwrap_frames"}
BAD_BOXES = [(-1.0, 20.0, 20.0), (20.0, float("nan"), 20.0), (20.0, 20.0, float("inf")), (-0.5, 0.0, 0.0)]
FAKE = 0x10000          # a made-up address: nothing may dereference it
BIG = 1 << 30


def box3(*v):
    return (C.c_double * 3)(*v)


def lag_array(*v):
    return (C.c_int32 * len(v))(*v)


def test_dynamics_header_table_and_exports_agree(lib):
    """What is particular to this header; that header, table and exports agree is tests/test_cabi_tables.py's."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    assert set(_lib.DYNAMICS_SIGNATURES) == NAMES
    assert lib.mdno_abi_version() == 15 == _lib.ABI_VERSION and lib.mdno_train_abi_version() == 1          # additive: both stay
    assert (CSRC / "dynamics.hip").exists()                                            # inside the library's content hash
    text = HEADER.read_text()
    assert int(re.search(r"#define MDNO_DYN_ORIGIN_CHUNK (\d+)", text).group(1)) == ops.DYNAMICS_ORIGIN_CHUNK
    assert int(re.search(r"#define MDNO_DYN_ATOM_TILE (\d+)", text).group(1)) == ops.DYNAMICS_ATOM_TILE


def disp(lib, frames=FAKE, S=10, M=2, N=5, lags=(0, 1, 9), n_lags=None, stride=1, com=0, r_max=4.0, n_bins=7, sum2=FAKE,
         sum4=FAKE, counts=FAKE, ws=FAKE, ws_bytes=BIG):
    arr = lag_array(*lags) if lags is not None else None
    return lib.mdno_displacement_stats(frames, S, M, N, arr, len(lags) if n_lags is None else n_lags, stride, com, r_max,
                                       n_bins, sum2, sum4, counts, ws, ws_bytes, None)


def vacf(lib, frames=FAKE, S=10, M=2, N=5, lags=(0, 1, 8), n_lags=None, stride=1, com=0, corr=FAKE, ws=FAKE, ws_bytes=BIG):
    arr = lag_array(*lags) if lags is not None else None
    return lib.mdno_velocity_autocorrelation(frames, S, M, N, arr, len(lags) if n_lags is None else n_lags, stride, com, corr,
                                             ws, ws_bytes, None)


def unwrap(lib, frames=FAKE, S=4, M=2, N=5, box=(16.0, 16.0, 0.0), out=FAKE + (1 << 20)):
    return lib.mdno_unwrap_frames(frames, S, M, N, box3(*box) if box is not None else None, out, None)


def test_entry_points_refuse_before_device_work(lib):
    """No pointer below is a device pointer: a call that got as far as a launch would fault, not return a code."""
    from molecular_dynamics_neural_operator_amd import _lib
    E = _lib.EINVAL
    err = lib.mdno_last_error
    # lags
    assert disp(lib, lags=(0, 10)) == E and b"lag[1] = 10" in err()                      # a lag >= S
    assert disp(lib, lags=(-1, 2)) == E and b"lag[0] = -1" in err()                      # a negative lag
    assert vacf(lib, lags=(0, 9)) == E and b"lag[1] = 9" in err()                        # velocities: S - 2 at most
    assert vacf(lib, lags=(-3,)) == E and b"lag[0]" in err()
    assert vacf(lib, S=1, lags=(0,)) == E and b"lag[0]" in err()                         # no velocity from one frame
    for f in (disp, vacf):
        assert f(lib, stride=0) == E and b"origin_stride" in err()
        assert f(lib, stride=-2) == E and b"origin_stride" in err()
        assert f(lib, lags=(0,), n_lags=0) == E and b"n_lags" in err()
        assert f(lib, lags=(0,) * 1025) == E and b"n_lags=1025" in err()
        assert f(lib, lags=None, n_lags=2) == E and b"lags" in err()
        assert f(lib, S=-1) == E and f(lib, M=-1) == E and f(lib, N=-1) == E
        assert f(lib, frames=None) == E and b"null pointer" in err()
        assert f(lib, M=65536) == _lib.EUNSUPPORTED and b"grid" in err()
    assert disp(lib, S=0, lags=(0,) * 1024) == 0 and disp(lib, S=0, lags=(0,) * 1025) == E          # 1,024 lags are allowed
    # histogram arguments
    for n_bins in (-1, 4097, 1 << 20):
        assert disp(lib, n_bins=n_bins) == E and b"n_bins" in err(), n_bins
    for r_max in (0.0, -4.0, float("nan"), float("inf")):
        assert disp(lib, r_max=r_max) == E and b"r_max" in err(), r_max
    # null outputs
    assert disp(lib, sum2=None) == E and b"null pointer" in err()
    assert disp(lib, sum4=None) == E and b"null pointer" in err()
    assert disp(lib, counts=None) == E and b"null pointer" in err()
    assert vacf(lib, corr=None) == E and b"null pointer" in err()
    # a short or missing workspace
    need = lib.mdno_displacement_stats_workspace_bytes(10, 2, 5, 3, 7)
    assert need > 0
    assert disp(lib, ws_bytes=need - 1) == E and b"workspace" in err()
    assert disp(lib, ws=None) == E and b"workspace" in err()
    need = lib.mdno_velocity_autocorrelation_workspace_bytes(10, 2, 5, 3)
    assert need > 0 and vacf(lib, ws_bytes=need - 1) == E and b"workspace" in err()
    assert vacf(lib, ws=None) == E
    # nothing to do: no frame is looked at, whatever the pointers (the arguments are still checked first)
    for f in (disp, vacf):
        for kw in ({"S": 0}, {"M": 0}):
            assert f(lib, **kw) == 0
            assert f(lib, frames=None, lags=(5, 77), ws=None, ws_bytes=0, **kw) == 0
            assert f(lib, stride=0, **kw) == E and f(lib, lags=(0,), n_lags=0, **kw) == E
    assert disp(lib, S=0, sum2=None, sum4=None, counts=None) == 0 and disp(lib, S=0, n_bins=4097) == E
    assert vacf(lib, M=0, corr=None) == 0
    # unwrap
    for bad in BAD_BOXES:
        assert unwrap(lib, box=bad) == E and b"box[" in err(), bad
    assert unwrap(lib, box=None) == E and b"null box" in err()
    assert unwrap(lib, frames=None) == E and b"null pointer" in err()
    assert unwrap(lib, out=None) == E and b"null pointer" in err()
    assert unwrap(lib, out=FAKE) == E and b"overlaps" in err()                           # out == frames
    assert unwrap(lib, out=FAKE + 8) == E and b"overlaps" in err()                       # or any part of it
    assert unwrap(lib, S=-1) == E and unwrap(lib, N=-1) == E
    for kw in ({"S": 0}, {"M": 0}, {"N": 0}):
        assert unwrap(lib, frames=None, out=None, **kw) == 0
        assert unwrap(lib, box=(-1.0, 0.0, 0.0), **kw) == E


def test_workspace_bytes_are_monotone(lib):
    base = dict(S=100, M=4, N=300, n_lags=9, n_bins=64)
    d = lib.mdno_displacement_stats_workspace_bytes
    v = lib.mdno_velocity_autocorrelation_workspace_bytes
    b0 = d(*base.values())
    assert b0 >= 100 * 4 * 3 * 8 + 4 * 9 * 2 * 2 * 2 * 8                  # the centroids and one partial pair per (m, l, chunk, tile)
    for key in base:
        prev = 0
        for scale in (1, 2, 3, 7, 40):
            args = dict(base)
            args[key] = base[key] * scale
            cur = d(*args.values())
            assert cur >= prev and cur >= b0, (key, scale)
            prev = cur
            if key != "n_bins":
                va = [args[k] for k in ("S", "M", "N", "n_lags")]
                assert 0 < v(*va) <= cur
    assert d(0, 4, 300, 9, 64) == 0 and d(100, 0, 300, 9, 64) == 0 and d(100, 4, 0, 9, 0) > 0
    # the stated size suffices for every stride and lag: the most partials a lag can have is at stride 1, lag 0
    from molecular_dynamics_neural_operator_amd import ops
    chunks = -(-100 // ops.DYNAMICS_ORIGIN_CHUNK)
    tiles = -(-300 // ops.DYNAMICS_ATOM_TILE)
    assert b0 >= 100 * 4 * 3 * 8 + 4 * 9 * chunks * tiles * 2 * 8


def test_python_arguments_are_checked_without_a_device():
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    x = torch.zeros(6, 2, 5, 3)
    for call in (lambda: ops.displacement_stats(x, [0, 1]), lambda: forecast.displacement_stats(x),
                 lambda: ops.velocity_autocorrelation(x, [0, 1]), lambda: forecast.velocity_autocorrelation(x),
                 lambda: ops.unwrap_frames(x, (16.0, 16.0, 16.0)), lambda: forecast.unwrap(x, (16.0, 0.0, 0.0))):
        with pytest.raises(MdnoError, match="CPU tensor"):
            call()
    for lags in ([6], [-1], [0, 2.5], [], list(range(1025)), "ab"):
        with pytest.raises(MdnoError, match="lag"):
            ops.check_lags(lags, 6)
    with pytest.raises(MdnoError, match="lag 5"):
        ops.check_lags([0, 5], 6, 1, "velocity_autocorrelation")
    assert ops.check_lags(torch.tensor([0, 5]), 6) == [0, 5] and ops.check_lags(range(3), 6) == [0, 1, 2]
    for stride in (0, -1, 1.5, "x"):
        with pytest.raises(MdnoError, match="origin_stride"):
            ops.check_origin_stride(stride)
    for bad in BAD_BOXES + [(20.0, 20.0), "abc", None]:
        with pytest.raises(MdnoError, match="box"):
            ops.unwrap_frames(x, bad)
    assert [ops.n_origins(10, t) for t in (0, 1, 9, 10)] == [10, 9, 1, 0]
    assert [ops.n_origins(10, t, 3) for t in (0, 1, 2, 3, 9)] == [4, 3, 3, 3, 1]
    assert ops.n_origins(10, 8, 1, 1) == 1 and ops.n_origins(10, 9, 1, 1) == 0
    for S in (1, 2, 3, 4, 40, 130, 1000, 100000):
        lags = forecast.default_lags(S)
        assert lags[0] == 0 and lags == sorted(set(lags)) and lags[-1] == max((S - 1) // 2, 0) and len(lags) <= 34
        assert forecast.default_lags(S, 1)[-1] == max((S - 2) // 2, 0)
    assert len(forecast.default_lags(1000)) >= 28 and forecast.default_lags(1000)[:4] == [0, 1, 2, 3]


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_properties():
    """Lag 0, a rigid translation, the velocity identity, non-finite coordinates, hand-made bins."""
    import test_gpu_dynamics as T
    x = T.walk(40, 65)
    lags = [0, 1, 7, 39]
    for com in (False, True):
        for stride in (1, 3):
            st = ref.displacement_stats(x, lags, stride, com, 4.0, 64)
            assert st.n_samples.tolist() == [ref.n_origins(40, t, stride) * 65 for t in lags]
            assert not st.sum2[:, 0].any() and not st.sum4[:, 0].any()              # lag 0: zero displacement
            assert (st.counts[:, 0, 0] == st.n_samples[0]).all() and not st.counts[:, 0, 1:].any()
            assert not st.gate2[:, 0].any() and (st.gate2[:, 1:] > 0).all() and (st.gate2 < 1e-9 * np.maximum(st.sum2, 1)).all()
            assert (st.counts.sum(-1) <= st.n_samples[None]).all() and st.beyond > 0
            assert st.beyond == int((st.n_samples[None] - st.counts.sum(-1)).sum())
            assert np.isfinite(st.margin) and st.margin > 0
    # a rigid translation by an integer vector per frame: exact, and exactly zero once the centroid's motion is removed
    x0 = np.random.default_rng(3).integers(0, 32, size=(1, 2, 8, 3))          # (8 atoms: the centroid is exact)
    v = np.array([1, -2, 3])
    rigid = (x0 + np.arange(12)[:, None, None, None] * v).astype(np.float32)
    st = ref.displacement_stats(rigid, [0, 1, 5], 1, False, 16.0, 16)
    for l, tau in enumerate([0, 1, 5]):
        n = (12 - tau) * 8
        assert (st.sum2[:, l] == n * tau * tau * 14).all() and (st.sum4[:, l] == n * (tau * tau * 14) ** 2).all()
    assert (st.counts[:, 1, 3] == 11 * 8).all()                                      # sqrt(14) = 3.74: bin 3 of width 1
    assert st.counts[:, 2].sum() == 0                                                # 5 sqrt(14) = 18.7 >= r_max
    zero = ref.displacement_stats(rigid, [0, 1, 5], 1, True, 16.0, 16)
    assert not zero.sum2.any() and not zero.sum4.any() and (zero.counts[:, :, 0] == zero.n_samples[None]).all()
    # corr at lag 0 is sum2 at lag 1: the same terms
    for com in (False, True):
        corr, gate, ns = ref.velocity_autocorrelation(x, [0, 1, 38], 1, com)
        one = ref.displacement_stats(x, [1], 1, com)
        assert np.array_equal(corr[:, 0], one.sum2[:, 0]) and ns[0] == one.n_samples[0] and ns[2] == 65
        assert (np.abs(corr[:, 1]) < corr[:, 0]).all() and (gate > 0).all()
    # one atom with its centroid removed does not move
    st = ref.displacement_stats(T.walk(20, 1), [1, 5], 1, True, 4.0, 8)
    assert not st.sum2.any() and (st.counts[:, :, 0] == st.n_samples[None]).all()
    # a NaN in frame 7 of member 1: exactly the lags with an origin t or t + tau == 7 go non-finite, member 0 and 2 keep
    # their bits, and the counts lose exactly the samples that touch it
    bad = x.copy()
    bad[7, 1, 3, 0] = np.nan
    clean = ref.displacement_stats(x, lags, 3, False, 4.0, 64)
    st = ref.displacement_stats(bad, lags, 3, False, 4.0, 64)
    touched = [any(t == 7 or t + tau == 7 for t in ref.origins(40, tau, 3)) for tau in lags]
    assert touched == [False, True, True, False]
    assert np.isnan(st.sum2[1]).tolist() == touched and np.isnan(st.sum4[1]).tolist() == touched
    assert np.array_equal(st.sum2[[0, 2]], clean.sum2[[0, 2]]) and np.array_equal(st.counts[[0, 2]], clean.counts[[0, 2]])
    lost = clean.counts[1].sum(-1) - st.counts[1].sum(-1)
    assert lost.tolist() == [0, 1, 1, 0]                                             # (both samples lie inside r_max)


def test_restatement_unwrap_returns_the_input_bits():
    """A random walk on the grid 2^-10 in a box of 16: wrapping is exact, steps stay below L / 2, and unwrap returns the walk
    bit for bit; an open axis is a copy; a never-wrapped trajectory is unchanged."""
    rng = np.random.default_rng(5)
    S, M, N, L = 200, 2, 7, 16.0
    x0 = rng.integers(0, 16 * 1024, size=(M, N, 3))
    steps = np.clip(np.rint(rng.normal(0, 1.5, size=(S - 1, M, N, 3)) * 1024), -7 * 1024, 7 * 1024).astype(np.int64)
    grid = np.concatenate([x0[None], x0[None] + np.cumsum(steps, 0)])
    walk = (grid / 1024.0).astype(np.float32)
    assert np.array_equal(walk.astype(np.float64) * 1024.0, grid) and np.abs(walk).max() > 2 * L          # it leaves the box
    for box in ((L, L, L), (L, L, 0.0)):
        w = ref.wrap(walk, box)
        per = [a for a in range(3) if box[a] > 0]
        assert (w[..., per] >= 0).all() and (w[..., per] < L).all() and (w != walk).any()
        back = ref.unwrap(w, box)
        assert np.array_equal(back.view(np.int32), walk.view(np.int32))
    assert np.array_equal(ref.unwrap(ref.wrap(walk, (L, L, L)), (0.0, 0.0, 0.0)), ref.wrap(walk, (L, L, L)))      # open: a copy
    inside = (walk[:5] * 0.01 + 8.0).astype(np.float32)                      # never leaves [0, L), steps far below L / 2
    assert np.array_equal(ref.unwrap(inside, (L, L, L)).view(np.int32), inside.view(np.int32))
    neg = np.array([[[-0.0, 1.0, 2.0]]] * 3, dtype=np.float32)
    assert np.array_equal(ref.unwrap(neg, (L, L, L)).view(np.int32), neg.view(np.int32))


def test_gpu_cases_meet_their_condition():
    """The 120 combinations tests/test_gpu_dynamics.py compares exactly, and its chunk-straddling cases: no sample within
    1e-9 bins of an edge, in the restatement alone; the strict cut at r_max is exercised."""
    import test_gpu_dynamics as T
    worst, cut, n = float("inf"), 0, 0
    for N in T.SIZES:
        for key in T.SHAPES:
            for stride in T.STRIDES:
                for com in (False, True):
                    st = T.expected(N, key, stride, com)[0]
                    worst, cut, n = min(worst, st.margin), cut + (st.beyond > 0), n + 1
    for key in T.CHUNK_SHAPES:
        for N in T.CHUNK_SIZES:
            for stride in T.STRIDES:
                worst = min(worst, T.expected(N, key, stride, True)[0].margin)
    print(f"smallest margin over the {n} GPU cases: {worst} bins; {cut} of them have samples beyond r_max")
    assert n == 120 and worst >= 1e-9 and cut >= 40
    # the chunk cases put origin counts of CHUNK - 1, CHUNK and CHUNK + 1 next to each other
    from molecular_dynamics_neural_operator_amd import ops
    c = ops.DYNAMICS_ORIGIN_CHUNK
    seen = set()
    for key, (S, lags) in T.CHUNK_SHAPES.items():
        for stride in T.STRIDES:
            seen |= {ref.n_origins(S, t, stride) for t in lags} | {ref.n_origins(S, t, stride, 1) for t in lags if t <= S - 2}
    assert {c - 1, c, c + 1} <= seen


# ------------------------------------------------------------------------------------------------ DisplacementStats
def close(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool((np.abs(a - b) <= rel * np.abs(b)).all())


def test_displacement_stats_arithmetic():
    from molecular_dynamics_neural_operator_amd.forecast import DisplacementStats
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    lags = torch.tensor([0, 1, 2, 4])
    n = torch.tensor([40, 30, 20, 10])
    sum2 = torch.tensor([[0.0, 60.0, 80.0, 80.0], [0.0, 3.0, 4.0, 4.0]], dtype=torch.float64)
    sum4 = torch.tensor([[0.0, 200.0, 640.0, 1280.0], [0.0, 0.5, 4.0 / 3.0, 8.0 / 3.0]], dtype=torch.float64)
    counts = torch.tensor([[[40, 0, 0, 0], [10, 10, 5, 5], [0, 0, 10, 10], [0, 0, 0, 5]],
                           [[40, 0, 0, 0], [30, 0, 0, 0], [0, 20, 0, 0], [5, 0, 0, 5]]])
    d = DisplacementStats(sum2, sum4, counts, lags, n, 2.0, 4)
    msd = d.msd()
    assert msd.dtype == torch.float64 and msd.tolist() == [[0.0, 2.0, 4.0, 8.0], [0.0, 0.1, 0.2, 0.4]]
    a2 = d.non_gaussian()
    assert torch.isnan(a2[:, 0]).all()                                                 # <r^2> = 0 at lag 0
    # member 0: <r^4> = 20/3, 32, 128 against <r^2>^2 = 4, 16, 64: alpha_2 = 0, 0.2, 0.2.  member 1: Gaussian, 5/3 <r^2>^2
    assert abs(float(a2[0, 1])) < 1e-15 and close(a2[0, 2:], [0.2, 0.2], 1e-12 * 6)
    assert (a2[1, 1:].abs() < 1e-12).all()
    assert d.edges().tolist() == [0.0, 0.5, 1.0, 1.5, 2.0]
    g = d.van_hove()
    assert g.shape == (2, 4, 4) and close(g[0, 1], [10 / 15, 10 / 15, 5 / 15, 5 / 15]) and close(g[0, 3], [0, 0, 0, 1.0])
    assert close((g * 0.5).sum(-1)[0], [1.0, 1.0, 1.0, 0.5])                          # the fraction below r_max
    tv = d.total_variation(d)
    assert tv.shape == (2, 4) and not tv.any()
    one = DisplacementStats(sum2[1:], sum4[1:], counts[1:], lags, n, 2.0, 4)          # a truth with M = 1 broadcasts
    assert close(d.total_variation(one)[0], [0.0, 2 / 3, 1.0, 0.5]) and not d.total_variation(one)[1].any()
    assert close(one.total_variation(d)[0], [0.0, 2 / 3, 1.0, 0.5])
    for other in (DisplacementStats(sum2, sum4, counts, lags, n, 2.5, 4), DisplacementStats(sum2, sum4, counts[..., :3], lags, n, 2.0, 3),
                  DisplacementStats(sum2[:, :3], sum4[:, :3], counts[:, :3], lags[:3], n[:3], 2.0, 4), counts):
        with pytest.raises(MdnoError, match="same lags, r_max and n_bins"):
            d.total_variation(other)
    # an exactly linear MSD = 6 D tau dt + c: the slope over any slice, whatever the intercept
    D, dt = 0.125, 0.5
    lin = torch.stack([6 * D * dt * lags.double() * n, (6 * 2 * D * dt * lags.double() + 7.0) * n])
    e = DisplacementStats(lin, sum4, None, lags, n)
    assert close(e.diffusion_coefficient(dt), [D, 2 * D]) and close(e.diffusion_coefficient(dt, first=1), [D, 2 * D])
    assert close(e.diffusion_coefficient(dt, 1, 3), [D, 2 * D]) and close(e.diffusion_coefficient(2 * dt), [D / 2, D])
    with pytest.raises(MdnoError, match="a slope needs two"):
        e.diffusion_coefficient(dt, 3)
    for method in (e.van_hove, e.distribution, e.edges):
        with pytest.raises(MdnoError, match="no histogram"):
            method()
    # a lag without samples has no mean
    empty = DisplacementStats(sum2, sum4, counts, lags, torch.tensor([40, 30, 20, 0]), 2.0, 4)
    assert torch.isnan(empty.msd()[:, 3]).all() and torch.isnan(empty.van_hove()[:, 3]).all()
    both = DisplacementStats.cat([d, one])
    assert both.sum2.shape == (3, 4) and torch.equal(both.sum2[2], sum2[1]) and torch.equal(both.counts[2], counts[1])
    assert torch.equal(both.lags, lags) and torch.equal(both.n_samples, n) and (both.r_max, both.n_bins) == (2.0, 4)
    assert DisplacementStats.cat([e, e]).counts is None
    k = d.cpu()
    assert torch.equal(k.sum4, sum4) and torch.equal(k.counts, counts) and (k.r_max, k.n_bins) == (2.0, 4)
    assert math.isclose(float(d.distribution()[0, 1].sum()), 1.0)
