"""Internal coordinates on the device (include/mdno_internal.h; csrc/internal.hip) against the numpy restatement
(tests/internal_ref.py: the header's fp64 operations in the header's order).

Gates:
    default mode   BIT-EQUAL to the restatement in f64 output, bit-equal to its value rounded once in f32 output, in both
                   forms and between them: the rule uses + - x / sqrt rint only, each correctly rounded, in a fixed order,
                   without contraction.  (A NaN equals a NaN: the sign and payload of an invalid operation's result are not
                   the rule's.)
    radians mode   |angle - longdouble acos / atan2 of the restatement's own fp64 c / (y, x)| in units of
                   2^-52 max(|angle|, 1).  No bound for fp64 acos / atan2 is documented in the installed ROCm; measured on
                   the first run on an MI355X, the largest over the four cases: acos 0.593, atan2 1.074.  The gate is twice
                   the larger, RADIANS_GATE.
    histogram      counts and n_nan exactly.
Shapes are sized from the header's constants (workgroup 256, IC_LDS_ATOMS, IC_FRAMES_PER_GROUP, IC_FEATURE_CHUNK,
IC_HIST_ROWS / TABLE / COLUMNS), none is the workload's own."""
import math

import numpy as np
import pytest
import torch

import internal_ref as ref

pytestmark = pytest.mark.gpu

WG, LDS_ATOMS, GROUP_MAX, CHUNK = 256, 2048, 16, 8192
RADIANS_GATE = 2 * 1.074         # see the module docstring


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def on(dev, x):
    return torch.from_numpy(np.array(x, order="C")).to(dev)                # (a copy: the shared inputs are read-only)


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    """Bit-equal, a NaN matching any NaN."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    view = np.int64 if got.dtype == np.float64 else np.int32
    return bool(np.all((got.view(view) == want.view(view)) | (np.isnan(got) & np.isnan(want))))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and same_bits(a.cpu().numpy(), b.cpu().numpy())


def tuples(rng, n, width, N):
    """n index tuples of distinct atoms (where N allows it)."""
    if n == 0:
        return np.zeros((0, width), np.int32)
    if N < width:
        return rng.integers(0, N, size=(n, width)).astype(np.int32)
    first = rng.integers(0, N, size=(n, 1))
    steps = np.stack([rng.choice(np.arange(1, N), size=width - 1, replace=False) for _ in range(n)]) if N <= 64 else \
        np.cumsum(rng.integers(1, (N - 1) // (width - 1) + 1, size=(n, width - 1)), 1)
    return np.concatenate([first, (first + steps) % N], 1).astype(np.int32)


def case(N, F, P, A, T, seed):
    rng = np.random.default_rng(seed)
    frames = (rng.normal(size=(F, N, 3)) * 3.0).astype(np.float32)
    return frames, tuples(rng, P, 2, N), tuples(rng, A, 3, N), tuples(rng, T, 4, N)


def forms_of(N):
    return ("lds", "global") if N <= LDS_ATOMS else ("global",)


def run(dev, frames, pairs, triples, quads, **kw):
    from molecular_dynamics_neural_operator_amd import ops
    dp, dt, dq = (on(dev, a) if a is not None and len(a) else None for a in (pairs, triples, quads))
    return ops.internal_features(on(dev, frames), dp, dt, dq, **kw)


def check_case(dev, frames, pairs, triples, quads, box=None):
    """Both forms, both output types, against the restatement; returns the f64 result of the automatic form."""
    N = frames.shape[1]
    want = ref.features(frames, pairs, triples, quads, box)
    with np.errstate(over="ignore"):
        want32 = want.astype(np.float32)
    outs = []
    for form in forms_of(N) + ("auto",):
        got = run(dev, frames, pairs, triples, quads, box=box, dtype=torch.float64, form=form)
        got32 = run(dev, frames, pairs, triples, quads, box=box, dtype=torch.float32, form=form)
        assert got.shape == want.shape == got32.shape and got.dtype == torch.float64 and got32.dtype == torch.float32
        g, g32 = got.cpu().numpy(), got32.cpu().numpy()
        bad = np.argwhere(~((g.view(np.int64) == want.view(np.int64)) | (np.isnan(g) & np.isnan(want))))
        assert same_bits(g, want), (form, len(bad), bad[:4].tolist(), [(g[tuple(b)], want[tuple(b)]) for b in bad[:4]])
        assert same_bits(g32, want32), form
        outs.append(got)
    assert all(same(outs[0], o) for o in outs[1:])
    return outs[-1]


def test_header_constants():
    from molecular_dynamics_neural_operator_amd import ops
    assert (ops.IC_WORKGROUP, ops.IC_LDS_ATOMS, ops.IC_MAX_GROUP_FRAMES, ops.IC_FEATURE_CHUNK) == (WG, LDS_ATOMS, GROUP_MAX, CHUNK)
    assert ops.ic_frames_per_group(28) == GROUP_MAX and ops.ic_frames_per_group(504) == 4
    assert ops.ic_frames_per_group(LDS_ATOMS) == 1 == ops.ic_frames_per_group(LDS_ATOMS + 1)


# ================================================================================================ 1. the rule, bit for bit
@pytest.mark.parametrize("N", [1, 4, 5, 28, 63, 64, 65, 504, LDS_ATOMS, LDS_ATOMS + 1])
def test_features_equal_the_restatement_at_every_size(dev, N):
    """All three kinds, counts around the workgroup size, three frames (more than one group at the large N, a part of one
    at the small)."""
    frames, pairs, triples, quads = case(N, 3, WG + 1, WG - 1, WG, seed=N)
    out = check_case(dev, frames, pairs, triples, quads)
    assert out.shape == (3, 4 * WG)
    if N >= 4:
        assert not bool(torch.isnan(out).any())


@pytest.mark.parametrize("F", [0, 1, 2, GROUP_MAX - 1, GROUP_MAX, GROUP_MAX + 1])
def test_features_equal_the_restatement_at_every_frame_count(dev, F):
    from molecular_dynamics_neural_operator_amd import ops
    assert ops.ic_frames_per_group(28) == GROUP_MAX
    frames, pairs, triples, quads = case(28, F, WG + 1, 1, WG - 1, seed=100 + F)
    assert check_case(dev, frames, pairs, triples, quads).shape == (F, (WG + 1) + 1 + 2 * (WG - 1))


@pytest.mark.parametrize("kind", ["pairs", "quads"])
@pytest.mark.parametrize("n", [0, 1, WG - 1, WG, WG + 1])
def test_features_equal_the_restatement_at_every_count(dev, kind, n):
    frames, pairs, triples, quads = case(65, 3, n if kind == "pairs" else 0, 0, n if kind == "quads" else 0, seed=200 + n)
    assert check_case(dev, frames, pairs, triples, quads).shape == (3, n if kind == "pairs" else 2 * n)


def test_features_across_an_item_chunk(dev):
    """More index tuples than one workgroup owns: the chunk boundary falls among the quads, whose columns are pairs."""
    frames, pairs, triples, quads = case(65, GROUP_MAX + 1, CHUNK - 3, 1, 5, seed=300)
    assert check_case(dev, frames, pairs, triples, quads).shape == (GROUP_MAX + 1, CHUNK - 3 + 1 + 10)


# ================================================================================================ 2. radians
@pytest.mark.parametrize("N,seed", [(5, 1), (28, 2), (65, 3), (LDS_ATOMS + 1, 4)])
def test_radians_against_long_double(dev, N, seed):
    frames, pairs, triples, quads = case(N, 5, 3, WG + 1, WG + 1, seed=400 + seed)
    h_min, c_max = ref.conditioning(frames, triples, quads)
    assert h_min > 1e-6 and c_max < 1.0 - 1e-9, f"the input is near a singular geometry: h ratio {h_min}, |c| {c_max}"
    want = ref.radians_longdouble(frames, pairs, triples, quads)
    outs = [run(dev, frames, pairs, triples, quads, radians=True, dtype=torch.float64, form=form) for form in forms_of(N)]
    assert all(same(outs[0], o) for o in outs[1:])
    got = outs[0].cpu().numpy()
    assert got.shape == want.shape == (5, 3 + 2 * (WG + 1))
    assert same_bits(got[:, :3], want[:, :3].astype(np.float64))                       # distances are the rule's own
    err = np.abs(got.astype(np.longdouble) - want) / (np.longdouble(2.0) ** -52 * np.maximum(np.abs(want), 1.0))
    a, t = float(err[:, 3:3 + WG + 1].max()), float(err[:, 3 + WG + 1:].max())
    print(f"radians N={N}: acos {a:.3f}, atan2 {t:.3f} (units of 2^-52 max(|angle|, 1)); gate {RADIANS_GATE}")
    assert a <= RADIANS_GATE and t <= RADIANS_GATE
    assert float(np.abs(got[:, 3 + WG + 1:]).max()) > 2.0 and float(got[:, 3 + WG + 1:].min()) < -2.0    # the whole circle
    # f32 output: the same fp64 value rounded once
    got32 = run(dev, frames, pairs, triples, quads, radians=True, dtype=torch.float32)
    assert same_bits(got32.cpu().numpy(), got.astype(np.float32))


# ================================================================================================ 3. periodic boxes
@pytest.mark.parametrize("box", [(9.0, 9.0, 9.0), (9.0, 0.0, 7.5), (6.25, 11.0, 8.0)])
def test_features_under_a_box(dev, box):
    rng = np.random.default_rng(int(sum(box) * 4))
    N, F = 65, 3
    L = np.array([l if l > 0 else 9.0 for l in box])
    frames = (rng.random(size=(F, N, 3)) * L).astype(np.float32)
    near = rng.random(size=(F, N, 3)) < 0.3                                            # atoms a hair inside opposite faces
    frames = np.where(near, np.where(rng.random(size=(F, N, 3)) < 0.5, np.float32(1e-3), (L - 1e-3).astype(np.float32)), frames).astype(np.float32)
    frames[0, 0], frames[0, 1] = (0.0, 0.0, 0.0), (L / 2).astype(np.float32)           # exactly half a box apart: rint ties to even
    _, pairs, triples, quads = case(N, F, WG + 1, WG - 1, WG, seed=17)
    pairs[0] = (0, 1)
    out = check_case(dev, frames, pairs, triples, quads, box=box)
    free = check_case(dev, frames, pairs, triples, quads, box=None)
    assert not same(out, free)                                                         # (the box did something)
    P = len(pairs)
    limit = math.sqrt(sum((l / 2) ** 2 if l > 0 else 9.0 ** 2 for l in box))
    assert float(out[:, :P].max()) <= limit * (1 + 1e-6)                               # minimum images
    # an all-open box is no box
    assert same(run(dev, frames, pairs, triples, quads, box=(0.0, 0.0, 0.0), dtype=torch.float64), free)
    assert same(run(dev, frames, pairs, triples, quads, box=(0.0, 0.0, 0.0), dtype=torch.float64, form="global"), free)


# ================================================================================================ 4. degenerate input
def test_degenerate_and_non_finite_input_touch_their_own_features_only(dev):
    N, F = 28, GROUP_MAX + 1
    frames, pairs, triples, quads = case(N, F, 40, 40, 40, seed=500)
    base = check_case(dev, frames, pairs, triples, quads).cpu().numpy()
    assert not np.isnan(base).any()
    names = [("p", i) for i in range(40)] + [("a", i) for i in range(40)] + [("t", i // 2) for i in range(80)]
    cols = lambda kind, i: [c for c, n in enumerate(names) if n == (kind, i)]

    def others_unchanged(out, touched):
        keep = np.ones(base.shape[1], bool)
        keep[touched] = False
        return same_bits(out[:, keep], base[:, keep])

    # i == j, a zero-length bond, three collinear atoms (the same atom twice), indices -1 and N
    p2, t2, q2 = pairs.copy(), triples.copy(), quads.copy()
    p2[3] = (7, 7)
    t2[5] = (2, 9, 9)
    q2[11] = (4, 4, 8, 12)
    p2[20], t2[21], q2[22], q2[23] = (-1, 3), (1, 2, N), (N, 1, 2, 3), (5, 6, 7, -1)
    out = check_case(dev, frames, p2, t2, q2).cpu().numpy()
    assert (out[:, cols("p", 3)] == 0.0).all() and not np.signbit(out[:, cols("p", 3)]).any()
    for kind, i in (("a", 5), ("t", 11), ("p", 20), ("a", 21), ("t", 22), ("t", 23)):
        assert np.isnan(out[:, cols(kind, i)]).all(), (kind, i)
    touched = sum((cols(k, i) for k, i in (("p", 3), ("a", 5), ("t", 11), ("p", 20), ("a", 21), ("t", 22), ("t", 23))), [])
    assert len(touched) == 10 and others_unchanged(out, touched)
    # three distinct collinear atoms, exactly (equal bond vectors of a few bits): j, k, l along a general direction (n2 = 0),
    # and i, j, k along an axis (n1 = 0, and b1 . n2 is formed without rounding)
    i, j, k, l = quads[0]
    step = np.array([0.5, 1.25, -0.75], np.float32)
    line = frames.copy()
    line[:, j] = (1.0, -2.0, 0.5)
    line[:, k], line[:, l] = line[:, j] + step, line[:, j] + 2 * step
    out = check_case(dev, line, pairs, triples, quads).cpu().numpy()
    assert np.isnan(out[:, cols("t", 0)]).all()
    line = frames.copy()
    line[:, i] = (1.0, -2.0, 0.5)
    line[:, j], line[:, k] = line[:, i] + np.float32([1.5, 0, 0]), line[:, i] + np.float32([3.0, 0, 0])
    out = check_case(dev, line, pairs, triples, quads).cpu().numpy()
    assert np.isnan(out[:, cols("t", 0)]).all()
    # a NaN and an Inf in one coordinate each, in one frame each: the features that touch the atom, in that frame, no others
    for value, frame, atom in ((np.nan, 2, 13), (np.inf, GROUP_MAX, 0), (-np.inf, 0, N - 1)):
        bad = frames.copy()
        bad[frame, atom, 1] = value
        out = check_case(dev, bad, pairs, triples, quads).cpu().numpy()
        hit = [c for c, (kind, i) in enumerate(names) if atom in {"p": pairs, "a": triples, "t": quads}[kind][i]]
        assert hit and len(hit) < base.shape[1]
        rows = np.arange(F) != frame
        assert same_bits(out[rows], base[rows])                                        # the other frames, every column
        keep = np.ones(base.shape[1], bool)
        keep[hit] = False
        assert same_bits(out[frame, keep], base[frame, keep])                          # this frame, the other columns
        assert not np.isfinite(out[frame, hit]).any()                                  # (an Inf gives Inf distances, NaN elsewhere)


def _run_guarded(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import ops
    res = []
    with Guard(fill, record_calls=False) as G:
        for N, F, form in ((28, GROUP_MAX + 1, "lds"), (65, 3, "global"), (LDS_ATOMS, 2, "lds"), (LDS_ATOMS + 1, 2, "auto")):
            frames, pairs, triples, quads = case(N, F, WG + 1, 7, WG - 1, seed=600 + N)
            pairs[0], quads[1] = (-1, N), (0, 1, 2, N)                                   # out-of-range indices read nothing
            args = [G.place(on(dev, a)) for a in (frames, pairs, triples, quads)]
            for dtype in (torch.float32, torch.float64):
                for radians in (False, True):
                    res.append(ops.internal_features(*args, box=(9.0, 0.0, 7.0), radians=radians, dtype=dtype, form=form).clone())
        for R, D, bins in ((1000, 17, 7), (ops.IC_HIST_ROWS + 1, 3, ops.IC_MAX_BINS), (5, ops.IC_HIST_COLUMNS + 1, 2)):
            x = np.random.default_rng(R).normal(size=(R, D)).astype(np.float32)
            res += [t.clone() for t in ops.column_histogram(G.place(on(dev, x)), -1.0, 1.0, bins)]
        G.verify()
    return res


def test_internal_entry_points_stay_inside_their_buffers(dev):
    """Every input and output inside guard bands under both fill bytes (tests/guarded.py): every band intact, and every
    result identical under 0x00 and 0xFF — nothing unset is read, an out-of-range index included."""
    from guarded import FILLS
    a, b = (_run_guarded(dev, fill) for fill in FILLS)
    assert len(a) == len(b) == 4 * 4 + 3 * 2
    for i, (u, v) in enumerate(zip(a, b)):
        assert same(u, v) if u.is_floating_point() else torch.equal(u, v), i


# ================================================================================================ 5. independence
def test_a_feature_depends_on_its_frame_and_its_tuple_alone(dev):
    N, F = 28, 2 * GROUP_MAX + 3
    frames, pairs, triples, quads = case(N, F, WG + 1, WG - 1, WG, seed=700)
    full = run(dev, frames, pairs, triples, quads, dtype=torch.float64)
    for f in (0, GROUP_MAX - 1, GROUP_MAX, F - 1):                                     # a frame alone or inside a batch
        for form in ("lds", "global"):
            assert same(run(dev, frames[f:f + 1], pairs, triples, quads, dtype=torch.float64, form=form), full[f:f + 1])
    # a tuple wherever it stands: reversed lists, and alone
    rev = run(dev, frames, pairs[::-1], triples[::-1], quads[::-1], dtype=torch.float64)
    P, A, T = len(pairs), len(triples), len(quads)
    assert same(rev[:, :P].flip(1), full[:, :P]) and same(rev[:, P:P + A].flip(1), full[:, P:P + A])
    assert same(rev[:, P + A:].reshape(F, T, 2).flip(1).reshape(F, 2 * T), full[:, P + A:])
    alone = run(dev, frames, None, None, quads[WG - 1:WG], dtype=torch.float64)
    assert same(alone, full[:, P + A + 2 * (WG - 1):P + A + 2 * WG])
    alone = run(dev, frames, pairs[7:8], triples[9:10], None, dtype=torch.float64, form="global")
    assert same(alone, torch.stack([full[:, 7], full[:, P + 9]], 1))
    # [S, M, N, 3] is the flat stack, reshaped
    from molecular_dynamics_neural_operator_amd import forecast
    ft = forecast.Featurizer.of(pairs, triples, quads, n_atoms=N).to(dev)
    sm = forecast.internal_coordinates(on(dev, frames[:2 * GROUP_MAX]).reshape(GROUP_MAX, 2, N, 3), ft, dtype=torch.float64)
    assert sm.shape == (GROUP_MAX, 2, ft.dim()) and same(sm.reshape(2 * GROUP_MAX, -1), full[:2 * GROUP_MAX])
    cpu_ft = forecast.Featurizer.of(pairs, triples, quads, n_atoms=N)                  # indices still on the host: moved
    assert same(forecast.internal_coordinates(on(dev, frames), cpu_ft, dtype=torch.float64), full)


def test_engines_equal_the_free_function(dev):
    """A noisy 4-step, 8-member, N = 28 run under a box and without: both engines' internal_coordinates equal
    forecast.internal_coordinates on the gathered produced(...) frames bit for bit; the trajectory buffer is unchanged."""
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
    ft = forecast.Featurizer.backbone(28).to(dev)
    for cls in (RolloutEngine, GroupedRolloutEngine):
        for box in (None, (40.0, 40.0, 0.0)):
            eng = cls(model, 8, 28, 3, 8.0, max_steps=4, device=dev, noise_sigma=0.05, noise_seed=7, box=box)
            eng.run(wins, aa, 4)
            before = eng.frames().clone()
            for first, steps in ((0, None), (1, 2)):
                n = 4 - first if steps is None else steps
                produced = eng.produced(first, n).contiguous()
                for radians, dtype in ((False, torch.float32), (True, torch.float64)):
                    want = forecast.internal_coordinates(produced, ft, box=box, radians=radians, dtype=dtype)
                    got = eng.internal_coordinates(ft, radians=radians, dtype=dtype, first_step=first, steps=steps)
                    assert got.shape == (n, 8, ft.dim(radians)) and same(got, want), (cls.__name__, box, first)
            assert torch.equal(eng.frames(), before)
            eng.close()


# ================================================================================================ 6. column histogram
@pytest.mark.parametrize("D", [1, 17])
@pytest.mark.parametrize("n_bins", [1, 2, 4096])
@pytest.mark.parametrize("R", [0, 1, 1000])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_column_histogram_equals_the_restatement(dev, D, n_bins, R, dtype):
    from molecular_dynamics_neural_operator_amd import ops
    rng = np.random.default_rng(1000 * D + n_bins + R)
    lo = (rng.normal(size=D) - 2.0).round(3)
    hi = lo + np.abs(rng.normal(size=D)) + 2.0
    x = rng.normal(size=(R, D)) * 2.0
    edges = lo + (hi - lo) * rng.integers(0, n_bins + 1, size=(R, D)) / n_bins         # on lo, on hi and on bin edges
    pick = rng.random(size=(R, D))
    x = np.where(pick < 0.2, edges, x)
    x = np.where((pick >= 0.2) & (pick < 0.3), np.nan, x)
    x = np.where((pick >= 0.3) & (pick < 0.33), np.inf, x)
    x = np.where((pick >= 0.33) & (pick < 0.36), -np.inf, x)
    if R:
        x[0, :] = lo
        x[-1, :] = hi
        x[R // 2, :] = np.nextafter(hi, -np.inf)                                       # the rounding case b == n_bins
    x = x.astype(np.float32 if dtype == "f32" else np.float64)
    for shared in (False, True):
        l, h = (float(lo[0]), float(hi[0])) if shared else (lo.tolist(), hi.tolist())
        want_c, want_n = ref.column_histogram(x, l if shared else lo, h if shared else hi, n_bins)
        counts, n_nan = ops.column_histogram(on(dev, x), l, h, n_bins)
        assert counts.shape == (D, n_bins + 2) and counts.dtype == torch.int64 and n_nan.shape == (D,)
        assert np.array_equal(counts.cpu().numpy(), want_c) and np.array_equal(n_nan.cpu().numpy(), want_n)
        assert bool((counts.sum(1) + n_nan == R).all())


def test_column_histogram_across_row_blocks_column_tiles_and_launches(dev):
    from molecular_dynamics_neural_operator_amd import forecast, ops
    rng = np.random.default_rng(9)
    for R, D, n_bins in ((ops.IC_HIST_ROWS + 1, 3, 100), (7, ops.IC_HIST_COLUMNS + 1, 5), (2 * ops.IC_HIST_ROWS + 5, 65, 127),
                         (33, 2, ops.IC_HIST_TABLE // 2 - 2), (33, 3, ops.IC_HIST_TABLE // 2 - 1)):
        x = rng.normal(size=(R, D)).astype(np.float32)
        lo = np.linspace(-2.0, -1.0, D)
        hi = np.linspace(1.0, 3.0, D)
        want_c, want_n = ref.column_histogram(x, lo, hi, n_bins)
        counts, n_nan = ops.column_histogram(on(dev, x), lo.tolist(), hi.tolist(), n_bins)
        assert np.array_equal(counts.cpu().numpy(), want_c) and np.array_equal(n_nan.cpu().numpy(), want_n), (R, D, n_bins)
    # groups of columns that share their ranges, across the columns of one launch
    G, D = 3, ops.IC_HIST_COLUMNS + 1
    x = rng.normal(size=(50, G * D)).astype(np.float32)
    lo, hi = np.linspace(-2.0, -1.0, D), np.linspace(1.0, 3.0, D)
    counts, n_nan = ops.column_histogram(on(dev, x), lo.tolist(), hi.tolist(), 9, groups=G)
    want_c, want_n = ref.column_histogram(x, np.tile(lo, G), np.tile(hi, G), 9)
    assert np.array_equal(counts.cpu().numpy(), want_c) and np.array_equal(n_nan.cpu().numpy(), want_n)
    # forecast.feature_histograms: [S, M, D] is per member
    x = rng.normal(size=(50, 3, 4)).astype(np.float32)
    lo, hi = [-1.0, -2.0, -0.5, 0.0], [1.0, 2.0, 0.5, 3.0]
    h = forecast.feature_histograms(on(dev, x), lo, hi, 6)
    assert h.counts.shape == (3, 4, 8) and h.n_nan.shape == (3, 4)
    for m in range(3):
        assert np.array_equal(h.counts[m].cpu().numpy(), ref.column_histogram(x[:, m], lo, hi, 6)[0])
    flat = forecast.feature_histograms(on(dev, x[:, 1]), lo, hi, 6)
    assert torch.equal(flat.counts, h.counts[1]) and float(h.total_variation(flat)[1].max()) == 0.0
    assert h.outside().shape == (3, 4) and float(h.outside()[:, 0].min()) > 0.1
    got_lo, got_hi = forecast.feature_ranges(on(dev, x))
    assert got_lo == x.reshape(-1, 4).min(0).astype(np.float64).tolist()
    assert got_hi == [math.nextafter(float(v), math.inf) for v in x.reshape(-1, 4).max(0)]
    inside = forecast.feature_histograms(on(dev, x), got_lo, got_hi, 6)
    assert float(inside.outside().max()) == 0.0


# ================================================================================================ 7. end to end
BOND = 3.8
HINGES = (9, 18)                     # the pseudo-dihedrals (i - 3, i - 2, i - 1, i) that hop
BASINS = (1.0, -2.0)                 # radians


def hopping_chain(S, M, N, seed):
    """A chain of N sites with bond length 3.8 and fixed pseudo-angles whose pseudo-dihedrals HINGES hop, each on its own,
    between the two BASINS with probability 0.1 per step; nothing else moves, so the run visits four conformations.
    -> (f64 [S, M, N, 3] centred per frame, basin of every hinge i8 [S, M, 2])."""
    rng = np.random.default_rng(seed)
    state = np.zeros((S, M, 2), np.int8)
    for t in range(1, S):
        state[t] = np.where(rng.random((M, 2)) < 0.1, 1 - state[t - 1], state[t - 1])
    theta = np.broadcast_to(1.9 + 0.1 * np.sin(np.arange(N)), (S, M, N))
    phi = np.broadcast_to(-1.0 + 0.5 * np.cos(1.7 * np.arange(N)), (S, M, N)).copy()
    for h, i in enumerate(HINGES):
        phi[:, :, i] = np.where(state[:, :, h] == 0, BASINS[0], BASINS[1])
    x = np.zeros((S, M, N, 3))
    x[:, :, 1] = (BOND, 0.0, 0.0)
    x[:, :, 2, 0] = BOND - BOND * np.cos(theta[:, :, 2])
    x[:, :, 2, 1] = BOND * np.sin(theta[:, :, 2])
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    for i in range(3, N):
        a, b, c = x[:, :, i - 3], x[:, :, i - 2], x[:, :, i - 1]
        bc = unit(c - b)
        n = unit(np.cross(b - a, bc))
        m = np.cross(n, bc)
        th, ph = theta[:, :, i, None], phi[:, :, i, None]
        x[:, :, i] = c + BOND * (-np.cos(th) * bc + np.sin(th) * np.cos(ph) * m + np.sin(th) * np.sin(ph) * n)
    return x - x.mean(2, keepdims=True), state


def random_rotations(n, seed):
    rng = np.random.default_rng(seed)
    q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    return q * np.sign(np.linalg.det(q))[:, None, None]


def end_to_end_case(seed=3):
    """(truth f32 [S, M, N, 3], the same frames each turned by its own random rotation about its centroid, basins, the
    restatement's features of the truth f64 [S M, 428], the bound per column).  First-order bounds with
    X = max |coordinate| < 64: a coordinate rounded to fp32 is off by <= 2^-24 X, a bond-vector component by <= 2^-23 X, a
    distance by <= sqrt(3) 2^-23 X, and between the two rounded sets by twice that: dd.  A bond direction turns by
    <= dd / 3.8 between the sets; the cosine of an angle moves by <= 2 of those, a plane normal turns by <= 2 / sin(angle) of
    them and a dihedral by two normals' worth, <= 4 / sin_min; da = 6 dd / 3.8 / sin_min bounds every unitless column."""
    from molecular_dynamics_neural_operator_amd.forecast import Featurizer
    S, M, N = 200, 2, 28
    x, state = hopping_chain(S, M, N, seed)
    rot = random_rotations(S * M, seed + 1).reshape(S, M, 3, 3)
    truth = x.astype(np.float32)
    turned = np.einsum("smij,smnj->smni", rot, x).astype(np.float32)
    X = float(max(np.abs(truth).max(), np.abs(turned).max()))
    assert X < 64.0
    ft = Featurizer.backbone(N)
    P, A = ft.pairs.shape[0], ft.triples.shape[0]
    want = ref.features(truth.reshape(-1, N, 3), ft.pairs.tolist(), ft.triples.tolist(), ft.quads.tolist())
    sin_min = float(np.sqrt(1.0 - want[:, P:P + A] ** 2).min())
    assert sin_min > 0.8 and float(want[:, :N - 1].min()) > BOND - 1e-4
    dd = 2.0 * math.sqrt(3.0) * 2.0 ** -23 * X
    da = 6.0 * dd / (BOND - 1e-4) / sin_min
    assert dd < 3e-5 and da < 1e-4
    return truth, turned, state, want, np.concatenate([np.full(P, dd), np.full(ft.dim() - P, da)]), ft


def test_end_to_end_a_rotated_run_is_the_same_run(dev):
    """N = 28, S = 200, M = 2: the truth hops between the two basins of two pseudo-dihedrals, the run is the truth with every
    frame turned by a different random rotation.  Its internal coordinates are the truth's to first order (end_to_end_case
    has the bounds), its per-column histograms are the truth's, and a discretization of the truth in internal coordinates
    gives it the truth's labels — none of which holds for its Cartesian coordinates."""
    from molecular_dynamics_neural_operator_amd import forecast
    truth, turned, state, want, tol, ft = end_to_end_case()
    S, M, N = truth.shape[:3]
    P, A = ft.pairs.shape[0], ft.triples.shape[0]
    for h in range(2):                                                                 # both basins of both hinges, several hops
        assert 20 < state[..., h].sum() < S * M - 20 and (np.abs(np.diff(state[..., h], axis=0)).sum(0) >= 4).all()
    ft = ft.to(dev)
    f_truth = forecast.internal_coordinates(on(dev, truth), ft, dtype=torch.float64)
    f_run = forecast.internal_coordinates(on(dev, turned), ft, dtype=torch.float64)
    assert f_truth.shape == (S, M, 428) and same_bits(f_truth.cpu().numpy().reshape(-1, 428), want)
    diff = (f_run - f_truth).abs().reshape(-1, 428).max(0).values.cpu().numpy()
    print(f"end to end: largest |run - truth| / bound = {float((diff / tol).max()):.3f} (bounds {tol[0]:.2e}, {tol[-1]:.2e})")
    assert (diff <= tol).all() and float(diff.max()) > 0.0
    for h, i in enumerate(HINGES):                                                     # sin t (i-3)-(i-2)-(i-1)-i tells the basin
        s = f_run[:, :, P + A + 2 * (i - 3) + 1].cpu().numpy()
        assert ((s > 0.5) == (state[..., h] == 0)).all() and ((s < -0.5) == (state[..., h] == 1)).all()

    # three bins over the truth's range widened by 100 bounds; no truth value lies within two bounds of an edge (asserted
    # on the restatement), so no value of the run falls into another bin: total variation exactly 0
    lo, hi = want.min(0) - 100 * tol, want.max(0) + 100 * tol
    for e in (1, 2):
        assert (np.abs(want - (lo + (hi - lo) * e / 3)) > 2 * tol).all(), "a truth value sits on a bin edge: choose another seed"
    h_truth = forecast.feature_histograms(f_truth.to(torch.float32), lo.tolist(), hi.tolist(), 3)
    h_run = forecast.feature_histograms(f_run.to(torch.float32), lo.tolist(), hi.tolist(), 3)
    assert h_truth.counts.shape == (M, 428, 5) and int(h_truth.counts.sum()) == S * M * 428 and int(h_truth.n_nan.sum()) == 0
    assert np.array_equal(h_truth.counts.sum(0).cpu().numpy(), ref.column_histogram(want.astype(np.float32), lo, hi, 3)[0])
    assert float(h_run.total_variation(h_truth).max()) == 0.0 and float(h_run.outside().max()) == 0.0
    pooled = forecast.FeatureHistograms(h_truth.counts.sum(0), h_truth.n_nan.sum(0), lo, hi)
    assert float(h_run.total_variation(pooled).max()) > 0.01                           # (the members differ from their pool)

    # states: k-centres in the internal coordinates; the near-tie assertion of the Markov tests on the truth's dist2 gaps
    disc = forecast.discretize(on(dev, truth), 4, featurizer=ft)
    assert disc.reference is None and disc.n_states == 4 and disc.centres.shape == (4, 428) and disc.featurizer is ft
    a_truth, a_run = disc.assign(on(dev, truth)), disc.assign(on(dev, turned))
    c = disc.centres.cpu().numpy().astype(np.float64)
    rows = want.astype(np.float32).astype(np.float64)
    d2 = ((rows[:, None, :] - c[None]) ** 2).sum(-1)
    order = np.sort(d2, 1)
    shift = float(np.sqrt((tol ** 2).sum())) + math.sqrt(428.0) * 2.0 ** -24 * 64.0   # how far a row of the run lies from the
    bound = 2.0 * np.sqrt(order[:, :2]) * shift + shift ** 2                          # truth's (f32 rows); its effect on a d2
    gap = (order[:, 1] - order[:, 0]) / bound.sum(1)
    assert gap.min() > 2.0, f"the truth has a near-tie: gap / bounds = {gap.min()}"
    labels = a_truth.labels.cpu().numpy()
    assert np.array_equal(labels.reshape(-1), d2.argmin(1)) and a_run.labels.shape == (S, M)
    assert torch.equal(a_run.labels, a_truth.labels)
    conformation = state[..., 0] + 2 * state[..., 1]
    assert len(set(zip(labels.reshape(-1).tolist(), conformation.reshape(-1).tolist()))) == 4      # a state per conformation
    assert float(a_run.outside(disc.radius + shift).max()) == 0.0 and float(disc.radius) < 1e-3
    # the Cartesian path with a fixed reference is what it was: superpose -> k-centres -> assign, bit for bit
    reference = on(dev, truth[0, 0])
    cart = forecast.discretize(on(dev, truth), 4, reference=reference)
    aligned = forecast.superpose(on(dev, truth), reference)[0].reshape(S * M, 3 * N)
    centres = forecast.kcenters(aligned, 4)[0]
    assert cart.featurizer is None and cart.box is None and cart.reference is reference and same(cart.centres, centres)
    assert torch.equal(cart.assign(on(dev, truth)).labels.reshape(-1), forecast.assign(aligned, centres).labels)

