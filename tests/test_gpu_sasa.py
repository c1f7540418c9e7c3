"""Shrake-Rupley counts on the device (include/mdno_surface.h, csrc/surface.hip) against the numpy
fp64 restatement of the header's rule (tests/sasa_ref.py).  Every operation of the rule is an IEEE operation rounded once and
"buried" is an OR, so there is no tolerance anywhere in this file: the counts are EQUAL, in both kernel forms."""
import functools

import numpy as np
import pytest
import torch

import sasa_ref as R

pytestmark = pytest.mark.gpu

CAP = 2048          # MDNOSA_STAGED_ATOMS
PROBE = 1.4
FORMS = ("auto", "lds", "tiled")
DENSITY = 0.002     # atoms per cubic A of the gas: e^(-905 * 0.002) = 16 % of its atoms have no neighbour within 6 A


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib, ops
    _lib.load()
    assert ops.SA_STAGED_ATOMS == CAP and ops.SA_MAX_POINTS == 1024
    return torch.device("cuda:0")


def on(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def radii(N, seed):
    """Expanded radii: van der Waals radii drawn from 1.2 .. 2.0, plus the probe, one fp64 add each."""
    return np.random.default_rng(seed).uniform(1.2, 2.0, size=N) + PROBE


def blob_and_gas(F, N, seed, span):
    """F frames of N atoms: a gas uniform in [-0.2 L, 1.3 L) per axis, L = span[a] / 1.5, whose first N // 3 atoms (24 at the
    most) are a blob inside a ball of radius 2 A instead — its inner atoms are covered from every side (count 0), the lone
    atoms of the gas see nobody (count P) and those with a neighbour or two lie between."""
    rng = np.random.default_rng(seed)
    span = np.asarray(span, dtype=np.float64)
    x = (rng.random((F, N, 3)) * 1.5 - 0.2) * (span / 1.5)
    nb = min(N // 3, 24)
    if nb:
        u = rng.normal(size=(F, nb, 3))
        u *= (2.0 * rng.random((F, nb, 1)) ** (1.0 / 3.0)) / np.linalg.norm(u, axis=-1, keepdims=True)
        x[:, :nb] = x[:, :1] + u
    return x.astype(np.float32)


def case_box(kind, N, reach):
    """(box, span of the atoms per axis): no box, a cubic one at the gas density, or a slab whose two periodic axes are
    EXACTLY 2 * reach (the least the box check admits) and whose open axis is long enough for the same density."""
    cube = max((N / DENSITY) ** (1.0 / 3.0), 2.0 * reach)
    if kind == "open":
        return None, (cube,) * 3
    if kind == "cubic":
        return (cube,) * 3, (1.5 * cube,) * 3
    edge = 2.0 * reach
    return (edge, edge, 0.0), (1.5 * edge, 1.5 * edge, max(N / (DENSITY * edge * edge), 2.0 * reach))


@functools.lru_cache(maxsize=None)
def reference_case(N, P, kind):
    """(frames f32 [3, N, 3], R, U, box, counts of the restatement) — computed once, never changed."""
    Rr = radii(N, 100 + N)
    reach = 2.0 * float(Rr.max())
    box, span = case_box(kind, N, reach)
    x = blob_and_gas(3, N, 7 * N + P + len(kind), span)
    U = R.golden_spiral(P)
    counts, m_point, m_pair = R.exposed_points(x, Rr, U, box)
    return x, Rr, U, box, reach, counts, m_point, m_pair


def device_counts(dev, x, Rr, U, box=None, reach=None, form="auto"):
    from molecular_dynamics_neural_operator_amd import ops
    got = ops.exposed_points(on(dev, x), on(dev, Rr), on(dev, U), box=box, reach=2.0 * float(np.max(Rr)) if reach is None else reach,
                             form=form)
    assert got.dtype == torch.int32 and got.shape == x.shape[:-1]
    return got.cpu().numpy()


# ================================================================================================ 1. equal to the restatement
PAIRS = [(1, 96), (2, 1), (63, 64), (64, 65), (65, 1024), (129, 96), (257, 960), (513, 96)]


@pytest.mark.parametrize("kind", ["open", "cubic", "slab"])
@pytest.mark.parametrize("N,P", PAIRS)
def test_counts_equal_the_restatement(dev, N, P, kind):
    x, Rr, U, box, reach, want, m_point, m_pair = reference_case(N, P, kind)
    # what the restatement alone must show before the device is asked: no comparison near its boundary, every kind of atom
    assert min(m_point, m_pair) >= 1e-9, (m_point, m_pair)
    if kind == "slab":
        assert box[0] == box[1] == 2.0 * reach and box[2] == 0.0
    if N >= 63:
        for f in range(3):
            assert (want[f] == 0).any() and (want[f] == P).any() and ((want[f] > 0) & (want[f] < P)).any(), (f, np.bincount(want[f]))
    if N == 1:
        assert (want == P).all()
    for form in FORMS:
        assert np.array_equal(device_counts(dev, x, Rr, U, box, reach, form), want), (form, "F = 3")
        assert np.array_equal(device_counts(dev, x[:1], Rr, U, box, reach, form), want[:1]), (form, "F = 1")


# ================================================================================================ 2. exact by construction
AXES = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])


@pytest.mark.parametrize("form", FORMS)
def test_cases_that_are_exact_by_construction(dev, form):
    """Custom point tables and coordinates whose every product and sum is exact in fp64, so the strict tests sit ON their
    boundaries and the expected rows are written out by hand."""
    # R_i = 3 at the origin, R_j = 4 at (3, 4, 0), distance 5 < 7: neighbours.  The points of atom 0 are (+-3, 0, 0),
    # (0, +-3, 0), (0, 0, +-3); e = q - d and t = |e|^2 against 16:
    #   (3, 0, 0): (0, -4, 0) 16, NOT < 16: exposed      (-3, 0, 0): (-6, -4, 0) 52: exposed
    #   (0, 3, 0): (-3, -1, 0) 10: buried                (0, -3, 0): (-3, -7, 0) 58: exposed
    #   (0, 0, +-3): (-3, -4, +-3) 34: exposed
    # The points of atom 1 are 4 * axes, d = (-3, -4, 0), against 9:
    #   (4, 0, 0): (7, 4, 0) 65   (-4, 0, 0): (-1, 4, 0) 17   (0, 4, 0): (3, 8, 0) 73   (0, -4, 0): (3, 0, 0) 9, NOT < 9
    #   (0, 0, +-4): (3, 4, +-4) 41                       -> all six exposed
    x = np.array([[[0.0, 0, 0], [3.0, 4.0, 0]]], dtype=np.float32)
    got = device_counts(dev, x, np.array([3.0, 4.0]), AXES, form=form)
    assert got.tolist() == [[5, 6]]
    assert R.exposed_points(x, np.array([3.0, 4.0]), AXES)[0].tolist() == [[5, 6]]
    # two atoms of R = 2.5 at distance exactly 5 (3-4-5): sqrt(25) = 5 is NOT < 5, they are not neighbours, and the point
    # 2.5 * (0.6, 0.8, 0) of the first, which touches the second's centre line, is never tested against it
    table = np.concatenate([AXES, [[0.6, 0.8, 0.0]]])
    x = np.array([[[1.0, 1.0, 1.0], [4.0, 5.0, 1.0]]], dtype=np.float32)
    assert device_counts(dev, x, np.array([2.5, 2.5]), table, form=form).tolist() == [[7, 7]]
    # half an A closer they are neighbours (s = 22.25), and that point is buried: e = (-1, -2, 0), t = 5 < 6.25
    x[0, 1, 0] = 3.5
    assert device_counts(dev, x, np.array([2.5, 2.5]), table, form=form).tolist() == [[6, 7]]
    # coincident equal atoms: d = 0, t = |q|^2 = R^2 exactly for axis points, NOT < R^2: everything exposed
    x = np.array([[[2.0, -1.0, 0.5]] * 3], dtype=np.float32)
    assert device_counts(dev, x, np.array([2.0, 2.0, 2.0]), AXES, form=form).tolist() == [[6, 6, 6]]
    # a small atom deep inside a large one: |q - d| <= 1 + 0.5 < 4: every point buried; the large one sees |4 u + d| >= 3.5 > 1
    x = np.array([[[0.0, 0, 0], [0.5, 0, 0]]], dtype=np.float32)
    assert device_counts(dev, x, np.array([1.0, 4.0]), AXES, form=form).tolist() == [[0, 6]]
    # one atom: P, whatever P
    for P in (1, 64, 65, 1024):
        assert device_counts(dev, x[:, :1], np.array([3.0]), R.golden_spiral(P), form=form).tolist() == [[P]]


# ================================================================================================ 3. long lists, large N
@functools.lru_cache(maxsize=None)
def crowd():
    """300 atoms inside a ball of radius 2 A (every one a neighbour of every other: 299 > any chunk) and 5 far away."""
    rng = np.random.default_rng(5)
    u = rng.normal(size=(2, 300, 3))
    u *= (2.0 * rng.random((2, 300, 1)) ** (1.0 / 3.0)) / np.linalg.norm(u, axis=-1, keepdims=True)
    far = 50.0 * (1.0 + np.arange(5))[None, :, None] * np.ones((2, 1, 3))
    x = np.concatenate([u + 10.0, far + 10.0], axis=1).astype(np.float32)
    x = x[:, np.random.default_rng(6).permutation(305)]           # the far ones anywhere in the walk
    Rr = radii(305, 8)
    U = R.golden_spiral(96)
    return x, Rr, U, R.exposed_points(x, Rr, U)


@pytest.mark.parametrize("form", FORMS)
def test_a_neighbour_list_longer_than_any_chunk(dev, form):
    x, Rr, U, (want, m_point, m_pair) = crowd()
    assert min(m_point, m_pair) >= 1e-9 and (want == 96).sum() == 10 and (want == 0).any() and ((want > 0) & (want < 96)).any()
    assert np.array_equal(device_counts(dev, x, Rr, U, form=form), want)


@functools.lru_cache(maxsize=None)
def above_the_cap():
    N = CAP + 1
    Rr = radii(N, 9)
    side = (N / DENSITY) ** (1.0 / 3.0)
    x = blob_and_gas(2, N, 10, (side,) * 3)
    U = R.golden_spiral(96)
    return x, Rr, U, R.exposed_points(x, Rr, U)


@pytest.mark.parametrize("form", ["auto", "tiled"])
def test_one_atom_above_the_staging_cap_goes_through_the_global_form(dev, form):
    from molecular_dynamics_neural_operator_amd import MdnoError
    x, Rr, U, (want, m_point, m_pair) = above_the_cap()
    assert min(m_point, m_pair) >= 1e-9 and (want == 0).any() and (want == 96).any()
    assert np.array_equal(device_counts(dev, x, Rr, U, form=form), want)
    with pytest.raises(MdnoError, match="staged form holds at most 2048"):
        device_counts(dev, x, Rr, U, form="lds")
    assert np.array_equal(device_counts(dev, x[:, :CAP], Rr[:CAP], U, form="lds"), device_counts(dev, x[:, :CAP], Rr[:CAP], U, form="tiled"))


# ================================================================================================ 4. non-finite atoms
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", ["open", "cubic"])
def test_a_nan_or_inf_atom_gets_minus_one_and_is_nobodys_neighbour(dev, kind, form):
    x, Rr, U, box, reach, want, _, _ = reference_case(129, 96, kind)
    x = x.copy()
    bad = {0: (3, 0, np.nan), 1: (70, 2, np.inf), 2: (128, 1, -np.inf)}          # frame -> (atom, component, value)
    for f, (i, a, v) in bad.items():
        x[f, i, a] = v
    got = device_counts(dev, x, Rr, U, box, reach, form)
    assert np.array_equal(got, R.exposed_points(x, Rr, U, box)[0])
    for f, (i, _, _) in bad.items():
        keep = np.arange(129) != i
        assert got[f, i] == -1 and (got[f, keep] >= 0).all()
        alone = device_counts(dev, x[f:f + 1, keep], Rr[keep], U, box, reach, form)
        assert np.array_equal(got[f, keep], alone[0])              # exactly the frame with that atom deleted


# ================================================================================================ 5. invariances
@pytest.mark.parametrize("form", FORMS)
def test_invariances_are_exact(dev, form):
    rng = np.random.default_rng(11)
    N, P, L = 129, 96, 32.0
    x = rng.integers(0, int(L * 16), size=(3, N, 3)).astype(np.float32) / 16.0          # multiples of 2^-4 in [0, 32)
    x[:, :24] = x[:, :1] + rng.integers(-24, 25, size=(3, 24, 3)).astype(np.float32) / 16.0
    Rr = radii(N, 12)
    U = R.golden_spiral(P)
    box = (L, L, L)
    base = device_counts(dev, x, Rr, U, box, form=form)
    assert (base == 0).any() and (base == P).any() and np.array_equal(base, R.exposed_points(x, Rr, U, box)[0])
    moved = x + (L * rng.integers(-3, 4, size=(3, N, 3))).astype(np.float32)            # whole box vectors, exact in fp32
    assert np.array_equal(device_counts(dev, moved, Rr, U, box, form=form), base)
    perm = rng.permutation(N)
    assert np.array_equal(device_counts(dev, x[:, perm], Rr[perm], U, box, form=form), base[:, perm])
    assert np.array_equal(device_counts(dev, x, Rr, U[rng.permutation(P)], box, form=form), base)
    for f in range(3):
        assert np.array_equal(device_counts(dev, x[f:f + 1], Rr, U, box, form=form)[0], base[f])


# ================================================================================================ 6. identity with what exists
@pytest.mark.parametrize("kind", ["open", "cubic"])
def test_an_atom_is_covered_somewhere_only_if_the_contact_map_gives_it_a_neighbour(dev, kind):
    from molecular_dynamics_neural_operator_amd import ops
    x, _, U, _, _, _, _, _ = reference_case(257, 960, kind)
    Rone = 1.7 + PROBE
    box, _ = case_box(kind, 257, 2.0 * Rone)
    counts = ops.exposed_points(on(dev, x), torch.full((257,), Rone, dtype=torch.float64, device=dev), on(dev, U), box=box, reach=2.0 * Rone)
    maps = ops.contact_maps(on(dev, x), 2.0 * Rone, box=box)       # sqrt(s) < 2 R: the neighbour test at one radius
    has_neighbour = (maps.sum(-1) - maps.diagonal(dim1=-2, dim2=-1)) > 0
    assert bool((~(counts < 960) | has_neighbour).all())          # covered somewhere -> an off-diagonal 1 in its row
    assert bool((counts[~has_neighbour] == 960).all()) and bool((~has_neighbour).any()) and bool((counts < 960).any())


# ================================================================================================ 7. entry points
def test_leading_dimensions_and_the_classes(dev):
    from molecular_dynamics_neural_operator_amd import forecast
    x, Rr, U, box, reach, want, _, _ = reference_case(65, 1024, "cubic")
    sp = forecast.Spheres(Rr - PROBE, probe=PROBE, n_points=1024)
    assert np.array_equal(sp.R.numpy(), (Rr - PROBE) + PROBE) and np.array_equal(sp.points.numpy(), U)
    Rr2 = sp.R.numpy()                                             # ((R - p) + p may differ from R in the last bit)
    want2 = R.exposed_points(x, Rr2, U, box)[0]
    frames = on(dev, np.stack([x, x[::-1]], axis=1))               # [S = 3, M = 2, N, 3]
    area = forecast.surface_area(frames, sp, box=box)
    assert area.counts.shape == (3, 2, 65) and area.counts.dtype == torch.int32 and area.n_points == 1024
    assert np.array_equal(area.counts[:, 0].cpu().numpy(), want2) and np.array_equal(area.counts[:, 1].cpu().numpy(), want2[::-1])
    assert sp.to(dev) is sp.to(dev) and area.R.device.type == "cuda"
    per_atom = area.per_atom().cpu().numpy()
    assert np.array_equal(per_atom[:, 0], (4.0 * np.pi) * (Rr2 * Rr2) * (want2.astype(np.float64) / 1024.0))
    assert area.total().shape == (3, 2) and area.mean().shape == (2, 65) and area.difference(area).tolist() == [0.0, 0.0]
    flat = forecast.surface_area(frames.reshape(6, 65, 3), sp, box=box)
    assert torch.equal(flat.counts.reshape(3, 2, 65), area.counts)
    none = forecast.surface_area(frames[:0], sp, box=box)
    assert none.counts.shape == (0, 2, 65)


def test_engines_equal_the_free_function_in_their_own_box(dev):
    """A noisy 4-step, 8-member, N = 28 run without a box and under one that folds the chain onto itself: both engines'
    surface_area equals the stand-alone call on the frames() bit for bit, in the engine's own box, and a grouped engine's
    result is that of one engine holding every member."""
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
    sp = forecast.Spheres(radii(28, 3) - PROBE, probe=PROBE)       # reach <= 6.8: a box of 16 passes
    results = {}
    for box in (None, (16.0, 16.0, 0.0)):
        for cls in (RolloutEngine, GroupedRolloutEngine):
            eng = cls(model, 8, 28, 3, 8.0, max_steps=4, device=dev, noise_sigma=0.05, noise_seed=7, box=box)
            eng.run(wins, aa, 4)
            before = eng.frames().clone()
            want = forecast.surface_area(eng.frames().contiguous(), sp, box=box)
            got = eng.surface_area(sp)
            assert got.counts.shape == (4, 8, 28) and torch.equal(got.counts, want.counts) and got.n_points == 96
            part = eng.surface_area(sp, first_step=1, steps=2)
            assert torch.equal(part.counts, want.counts[1:3])
            results[(box, cls.__name__)] = (before, got.counts.clone())
            assert torch.equal(eng.frames(), before)
            eng.close()
    for box in (None, (16.0, 16.0, 0.0)):
        (fu, cu), (fg, cg) = results[(box, "RolloutEngine")], results[(box, "GroupedRolloutEngine")]
        assert torch.equal(fu, fg) and torch.equal(cu, cg)
    open_frames, open_counts = results[(None, "RolloutEngine")]
    boxed = forecast.surface_area(open_frames, sp, box=(16.0, 16.0, 0.0))
    assert not torch.equal(boxed.counts, open_counts)             # the box matters on this chain, so "its own box" is a statement


# ================================================================================================ 8. guard bands
def _run_guarded(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import ops
    res = []
    with Guard(fill, record_calls=False) as G:
        for N, P, F in ((1, 1, 2), (5, 65, 1), (65, 96, 3), (257, 1024, 2), (CAP + 1, 64, 1)):
            side = max((N / DENSITY) ** (1.0 / 3.0), 14.0)
            x = G.place(on(dev, blob_and_gas(F, N, N + P, (side,) * 3)))
            Rr, U = G.place(on(dev, radii(N, N))), G.place(on(dev, R.golden_spiral(P)))
            for box in (None, (0.0, side, side)):
                for form in (("tiled",) if N > CAP else ("lds", "tiled")):
                    counts = ops.exposed_points(x, Rr, U, box=box, reach=6.8, form=form)          # counts (and any workspace): guarded
                    res.append(counts.clone())
        G.verify()
    return res


def test_the_entry_point_stays_inside_its_buffers_and_writes_every_count(dev):
    """mdnosa_exposed_points inside guard bands under both fill bytes and in both forms: every band intact, and every count
    equal under both fills (nothing unset is read, every element is written: 0xFF would leave -1 and 0x00 a 0)."""
    from guarded import FILLS
    a, b = (_run_guarded(dev, fill) for fill in FILLS)
    assert len(a) == len(b) == 4 * 4 + 2
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v) and bool((u >= 1).any()), i       # (finite frames: no -1 of the kernel's own; lone atoms: P >= 1)


# ================================================================================================ 9. refusals
def test_refusals_come_before_any_launch(dev):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import MdnoError, _lib, ops
    x, Rr, U = on(dev, blob_and_gas(2, 5, 1, (20.0,) * 3)), on(dev, radii(5, 1)), on(dev, R.golden_spiral(8))
    with Guard(0xFF, record_calls=False) as G:
        for kw in (dict(box=(13.5, 0.0, 0.0), reach=6.8), dict(form="global"), dict(reach=0.0), dict(reach=float("nan")),
                   dict(points=on(dev, np.zeros((1025, 3)))), dict(points=on(dev, np.zeros((0, 3)))), dict(points=U.float()),
                   dict(R=Rr[:4]), dict(R=Rr.float()), dict(R=Rr.cpu()), dict(points=U.cpu())):
            args = {"R": Rr, "points": U, "reach": 6.8, **kw}
            with pytest.raises(MdnoError):
                ops.exposed_points(x, args.pop("R"), args.pop("points"), **args)
        lib = _lib.load()
        counts = torch.empty((2, 5), dtype=torch.int32, device=dev)          # guarded: a refused call writes nothing
        head = (x.data_ptr(), 2, 5, Rr.data_ptr(), U.data_ptr())
        tail = (counts.data_ptr(), 0, None, 0, torch.cuda.current_stream().cuda_stream)
        import ctypes
        small = (ctypes.c_double * 3)(13.5, 0.0, 0.0)
        for call in ((*head, 0, None, 6.8, *tail), (*head, 1025, None, 6.8, *tail), (*head, 8, None, 0.0, *tail),
                     (*head, 8, None, float("inf"), *tail), (*head, 8, small, 6.8, *tail),
                     (*head, 8, None, 6.8, counts.data_ptr(), 3, None, 0, tail[-1]), (x.data_ptr(), -1, 5, *head[3:], 8, None, 6.8, *tail),
                     (None, 2, 5, *head[3:], 8, None, 6.8, *tail), (*head[:4], None, 8, None, 6.8, *tail),
                     (*head, 8, None, 6.8, None, *tail[1:])):
            assert lib.mdnosa_exposed_points(*call) == _lib.EINVAL, call
        assert lib.mdnosa_exposed_points(None, 0, 5, None, None, 8, None, 6.8, None, 0, None, 0, tail[-1]) == _lib.OK      # F == 0
        assert lib.mdnosa_workspace_bytes(2, 5, 8, 0) == 0
        G.untouched()
        G.verify()
