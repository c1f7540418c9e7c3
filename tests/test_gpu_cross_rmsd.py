"""Structural coverage on the device (ops.cross_rmsd, csrc/conformations.hip) against tests/cross_rmsd_ref.py, the numpy
fp64 restatement of include/mdno_conformations.h, under the project's own gate for a superposed rmsd^2,
|matrix^2 - reference| <= 8 * 2^-52 * G (derived in the helper's docstring; it holds for any order of the sums).  The row
and column minima are compared BITWISE with the device's own matrix, and through the gate with the reference.

Shapes: the smallest at which the kernel can go wrong — S and Fb at 1, T - 1, T, T + 1 and 2 T + 1 for the frame tile T of
the header, N at 1 .. 7, 28, C - 1, C, C + 1, 2 C + 1 for the atom chunk C and the workload's 504, one and three members, a
seeded selection with S M != Fb throughout.  Inputs: the rmsd_cases() families of tests/test_gpu_forecast.py stacked so that
every (row, column) has its own expected value — a swapped row and column, or the f32 row map on the f64 MFMA, fails every
off-diagonal element.  Every test prints its largest |d rmsd^2| / (2^-52 G)."""
import functools

import numpy as np
import pytest
import torch

import cross_rmsd_ref as ref

pytestmark = pytest.mark.gpu

T, C = 32, 32               # MDNO_CONF_FRAME_TILE, MDNO_CONF_ATOM_CHUNK (test_header_constants holds them to the header)
EDGES = (1, T - 1, T, T + 1, 2 * T + 1)
ATOMS = (1, 2, 3, 4, 5, 7, 28, C - 1, C, C + 1, 2 * C + 1, 504)


def shapes():
    """One (S, M, N, Fb) per N of ATOMS, S and Fb walking EDGES from a seeded start, M in {1, 3}, S M != Fb."""
    rng = np.random.default_rng(2026)
    out = []
    for i, N in enumerate(ATOMS):
        S, Fb, M = EDGES[(i + int(rng.integers(5))) % 5], EDGES[(2 * i + int(rng.integers(5))) % 5], (1, 3)[i % 2]
        if S * M == Fb:
            Fb = EDGES[(EDGES.index(Fb) + 1) % 5]
        out.append((S, M, N, Fb))
    assert {s[0] for s in out} == set(EDGES) and {s[3] for s in out} == set(EDGES), out
    return out + [(64, 2, 504, 48)]                 # and one workload-shaped case


SHAPES = shapes()
NAMES = ("matrix", "nearest", "nearest_index", "cover", "cover_step")


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def on(dev, x):
    return torch.from_numpy(np.array(x, order="C")).to(dev)                # (a copy: the shared inputs are read-only)


def bits(x):
    return x.contiguous().view(torch.int64) if x.is_floating_point() else x


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def case(S, M, N, Fb):
    """(A, B, kinds of A, kinds of B, reference Result): computed once, shared, never written to."""
    A, B, ka, kb = ref.stacked(S, M, N, Fb, seed=1000 * N + 10 * S + Fb)
    for x in (A, B):
        x.setflags(write=False)
    return A, B, ka, kb, ref.cross_rmsd(A, B)


@functools.lru_cache(maxsize=None)
def device_result(S, M, N, Fb):
    from molecular_dynamics_neural_operator_amd import forecast
    A, B = case(S, M, N, Fb)[:2]
    dev = torch.device("cuda:0")
    return forecast.cross_rmsd(on(dev, A), on(dev, B)).cpu()


def gate_ratio(got, r):
    """(largest |got^2 - reference rmsd^2| / (2^-52 G) over the valid pairs, all inside the gate)."""
    ok = ~np.isnan(r.matrix2)
    assert np.array_equal(np.isnan(got), ~ok)
    d = np.abs(got[ok] ** 2 - r.matrix2[ok])
    G = r.G[ok]
    assert np.all(d[G == 0] == 0)
    ratio = float((d[G > 0] / (ref.U52 * G[G > 0])).max()) if (G > 0).any() else 0.0
    return ratio, bool(np.all(d <= ref.GATE * G))


def test_header_constants():
    from molecular_dynamics_neural_operator_amd import ops
    assert (ops.CONF_FRAME_TILE, ops.CONF_ATOM_CHUNK) == (T, C)


# ================================================================================================ 1. parity
@pytest.mark.parametrize("S,M,N,Fb", SHAPES)
def test_matrix_equals_the_restatement(dev, S, M, N, Fb):
    A, B, ka, kb, r = case(S, M, N, Fb)
    got = device_result(S, M, N, Fb).matrix.numpy()
    assert got.dtype == np.float64 and got.shape == (S, M, Fb) and np.all(got >= 0)
    ratio, inside = gate_ratio(got, r)
    print(f"S={S} M={M} N={N} Fb={Fb}: largest |d rmsd^2| / (2^-52 G) = {ratio:.3f} (allowed 8)")
    assert inside
    # identical frames and the exact rigid copy are within the gate of 0; a mirror image is NOT small
    assert (ka[0][0], kb[0]) == ("identical", "identical") and got[0, 0, 0] ** 2 <= ref.GATE * r.G[0, 0, 0]
    if Fb >= 2:
        assert kb[1] == "rigid copy" and got[0, 0, 1] ** 2 <= ref.GATE * r.G[0, 0, 1]
    if Fb >= 3 and N >= 5:
        assert kb[2] == "mirror image" and got[0, 0, 2] ** 2 * N > 1e-2 * r.G[0, 0, 2]
    # every (row, column) has its own expected value (but column 1, the rigid copy of column 0, which may repeat it): the
    # off-diagonal elements tell a transposed or mis-mapped tile apart
    if N >= 5:
        assert np.unique(r.matrix2).size >= 0.95 * r.matrix2.size


# ================================================================================================ 2. reductions
@pytest.mark.parametrize("S,M,N,Fb", SHAPES)
def test_minima_are_those_of_the_devices_own_matrix(dev, S, M, N, Fb):
    r = case(S, M, N, Fb)[4]
    d = device_result(S, M, N, Fb)
    m = d.matrix.numpy()
    near, near_i = ref.lowest_min(m, 2)
    cover, cover_s = ref.lowest_min(m, 0)
    assert np.array_equal(d.nearest_index.numpy(), near_i) and np.array_equal(d.cover_step.numpy(), cover_s)
    assert d.nearest.numpy().tobytes() == near.tobytes() and d.cover.numpy().tobytes() == cover.tobytes()      # a min is exact
    assert d.nearest_index.dtype == torch.int64 and d.cover_step.dtype == torch.int64
    # against the reference: the frame the device chose is, to the reference, within two gates of its best
    worst = 0.0
    for s in range(S):
        for mm in range(M):
            j = int(near_i[s, mm])
            slack = r.matrix2[s, mm, j] - r.nearest[s, mm] ** 2
            assert slack <= 2 * ref.GATE * r.G[s, mm, j], (s, mm, j)
            worst = max(worst, slack / (ref.U52 * r.G[s, mm, j]) if r.G[s, mm, j] > 0 else 0.0)
    for mm in range(M):
        for j in range(Fb):
            s = int(cover_s[mm, j])
            slack = r.matrix2[s, mm, j] - r.cover[mm, j] ** 2
            assert slack <= 2 * ref.GATE * r.G[s, mm, j], (s, mm, j)
            worst = max(worst, slack / (ref.U52 * r.G[s, mm, j]) if r.G[s, mm, j] > 0 else 0.0)
    print(f"S={S} M={M} N={N} Fb={Fb}: largest reference slack of a chosen index / (2^-52 G) = {worst:.3f} (allowed 16)")


@pytest.mark.parametrize("N", [5, C + 1])
def test_constructed_ties_go_to_the_lowest_index(dev, N):
    """A duplicated reference frame (columns 3 and T + 2, in different column tiles) and a duplicated step of member 1 (steps
    1 and T + 3, in different row tiles): equal bits by position independence, so the lower index must win both."""
    from molecular_dynamics_neural_operator_amd import forecast
    S, M, Fb = T + 5, 2, T + 4
    A, B = (x.copy() for x in case(S, M, N, Fb)[:2])
    rng = np.random.default_rng(N)
    base = A[0, 0].astype(np.float64)                                                       # the cloud itself
    dup_b, dup_a = ((base + rng.normal(scale=1.0, size=base.shape)).astype(np.float32) for _ in range(2))
    B[3] = B[T + 2] = dup_b
    A[1, 1] = A[T + 3, 1] = dup_a
    A[2, 0] = dup_b                                 # row (2, 0) is that frame itself: its best is met at columns 3 and T + 2
    B[5] = dup_a                                    # column 5: member 1's best is met at steps 1 and T + 3
    d = forecast.cross_rmsd(on(dev, A), on(dev, B)).cpu()
    m = d.matrix.numpy()
    assert m[:, :, 3].tobytes() == m[:, :, T + 2].tobytes() and m[1, 1].tobytes() == m[T + 3, 1].tobytes()
    near_i, cover_s = d.nearest_index.numpy(), d.cover_step.numpy()
    assert not (near_i == T + 2).any() and not (cover_s[1] == T + 3).any()
    assert np.array_equal(near_i, ref.lowest_min(m, 2)[1]) and np.array_equal(cover_s, ref.lowest_min(m, 0)[1])
    assert int(near_i[2, 0]) == 3 and int(cover_s[1, 5]) == 1                               # the tie is really met
    ratio, inside = gate_ratio(m, ref.cross_rmsd(A, B))
    print(f"ties N={N}: largest |d rmsd^2| / (2^-52 G) = {ratio:.3f} (allowed 8)")
    assert inside


# ================================================================================================ 3. optional outputs
@pytest.mark.parametrize("S,M,N,Fb", [SHAPES[4], SHAPES[9]])
def test_optional_outputs_do_not_change_a_bit(dev, S, M, N, Fb):
    from molecular_dynamics_neural_operator_amd import forecast, ops
    A, B = case(S, M, N, Fb)[:2]
    full = device_result(S, M, N, Fb)
    a, b = on(dev, A), on(dev, B)
    lean = forecast.cross_rmsd(a, b, matrix=False).cpu()
    assert lean.matrix is None
    for name in NAMES[1:]:
        assert same(getattr(lean, name), getattr(full, name)), name
    only = ops.cross_rmsd(a, b, matrix=True, nearest=False, cover=False)
    assert only[1:] == (None, None, None, None) and same(only[0].cpu(), full.matrix)
    n_only = ops.cross_rmsd(a, b, matrix=False, nearest=True, cover=False)
    c_only = ops.cross_rmsd(a, b, matrix=False, nearest=False, cover=True)
    assert n_only[0] is None and n_only[3] is None and c_only[0] is None and c_only[1] is None
    assert same(n_only[1].cpu(), full.nearest) and same(n_only[2].cpu(), full.nearest_index)
    assert same(c_only[3].cpu(), full.cover) and same(c_only[4].cpu(), full.cover_step)
    ratio, inside = gate_ratio(only[0].cpu().numpy(), case(S, M, N, Fb)[4])
    print(f"S={S} M={M} N={N} Fb={Fb} matrix only: largest |d rmsd^2| / (2^-52 G) = {ratio:.3f} (allowed 8)")
    assert inside


# ================================================================================================ 4. position independence
@pytest.mark.parametrize("S,M,N,Fb", [(2 * T + 1, 3, C + 1, T + 1), (T + 1, 3, 504, 2 * T + 1)])
def test_an_elements_bits_depend_on_its_two_frames_alone(dev, S, M, N, Fb):
    from molecular_dynamics_neural_operator_amd import forecast
    A, B = case(S, M, N, Fb)[:2]
    full = device_result(S, M, N, Fb)
    a, b = on(dev, A), on(dev, B)
    again = forecast.cross_rmsd(a, b).cpu()
    for name in NAMES:
        assert same(getattr(again, name), getattr(full, name)), name                       # two runs: the same bits
    rng = np.random.default_rng(S + N)
    steps = np.sort(rng.choice(S, size=S // 2 + 1, replace=False))
    members = np.array([2, 0])
    cols = np.sort(rng.choice(Fb, size=Fb // 2 + 2, replace=False))
    sub = forecast.cross_rmsd(on(dev, A[steps][:, members]), on(dev, B[cols])).cpu()
    want = full.matrix[torch.from_numpy(steps)][:, torch.from_numpy(members)][:, :, torch.from_numpy(cols)]
    assert same(sub.matrix, want)                                                           # other tiles, other lanes: the same bits
    for m in range(M):                                                                      # a member scored alone
        alone = forecast.cross_rmsd(on(dev, A[:, m:m + 1]), b).cpu()
        assert same(alone.matrix, full.matrix[:, m:m + 1]) and same(alone.nearest, full.nearest[:, m:m + 1])
        assert same(alone.nearest_index, full.nearest_index[:, m:m + 1])
        assert same(alone.cover, full.cover[m:m + 1]) and same(alone.cover_step, full.cover_step[m:m + 1])
    plain = forecast.cross_rmsd(on(dev, A[:, 1]), b).cpu()                                  # a plain stack [F, N, 3] is M = 1
    assert same(plain.matrix, full.matrix[:, 1:2])
    ratio, inside = gate_ratio(sub.matrix.numpy(), ref.cross_rmsd(A[steps][:, members], B[cols]))
    print(f"S={S} M={M} N={N} Fb={Fb} sub-selection: largest |d rmsd^2| / (2^-52 G) = {ratio:.3f} (allowed 8)")
    assert inside


# ================================================================================================ 5. non-finite frames
@pytest.mark.parametrize("S,M,N,Fb", [(T + 1, 3, C + 1, T + 1), (T - 1, 1, 504, 2 * T + 1)])
def test_a_non_finite_frame_spoils_exactly_its_row_or_column(dev, S, M, N, Fb):
    from molecular_dynamics_neural_operator_amd import forecast
    A, B = (x.copy() for x in case(S, M, N, Fb)[:2])
    clean = device_result(S, M, N, Fb)
    s0, m0, j0 = S - 2, M - 1, Fb - 3
    A[s0, m0, N // 2, 1] = np.nan
    B[j0, N - 1, 2] = np.inf
    d = forecast.cross_rmsd(on(dev, A), on(dev, B)).cpu()
    mask = torch.zeros(S, M, Fb, dtype=torch.bool)
    mask[s0, m0, :] = True
    mask[:, :, j0] = True
    assert bool(torch.isnan(d.matrix[mask]).all())
    assert torch.equal(bits(d.matrix)[~mask], bits(clean.matrix)[~mask])                   # every other element: the same bits
    assert int(d.nearest_index[s0, m0]) == -1 and bool(torch.isnan(d.nearest[s0, m0]))
    assert bool((d.cover_step[:, j0] == -1).all()) and bool(torch.isnan(d.cover[:, j0]).all())
    assert not bool((d.nearest_index == j0).any()) and not bool((d.cover_step[m0] == s0).any())           # never chosen
    m = d.matrix.numpy()
    near, near_i = ref.lowest_min(m, 2)
    cover, cover_s = ref.lowest_min(m, 0)
    assert np.array_equal(d.nearest_index.numpy(), near_i) and np.array_equal(d.cover_step.numpy(), cover_s)
    assert d.nearest.numpy().tobytes() == near.tobytes() and d.cover.numpy().tobytes() == cover.tobytes()
    ratio, inside = gate_ratio(m, ref.cross_rmsd(A, B))
    print(f"S={S} M={M} N={N} Fb={Fb} with a NaN row and an Inf column: largest |d rmsd^2| / (2^-52 G) = {ratio:.3f} (allowed 8)")
    assert inside
    # a member with no valid step; then no valid reference frame at all
    A[:, m0, 0, 0] = -np.inf
    d = forecast.cross_rmsd(on(dev, A), on(dev, B)).cpu()
    assert bool((d.cover_step[m0] == -1).all()) and bool(torch.isnan(d.cover[m0]).all()) and bool(torch.isnan(d.matrix[:, m0]).all())
    assert bool((d.nearest_index[:, m0] == -1).all()) and bool(torch.isnan(d.precision(1.0)[m0])) and bool(torch.isnan(d.coverage(1.0)[m0]))
    if M > 1:
        assert torch.equal(bits(d.matrix[:, 0])[:, torch.arange(Fb) != j0], bits(clean.matrix[:, 0])[:, torch.arange(Fb) != j0])
    B[:, 0, 0] = np.nan
    d = forecast.cross_rmsd(on(dev, A), on(dev, B)).cpu()
    assert bool(torch.isnan(d.matrix).all()) and bool(torch.isnan(d.nearest).all()) and bool(torch.isnan(d.cover).all())
    assert bool((d.nearest_index == -1).all()) and bool((d.cover_step == -1).all())


# ================================================================================================ 6. the self matrix
@pytest.mark.parametrize("F,N", [(T + 1, 7), (2 * T + 1, C + 1), (T, 504)])
def test_self_matrix(dev, F, N):
    """A and B the SAME buffer: the diagonal within the gate of 0, m[i, j]^2 and m[j, i]^2 within two gates of each other
    (the symmetry is not exploited: S and its transpose give Horn matrices equal in exact arithmetic only)."""
    from molecular_dynamics_neural_operator_amd import forecast
    A = case(F, 1, N, 3)[0]
    a = on(dev, A[:, 0])
    d = forecast.cross_rmsd(a, a).cpu()
    m = d.matrix.numpy()[:, 0]
    r = ref.cross_rmsd(A, A[:, 0])
    ratio, inside = gate_ratio(d.matrix.numpy(), r)
    G = r.G[:, 0]
    asym = np.abs(m ** 2 - m.T ** 2)
    print(f"self F={F} N={N}: largest |d rmsd^2| / (2^-52 G) = {ratio:.3f} (allowed 8), largest |m_ij^2 - m_ji^2| / (2^-52 G) = "
          f"{float((asym[G > 0] / (ref.U52 * G[G > 0])).max()):.3f} (allowed 16)")
    assert inside and np.all(np.diag(m) ** 2 <= ref.GATE * np.diag(G)) and np.all(asym <= 2 * ref.GATE * G)
    assert np.array_equal(d.nearest_index.numpy(), ref.lowest_min(d.matrix.numpy(), 2)[1])


# ================================================================================================ 7. empty shapes
def test_empty_shapes(dev):
    """S M == 0 or Fb == 0: what has no counterpart is NaN and -1, nothing else is written.  N == 0: zeros, index 0."""
    from molecular_dynamics_neural_operator_amd import forecast
    z = lambda *s: torch.zeros(s, device=dev)
    d = forecast.cross_rmsd(z(4, 2, 5, 3), z(0, 5, 3))
    assert d.matrix.shape == (4, 2, 0) and d.cover.shape == (2, 0) and d.cover_step.shape == (2, 0)
    assert bool(torch.isnan(d.nearest).all()) and bool((d.nearest_index == -1).all()) and d.nearest.shape == (4, 2)
    d = forecast.cross_rmsd(z(0, 2, 5, 3), z(3, 5, 3))
    assert d.matrix.shape == (0, 2, 3) and d.nearest.shape == (0, 2)
    assert bool(torch.isnan(d.cover).all()) and bool((d.cover_step == -1).all()) and d.cover.shape == (2, 3)
    d = forecast.cross_rmsd(z(4, 0, 5, 3), z(3, 5, 3))
    assert d.matrix.shape == (4, 0, 3) and d.nearest.shape == (4, 0) and d.cover.shape == (0, 3)
    d = forecast.cross_rmsd(z(T + 1, 2, 0, 3), z(3, 0, 3))
    assert not d.matrix.any() and not d.nearest.any() and not d.cover.any() and d.matrix.shape == (T + 1, 2, 3)
    assert not d.nearest_index.any() and not d.cover_step.any()
    assert d.precision(0.0).tolist() == [1.0, 1.0] and d.coverage(0.0).tolist() == [1.0, 1.0]


# ================================================================================================ 8. the engines
def _engine_inputs(M):
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    N, W = 28, 3
    base = syn.chain_frame(N, seed=1)
    traj = syn.ou_trajectory(base, W + 6, seed=2)
    wins = syn.ensemble_windows(traj[:W], M, sigma=0.1, seed0=100)              # [M, W, N, 3]
    truth = torch.from_numpy(np.ascontiguousarray(traj[W:W + 6]).astype(np.float32))
    return (torch.from_numpy(np.ascontiguousarray(wins.transpose(1, 0, 2, 3))), torch.from_numpy(syn.amino_acids(N, seed=1)), truth)


def _model(dev):
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    model = KernelNN(64, 128, 2, 6, 7, 3, 20, 4)
    model.load_state_dict(near_identity_state_dict(64, 128, seed=0, kernel_gain=1e-3, feature_gain=0.1))
    return model.eval().to(dev)


def test_engines_score_their_own_frames(dev):
    """A noisy 4-step, 8-member, N = 28 run against 6 true frames: both engines' cross_rmsd equals forecast.cross_rmsd on
    engine.frames() bit for bit, also from a non-zero first step and without the matrix; the trajectory buffer is unchanged."""
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine, RolloutEngine
    wins, aa, truth = _engine_inputs(8)
    truth = truth.to(dev)
    model = _model(dev)
    for cls in (RolloutEngine, GroupedRolloutEngine):
        eng = cls(model, 8, 28, 3, 8.0, max_steps=4, device=dev, noise_sigma=0.05, noise_seed=7)
        eng.run(wins, aa, 4)
        before = eng.frames().clone()
        e = eng.cross_rmsd(truth)
        w = forecast.cross_rmsd(eng.frames().contiguous(), truth)
        for name in NAMES:
            assert same(getattr(e, name), getattr(w, name)), (cls.__name__, name)
        assert e.matrix.shape == (4, 8, 6) and e.cover.shape == (8, 6) and bool(torch.isfinite(e.matrix).all())
        if cls is GroupedRolloutEngine:
            assert len(eng.engines) == 2
        part = eng.cross_rmsd(truth, first_step=1, steps=2, matrix=False)
        assert part.matrix is None and same(part.nearest, e.nearest[1:3]) and same(part.nearest_index, e.nearest_index[1:3])
        assert same(part.cover, torch.from_numpy(ref.lowest_min(e.matrix[1:3].cpu().numpy(), 0)[0]).to(dev))
        assert torch.equal(eng.frames(), before)
        r = ref.cross_rmsd(before.cpu().numpy(), truth.cpu().numpy())
        ratio, inside = gate_ratio(e.matrix.cpu().numpy(), r)
        print(f"{cls.__name__}: largest |d rmsd^2| / (2^-52 G) = {ratio:.3f} (allowed 8)")
        assert inside and bool((e.precision(100.0) == 1).all()) and bool((e.coverage(100.0) == 1).all())
        eng.close()


# ================================================================================================ 9. guard bands
def _run_guarded(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import _lib, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError, ptr, stream_ptr
    lib = _lib.load()
    res = []
    with Guard(fill, record_calls=False) as G:
        for S, M, N, Fb in ((T + 1, 3, C + 1, T - 1), (1, 1, 1, 1), (T, 1, 504, 2 * T + 1)):
            A, B = case(S, M, N, Fb)[:2]
            a, b = G.place(on(dev, A)), G.place(on(dev, B))
            for flags in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
                res.extend(t.clone() for t in ops.cross_rmsd(a, b, *flags) if t is not None)
        G.verify()
        # rows past the stated shapes stay untouched: outputs of S + 1 steps and M + 1 members' columns given to a call over
        # S and M, the workspace exactly as stated
        S, M, N, Fb = T + 1, 3, C + 1, T - 1
        A, B = case(S, M, N, Fb)[:2]
        a, b = G.place(on(dev, A)), G.place(on(dev, B))
        matrix = torch.empty((S + 1, M, Fb), dtype=torch.float64, device=dev)
        near, near_i = torch.empty((S + 1, M), dtype=torch.float64, device=dev), torch.empty((S + 1, M), dtype=torch.int64, device=dev)
        cover, cover_s = torch.empty((M + 1, Fb), dtype=torch.float64, device=dev), torch.empty((M + 1, Fb), dtype=torch.int64, device=dev)
        nbytes = lib.mdnoconf_cross_rmsd_workspace_bytes(S, M, N, Fb, 1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert lib.mdnoconf_cross_rmsd(ptr(a), S, M, ptr(b), Fb, N, ptr(matrix), ptr(near), ptr(near_i), ptr(cover), ptr(cover_s),
                                       ptr(ws), nbytes, stream_ptr(dev)) == 0
        G.verify()
        for t in (matrix, near, near_i, cover, cover_s):
            assert (t[-1].cpu().reshape(-1).view(torch.uint8) == fill).all()
        assert bool(torch.isfinite(matrix[:S]).all())
        res.extend([matrix[:S].clone(), near[:S].clone(), near_i[:S].clone(), cover[:M].clone(), cover_s[:M].clone()])
        # a refused call writes nothing
        since = len(G.records)
        t_m = torch.empty((S, M, Fb), dtype=torch.float64, device=dev)
        t_n, t_ni = torch.empty((S, M), dtype=torch.float64, device=dev), torch.empty((S, M), dtype=torch.int64, device=dev)
        t_c, t_cs = torch.empty((M, Fb), dtype=torch.float64, device=dev), torch.empty((M, Fb), dtype=torch.int64, device=dev)
        t_ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        for kw, wb in (({"S": -1}, nbytes), ({}, nbytes - 1), ({"near_i": None}, nbytes), ({"cover": None}, nbytes)):
            p = dict(S=S, near_i=ptr(t_ni), cover=ptr(t_c))
            p.update(kw)
            rc = lib.mdnoconf_cross_rmsd(ptr(a), p["S"], M, ptr(b), Fb, N, ptr(t_m), ptr(t_n), p["near_i"], p["cover"], ptr(t_cs),
                                         ptr(t_ws), wb, stream_ptr(dev))
            assert rc == _lib.EINVAL, (kw, wb)
        with pytest.raises(MdnoError):
            ops.cross_rmsd(a, b[:, :N - 1])
        with pytest.raises(MdnoError):
            ops.cross_rmsd(a, b, False, False, False)
        G.untouched(since)
        G.verify()
    return res


def test_cross_rmsd_entry_point_stays_inside_its_buffers(dev):
    """Every output and the workspace inside guard bands under both fill bytes, one to three tiles per side, one to sixteen
    atom chunks, every combination of outputs: every band intact, every result identical under 0x00 and 0xFF (nothing unset
    is read), rows past the stated shapes untouched, a refused call writes nothing."""
    from guarded import FILLS
    a, b = (_run_guarded(dev, fill) for fill in FILLS)
    assert len(a) == len(b) == 3 * (5 + 1 + 2 + 2) + 5
    for i, (u, v) in enumerate(zip(a, b)):
        assert not torch.isnan(u.double()).any() and same(u, v), i
    S, M, N, Fb = T + 1, 3, C + 1, T - 1
    full = device_result(S, M, N, Fb)
    for u, name in zip(a[:5], NAMES):
        assert same(u.cpu(), getattr(full, name)), name
    ratio, inside = gate_ratio(a[0].cpu().numpy(), case(S, M, N, Fb)[4])
    print(f"guarded S={S} M={M} N={N} Fb={Fb}: largest |d rmsd^2| / (2^-52 G) = {ratio:.3f} (allowed 8)")
    assert inside
