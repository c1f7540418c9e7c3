"""Orthorhombic periodic boundary conditions (include/mdno_pbc.h, csrc/pbc.h, csrc/pbc.hip)
against a numpy fp64 restatement of the rule (`pbc_graph` below): the periodic radius graph bit for bit, the forward on
periodic samples and the periodic rollout against the oracle on the restatement's edges, periodic scoring as exact
integers, guard bands around every new entry point that writes caller memory.

The restatement follows the header line by line: d = x_j - x_i in fp64 on the fp32 coordinates, k = rint(d * (1 / L))
(numpy's rint is round-half-even; every operation below is a separate array operation, so nothing is contracted),
d' = d - k * L, kept iff sqrt((dx'^2 + dy'^2) + dz'^2) < cutoff, attribute row [(float)(x_j - k * L), x_i].  Exact
comparison needs inputs on which a last-bit difference in sqrt or rint could not change the answer: `check_condition`
asserts that no pair lies within 1e-9 (relative) of the cutoff and no d / L within 1e-9 of a half-integer."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


# ================================================================================================ the restatement
def pbc_graph(pos, cutoff, box):
    """pos f32 [N, 3] -> dict(row_ptr, src, dst, attr f32 [E, 6], keep bool [N, N] (keep[i, j]: edge j -> i),
    margin = min | dist - cutoff |, half = min distance of a d / L from a half-integer over the periodic axes)."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    p = pos.astype(np.float64)
    L = np.asarray(box, dtype=np.float64)
    periodic = L > 0.0
    inv = np.zeros(3)
    inv[periodic] = 1.0 / L[periodic]
    d = p[None, :, :] - p[:, None, :]                     # d[i, j] = x_j - x_i
    q = d * inv
    k = np.where(periodic, np.rint(q), 0.0)
    shift = k * L
    dp = d - shift
    s = (dp[..., 0] * dp[..., 0] + dp[..., 1] * dp[..., 1]) + dp[..., 2] * dp[..., 2]
    dist = np.sqrt(s)
    keep = dist < cutoff
    dst, src = np.nonzero(keep)                           # row-major: destinations ascending, sources ascending in a row
    image = (p[src] - shift[dst, src]).astype(np.float32)
    attr = np.concatenate([image, pos[dst]], axis=1)
    row_ptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int32)
    frac = np.abs(q - np.floor(q) - 0.5)[..., periodic]
    return dict(row_ptr=row_ptr, src=src.astype(np.int32), dst=dst.astype(np.int32), attr=attr, keep=keep,
                margin=float(np.abs(dist - cutoff).min()), half=float(frac.min()) if frac.size else 1.0, cutoff=float(cutoff))


def check_condition(g):
    """The input condition of an exact comparison (module docstring).  A condition on the inputs, not a measurement."""
    assert g["margin"] / g["cutoff"] >= 1e-9, f"a pair lies within 1e-9 of the cutoff ({g['margin']}): pick another seed"
    assert g["half"] >= 1e-9, f"a d / L lies within 1e-9 of a half-integer ({g['half']}): pick another seed"


def pbc_graph_members(pos, n_atoms, cutoff, box):
    """pos f32 [M * N, 3]: the block-diagonal graph of M members (no cross-member edge), global row numbers."""
    parts = [pbc_graph(pos[o:o + n_atoms], cutoff, box) for o in range(0, pos.shape[0], n_atoms)]
    row_ptr, src, dst, off = [np.zeros(1, np.int32)], [], [], 0
    for m, g in enumerate(parts):
        check_condition(g)
        row_ptr.append(g["row_ptr"][1:] + off)
        src.append(g["src"] + m * n_atoms)
        dst.append(g["dst"] + m * n_atoms)
        off += g["src"].size
    return dict(row_ptr=np.concatenate(row_ptr), src=np.concatenate(src), dst=np.concatenate(dst),
                attr=np.concatenate([g["attr"] for g in parts]))


def random_frame(n, box, seed, open_extent=12.0):
    """Unwrapped coordinates: uniform in the cell centred at the origin, then moved by -2 .. 2 whole box lengths per
    atom and axis (up to 2.5 L outside the origin, both signs); an open axis is uniform in +-open_extent / 2."""
    rng = np.random.default_rng(seed)
    L = np.broadcast_to(np.asarray(box, dtype=np.float64), (3,))
    ext = np.where(L > 0, L, open_extent)
    pos = (rng.random((n, 3)) - 0.5) * ext + rng.integers(-2, 3, size=(n, 3)) * L
    return pos.astype(np.float32)


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_graph(dev, pos, n_atoms, cutoff, box, **kw):
    from molecular_dynamics_neural_operator_amd import ops
    g, attr = ops.radius_graph_pbc(torch.from_numpy(pos).to(dev), n_atoms, cutoff, box, **kw)
    e = int(g.num_edges.item())
    return g, attr, e


def assert_graph_equal(g, attr, e, want):
    assert e == want["src"].size and int(g.status.item()) == 0
    assert np.array_equal(g.row_ptr.cpu().numpy(), want["row_ptr"])
    assert np.array_equal(g.src[:e].cpu().numpy(), want["src"]) and np.array_equal(g.dst[:e].cpu().numpy(), want["dst"])
    if attr is not None:
        assert np.array_equal(bits(attr[:e].cpu().numpy()), bits(want["attr"]))


# ================================================================================================ 1. the graph, exactly
CUT = 4.0
BOXES = {"cubic": (9.0, 9.0, 9.0), "three_lengths": (8.5, 10.0, 13.0), "open_axis": (9.0, 0.0, 11.0),
         "exactly_two_cutoffs": (8.0, 8.0, 8.0)}
# (M, N): the 64-lane tails of a row (63, 64, 65, 130), the 4-rows-per-block tails (1, 2, 63, 65, 130 rows), member
# offsets and no cross-member edge (3 x 37)
SHAPES = [(1, 1), (1, 2), (1, 63), (1, 64), (1, 65), (1, 130), (3, 37)]


@pytest.mark.parametrize("box", sorted(BOXES))
@pytest.mark.parametrize("M,N", SHAPES)
def test_graph_equals_the_restatement(dev, M, N, box):
    L = BOXES[box]
    pos = np.concatenate([random_frame(N, L, seed=1000 * N + 10 * m + len(box)) for m in range(M)])
    want = pbc_graph_members(pos, N, CUT, L)
    g, attr, e = device_graph(dev, pos, N, CUT, L)
    print(f"M={M} N={N} {box}: {e} edges, {e / (M * N):.1f} per atom")
    assert_graph_equal(g, attr, e, want)
    if N >= 63:          # most edges cross a face: the open graph of the same atoms is another graph
        assert e > pbc_graph_members(pos, N, CUT, (0.0, 0.0, 0.0))["src"].size
    # topology only: the same CSR
    g2, attr2, e2 = device_graph(dev, pos, N, CUT, L, with_attr=False)
    assert attr2 is None
    assert_graph_equal(g2, None, e2, want)


def test_exact_tie_gives_no_edge(dev):
    """x = 0.5 and 8.5 with L = 16 and cutoff 8: d / L = +-0.5 exactly, the image is 8 away whichever way the tie
    rounds, and 8 < 8 is false: self-loops only, from both sides."""
    pos = np.array([[0.5, 1.0, 1.0], [8.5, 1.0, 1.0]], dtype=np.float32)
    g, attr, e = device_graph(dev, pos, 2, 8.0, (16.0, 16.0, 16.0))
    assert e == 2 and g.src[:2].tolist() == [0, 1] and g.dst[:2].tolist() == [0, 1] and g.row_ptr.tolist() == [0, 1, 2]
    assert np.array_equal(bits(attr[:2].cpu().numpy()), bits(np.concatenate([pos, pos], 1)))
    # one ulp closer and the pair is an edge through the face, imaged to the far side of the destination
    pos[1, 0] = np.nextafter(np.float32(8.5), np.float32(9.0))
    want = pbc_graph(pos, 8.0, (16.0, 16.0, 16.0))
    g, attr, e = device_graph(dev, pos, 2, 8.0, (16.0, 16.0, 16.0))
    assert e == 4
    assert_graph_equal(g, attr, e, want)
    assert float(attr[0, 0]) == 0.5 and float(attr[1, 0]) < -7.49 and float(attr[2, 0]) > 16.49


def test_big_box_is_the_open_graph(dev):
    """L = 1e6: k = 0 for every pair, and the CSR and the attributes are those of the open graph, bit for bit."""
    from molecular_dynamics_neural_operator_amd import ops
    for M, N in ((1, 130), (3, 37)):
        pos = np.concatenate([random_frame(N, (9.0, 9.0, 9.0), seed=77 + m) for m in range(M)])
        tp = torch.from_numpy(pos).to(dev)
        for box in ((1e6, 1e6, 1e6), (0.0, 0.0, 0.0), (1e6, 0.0, 1e6)):
            g, attr, e = device_graph(dev, pos, N, CUT, box)
            o = ops.radius_graph(tp, N, CUT)
            assert e == int(o.num_edges.item()) and e > M * N
            assert torch.equal(g.row_ptr, o.row_ptr) and torch.equal(g.src[:e], o.src[:e]) and torch.equal(g.dst[:e], o.dst[:e])
            want = torch.cat([tp[o.src[:e].long()], tp[o.dst[:e].long()]], dim=1)
            assert np.array_equal(bits(attr[:e].cpu().numpy()), bits(want.cpu().numpy()))


def test_lattice_translation(dev):
    """L = 32, coordinates on a 2^-10 grid (every difference, shift and image is exact): atoms moved by whole box
    vectors keep their CSR, and an edge's attributes move with its DESTINATION."""
    rng = np.random.default_rng(5)
    N, L = 90, 32.0
    pos = (rng.integers(0, 32 * 1024, size=(N, 3)) / 1024.0).astype(np.float32)
    move = (rng.integers(-2, 3, size=(N, 3)) * L).astype(np.float32)
    move[::3] = 0.0
    g0, a0, e0 = device_graph(dev, pos, N, 8.0, (L, L, L))
    g1, a1, e1 = device_graph(dev, pos + move, N, 8.0, (L, L, L))
    assert_graph_equal(g0, a0, e0, pbc_graph(pos, 8.0, (L, L, L)))
    assert e0 == e1 and e0 > 4 * N and torch.equal(g0.row_ptr, g1.row_ptr) and torch.equal(g0.src[:e0], g1.src[:e0])
    by_dst = torch.from_numpy(move).to(dev)[g0.dst[:e0].long()]
    assert torch.equal(a1[:e0], a0[:e0] + torch.cat([by_dst, by_dst], dim=1))
    assert bool((move != 0).any())


def test_overflow_sets_the_status_bit(dev):
    from molecular_dynamics_neural_operator_amd._lib import STATUS_EDGE_OVERFLOW
    L = BOXES["three_lengths"]
    pos = random_frame(130, L, seed=3)
    want = pbc_graph(pos, CUT, L)
    E = want["src"].size
    for cap in (E - 1, E - 70, 130):
        g, attr, e = device_graph(dev, pos, 130, CUT, L, edge_cap=cap)
        assert e == cap and int(g.status.item()) & STATUS_EDGE_OVERFLOW and int(g.row_ptr[-1]) == cap
        assert np.array_equal(g.src[:cap].cpu().numpy(), want["src"][:cap])
        assert np.array_equal(bits(attr[:cap].cpu().numpy()), bits(want["attr"][:cap]))
    g, attr, e = device_graph(dev, pos, 130, CUT, L, edge_cap=E)          # exactly full: no overflow
    assert_graph_equal(g, attr, e, want)


# ================================================================================================ 2. forward
FWD_N, FWD_W, FWD_CUT, FWD_BOX = 40, 3, 6.0, (12.5, 13.0, 14.0)


@functools.lru_cache(maxsize=None)
def forward_inputs():
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    sd = near_identity_state_dict(64, 128, seed=5, kernel_gain=3e-2, feature_gain=0.3, kernel_to_coords=1.0)
    wins = [torch.from_numpy(syn.jitter_window(random_frame(FWD_N, FWD_BOX, seed=40 + i), FWD_W, seed=i)) for i in range(2)]
    aa = torch.from_numpy(syn.amino_acids(FWD_N, seed=6))
    return sd, wins, aa


@functools.lru_cache(maxsize=None)
def forward_reference():
    """The oracle on the restatement's edges and attributes, once for all six configurations."""
    from oracle import graph_kernel_oracle as O
    sd, wins, aa = forward_inputs()
    graphs, outs = [], []
    for win in wins:
        g = pbc_graph(win[-1].numpy(), FWD_CUT, FWD_BOX)
        check_condition(g)
        ei = torch.from_numpy(np.stack([g["src"], g["dst"]]).astype(np.int64))
        outs.append(O.kernelnn_forward(sd, win, aa, ei, torch.from_numpy(g["attr"]), 2, hoist=True))
        graphs.append((ei, g["attr"]))
    return graphs, outs


@pytest.mark.parametrize("conv_mode", ["materialized", "factored"])
@pytest.mark.parametrize("gemm_mode", ["split_f16", "split_bf16", "f32"])
def test_forward_on_periodic_samples(dev, gemm_mode, conv_mode):
    from test_gpu_parity import close
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN, construct_pairdata
    sd, wins, aa = forward_inputs()
    graphs, want = forward_reference()
    model = KernelNN(64, 128, 2, 6, 7, 3, 20, 4)
    model.load_state_dict(sd)
    model.eval().to(dev)
    model.gemm_mode, model.conv_mode = gemm_mode, conv_mode
    samples = [construct_pairdata(w, aa, FWD_CUT, box=FWD_BOX) for w in wins]
    for s, (ei, attr) in zip(samples, graphs):
        assert torch.equal(s.edge_index.cpu(), ei) and np.array_equal(bits(s.edge_attr.cpu().numpy()), bits(attr))
        assert ei.shape[1] > 10 * FWD_N
    with torch.no_grad():
        outs = [model(s) for s in samples]
        both = model(samples)
    for i in range(2):
        close(outs[i], want[i], name=f"periodic sample {i} {gemm_mode} {conv_mode}")
        assert torch.equal(both[i * FWD_N:(i + 1) * FWD_N], outs[i])
    # the same window in an open box is another graph and another output
    with torch.no_grad():
        assert not torch.equal(model(construct_pairdata(wins[0], aa, FWD_CUT)), outs[0])


# ================================================================================================ 3. rollout
R_M, R_N, R_W, R_STEPS, R_CUT, R_BOX = 2, 64, 3, 4, 8.0, (17.0, 17.2, 17.6)
R_SEED = 6          # searched on the CPU: min | dist - cutoff | >= 1e-3 A over every step of both host loops below
R_SIGMA, R_NOISE_SEED, R_IDS = 0.05, 0x5EED0123456789AB, (9, 4)
R_DEPTH = 2


@functools.lru_cache(maxsize=None)
def rollout_inputs(seed=R_SEED):
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    sd = near_identity_state_dict(64, 128, seed=1, kernel_gain=1e-2, feature_gain=1e-1, kernel_to_coords=1.0)
    # A jittered 4 x 4 x 4 lattice filling the cell (a liquid-like frame of 64 atoms has ~600 pairs per Angstrom of
    # distance at the cutoff, and two members over two four-step loops would then come within 1e-3 A of it in all but
    # one seed in 10^5): the cutoff lies between the third and the fourth shell (7.5 and 8.5 A), the jitter's tails
    # reach it, so the graph still changes from step to step, and every atom has neighbours across each face.
    rng = np.random.default_rng(seed)
    cell = np.asarray(R_BOX) / 4.0
    grid = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    base = ((grid + 0.5) * cell - np.asarray(R_BOX) / 2.0 + rng.normal(scale=0.12, size=(R_N, 3))).astype(np.float32)
    base = base[rng.permutation(R_N)]
    base[::5] += (rng.integers(-1, 2, size=(len(base[::5]), 3)) * np.asarray(R_BOX)).astype(np.float32)      # some atoms unwrapped
    win = syn.jitter_window(base, R_W, seed=seed)
    wins = torch.from_numpy(syn.ensemble_windows(win, R_M, sigma=0.1, seed0=100 + seed)).permute(1, 0, 2, 3).contiguous()
    aa = torch.from_numpy(syn.amino_acids(R_N, seed=3))
    return sd, wins, aa          # wins [W, M, N, 3]


def host_rollout(noise=None, seed=R_SEED):
    """The reference loop on the host: the periodic graph of the newest frame from the restatement, the oracle's
    forward on its edges and attributes, the frame appended (plus noise[t, m] f32 [N, 3] if given).  Returns
    (frames [steps, M, N, 3], edges per step, min | dist - cutoff | over every graph built)."""
    from oracle import graph_kernel_oracle as O
    sd, wins, aa = rollout_inputs(seed)
    traj = wins.clone()
    edges, margin = [], float("inf")
    for t in range(R_STEPS):
        new, n_e = [], 0
        for m in range(R_M):
            window = traj[t:t + R_W, m]
            g = pbc_graph(window[-1].numpy(), R_CUT, R_BOX)
            margin = min(margin, g["margin"])
            n_e += g["src"].size
            ei = torch.from_numpy(np.stack([g["src"], g["dst"]]).astype(np.int64))
            out = O.kernelnn_forward(sd, window, aa, ei, torch.from_numpy(g["attr"]), R_DEPTH, hoist=True)
            new.append(out + noise[t, m] if noise is not None else out)
        edges.append(n_e)
        traj = torch.cat([traj, torch.stack(new)[None]])
    return traj[R_W:], edges, margin


@functools.lru_cache(maxsize=None)
def host_reference(noisy: bool):
    from molecular_dynamics_neural_operator_amd import ops
    noise = None
    if noisy:
        noise = torch.stack([ops.noise_fill(R_NOISE_SEED, R_IDS, t, R_N, sigma=R_SIGMA, device="cuda:0").view(R_M, R_N, 3)
                             for t in range(R_STEPS)]).cpu()
    return host_rollout(noise)


def make_model(dev, conv_mode):
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    sd, _, _ = rollout_inputs()
    model = KernelNN(64, 128, R_DEPTH, 6, 7, 3, 20, 4)
    model.load_state_dict(sd)
    model.eval().to(dev)
    model.conv_mode = conv_mode
    return model


def run_engine(dev, model, wins, aa, steps=R_STEPS, cls=None, before_step=None, **kw):
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    eng = (cls or RolloutEngine)(model, wins.shape[1], R_N, R_W, R_CUT, max_steps=kw.pop("max_steps", steps), device=dev, **kw)
    eng.reset(wins, aa)
    if before_step:
        before_step(eng)
    eng.step(steps)
    eng.synchronize()
    out = eng.frames().clone()
    info = dict(edges=eng.edges_per_step.cpu().tolist()[:steps], spl=getattr(eng, "steps_per_launch", None),
                mode=eng.conv_mode)
    eng.close()
    return out, info


def assert_gate(got, ref, what):
    got, ref = got.cpu().numpy(), ref.numpy()
    err = float(np.abs(got - ref).max())
    print(f"{what}: max abs err {err:.3e}, max|ref| {float(np.abs(ref).max()):.3e}")
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


@pytest.mark.parametrize("conv_mode", ["materialized", "factored"])
def test_rollout_against_the_host_loop(dev, conv_mode):
    """M = 2, N = 64 (128 rows: the open step of this size is the fused short-chain head, which a periodic step must
    not take), W = 3, 4 steps: edges per step equal, frames within the gate of test_rollout_vs_oracle_full_width;
    graph replay and plain launches, the member alone, a group of one and the whole batch give the same bits."""
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine
    _, wins, aa = rollout_inputs()
    ref, edges, margin = host_reference(False)
    print("min |dist - cutoff| over the host loop:", margin, "edges per step", edges)
    assert margin >= 1e-3
    model = make_model(dev, conv_mode)
    got, info = run_engine(dev, model, wins, aa, box=R_BOX)
    assert info["mode"] == conv_mode and info["spl"] == 1
    assert info["edges"] == edges
    assert_gate(got, ref, f"periodic rollout {conv_mode}")
    plain, info_p = run_engine(dev, model, wins, aa, box=R_BOX, use_graph=False)
    assert info_p["spl"] == 0 and info_p["edges"] == edges and torch.equal(plain, got)
    grouped, info_g = run_engine(dev, model, wins, aa, cls=GroupedRolloutEngine, groups=2, box=R_BOX)
    assert info_g["edges"] == edges
    for m in range(R_M):
        alone, _ = run_engine(dev, model, wins[:, m:m + 1].contiguous(), aa, box=R_BOX)
        assert torch.equal(grouped[:, m:m + 1], alone), m
        assert torch.equal(got[:, m:m + 1], alone), m
    # the open rollout of the same windows is another trajectory (fewer edges)
    opn, info_o = run_engine(dev, model, wins, aa)
    assert not torch.equal(opn, got) and all(a < b for a, b in zip(info_o["edges"], edges))


@pytest.mark.parametrize("use_graph", [True, False])
def test_box_taken_back_is_the_plain_rollout(dev, use_graph):
    """set_box(NULL) after set_box(box): the bits, the edge counts and the steps per graph launch (8: the short-chain
    graph is captured again) of an engine that never had a box; all-open boxes are no box."""
    _, wins, aa = rollout_inputs()
    model = make_model(dev, "materialized")
    never, info_n = run_engine(dev, model, wins, aa, steps=9, use_graph=use_graph)
    back, info_b = run_engine(dev, model, wins, aa, steps=9, use_graph=use_graph, box=R_BOX, before_step=lambda e: e.set_box(None))
    zero, info_z = run_engine(dev, model, wins, aa, steps=9, use_graph=use_graph, box=(0.0, 0.0, 0.0))
    assert info_n["spl"] == (8 if use_graph else 0)
    for out, info in ((back, info_b), (zero, info_z)):
        assert torch.equal(out, never) and info["edges"] == info_n["edges"] and info["spl"] == info_n["spl"]
    # and the other way round: a box given after reset() is the box given at construction; 9 steps = 8 + 1 replayed
    late, info_l = run_engine(dev, model, wins, aa, steps=9, use_graph=use_graph, before_step=lambda e: e.set_box(R_BOX))
    early, info_e = run_engine(dev, model, wins, aa, steps=9, use_graph=use_graph, box=R_BOX)
    assert torch.equal(late, early) and info_l["edges"] == info_e["edges"] and not torch.equal(late, never)
    assert info_e["spl"] == info_l["spl"] == (8 if use_graph else 0)
    single, _ = run_engine(dev, model, wins, aa, steps=4, use_graph=use_graph, box=R_BOX)
    assert torch.equal(early[:4], single)


def test_noisy_periodic_rollout(dev):
    """noise_sigma > 0 composes: the frames are the host loop's with ops.noise_fill's values added to every produced
    frame before the next graph reads it."""
    _, wins, aa = rollout_inputs()
    ref, edges, margin = host_reference(True)
    clean, _, _ = host_reference(False)
    print("min |dist - cutoff| over the noisy host loop:", margin)
    assert margin >= 1e-3 and not torch.equal(ref, clean)
    model = make_model(dev, "factored")
    noise = dict(noise_sigma=R_SIGMA, noise_seed=R_NOISE_SEED, member_ids=R_IDS)
    got, info = run_engine(dev, model, wins, aa, box=R_BOX, **noise)
    assert info["edges"] == edges
    assert_gate(got, ref, "noisy periodic rollout")
    plain, _ = run_engine(dev, model, wins, aa, box=R_BOX, use_graph=False, **noise)
    assert torch.equal(plain, got)


def test_engine_timer_and_regrown_capacity(dev):
    """Timer id 4 covers the periodic graph, and a plan re-created with a larger capacity gets a new attribute buffer
    and its box again: the frames of an engine that had room from the start."""
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    _, wins, aa = rollout_inputs()
    _, edges, _ = host_reference(False)
    model = make_model(dev, "materialized")
    want, _ = run_engine(dev, model, wins, aa, box=R_BOX)
    eng = RolloutEngine(model, R_M, R_N, R_W, R_CUT, max_steps=R_STEPS, edge_cap=max(edges) - 1, device=dev, box=R_BOX)
    eng.reset(wins, aa)
    eng._fit_cap = True          # (the fit itself applies from N > 256 on: treat this capacity as a fitted one)
    eng.step(R_STEPS)
    eng.synchronize()
    assert len(eng.regrown) == 1 and eng._box_attr.shape == (eng.edge_cap, 6) and eng.edge_cap > max(edges)
    assert eng.edges_per_step.cpu().tolist() == edges and torch.equal(eng.frames(), want)
    eng.reset(wins, aa)
    eng.attach_timer(64)
    eng.step(2)
    times = eng.read_timer()
    eng.detach_timer()
    assert times["radius_graph"][1] == 2 and times["radius_graph"][0] > 0.0
    assert torch.equal(eng.frames(), want[:2])
    eng.close()


# ================================================================================================ 4. scoring
S_BOX, S_CUT = (17.0, 18.5, 0.0), 8.0


@functools.lru_cache(maxsize=None)
def scoring_inputs(N):
    S, M = 2, 2
    rng = np.random.default_rng(N)
    truth = np.stack([random_frame(N, S_BOX, seed=N + s, open_extent=20.0) for s in range(S)])          # [S, N, 3]
    frames = (truth[:, None] + rng.normal(scale=0.8, size=(S, M, N, 3))).astype(np.float32)
    counts = np.zeros((S, M, 3), dtype=np.int64)
    maps = np.zeros((S, M, N, N), dtype=np.uint8)
    for s in range(S):
        gt = pbc_graph(truth[s], S_CUT, S_BOX)
        check_condition(gt)
        for m in range(M):
            gf = pbc_graph(frames[s, m], S_CUT, S_BOX)
            check_condition(gf)
            counts[s, m] = (gf["keep"].sum(), gt["keep"].sum(), (gf["keep"] & gt["keep"]).sum())
            maps[s, m] = gf["keep"]
    return torch.from_numpy(frames), torch.from_numpy(truth), counts, maps


@pytest.mark.parametrize("N,form", [(37, "lds"), (37, "auto"), (300, "lds"), (300, "tiled"), (37, "tiled")])
def test_periodic_scoring_counts_exactly(dev, N, form):
    """Contacts under the minimum-image rule as exact integers in both kernel forms (N = 300: two 256-atom pair
    tiles, diagonal and off-diagonal); mse, rmsd and first_nonfinite carry the bits of the call without a box."""
    from molecular_dynamics_neural_operator_amd import forecast
    frames, truth, counts, maps = scoring_inputs(N)
    fd, td = frames.to(dev), truth.to(dev)
    sc = forecast.score_forecast(fd, td, S_CUT, form=form, box=S_BOX)
    op = forecast.score_forecast(fd, td, S_CUT, form=form)
    assert np.array_equal(sc.contacts.cpu().numpy(), counts)
    assert bool((sc.contacts[..., 0] > op.contacts[..., 0]).all())          # faces add contacts
    assert torch.equal(sc.mse.view(torch.int64), op.mse.view(torch.int64))
    assert torch.equal(sc.rmsd.view(torch.int64), op.rmsd.view(torch.int64))
    assert torch.equal(sc.first_nonfinite, op.first_nonfinite) and sc.first_nonfinite.tolist() == [-1, -1]
    per_member = forecast.score_forecast(fd, td[:, None].expand(-1, 2, -1, -1).contiguous(), S_CUT, form=form, box=S_BOX)
    assert torch.equal(per_member.contacts, sc.contacts)
    got = forecast.contact_maps(fd, S_CUT, box=S_BOX)
    assert got.shape == (2, 2, N, N) and np.array_equal(got.cpu().numpy(), maps)
    assert np.array_equal(got.sum((2, 3)).cpu().numpy(), counts[..., 0])
    # an all-open box is the open call
    assert torch.equal(forecast.contact_maps(fd, S_CUT, box=(0, 0, 0)), forecast.contact_maps(fd, S_CUT))
    # a non-finite coordinate is in no contact, and its member's step is flagged as without a box
    bad = fd.clone()
    bad[1, 0, 5, 0] = float("nan")
    scb = forecast.score_forecast(bad, td, S_CUT, form=form, box=S_BOX)
    assert scb.first_nonfinite.tolist() == [1, -1] and int(scb.contacts[1, 0, 0]) < int(sc.contacts[1, 0, 0])
    assert torch.equal(scb.contacts[0], sc.contacts[0]) and torch.equal(scb.contacts[1, 1], sc.contacts[1, 1])


def test_engine_scores_in_its_own_box(dev):
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine, RolloutEngine
    _, wins, aa = rollout_inputs()
    model = make_model(dev, "materialized")
    truth = wins[-1:, 0].expand(R_STEPS, -1, -1).contiguous().to(dev)
    for cls in (RolloutEngine, GroupedRolloutEngine):
        eng = cls(model, R_M, R_N, R_W, R_CUT, max_steps=R_STEPS, device=dev, box=R_BOX)
        fr = eng.run(wins, aa, R_STEPS).clone()
        own, opn = eng.score(truth), eng.score(truth, box=None)
        assert torch.equal(own.contacts, forecast.score_forecast(fr, truth, R_CUT, box=R_BOX).contacts)
        assert torch.equal(opn.contacts, forecast.score_forecast(fr, truth, R_CUT).contacts)
        assert bool((own.contacts[..., 0] > opn.contacts[..., 0]).all())
        eng.close()


# ================================================================================================ 5. guard bands
COVERED = {"mdno_radius_graph_pbc", "mdno_rollout_plan_set_box", "mdno_forecast_score_pbc", "mdno_contact_maps_pbc"}


def _run_guarded(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import _lib, forecast, ops
    from molecular_dynamics_neural_operator_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    L = BOXES["three_lengths"]
    pos = random_frame(65, L, seed=3)
    E = pbc_graph(pos, CUT, L)["src"].size
    _, wins, aa = rollout_inputs()
    model = make_model(dev, "factored")
    frames, truth, _, _ = scoring_inputs(37)
    big, big_truth, _, _ = scoring_inputs(300)
    res = []
    with Guard(fill, record_calls=False) as G:
        for cap in (E, E - 3, 65):          # the attribute buffer exactly full, and one short of the graph: rows < cap only
            g, attr = ops.radius_graph_pbc(G.place(torch.from_numpy(pos).to(dev)), 65, CUT, L, edge_cap=cap)
            res += [g.row_ptr.clone(), g.src.clone(), g.dst.clone(), attr.clone(), g.num_edges.clone(), g.status.clone()]
        # dst = NULL, then edge_attr = NULL (ops always passes both)
        tp = G.place(torch.from_numpy(pos).to(dev))
        box = ops.box_arg(L)
        for with_dst, with_attr in ((False, True), (True, False), (False, False)):
            row_ptr = torch.empty(66, dtype=torch.int32, device=dev)
            src = torch.empty(E, dtype=torch.int32, device=dev)
            dst = torch.empty(E, dtype=torch.int32, device=dev) if with_dst else None
            attr = torch.empty((E, 6), dtype=torch.float32, device=dev) if with_attr else None
            ne = torch.zeros(1, dtype=torch.int32, device=dev)
            st = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(lib.mdno_radius_graph_pbc(ptr(tp), 1, 65, CUT, box, ptr(row_ptr), ptr(src), ptr(dst), ptr(attr), E,
                                                 ptr(ne), ptr(st), stream_ptr(dev)), "mdno_radius_graph_pbc")
            res += [row_ptr.clone(), src.clone(), ne.clone(), st.clone()] + [t.clone() for t in (dst, attr) if t is not None]
        for fr, tr, form in ((frames, truth, "lds"), (frames, truth, "tiled"), (big, big_truth, "tiled")):
            sc = forecast.score_forecast(G.place(fr.to(dev)), G.place(tr.to(dev)), S_CUT, form=form, box=S_BOX)
            res += [sc.mse.clone(), sc.rmsd.clone(), sc.contacts.clone(), sc.first_nonfinite.clone()]
        res.append(forecast.contact_maps(G.place(frames.to(dev)), S_CUT, box=S_BOX).clone())
        res.append(forecast.contact_maps(G.place(frames[0, 0, :35].contiguous().to(dev)), S_CUT, box=S_BOX).clone())   # 1,225 B: a tail
        for use_graph in (True, False):          # traj, workspace, counters and the engine's attribute buffer: all guarded
            out, _ = run_engine(dev, model, wins, aa, steps=3, use_graph=use_graph, box=R_BOX)
            res.append(out)
        G.verify()
    return res


def test_pbc_entry_points_stay_inside_their_buffers(dev):
    """Every entry point of include/mdno_pbc.h that writes caller memory, inside guard bands under both fill bytes:
    every band intact, and every output bitwise equal under both fills (nothing unset is read, nothing written at or
    past edge_cap)."""
    from pathlib import Path
    from guarded import FILLS, header_functions, writes_memory
    header = Path(__file__).resolve().parents[1] / "include" / "mdno_pbc.h"
    writing = {n for n, params in header_functions(header).items() if writes_memory(params)}
    assert writing == COVERED, writing ^ COVERED
    a, b = (_run_guarded(dev, fill) for fill in FILLS)
    assert len(a) == len(b) and len(a) > 40
    for i, (u, v) in enumerate(zip(a, b)):
        assert not torch.isnan(u.double()).any() and torch.equal(u, v), i
    assert torch.equal(a[-1], a[-2])          # graph replay = plain launches
