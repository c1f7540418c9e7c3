"""Gradients with respect to the model's inputs and training through unrolled rollouts (include/mdno_unroll.h,
csrc/input_grad.hip, training.unrolled_forward): one step's input gradients, the new kernels
one by one and the unrolled step end to end against fp64 autograd over the oracle's formulas; what stays as it was;
a short Adam run; guard bands around every buffer the new entry points write."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GEMM_MODES = ("f32", "split_bf16", "split_f16")
WINDOW = 4
EPS = 2.0 ** -24                  # fp32 unit roundoff


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def make_model(k, depth, dev, seed=3):
    """Seeded reference init with the last edge-MLP layer x 0.2 (tests/test_gpu_train_factored.py make_model)."""
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    torch.manual_seed(seed)
    model = KernelNN(64, k, depth, 6, 7, 3, 20, 4)
    with torch.no_grad():
        for p_ in model.conv1.net.layers[4].parameters():
            p_.mul_(0.2)
    return model.to(dev).train()


# ================================================================================================ 1. one step's input gradients
# (members x atoms, ker_width, depth); the last: a row count that is no multiple of 64 and a width (100) that tiles none
# of the wide GEMMs (their fp32 forms run; the factored form does not apply)
CASES = {"1x30": ((1, 30), 128, 1), "3x23": ((3, 23), 256, 2), "1x65": ((1, 65), 100, 1)}
STEP_PARAMS = [(c, m, "materialized") for c in CASES for m in GEMM_MODES] + \
              [(c, m, "factored") for c in CASES if CASES[c][1] % 128 == 0 for m in GEMM_MODES]


def box_samples(members, n_atoms):
    """Box samples with coordinates of order 1 (density 0.5: the LSTM's gates are not saturated) as PairData."""
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    from oracle import graph_kernel_oracle as O
    out = []
    for m in range(members):
        base = syn.box_frame(n_atoms, 0.5, seed=m)
        win = syn.jitter_window(base, WINDOW, seed=m)
        aa = torch.from_numpy(syn.amino_acids(n_atoms, seed=m))
        pd = O.construct_pairdata(win, aa, 8.0)
        rng = np.random.default_rng(1000 + m)
        y = torch.from_numpy((win[-1] + rng.normal(scale=0.1, size=win[-1].shape)).astype(np.float32))
        out.append(PairData(aa, pd["x_position"], y, pd["edge_attr"], pd["edge_index"]))
    return out


@functools.lru_cache(maxsize=None)
def oracle_input_grads(case):
    """fp64: loss, out, parameter gradients, d loss / d x_position [W, B*N, 3] and d loss / d edge_attr [E, 6], with
    the inputs as leaves."""
    from oracle import graph_kernel_oracle as O
    (members, n_atoms), k, depth = CASES[case]
    samples = box_samples(members, n_atoms)
    sd = make_model(k, depth, "cpu").state_dict()
    params = {n: v.detach().double().clone().requires_grad_(True) for n, v in sd.items() if not n.startswith("conv2.net.")}
    xs = [s.x_position.double().requires_grad_(True) for s in samples]
    eas = [s.edge_attr.double().requires_grad_(True) for s in samples]
    outs = [O.kernelnn_forward_autograd(params, x, s.x_aminoacid, s.edge_index, ea, depth) for s, x, ea in zip(samples, xs, eas)]
    out, y = torch.cat(outs), torch.cat([s.y for s in samples]).double()
    loss = O.lp_loss_rel(out.view(members, -1), y.view(members, -1), size_average=False)
    names = list(params)
    grads = torch.autograd.grad(loss, [params[n] for n in names] + xs + eas)
    g = dict(zip(names, grads[:len(names)]))
    for n in list(g):
        if n.startswith("conv1.net."):
            g["conv2.net." + n[len("conv1.net."):]] = g[n]
    gx = torch.cat(grads[len(names):len(names) + members], dim=1)
    gea = torch.cat(grads[len(names) + members:], dim=0)
    return float(loss.detach()), out.detach(), g, gx, gea


def device_input_grads(model, samples, dev):
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import collate, train_forward
    model.zero_grad(set_to_none=True)
    batch = collate([s.to(dev) for s in samples])
    batch.x_position = batch.x_position.detach().clone().requires_grad_(True)
    batch.edge_attr = batch.edge_attr.detach().clone().requires_grad_(True)
    B = len(samples)
    out = train_forward(model, batch)
    loss = LpLoss(size_average=False)(out.view(B, -1), batch.y.view(B, -1))
    loss.backward()
    return (loss.detach().clone(), out.detach().clone(), {n: p_.grad.clone() for n, p_ in model.named_parameters()},
            batch.x_position.grad, batch.edge_attr.grad)


@pytest.mark.parametrize("case,gemm_mode,conv_mode", STEP_PARAMS)
def test_input_gradients_of_one_step_vs_fp64(dev, case, gemm_mode, conv_mode):
    """x_position.grad per frame and edge_attr.grad: rel. L2 < 1e-4 against fp64 (the project's gate for gradients);
    loss 1e-5, outputs 1e-5, parameter gradients 1e-4 as they always were; a second pass gives the same bits."""
    (members, n_atoms), k, depth = CASES[case]
    samples = box_samples(members, n_atoms)
    model = make_model(k, depth, dev)
    model.gemm_mode, model.train_conv_mode = gemm_mode, conv_mode
    want_loss, want_out, want_grads, want_gx, want_gea = oracle_input_grads(case)
    loss, out, grads, gx, gea = device_input_grads(model, samples, dev)
    assert gx is not None and gea is not None, "the inputs got no gradient"
    assert tuple(gx.shape) == tuple(want_gx.shape) and tuple(gea.shape) == tuple(want_gea.shape)
    ex = [rel_err(gx[t], want_gx[t]) for t in range(WINDOW)]
    eea = rel_err(gea, want_gea)
    errs = {n: rel_err(g, want_grads[n]) for n, g in grads.items()}
    print(case, gemm_mode, conv_mode, "x_position.grad per frame", [f"{e:.1e}" for e in ex], "norms",
          [f"{float(want_gx[t].norm()):.1e}" for t in range(WINDOW)], "edge_attr.grad", f"{eea:.1e}", "loss",
          abs(float(loss) - want_loss) / abs(want_loss), "out", rel_err(out, want_out), "params", f"{max(errs.values()):.1e}")
    assert all(float(want_gx[t].norm()) > 0 for t in range(WINDOW)) and float(want_gea.norm()) > 0
    for t, e in enumerate(ex):
        assert e < 1e-4, (t, e)
    assert eea < 1e-4, eea
    assert abs(float(loss) - want_loss) < 1e-5 * abs(want_loss)
    assert rel_err(out, want_out) < 1e-5
    for n, e in errs.items():
        assert e < 1e-4, (n, e)
    loss2, out2, grads2, gx2, gea2 = device_input_grads(model, samples, dev)
    assert torch.equal(loss, loss2) and torch.equal(out, out2) and torch.equal(gx, gx2) and torch.equal(gea, gea2)
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), n


# ================================================================================================ 2. the kernels one by one
def test_edge_mlp_input_bwd_vs_fp64(dev):
    """d_edge_attr = gz1 . W0 for E in {0, 1, 63, 65, 130, 1000} x k in {1, 100, 128, 384, 1024} x ker_in in {1, 6, 8},
    the device count below the capacity: rows past it keep what they held; and k in {7, 102} (no multiple of 4: 4-byte
    loads), {1026, 1100} (more than the 1,024 columns of W0 that are resident at a time) at ker_in 6.  The bound is the
    one any fp32 summation order satisfies, |err| <= (k + 2) eps sum_c |gz1[e, c] W0[c, j]| per element (Higham,
    gamma_k), not a measured one."""
    from molecular_dynamics_neural_operator_amd import ops
    g = torch.Generator().manual_seed(0)
    worst = 0.0
    for E in (0, 1, 63, 65, 130, 1000):
        for k in (1, 100, 128, 384, 1024, 7, 102, 1026, 1100):
            for ker_in in ((1, 6, 8) if k in (1, 100, 128, 384, 1024) else (6,)):
                cap = E + 5
                gz1 = torch.randn(cap, k, generator=g)
                gz1[torch.rand(cap, k, generator=g) < 0.5] = 0.0          # (masked by a ReLU)
                w0 = torch.randn(k, ker_in, generator=g)
                out = torch.full((cap, ker_in), 7.5, device=dev)
                ne = torch.tensor([E], dtype=torch.int32, device=dev)
                got = ops.edge_mlp_input_bwd(gz1.to(dev), w0.to(dev), ne, out=out).cpu()
                want = gz1.double() @ w0.double()
                bound = (k + 2) * EPS * (gz1.double().abs() @ w0.double().abs())
                assert torch.equal(got[E:], torch.full((cap - E, ker_in), 7.5)), (E, k, ker_in)
                err = (got[:E].double() - want[:E]).abs()
                assert bool((err <= bound[:E]).all()), (E, k, ker_in, float(err.max()))
                if E:
                    worst = max(worst, rel_err(got[:E], want[:E]))
                again = ops.edge_mlp_input_bwd(gz1.to(dev), w0.to(dev), ne).cpu()
                assert torch.equal(again[:E], got[:E])
    print("edge_mlp_input_bwd worst rel. L2", worst)
    assert ops.edge_mlp_input_bwd(torch.empty(0, 128, device=dev), torch.randn(128, 6, device=dev),
                                  torch.zeros(1, dtype=torch.int32, device=dev)).shape == (0, 6)


def arbitrary_edges(n=17, members=3, seed=4):
    """A directed list over `members` samples with self-loops, repeated pairs, atoms without in-edges, without
    out-edges and without either."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for m in range(members):
        s, d = rng.integers(0, n - 3, size=60), rng.integers(0, n - 3, size=60)      # atoms n-3 .. n-1: see below
        keep = (s != 2) & (d != 4)                                                   # 2: no out-edge, 4: no in-edge
        s, d = s[keep], d[keep]
        s = np.concatenate([s, [0, 0, 0, 5, 5, n - 3, 1]])                           # (0, 1) three times, (5, 5) twice,
        d = np.concatenate([d, [1, 1, 1, 5, 5, 6, n - 2]])                           # n-3 only a source, n-2 only a target
        src.append(s + m * n)                                                        # n-1: isolated
        dst.append(d + m * n)
    return torch.from_numpy(np.stack([np.concatenate(src), np.concatenate(dst)])).long(), n * members


def test_edge_attr_from_pos_and_its_adjoint(dev):
    """Forward against a gather, the adjoint against index_add_ in fp64 (bound: (terms + 2) eps sum |terms| per
    element), and <from_pos(p), g> = <p, pos_bwd(g)> within the bound that implies."""
    from molecular_dynamics_neural_operator_amd import ops
    ei, R = arbitrary_edges()
    E = ei.shape[1]
    gen = torch.Generator().manual_seed(1)
    pos, g = torch.randn(R, 3, generator=gen), torch.randn(E, 6, generator=gen)
    graph = ops.coo_to_csr(ei.to(dev), R)
    by_src = ops.source_sorted(graph, R)
    src, dst, perm = graph.src[:E].long().cpu(), graph.dst[:E].long().cpu(), graph.perm[:E].long().cpu()
    assert torch.equal(torch.stack([src, dst]), ei[:, perm])                         # CSR position p = input edge perm[p]
    ea = ops.edge_attr_from_pos(pos.to(dev), graph).cpu()
    assert torch.equal(ea, torch.cat([pos[src], pos[dst]], dim=1))
    d_pos = ops.edge_attr_pos_bwd(g.to(dev), graph, by_src, R).cpu()
    want = torch.zeros(R, 3, dtype=torch.float64).index_add_(0, src, g[:, :3].double()).index_add_(0, dst, g[:, 3:].double())
    mag = torch.zeros(R, 3, dtype=torch.float64).index_add_(0, src, g[:, :3].double().abs()).index_add_(0, dst, g[:, 3:].double().abs())
    terms = torch.bincount(src, minlength=R) + torch.bincount(dst, minlength=R)
    bound = (terms.double()[:, None] + 2) * EPS * mag
    assert bool(((d_pos.double() - want).abs() <= bound).all())
    for a in (2, 4, R // 3 - 1):                                                     # no out-edge, no in-edge, isolated
        assert int((src == a).sum()) == 0 or int((dst == a).sum()) == 0
    assert torch.equal(d_pos[R // 3 - 1], torch.zeros(3))
    lhs = float((ea.double() * g.double()).sum())
    rhs = float((pos.double() * d_pos.double()).sum())
    assert abs(lhs - rhs) <= float((pos.double().abs() * bound).sum()), (lhs, rhs)
    assert torch.equal(ops.edge_attr_pos_bwd(g.to(dev), graph, by_src, R).cpu(), d_pos)


def prologue_state(emb_dim, notebook, seed=5):
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    torch.manual_seed(seed)
    sd = {n: v.detach().clone() for n, v in KernelNN(64, 32, 1, 6, emb_dim + 3, 3, 20, emb_dim).state_dict().items()}
    if notebook:
        sd = {n: v for n, v in sd.items() if not n.startswith(("lstm", "conv2"))}
    return sd


def prologue_fp64(sd, frames, aa, g0):
    """d (sum x0 * g0) / d frames in fp64 autograd: frames [W, R, 3]."""
    import torch.nn.functional as F
    from oracle import graph_kernel_oracle as O
    p = {n: v.double() for n, v in sd.items()}
    x = frames.double().requires_grad_(True)
    if "lstm.weight_ih_l0" in p:
        h = F.linear(O.lstm_last_hidden_functional(x, p), p["lstm_fc.weight"], p["lstm_fc.bias"])
    else:
        h = x[-1]
    x0 = F.relu(F.linear(torch.cat((F.embedding(aa, p["emb.weight"]), h), dim=1), p["fc1.weight"], p["fc1.bias"]))
    return torch.autograd.grad((x0 * g0.double()).sum(), x)[0]


PROLOGUE_CASES = [(W, R, emb, False) for W in (1, 4, 16) for R in (1, 65, 130) for emb in (0, 4)] + \
                 [(1, R, 4, True) for R in (1, 65, 130)]


def test_node_prologue_bwd_frames_vs_fp64(dev):
    """d_frames for W in {1, 4, 16}, R in {1, 65, 130}, embedding_dim 0 and 4, and the notebook-era model (no LSTM):
    the whole tensor at rel. L2 < 1e-4 (the project's gate for a gradient against fp64), every frame at that gate up to
    the window of test 1 (W <= 4); the parameter gradients it also writes are mdno_node_prologue_bwd's bit for bit.
    R = 130 also runs as two members of 65 sharing one amino-acid list."""
    from molecular_dynamics_neural_operator_amd import ops
    gen = torch.Generator().manual_seed(2)
    for W, R, emb, notebook in PROLOGUE_CASES:
        sd = prologue_state(emb, notebook)
        pack = ops.ParamPack(sd, 1, dev)
        for M in ((1, 2) if R == 130 else (1,)):
            N = R // M
            frames = torch.randn(W, R, 3, generator=gen)
            aa = torch.randint(0, 20, (N,), generator=gen)
            g0 = torch.randn(R, 64, generator=gen)
            f_dev = frames.view(W, M, N, 3).to(dev)
            x0 = ops.node_prologue(pack, f_dev, aa.to(dev))
            plain = ops.node_prologue_bwd(pack, f_dev, aa.to(dev), x0, g0.to(dev))
            both = ops.node_prologue_bwd(pack, f_dev, aa.to(dev), x0, g0.to(dev), need_frames=True)
            assert set(both) == set(plain) | {"frames"}
            for n in plain:
                assert torch.equal(plain[n], both[n]), (W, R, emb, notebook, n)
            got = both["frames"].view(W, R, 3).cpu()
            want = prologue_fp64(sd, frames, aa.repeat(M), g0)
            e = rel_err(got, want)
            per_frame = [rel_err(got[t], want[t]) for t in range(W)]
            print("prologue d_frames", (W, R, emb, notebook, M), f"{e:.1e}", [f"{v:.1e}" for v in per_frame[:4]])
            assert float(want.norm()) > 0 and e < 1e-4, (W, R, emb, notebook, M, e)
            if W <= 4:
                assert all(v < 1e-4 for v in per_frame), (W, R, emb, notebook, M, per_frame)
            if notebook:
                assert torch.equal(got[:-1], torch.zeros(W - 1, R, 3))


# ================================================================================================ 3. EdgeAttrFromPositions
def test_edge_attr_from_positions_is_the_forward_s_own(dev):
    """On a radius graph the function's output is, bit for bit, [pos[src], pos[dst]]; the eval-mode forward gives the
    same bits whether it forms its attributes from edge_pos or is handed these; and the training forward on them is
    that forward (factored: bitwise, as tests/test_gpu_train_factored.py holds it; materialised: the 1e-5 output gate)."""
    from molecular_dynamics_neural_operator_amd import ops, synthetic as syn
    from molecular_dynamics_neural_operator_amd.training import EdgeAttrFromPositions, _forward_step
    n = 40
    win = torch.from_numpy(syn.jitter_window(syn.box_frame(n, 0.1, seed=3), WINDOW, seed=3)).to(dev)
    aa = torch.from_numpy(syn.amino_acids(n, seed=3)).to(dev)
    frame = win[-1].contiguous()
    rg = ops.radius_graph(frame, n, 8.0)
    E = rg.edge_count()
    graph = ops.CSRGraph(rg.row_ptr, rg.src[:E], rg.dst[:E], rg.num_edges, E, None, rg.status, n_edges=E)
    ea = EdgeAttrFromPositions.apply(frame, graph)
    assert torch.equal(ea, torch.cat([frame[graph.src.long()], frame[graph.dst.long()]], dim=1))
    model = make_model(128, 1, dev)
    for conv_mode in ("materialized", "factored"):
        pack = model.param_pack(dev, conv_mode=conv_mode)
        with torch.no_grad():
            out_pos, _ = ops.kernelnn_forward(pack, win.view(WINDOW, 1, n, 3), aa, graph, edge_pos=frame)
            out_attr, _ = ops.kernelnn_forward(pack, win.view(WINDOW, 1, n, 3), aa, graph, edge_attr=ea)
        assert torch.equal(out_pos, out_attr), conv_mode
        model.train_conv_mode = conv_mode
        out_train = _forward_step(model, win, aa, 1, edge_attr=ea, graph=graph)[0].detach()
        if conv_mode == "factored":
            assert torch.equal(out_train, out_pos)
        else:
            assert rel_err(out_train, out_pos) < 1e-5


# ================================================================================================ 4. the unrolled step
N_CHAIN = 28
UNROLL_CONFIGS = {"d2w4k2": (2, 4, 2, (0,)), "d1w2k3": (1, 2, 3, (0,)), "d1w2k3_b2": (1, 2, 3, (0, 5))}
# Gate of test 4 for the loss and every parameter gradient: 4 x the worst rel. L2 measured on the device over the
# three gemm_modes, both conv forms and the three configurations, 4.913e-6 (see the test's docstring); the margin
# covers other seeds and the split modes' range rules.
UNROLL_GATE = 4 * 4.913e-6


@functools.lru_cache(maxsize=None)
def chain_dataset(window):
    import tempfile
    from pathlib import Path
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.dataset import ContactMapDataset, write_trajectory_npz
    traj = syn.ou_trajectory(syn.chain_frame(N_CHAIN, seed=0), 40, sigma=0.3, theta=0.1, seed=2)
    cms = [syn.contact_map(f, 8.0) for f in traj]
    path = Path(tempfile.mkdtemp(prefix="mdno_unroll_")) / "chain.npz"
    write_trajectory_npz(path, traj, cms, syn.amino_acids(N_CHAIN, seed=0))
    return ContactMapDataset(str(path), window_size=window, horizon=1), traj


def live_model(depth, dev, k=128):
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    model = KernelNN(64, k, depth, 6, 7, 3, 20, 4)
    model.load_state_dict(near_identity_state_dict(64, k, seed=0, kernel_gain=0.02, feature_gain=0.1, kernel_to_coords=1.0))
    return model.to(dev).train()


def replica(sd, samples, ys, depth, K, graphs, detach_window=False, detach_edge=False):
    """The unrolled step in fp64 autograd over the oracle's formulas, every sample on its own (B = 1 semantics).
    `graphs[k]` (k >= 1): the edge list [2, E] (sources; targets, batch-wide node ids) step k runs on — data."""
    from oracle import graph_kernel_oracle as O
    params = {n: v.detach().cpu().double().clone().requires_grad_(True) for n, v in sd.items() if not n.startswith("conv2.net.")}
    B, N = len(samples), samples[0].x_position.shape[1]
    outs = [[] for _ in range(K)]
    for b, s in enumerate(samples):
        xp, ei, ea = s.x_position.double(), s.edge_index, s.edge_attr.double()
        for k in range(K):
            if k:
                frame = outs[k - 1][b]
                fw = frame.detach() if detach_window else frame
                fe = frame.detach() if detach_edge else frame
                xp = torch.cat([xp[1:], fw[None]])
                g = graphs[k]
                mine = (g[1] >= b * N) & (g[1] < (b + 1) * N)
                ei = g[:, mine] - b * N
                assert int(ei.min()) >= 0 and int(ei.max()) < N                      # block-diagonal
                ea = torch.cat([fe[ei[0]], fe[ei[1]]], dim=1)
            outs[k].append(O.kernelnn_forward_autograd(params, xp, s.x_aminoacid, ei, ea, depth))
    loss = sum(O.lp_loss_rel(torch.cat(outs[k]).view(B, -1), ys[k].double().view(B, -1), size_average=False)
               for k in range(K)) / K
    names = list(params)
    g = dict(zip(names, torch.autograd.grad(loss, [params[n] for n in names])))
    for n in list(g):
        if n.startswith("conv1.net."):
            g["conv2.net." + n[len("conv1.net."):]] = g[n]
    return float(loss.detach()), [torch.cat(o).detach() for o in outs], g


def device_unrolled(model, batch, ys, K, detach):
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import unrolled_forward
    model.zero_grad(set_to_none=True)
    B = batch.num_graphs
    outs, graphs = unrolled_forward(model, batch, K, detach=detach)
    loss_fn = LpLoss(size_average=False)
    loss = sum(loss_fn(outs[k].view(B, -1), ys[k].view(B, -1)) for k in range(K)) / K
    loss.backward()
    return (loss.detach().clone(), [o.detach().clone() for o in outs], graphs,
            {n: p_.grad.clone() for n, p_ in model.named_parameters()})


def max_change(g_cut, g_full):
    return max(rel_err(g_cut[n], g_full[n]) for n in g_full if float(g_full[n].norm()) > 0)


@pytest.mark.parametrize("conv_mode", ("materialized", "factored"))
@pytest.mark.parametrize("gemm_mode", GEMM_MODES)
@pytest.mark.parametrize("config", list(UNROLL_CONFIGS))
def test_unrolled_step_vs_fp64(dev, config, gemm_mode, conv_mode):
    """Live weights, N = 28 chain, K = 2 and 3 steps, one and two samples: loss and every parameter gradient against the
    fp64 replica that takes the device's per-step edge lists as data; the lists themselves against ops.radius_graph
    and the oracle's radius_graph_coo of the device's own frames; `detach=True` against the replica with detached
    feedback.  The replica's gradient changes by >= 0.1 when the window path is cut and by >= 5e-3 when the edge path is
    (so neither path can be missing unnoticed).

    Gate: UNROLL_GATE = 4 x the worst rel. L2 (loss or any parameter gradient) measured on an MI355X over the 18 cases
    of this test, full and detached.  Measured worst per configuration, the six (gemm_mode, conv form) pairs within
    10 % of each other: d2w4k2 1.67e-6 (f32 materialised), d1w2k3 4.91e-6 (split_bf16 materialised), d1w2k3_b2 3.04e-6
    (split_f16 factored); always a parameter gradient (fc1.bias or emb.weight in 32 of the 36 runs), the loss itself 2e-8 .. 1.3e-7, the
    predicted frames 1.5e-7.  A CPU fp32 restatement of the same step gave 3e-6 .. 5e-6 (EXPERIMENTS.md)."""
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory
    from oracle import graph_kernel_oracle as O
    depth, W, K, idxs = UNROLL_CONFIGS[config]
    dset, traj = chain_dataset(W)
    samples = [dset[i] for i in idxs]
    B, N = len(idxs), N_CHAIN
    model = live_model(depth, dev)
    model.gemm_mode, model.train_conv_mode = gemm_mode, conv_mode
    batch = DeviceTrajectory(dset, dev).batch(idxs, unroll=K)
    ys = batch.y_unroll
    assert torch.equal(ys.cpu(), torch.stack([torch.cat([torch.from_numpy(traj[i + W + k]) for i in idxs]) for k in range(K)]))
    assert torch.equal(batch.y, ys[0])
    sd = {n: v.detach().cpu() for n, v in model.state_dict().items()}
    worst = 0.0
    for detach in (False, True):
        loss, outs, graphs, grads = device_unrolled(model, batch, ys, K, detach)
        lists = [None]
        for k in range(1, K):
            g, frame = graphs[k], outs[k - 1]
            E = g.edge_count()
            fresh = ops.radius_graph(frame, N, 8.0)
            assert fresh.edge_count() == E and torch.equal(fresh.row_ptr, g.row_ptr)
            assert torch.equal(fresh.src[:E], g.src[:E]) and torch.equal(fresh.dst[:E], g.dst[:E])
            coo = torch.cat([torch.from_numpy(O.radius_graph_coo(frame[b * N:(b + 1) * N].cpu().numpy(), 8.0)) + b * N
                             for b in range(B)], dim=1)
            assert torch.equal(torch.stack([g.dst[:E], g.src[:E]]).long().cpu(), coo)
            lists.append(torch.stack([g.src[:E], g.dst[:E]]).long().cpu())
        want_loss, want_outs, want = replica(sd, samples, ys.cpu(), depth, K, lists, detach_window=detach, detach_edge=detach)
        if not detach:
            cut_w = replica(sd, samples, ys.cpu(), depth, K, lists, detach_window=True)[2]
            cut_e = replica(sd, samples, ys.cpu(), depth, K, lists, detach_edge=True)[2]
            dw, de = max_change(cut_w, want), max_change(cut_e, want)
            print(config, "edges per step", [sum(int(s.edge_index.shape[1]) for s in samples)] +
                  [int(l.shape[1]) for l in lists[1:]], "window path", f"{dw:.2e}", "edge path", f"{de:.2e}")
            assert dw >= 0.1 and de >= 5e-3, (dw, de)
        e_loss = abs(float(loss) - want_loss) / abs(want_loss)
        e_out = max(rel_err(o, w) for o, w in zip(outs, want_outs))
        errs = {n: rel_err(g, want[n]) for n, g in grads.items() if float(want[n].norm()) > 0}
        worst = max(worst, e_loss, max(errs.values()))
        print(config, gemm_mode, conv_mode, "detach" if detach else "full", "loss", f"{e_loss:.2e}", "out", f"{e_out:.2e}",
              "worst grad", f"{max(errs.values()):.2e}", max(errs, key=errs.get))
        assert set(grads) == set(n for n, _ in model.named_parameters())
        assert e_loss < UNROLL_GATE, e_loss
        for n, e in errs.items():
            assert e < UNROLL_GATE, (n, e)
    print("MEASURED", config, gemm_mode, conv_mode, f"{worst:.3e}")


# ================================================================================================ 5. what stays as it was
def small_trajectory(dev, window=WINDOW, frames=40):
    dset, _ = chain_dataset(window)
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory
    return DeviceTrajectory(dset, dev)


def _train_three(dev, **kw):
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import Adam, train_epoch
    dtraj = small_trajectory(dev)
    model = make_model(128, 1, dev)
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
    res = train_epoch(model, [dtraj.batch(range(s, s + 4)) for s in (0, 4, 8)], opt, LpLoss(size_average=False), **kw)
    return res, {n: p_.detach().clone() for n, p_ in model.named_parameters()}


def test_unroll_1_is_the_one_step_path(dev):
    """train_epoch(unroll=1) over three batches: the parameters (and the returned pair) of a run without the argument,
    bit for bit, alone and together with noise_std."""
    for noise in ({}, dict(noise_std=0.02, noise_seed=7, epoch=1)):
        res_a, a = _train_three(dev, **noise)
        res_b, b = _train_three(dev, unroll=1, unroll_detach=False, **noise)
        assert res_a == res_b
        for n in a:
            assert torch.equal(a[n], b[n]), n


def test_plain_step_calls_no_new_entry_point(dev, monkeypatch):
    """A plain training step (no input requires grad, no unroll) under the guard: intact bands, and none of the
    entry points of include/mdno_unroll.h is called; the same step with x_position.requires_grad calls two of them."""
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import _lib
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import train_forward
    lib = _lib.load()
    called = []
    for name in _lib.UNROLL_SIGNATURES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda real, name: lambda *a: (called.append(name), real(*a))[1])(real, name))
    dtraj = small_trajectory(dev)
    model = make_model(128, 1, dev)
    for conv_mode in ("materialized", "factored"):
        model.train_conv_mode = conv_mode
        with Guard(0xFF) as G:
            batch = dtraj.batch(range(0, 4))
            out = train_forward(model, batch)
            LpLoss(size_average=False)(out.view(4, -1), batch.y.view(4, -1)).backward()
            G.verify()
            assert "mdno_node_prologue_bwd" in G.calls
        assert called == [], called
        batch = dtraj.batch(range(0, 4))
        batch.x_position.requires_grad_(True)
        batch.edge_attr.requires_grad_(True)
        out = train_forward(model, batch)
        LpLoss(size_average=False)(out.view(4, -1), batch.y.view(4, -1)).backward()
        assert sorted(called) == ["mdno_edge_mlp_input_bwd", "mdno_node_prologue_bwd_frames"], called
        called.clear()
    # detached unrolling runs the forward entry (the fed-back step's attributes) and none of the backward ones
    from molecular_dynamics_neural_operator_amd.training import unrolled_forward
    b2 = dtraj.batch(range(0, 4), unroll=2)
    outs, _ = unrolled_forward(model, b2, 2, detach=True)
    sum(o.sum() for o in outs).backward()
    assert sorted(called) == ["mdno_collate_targets", "mdno_edge_attr_from_pos"], called


COVERED = {"mdno_edge_mlp_input_bwd", "mdno_edge_attr_from_pos", "mdno_edge_attr_pos_bwd", "mdno_node_prologue_bwd_frames",
           "mdno_collate_targets"}


def _run_guarded(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory
    dset, _ = chain_dataset(WINDOW)
    gen = torch.Generator().manual_seed(9)
    ei, R = arbitrary_edges()
    E = ei.shape[1]
    t = dict(gz1=torch.randn(E, 100, generator=gen), w0=torch.randn(100, 6, generator=gen), gz1v=torch.randn(E, 384, generator=gen),
             w0v=torch.randn(384, 8, generator=gen), pos=torch.randn(R, 3, generator=gen), g=torch.randn(E, 6, generator=gen),
             frames=torch.randn(WINDOW, 1, 65, 3, generator=gen), g0=torch.randn(65, 64, generator=gen))
    aa = torch.randint(0, 20, (65,), generator=gen)
    sd = prologue_state(4, False)
    with Guard(fill, record_calls=False) as G:
        p = {n: G.place(v.to(dev)) for n, v in t.items()}
        graph = ops.coo_to_csr(G.place(ei.to(dev)), R)
        by_src = ops.source_sorted(graph, R)
        res = [ops.edge_mlp_input_bwd(p["gz1"], p["w0"], graph.num_edges).clone(),             # scalar loads, ker_in 6
               ops.edge_mlp_input_bwd(p["gz1v"], p["w0v"], graph.num_edges).clone(),           # 16-byte loads, ker_in 8
               ops.edge_attr_from_pos(p["pos"], graph).clone(),
               ops.edge_attr_pos_bwd(p["g"], graph, by_src, R).clone()]
        pack = ops.ParamPack(sd, 1, dev)
        x0 = ops.node_prologue(pack, p["frames"], G.place(aa.to(dev)))
        grads = ops.node_prologue_bwd(pack, p["frames"], aa.to(dev), x0, p["g0"], need_frames=True)
        res += [grads[n].clone() for n in sorted(grads)]
        batch = DeviceTrajectory(dset, dev).batch([3, 0, 33], unroll=3)                           # 33 = len - 3: the last one allowed
        res += [batch.y_unroll.clone(), batch.y.clone()]
        G.verify()
    return res


def test_unroll_entry_points_stay_inside_their_buffers(dev):
    """Every entry point of include/mdno_unroll.h that writes memory inside guard bands under both fill bytes: every
    band intact, and every output bitwise equal under both fills (nothing unset is read)."""
    from pathlib import Path
    from guarded import FILLS, header_functions, writes_memory
    header = Path(__file__).resolve().parents[1] / "include" / "mdno_unroll.h"
    writing = {n for n, params in header_functions(header).items() if writes_memory(params)}
    assert writing == COVERED, writing ^ COVERED
    a, b = (_run_guarded(dev, fill) for fill in FILLS)
    assert len(a) == len(b) == 16
    for i, (u, v) in enumerate(zip(a, b)):
        assert not torch.isnan(u).any() and torch.equal(u, v), i
    assert all(float(u.abs().max()) > 0 for u in a[:4])


# ================================================================================================ 6. a short Adam run
def _adam_run(dev):
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import Adam, train_epoch
    dtraj = small_trajectory(dev)
    model = make_model(128, 1, dev, seed=0)
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
    loss_fn = LpLoss(size_average=False)
    epochs = []
    for _ in range(2):                                                               # 2 x 5 batches of 4: ten steps
        batches = (dtraj.batch(range(s, s + 4), unroll=2) for s in range(0, 20, 4))
        epochs.append(train_epoch(model, batches, opt, loss_fn, unroll=2)[0])
    return epochs, {n: p_.detach().clone() for n, p_ in model.named_parameters()}


def test_short_adam_run_on_unrolled_steps(dev):
    """Ten Adam steps at K = 2, N = 28, batch 4, k = 128: finite, the second five steps' mean loss below the first
    five's, and a second run from the same seed ends with the same parameters bit for bit."""
    epochs, params = _adam_run(dev)
    print("unrolled Adam run: mean loss of steps 1-5", epochs[0], "of steps 6-10", epochs[1])
    assert all(np.isfinite(e) for e in epochs) and all(bool(torch.isfinite(p_).all()) for p_ in params.values())
    assert epochs[1] < epochs[0]
    epochs2, params2 = _adam_run(dev)
    assert epochs2 == epochs
    for n in params:
        assert torch.equal(params[n], params2[n]), n
