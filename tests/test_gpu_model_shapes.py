"""KernelNN at the sizes the reference's main() takes from its command line (--width, --kernel_width, --depth,
--out_width, --node_features, --edge_features, --num_embeddings, --embedding_dim, --window_size), away from the
width-64 configuration the rest of the suite builds:

  A  inference `model(data)` on the sample's own edge list (csrc/engine.hip): out and latent against the oracle's
     forward in fp64, widths 1-128 (generic conv kernel + separate fc2 launch off 64), ker_width 1-384 (the generic
     GEMM with row, column and K tails off the 128 tile), depth 0-3, embedding_dim 0-16, window 1-32, explicit edge
     attributes of 1, 5 and 8 columns; "factored" / "auto" bitwise "materialized" wherever the factored form does
     not apply (width 64 and ker_width % 128 == 0 only).
  B  free-running rollout (RolloutEngine) at widths 24-128, off-tile ker_width, depth 0-2, window 1 and 17.
  C  fp32 training (training.py) at width 64: loss, output and EVERY parameter gradient against the oracle's train
     step in fp64, ker_width 1-320 (ReLU backward rows that are not a multiple of 4), depth 0 (no conv: the conv
     parameters get no gradient), embedding_dim 0-16 (the three prologue-backward templates), out_width 1-7,
     window 1-16; a second pass bitwise equal; one epoch with training.Adam against torch.optim.Adam.
  D  what is not implemented is refused loudly before any device work, with the model and its gradients untouched
     (width != 64 training — width 1 used to broadcast into the 64-wide stack and read W_e out of bounds —, window
     > 16 training, bf16 training off the 128 tile, embedding_dim > 16, ker_in > 8, in_width != embedding_dim + 3,
     a rollout whose output is not a frame).

The cases are drawn once from fixed seeds: every listed value occurs, and the boundary pairs are added by hand.
Tolerances as tests/test_gpu_sweep.py (inference) and tests/test_gpu_train_sweep.py (training).
"""
import copy

import numpy as np
import pytest
import torch


def _cycle(rng, values, n):
    """n draws that contain every value (a fresh permutation per pass)."""
    out = []
    while len(out) < n:
        out += [values[i] for i in rng.permutation(len(values))]
    return out[:n]


# --------------------------------------------------------------------------- A: inference
def _fwd_cases():
    rng = np.random.default_rng(16102026)
    n = 70
    cols = dict(width=_cycle(rng, [1, 8, 24, 40, 64, 72, 128], n), k=_cycle(rng, [1, 16, 50, 96, 100, 130, 384], n),
                depth=_cycle(rng, [0, 1, 3], n), emb=_cycle(rng, [0, 1, 4, 5, 8, 9, 16], n),
                nemb=_cycle(rng, [1, 20, 33], n), out=_cycle(rng, [1, 3, 7], n), window=_cycle(rng, [1, 3, 10, 17, 32], n),
                atoms=_cycle(rng, [1, 2, 28, 65, 129], n), gemm=_cycle(rng, ["f32", "split_bf16", "split_f16"], n),
                conv=_cycle(rng, ["materialized", "factored", "auto"], n), attr=_cycle(rng, [6, 6, 1, 5, 8], n))
    out = [{k: v[i] for k, v in cols.items()} for i in range(n)]
    for c in out:
        if c["width"] > 64 and c["atoms"] == 129:      # (the fp64 oracle's W_e: E * width^2 <= 4e7)
            c["atoms"] = 65
    # boundary pairs: the factored form where it applies and just off it, the smallest model, the widest on the
    # largest graph, a K tail of one on the split GEMMs
    out += [dict(width=64, k=384, depth=3, emb=4, nemb=20, out=3, window=10, atoms=129, gemm="split_f16", conv="factored", attr=6),
            dict(width=64, k=384, depth=1, emb=9, nemb=33, out=7, window=3, atoms=65, gemm="split_bf16", conv="factored", attr=8),
            dict(width=64, k=130, depth=1, emb=4, nemb=20, out=3, window=1, atoms=65, gemm="split_f16", conv="factored", attr=6),
            dict(width=128, k=384, depth=1, emb=4, nemb=20, out=3, window=3, atoms=65, gemm="split_f16", conv="factored", attr=6),
            dict(width=72, k=384, depth=1, emb=16, nemb=33, out=3, window=32, atoms=129, gemm="f32", conv="auto", attr=6),
            dict(width=1, k=1, depth=3, emb=0, nemb=1, out=1, window=1, atoms=2, gemm="split_f16", conv="factored", attr=1),
            dict(width=128, k=130, depth=3, emb=5, nemb=33, out=7, window=17, atoms=129, gemm="split_bf16", conv="auto", attr=6),
            dict(width=64, k=129, depth=1, emb=8, nemb=20, out=3, window=10, atoms=28, gemm="split_f16", conv="materialized", attr=6)]
    for i, c in enumerate(out):
        c["id"] = i
    return out


def _model(width, k, depth, ker_in, emb, nemb, out_width, seed, dev):
    """Reference-order random init, the edge network scaled so that activations stay O(1) at every width (the
    attributes are raw coordinates, |p| up to ~40 A; a message sums `width` products), and positive biases, so
    that a narrow model is not all ReLU zeros after a few layers; a small output bias."""
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    torch.manual_seed(seed)
    model = KernelNN(width, k, depth, ker_in, emb + 3, out_width, nemb, emb)
    with torch.no_grad():
        model.conv1.net.layers[0].weight.mul_(0.25)
        for p_ in model.conv1.net.layers[4].parameters():
            p_.mul_(0.2 * min(1.0, (64.0 / width) ** 0.5))
        for b in (model.fc1.bias, model.conv1.bias, model.conv2.bias):
            b.abs_().add_(0.1)
        model.fc2.bias.mul_(0.1)       # (out_width x width 1: a bias of the size of w * latent cancels it)
    return model.to(dev)


def _sample(c, seed):
    """A window of a jittered chain, its last frame's radius graph (8 A, self-loops included) and edge attributes:
    the reference's [p_row, p_col] for ker_in 6, random columns otherwise."""
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    from oracle import graph_kernel_oracle as O
    N, W = c["atoms"], c["window"]
    win = syn.jitter_window(syn.chain_frame(N, seed=seed), W, seed=seed)
    aa = torch.from_numpy(np.random.default_rng(seed).integers(0, c["nemb"], size=N))
    s = O.construct_pairdata(win, aa, 8.0)
    ea = s["edge_attr"]
    if c["attr"] != 6:
        g = torch.Generator().manual_seed(seed)
        ea = (torch.rand(ea.shape[0], c["attr"], generator=g) * 2 - 1) * 5.0
    return PairData(x_aminoacid=aa, x_position=s["x_position"], edge_attr=ea, edge_index=s["edge_index"])


def _oracle_forward(sd, s, depth):
    """(out, latent) of the oracle's forward in fp64; the latent is the same forward with fc2 = identity."""
    from oracle import graph_kernel_oracle as O
    sd64 = {k: v.detach().cpu().double() for k, v in sd.items()}
    args = (s.x_position.cpu().double(), s.x_aminoacid.cpu(), s.edge_index.cpu(), s.edge_attr.cpu().double(), depth)
    width = sd64["fc1.weight"].shape[0]
    with torch.no_grad():
        out = O.kernelnn_forward_autograd(sd64, *args)
        lat = O.kernelnn_forward_autograd({**sd64, "fc2.weight": torch.eye(width, dtype=torch.float64),
                                           "fc2.bias": torch.zeros(width, dtype=torch.float64)}, *args)
    return out, lat


def _close(got, want, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    assert torch.isfinite(got).all(), what
    scale = max(float(want.abs().max()), 1e-30)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4 * scale, msg=lambda m: f"{what}: {m}")
    l2 = float((got - want).norm() / want.norm().clamp_min(1e-300))
    assert l2 <= 1e-5, (what, l2)


@pytest.mark.gpu
@pytest.mark.parametrize("c", _fwd_cases(), ids=lambda c: "w{width}k{k}d{depth}e{emb}x{nemb}o{out}W{window}n{atoms}a{attr}-{gemm}-{conv}".format(**c))
def test_forward_vs_fp64_oracle(c):
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    dev = torch.device("cuda:0")
    seed = 5100 + c["id"]
    s = _sample(c, seed)
    E = int(s.edge_index.shape[1])
    assert E * c["width"] ** 2 <= 4e7, "case too large for the fp64 oracle"
    model = _model(c["width"], c["k"], c["depth"], c["attr"], c["emb"], c["nemb"], c["out"], seed, dev).eval()
    model.gemm_mode, model.conv_mode = c["gemm"], c["conv"]
    sd = model.state_dict()
    pd = copy.copy(s).to(dev)
    with torch.no_grad():
        out, lat = model(pd, return_latent=True)
    assert out.shape == (c["atoms"], c["out"]) and lat.shape == (c["atoms"], c["width"])
    want_out, want_lat = _oracle_forward(sd, s, c["depth"])
    _close(lat, want_lat, "latent")
    _close(out, want_out, "out")
    factored = c["conv"] == "factored" and c["width"] == 64 and c["k"] % 128 == 0
    assert model._conv_mode_for_edges(dev, 1, c["atoms"], E) == ("factored" if factored else "materialized")
    if c["conv"] != "materialized" and not factored:
        model.conv_mode = "materialized"
        with torch.no_grad():
            m_out, m_lat = model(pd, return_latent=True)
        assert torch.equal(m_out, out) and torch.equal(m_lat, lat), "conv_mode fell back to a different computation"


# --------------------------------------------------------------------------- B: rollout
def _rollout_cases():
    rng = np.random.default_rng(17102026)
    n = 24
    cols = dict(width=_cycle(rng, [24, 40, 72, 128], n), k=_cycle(rng, [50, 96, 130], n), depth=_cycle(rng, [0, 1, 2], n),
                window=_cycle(rng, [1, 17], n), members=_cycle(rng, [1, 3], n), graph=_cycle(rng, [True, False], n),
                gemm=_cycle(rng, ["f32", "split_bf16", "split_f16"], n), atoms=_cycle(rng, [2, 28, 65], n))
    out = [{k: v[i] for k, v in cols.items()} for i in range(n)]
    for i, c in enumerate(out):
        c["id"] = i
        if c["width"] == 128 and c["atoms"] == 65:     # (oracle time: E * width^2)
            c["atoms"] = 28
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("c", _rollout_cases(), ids=lambda c: "w{width}k{k}d{depth}W{window}m{members}n{atoms}g{graph:d}-{gemm}".format(**c))
def test_rollout_vs_oracle(c):
    from molecular_dynamics_neural_operator_amd import _lib, synthetic as syn
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    from oracle import graph_kernel_oracle as O
    _lib.load()
    dev = torch.device("cuda:0")
    N, M, W, steps, seed, cutoff = c["atoms"], c["members"], c["window"], 3, 6100 + c["id"], 8.0
    sd = near_identity_state_dict(c["width"], c["k"], seed=seed, kernel_gain=2e-2, feature_gain=0.2, kernel_to_coords=1.0)
    model = KernelNN(c["width"], c["k"], c["depth"], 6, 7, 3, 20, 4)
    model.load_state_dict(sd)
    model.eval().to(dev)
    model.gemm_mode = c["gemm"]
    base = syn.jitter_window(syn.chain_frame(N, seed=seed), W, seed=seed)
    wins = syn.ensemble_windows(base, M, sigma=0.2, seed0=seed)                      # [M,W,N,3]
    aa = torch.from_numpy(syn.amino_acids(N, seed=seed))
    tm = torch.from_numpy(np.ascontiguousarray(wins.transpose(1, 0, 2, 3)))         # [W,M,N,3]
    eng = RolloutEngine(model, M, N, W, cutoff, max_steps=steps, device=dev, use_graph=c["graph"])
    traj = eng.run(tm, aa, steps).clone()
    edges = eng.edges_per_step.cpu().tolist()
    assert torch.isfinite(traj).all()
    want_edges = np.zeros(steps, dtype=np.int64)
    for m in range(M):
        s0 = O.construct_pairdata(wins[m], aa, cutoff)
        fc = O.recursive_propagation(sd, c["depth"], s0, steps, cutoff, hoist=True)
        ref = np.stack([f["x_position"][-1].numpy() for f in fc])
        got = traj[:, m].cpu().numpy()
        scale = max(float(np.abs(ref).max()), 1e-30)
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4 * scale, err_msg=f"member {m}")
        l2 = float(np.linalg.norm(got.astype(np.float64) - ref) / max(np.linalg.norm(ref.astype(np.float64)), 1e-300))
        assert l2 <= 1e-5, (m, l2)
        want_edges += np.array([s0["edge_index"].shape[1]] + [f["edge_index"].shape[1] for f in fc[:-1]])
    assert edges[:steps] == want_edges.tolist()
    if M > 1:       # the last member alone: bitwise the frames it produced inside the batch
        e1 = RolloutEngine(model, 1, N, W, cutoff, max_steps=steps, device=dev, use_graph=c["graph"])
        solo = e1.run(tm[:, M - 1:M].contiguous(), aa, steps)
        assert e1.conv_mode == eng.conv_mode == "materialized"
        assert torch.equal(solo[:, 0], traj[:, M - 1])


# --------------------------------------------------------------------------- C: training
def _train_cases():
    rng = np.random.default_rng(18102026)
    n = 60
    cols = dict(k=_cycle(rng, [1, 6, 32, 50, 96, 100, 130, 160, 200, 320], n), depth=_cycle(rng, [0, 1, 2], n),
                emb=_cycle(rng, [0, 1, 4, 5, 9, 16], n), nemb=_cycle(rng, [1, 33], n), out=_cycle(rng, [1, 3, 7], n),
                window=_cycle(rng, [1, 10, 16], n), batch=_cycle(rng, [1, 2, 3], n),
                mode=_cycle(rng, ["f32", "split_bf16", "split_f16"], n), atoms=_cycle(rng, [1, 2, 17, 28, 33, 65], n),
                cutoff=_cycle(rng, [5.0, 8.0], n))
    out = [{k: v[i] for k, v in cols.items()} for i in range(n)]
    for i, c in enumerate(out):
        c["id"] = i
    return out


def _train_samples(c, seed):
    """`batch` samples in the layout of ContactMapDataset (graph and attributes of the window's first frame), the
    target the next frame (out_width 3) or a random [N, out_width] field."""
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    N, B, W = c["atoms"], c["batch"], c["window"]
    rng = np.random.default_rng(seed)
    traj = syn.ou_trajectory(syn.chain_frame(N, seed=seed), W + B + 1, sigma=0.4, theta=0.1, seed=seed)
    aa = torch.from_numpy(rng.integers(0, c["nemb"], size=N))
    out = []
    for b in range(B):
        cm = syn.contact_map(traj[b], c["cutoff"]).reshape(2, -1)
        ei = torch.from_numpy(cm)
        p0 = torch.from_numpy(traj[b])
        y = torch.from_numpy(traj[b + W]) if c["out"] == 3 else \
            torch.from_numpy(rng.normal(scale=3.0, size=(N, c["out"])).astype(np.float32))
        out.append(PairData(x_aminoacid=aa, x_position=torch.from_numpy(np.ascontiguousarray(traj[b:b + W])), y=y,
                            edge_attr=torch.cat([p0[ei[0]], p0[ei[1]]], dim=1), edge_index=ei))
    return out


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.gpu
@pytest.mark.parametrize("c", _train_cases(), ids=lambda c: "k{k}d{depth}e{emb}x{nemb}o{out}W{window}b{batch}n{atoms}r{cutoff:g}-{mode}".format(**c))
def test_train_step_vs_fp64_oracle(c):
    from molecular_dynamics_neural_operator_amd import _lib
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN, LpLoss
    from molecular_dynamics_neural_operator_amd.training import train_forward
    from oracle import graph_kernel_oracle as O
    _lib.load()
    dev = torch.device("cuda:0")
    seed, B = 7300 + c["id"], c["batch"]
    samples = _train_samples(c, seed)
    torch.manual_seed(seed)
    model = KernelNN(64, c["k"], c["depth"], 6, c["emb"] + 3, c["out"], c["nemb"], c["emb"])
    with torch.no_grad():                      # keep activations O(1) through the random-init layers
        for p_ in model.conv1.net.layers[4].parameters():
            p_.mul_(0.2)
    model.to(dev).train()
    model.gemm_mode = c["mode"]
    out = model(samples)
    assert out.requires_grad and out.shape == (B * c["atoms"], c["out"])
    y = torch.cat([s.y for s in samples]).to(dev)
    loss = LpLoss(size_average=False)(out.view(B, -1), y.view(B, -1))
    loss.backward()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    as_dicts = [dict(x_position=s.x_position, x_aminoacid=s.x_aminoacid, y=s.y, edge_index=s.edge_index,
                     edge_attr=s.edge_attr) for s in samples]
    want_loss, want_out, want_grads = O.train_step(sd, as_dicts, c["depth"])
    assert abs(float(loss.detach()) - want_loss) < 1e-5 * abs(want_loss), (float(loss.detach()), want_loss)
    assert rel_err(out, want_out) < 1e-5, rel_err(out, want_out)
    ref_norm = float(want_grads["fc2.weight"].norm())
    for name, p_ in model.named_parameters():
        w = want_grads[name]
        if w is None:                          # depth 0: the conv block takes no part in the loss
            assert c["depth"] == 0 and name.startswith("conv"), name
            assert p_.grad is None, name
            continue
        assert p_.grad is not None, name
        if float(w.norm()) < 1e-12 * max(ref_norm, 1e-30):     # (a gradient that is exactly zero)
            assert float(p_.grad.norm()) <= 1e-6 * ref_norm, name
            continue
        assert rel_err(p_.grad, w) < 1e-4, (name, rel_err(p_.grad, w))
    g1 = {n: p_.grad.clone() for n, p_ in model.named_parameters() if p_.grad is not None}
    model.zero_grad()
    out2 = train_forward(model, samples)
    LpLoss(size_average=False)(out2.view(B, -1), y.view(B, -1)).backward()
    for n, p_ in model.named_parameters():
        if n in g1:
            assert torch.equal(p_.grad, g1[n]), n
        else:
            assert p_.grad is None, n


@pytest.mark.gpu
def test_train_epoch_adam_off_tile_matches_torch_adam():
    """Two batches at ker_width 100 (no GEMM tile fits, ReLU-backward rows of 100): train_epoch with training.Adam
    against the same steps taken by torch.optim.Adam on the gradients of the same HIP training forward."""
    from molecular_dynamics_neural_operator_amd import _lib, training
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN, LpLoss
    _lib.load()
    dev = torch.device("cuda:0")
    c = dict(atoms=28, batch=2, window=3, nemb=20, out=3, cutoff=8.0)
    batches = [_train_samples(c, 8100), _train_samples(c, 8101)]
    torch.manual_seed(8100)
    model = KernelNN(64, 100, 1, 6, 7, 3, 20, 4)
    with torch.no_grad():
        for p_ in model.conv1.net.layers[4].parameters():
            p_.mul_(0.2)
    model.to(dev).train()
    model.gemm_mode = "split_f16"
    twin = copy.deepcopy(model)
    start = {n: p_.detach().clone() for n, p_ in model.named_parameters()}
    loss_fn = LpLoss(size_average=False)
    avg, _ = training.train_epoch(model, batches, training.Adam(model.parameters(), lr=1e-3), loss_fn)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-3)
    losses = []
    for batch in batches:
        opt.zero_grad()
        out = training.train_forward(twin, batch)
        y = torch.cat([s.y for s in batch]).to(dev)
        loss = loss_fn(out.view(len(batch), -1), y.view(len(batch), -1))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert abs(avg - sum(losses) / len(losses)) <= 1e-6 * abs(avg)
    for (n, p_), (_, q_) in zip(model.named_parameters(), twin.named_parameters()):
        assert not torch.equal(p_.detach(), start[n]), f"{n} did not move"
        torch.testing.assert_close(p_.detach(), q_.detach(), rtol=1e-5, atol=1e-7, msg=lambda m: f"{n}: {m}")


# --------------------------------------------------------------------------- D: refusals
_TRAIN_REFUSALS = [
    # (id, KernelNN args (width, ker_width, depth, ker_in, in_width, out_width, num_embeddings, embedding_dim), window,
    #  train_precision, message)
    ("width1", (1, 32, 1, 6, 7, 3, 20, 4), 3, "fp32", "width 64"),
    ("width32", (32, 32, 1, 6, 7, 3, 20, 4), 3, "fp32", "width 64"),
    ("width128", (128, 32, 1, 6, 7, 3, 20, 4), 3, "fp32", "width 64"),
    ("window17", (64, 32, 1, 6, 7, 3, 20, 4), 17, "fp32", "window 17"),
    ("bf16-k100", (64, 100, 1, 6, 7, 3, 20, 4), 3, "bf16", "multiple of 128"),
    ("emb17", (64, 32, 1, 6, 20, 3, 20, 17), 3, "fp32", "embedding_dim=17"),
    ("in_width", (64, 32, 1, 6, 9, 3, 20, 4), 3, "fp32", "in_width=9"),
    ("ker_in9", (64, 32, 1, 9, 7, 3, 20, 4), 3, "fp32", "ker_in=9"),
]


def _refusal_sample(N, W, ker_in):
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    win = torch.from_numpy(syn.jitter_window(syn.chain_frame(N, seed=3), W, seed=3))
    ei = torch.from_numpy(syn.contact_map(win[0].numpy(), 8.0).reshape(2, -1))
    return PairData(x_aminoacid=torch.from_numpy(syn.amino_acids(N, seed=3)), x_position=win, y=win[-1].clone(),
                    edge_attr=torch.rand(ei.shape[1], ker_in), edge_index=ei)


def _assert_training_refused(dev, args, window, precision, message):
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.training import train_forward
    torch.manual_seed(0)
    model = KernelNN(*args).to(dev).train()
    model.train_precision = precision
    for p_ in model.parameters():
        p_.grad = torch.full_like(p_, 0.5)
    before = {n: (p_.detach().clone(), p_.grad.clone()) for n, p_ in model.named_parameters()}
    s = _refusal_sample(12, window, args[3])
    with pytest.raises(RuntimeError, match=message):
        model([s.to(dev)])
    with pytest.raises(RuntimeError, match=message):
        train_forward(model, [s])
    for n, p_ in model.named_parameters():
        assert torch.equal(p_.detach(), before[n][0]) and torch.equal(p_.grad, before[n][1]), n
    assert getattr(model, "_train_status", None) is None, "device work started before the refusal"


@pytest.mark.parametrize("case", _TRAIN_REFUSALS, ids=lambda c: c[0])
def test_training_refuses_unsupported_sizes_before_device_work(case):
    """On a CPU model: the refusal comes before the training path even looks for its device."""
    _, args, window, precision, message = case
    _assert_training_refused(torch.device("cpu"), args, window, precision, message)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _TRAIN_REFUSALS, ids=lambda c: c[0])
def test_training_refuses_unsupported_sizes_on_gpu(case):
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    _, args, window, precision, message = case
    _assert_training_refused(torch.device("cuda:0"), args, window, precision, message)


_PACK_REFUSALS = [
    ("emb17", (64, 32, 1, 6, 20, 3, 20, 17), "embedding_dim=17"),
    ("in_width", (64, 32, 1, 6, 9, 3, 20, 4), "in_width=9"),
    ("ker_in9", (64, 32, 1, 9, 7, 3, 20, 4), "ker_in=9"),
]


@pytest.mark.parametrize("case", _PACK_REFUSALS, ids=lambda c: c[0])
def test_param_pack_refuses_unsupported_sizes_on_the_host(case):
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    _, args, message = case
    with pytest.raises(MdnoError, match=message):
        ops.ParamPack(KernelNN(*args).state_dict(), args[2], "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("case", _PACK_REFUSALS, ids=lambda c: c[0])
def test_forward_refuses_unsupported_sizes(case):
    from molecular_dynamics_neural_operator_amd import _lib
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    _lib.load()
    dev = torch.device("cuda:0")
    _, args, message = case
    model = KernelNN(*args).to(dev).eval()
    before = {n: p_.detach().clone() for n, p_ in model.named_parameters()}
    with torch.no_grad(), pytest.raises(MdnoError, match=message):
        model(_refusal_sample(12, 3, args[3]).to(dev))
    for n, p_ in model.named_parameters():
        assert torch.equal(p_.detach(), before[n]), n


@pytest.mark.gpu
def test_rollout_refuses_an_output_that_is_not_a_frame():
    from molecular_dynamics_neural_operator_amd import _lib
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    _lib.load()
    for out_width in (1, 7):
        model = KernelNN(64, 128, 1, 6, 7, out_width, 20, 4).cuda().eval()
        with pytest.raises(MdnoError, match=f"out_width={out_width}"):
            RolloutEngine(model, 1, 12, 3, 8.0, max_steps=2)


@pytest.mark.parametrize("width", [1, 8, 128])
def test_conv_chain_refuses_other_widths_before_a_launch(width):
    """The chain entries read x_layers as [L, R, 64], W_e as [E, 4096] and roots as 64x64: any other shape is refused
    on the host (at width 1 a [R,1] stack used to reach the kernels and be read out of bounds)."""
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    R, E, depth = 5, 9, 1
    x = torch.zeros(2 * depth + 1, R, width)
    w_e = torch.zeros(E, width * width)
    root, bias = torch.zeros(width, width), torch.zeros(width)
    graph = ops.CSRGraph.__new__(ops.CSRGraph)
    with pytest.raises(MdnoError, match="nnconv_chain_fwd"):
        ops.nnconv_chain_fwd(x, graph, w_e, root, bias, root, bias, depth)
    with pytest.raises(MdnoError, match="nnconv_chain_bwd"):
        ops.nnconv_chain_bwd(torch.zeros(R, width), x, torch.ones(R), graph, w_e, root, root, depth)
    # the right stack with a W_e or a root of another width is refused too
    x64 = torch.zeros(2 * depth + 1, R, 64)
    with pytest.raises(MdnoError, match="w_e"):
        ops.nnconv_chain_fwd(x64, graph, w_e, torch.zeros(64, 64), torch.zeros(64), torch.zeros(64, 64), torch.zeros(64), depth)
    with pytest.raises(MdnoError, match="root"):
        ops.nnconv_chain_fwd(x64, graph, torch.zeros(E, 4096), root, bias, root, bias, depth)
    with pytest.raises(MdnoError, match="depth"):
        ops.nnconv_chain_fwd(torch.zeros(1, R, 64), graph, torch.zeros(E, 4096), torch.zeros(64, 64), torch.zeros(64),
                             torch.zeros(64, 64), torch.zeros(64), 0)
