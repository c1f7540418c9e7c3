"""Training through the factored conv (`model.train_conv_mode`, csrc/train_moment.hip, include/mdno_train.h) on dense
graphs: loss, outputs and every parameter gradient against the fp64 oracle, against the materialised training path
and against the eval-mode factored forward; reproducibility; arbitrary edge lists; the memory bound (no per-edge
64 x 64 object); "auto"; an Adam run; guard bands around every buffer the new entry points write."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GEMM_MODES = ("f32", "split_bf16", "split_f16")
# (members x atoms, ker_width, depth): a single sample; 3 x 70; R = 522 crosses the 512-destination chunk; R = 74.
# None of the row counts is a multiple of 64.  The oracle's fp64 W_e is E * 32 KiB: <= 0.9 GB at 9 x 58 (E = 28k).
# k384 (a half-live second block of 256 hidden units; no multiple of 256 for the split-f16 gemm_atb below H) and k1024
# (the width of the N = 504 box) on small boxes: E = 2,652 and 1,462.
CASES = {"single": ((1, 90), 128, 1), "3x70": ((3, 70), 256, 2), "9x58": ((9, 58), 128, 2), "2x37": ((2, 37), 256, 1),
         "k384": ((2, 37), 384, 2), "k1024": ((1, 40), 1024, 1)}
WINDOW = 4


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def box_samples(members, n_atoms, seed0=0):
    """Dense box samples (density 0.1, r = 8 A) as PairData on the host."""
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    from oracle import graph_kernel_oracle as O
    out = []
    for m in range(members):
        base = syn.box_frame(n_atoms, 0.1, seed=seed0 + m)
        win = syn.jitter_window(base, WINDOW, seed=seed0 + m)
        aa = torch.from_numpy(syn.amino_acids(n_atoms, seed=seed0 + m))
        pd = O.construct_pairdata(win, aa, 8.0)
        rng = np.random.default_rng(seed0 + 1000 + m)
        y = torch.from_numpy((win[-1] + rng.normal(scale=0.1, size=win[-1].shape)).astype(np.float32))
        out.append(PairData(aa, pd["x_position"], y, pd["edge_attr"], pd["edge_index"]))
    return out


def as_dicts(samples):
    return [dict(x_position=s.x_position.cpu(), x_aminoacid=s.x_aminoacid.cpu(), y=s.y.cpu(),
                 edge_index=s.edge_index.cpu(), edge_attr=s.edge_attr.cpu()) for s in samples]


def make_model(k, depth, dev, seed=3):
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    torch.manual_seed(seed)
    model = KernelNN(64, k, depth, 6, 7, 3, 20, 4)
    with torch.no_grad():                      # keep activations O(1) through the random-init layers
        for p_ in model.conv1.net.layers[4].parameters():
            p_.mul_(0.2)
    return model.to(dev).train()


def step(model, samples, dev):
    """loss, out and the gradients of one training pass (fresh .grad)."""
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import train_forward
    model.zero_grad(set_to_none=True)
    B = len(samples)
    out = train_forward(model, samples)
    y = torch.cat([s.y for s in samples]).to(dev)
    loss = LpLoss(size_average=False)(out.view(B, -1), y.view(B, -1))
    loss.backward()
    return loss.detach().clone(), out.detach().clone(), {n: p_.grad.clone() for n, p_ in model.named_parameters()}


@functools.lru_cache(maxsize=None)
def oracle_step(case):
    from oracle import graph_kernel_oracle as O
    (members, n_atoms), k, depth = CASES[case]
    samples = box_samples(members, n_atoms)
    model = make_model(k, depth, "cpu")
    sd = {n: v.detach().cpu() for n, v in model.state_dict().items()}
    return O.train_step(sd, as_dicts(samples), depth)


@pytest.mark.parametrize("gemm_mode", GEMM_MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_factored_gradients_vs_fp64(dev, case, gemm_mode):
    """Loss 1e-5, outputs 1e-5, every parameter's gradient rel. L2 < 1e-4 against oracle.train_step in fp64 (the gates
    of test_model_gradients_vs_fp64_replica), and a second identical pass gives the same bits."""
    (members, n_atoms), k, depth = CASES[case]
    samples = box_samples(members, n_atoms)
    model = make_model(k, depth, dev)
    model.gemm_mode, model.train_conv_mode = gemm_mode, "factored"
    want_loss, want_out, want_grads = oracle_step(case)
    loss, out, grads = step(model, samples, dev)
    errs = {n: rel_err(g, want_grads[n]) for n, g in grads.items()}
    print(case, gemm_mode, "loss", abs(float(loss) - want_loss) / abs(want_loss), "out", rel_err(out, want_out),
          "grad", {n: f"{e:.1e}" for n, e in errs.items()})
    assert abs(float(loss) - want_loss) < 1e-5 * abs(want_loss)
    assert rel_err(out, want_out) < 1e-5
    assert set(errs) == set(n for n, _ in model.named_parameters())
    for n, e in errs.items():
        assert e < 1e-4, (n, e)
    loss2, out2, grads2 = step(model, samples, dev)
    assert torch.equal(loss, loss2) and torch.equal(out, out2)
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), n


@pytest.mark.parametrize("gemm_mode", GEMM_MODES)
def test_factored_equals_materialized_and_eval_forward(dev, gemm_mode):
    """Same batch through both training paths: the fp64 gates between them; the factored training forward is bitwise
    the eval-mode factored forward; a sample's rows are bitwise the same alone and inside the batch."""
    samples = box_samples(3, 70)
    model = make_model(128, 2, dev)
    model.gemm_mode = gemm_mode
    model.train_conv_mode = "materialized"
    loss_m, out_m, grads_m = step(model, samples, dev)
    model.train_conv_mode = "factored"
    loss_f, out_f, grads_f = step(model, samples, dev)
    assert abs(float(loss_f) - float(loss_m)) < 1e-5 * abs(float(loss_m))
    assert rel_err(out_f, out_m) < 1e-5
    for n in grads_m:
        assert rel_err(grads_f[n], grads_m[n]) < 1e-4, (n, rel_err(grads_f[n], grads_m[n]))
    model.conv_mode = "factored"
    model.eval()
    with torch.no_grad():
        out_eval = model([s.to(dev) for s in samples])
    model.train()
    assert torch.equal(out_f, out_eval)
    _, out_one, _ = step(model, samples[1:2], dev)
    assert torch.equal(out_one, out_f[70:140])


def test_factored_arbitrary_edge_list(dev):
    """A random directed, non-symmetric edge list with isolated destinations, self-loops and no duplicates, random
    edge attributes, two members, R = 150: against fp64 autograd over the oracle's formulas."""
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    from oracle import graph_kernel_oracle as O
    rng = np.random.default_rng(11)
    samples = []
    for m in range(2):
        n = 75
        base = box_samples(1, n, seed0=40 + m)[0]
        pairs = rng.permutation(n * n)[:1500]                   # distinct (src, dst) pairs
        src, dst = pairs // n, pairs % n
        keep = ~np.isin(dst, (3, 17, n - 1))                    # destinations without any in-edge
        src, dst = src[keep], dst[keep]
        loops = np.array([0, 5, 40])                            # self-loops, unless the pair is already there
        have = set(zip(src.tolist(), dst.tolist()))
        extra = np.array([v for v in loops if (v, v) not in have], dtype=src.dtype)
        src, dst = np.concatenate([src, extra]), np.concatenate([dst, extra])
        assert len(set(zip(src.tolist(), dst.tolist()))) == len(src)
        ei = torch.from_numpy(np.stack([src, dst])).long()
        ea = torch.from_numpy(rng.normal(size=(len(src), 6)).astype(np.float32))
        samples.append(PairData(base.x_aminoacid, base.x_position, base.y, ea, ei))
    model = make_model(128, 2, dev)
    model.gemm_mode, model.train_conv_mode = "split_bf16", "factored"
    sd = {n: v.detach().cpu() for n, v in model.state_dict().items()}
    want_loss, want_out, want_grads = O.train_step(sd, as_dicts(samples), 2)
    loss, out, grads = step(model, samples, dev)
    assert abs(float(loss) - want_loss) < 1e-5 * abs(want_loss)
    assert rel_err(out, want_out) < 1e-5
    for n, g in grads.items():
        assert rel_err(g, want_grads[n]) < 1e-4, (n, rel_err(g, want_grads[n]))


def test_factored_memory_has_no_per_edge_matrix(dev):
    """E >= 30,000 at k = 128: the peak of a whole factored step (forward, loss, backward) stays below E * 4096 * 4
    bytes, the size of W_e alone; the materialised step on the same batch does not."""
    samples = [s.to(dev) for s in box_samples(2, 180)]
    E = sum(int(s.edge_index.shape[1]) for s in samples)
    assert E >= 30000
    model = make_model(128, 1, dev)
    model.gemm_mode = "split_bf16"
    peaks = {}
    for mode in ("factored", "materialized"):
        model.train_conv_mode = mode
        step(model, samples, dev)                      # (first use: library and allocator warm)
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step(model, samples, dev)
        torch.cuda.synchronize()
        peaks[mode] = (torch.cuda.max_memory_allocated(), base)
    print("E", E, "W_e bytes", E * 4096 * 4, "peaks (max allocated, allocated before)", peaks)
    assert peaks["factored"][0] < E * 4096 * 4
    assert peaks["materialized"][0] - peaks["materialized"][1] > E * 4096 * 4


def test_auto_follows_the_counted_graph_rule(dev):
    """N = 28 chains: "auto" is bitwise the materialised gradients.  One 200-atom box member (E = 18,858 >= 16,384, mean
    degree 94 >= 40): bitwise "factored"."""
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    from molecular_dynamics_neural_operator_amd.training import resolve_train_conv_mode
    from oracle import graph_kernel_oracle as O
    chains = []
    for m in range(3):
        win = syn.jitter_window(syn.chain_frame(28, seed=m), WINDOW, seed=m)
        aa = torch.from_numpy(syn.amino_acids(28, seed=m))
        pd = O.construct_pairdata(win, aa, 8.0)
        chains.append(PairData(aa, pd["x_position"], torch.from_numpy(win[-1] * 1.01), pd["edge_attr"], pd["edge_index"]))
    dense = box_samples(1, 200)
    assert dense[0].edge_index.shape[1] >= 16384
    model = make_model(128, 1, dev)
    for samples, same_as in ((chains, "materialized"), (dense, "factored")):
        model.train_conv_mode = "auto"
        E = sum(int(s.edge_index.shape[1]) for s in samples)
        assert resolve_train_conv_mode(model, len(samples), samples[0].x_aminoacid.shape[0], E) == same_as
        loss_a, out_a, grads_a = step(model, samples, dev)
        model.train_conv_mode = same_as
        loss_b, out_b, grads_b = step(model, samples, dev)
        assert torch.equal(loss_a, loss_b) and torch.equal(out_a, out_b)
        for n in grads_a:
            assert torch.equal(grads_a[n], grads_b[n]), (same_as, n)
    # and the two formulations are different code: their bits differ on the dense member
    model.train_conv_mode = "materialized"
    _, _, grads_m = step(model, dense, dev)
    assert any(not torch.equal(grads_m[n], grads_b[n]) for n in grads_m)


def test_factored_training_reduces_loss(dev, tmp_path):
    """train_epoch + DeviceTrajectory + training.Adam with train_conv_mode="factored" on a dense synthetic trajectory:
    the loss goes down, validate_epoch runs, and a bad amino-acid id still raises through check_train_status."""
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd._lib import MdnoIndexError
    from molecular_dynamics_neural_operator_amd.dataset import ContactMapDataset, write_trajectory_npz
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import Adam, DeviceTrajectory, train_epoch, train_forward, \
        check_train_status, validate_epoch
    n = 60
    base = syn.box_frame(n, 0.1, seed=5)
    traj = syn.ou_trajectory(base, 30, sigma=0.15, theta=0.2, seed=2)
    cms = [syn.contact_map(f, 8.0) for f in traj]
    path = tmp_path / "dense.npz"
    write_trajectory_npz(path, traj, cms, syn.amino_acids(n, seed=0))
    dset = ContactMapDataset(str(path), window_size=WINDOW, horizon=1)
    dtraj = DeviceTrajectory(dset, dev)
    model = make_model(128, 1, dev, seed=0)
    model.train_conv_mode = "factored"
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
    loss_fn = LpLoss(size_average=False)
    batches = lambda: (dtraj.batch(range(s, s + 4)) for s in range(0, 24, 4))
    first, _ = train_epoch(model, batches(), opt, loss_fn)
    for _ in range(3):
        last, _ = train_epoch(model, batches(), opt, loss_fn)
    print("factored training: first epoch", first, "fourth", last)
    assert np.isfinite(first) and last < first
    val, _ = validate_epoch(model, batches(), loss_fn)
    assert np.isfinite(val)
    bad = dtraj.batch([0, 1])
    bad.x_aminoacid = bad.x_aminoacid.clone()
    bad.x_aminoacid[3] = 25
    train_forward(model, bad)
    with pytest.raises(MdnoIndexError):
        check_train_status(model)


# ---------------------------------------------------------------------------------------------- bounds
def _bounds_inputs(dev):
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd.training import collate
    batch = collate(box_samples(9, 58))              # R = 522: two chunks, the second with 10 destinations
    R = batch.x_aminoacid.shape[0]
    g = torch.Generator().manual_seed(5)
    k, depth = 128, 1
    t = dict(x0=torch.rand(R, 64, generator=g), g_out=torch.randn(R, 64, generator=g),
             w0=torch.randn(k, 6, generator=g) * 0.3, b0=torch.randn(k, generator=g) * 0.1,
             w1=torch.randn(k, k, generator=g) / k ** 0.5, b1=torch.randn(k, generator=g) * 0.1,
             w2=torch.randn(4096, k, generator=g) * 0.02, b2=torch.randn(4096, generator=g) * 0.02,
             root1=torch.randn(64, 64, generator=g) / 8, bias1=torch.randn(64, generator=g) * 0.1,
             root2=torch.randn(64, 64, generator=g) / 8, bias2=torch.randn(64, generator=g) * 0.1)
    return batch, R, k, depth, {n: v.to(dev) for n, v in t.items()}


def _h_rows(h_img, E, k):
    """The valid extent of the H image: its first E rows, row-major."""
    return h_img.view(-1, k // 32, 128, 32).permute(0, 2, 1, 3).reshape(-1, k)[:E].clone()


def _run_guarded(dev, fill, gemm_mode):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import ops
    batch, R, k, depth, t = _bounds_inputs(dev)
    with Guard(fill) as G:
        p = {n: G.place(v) for n, v in t.items()}
        graph = ops.coo_to_csr(G.place(batch.edge_index.to(dev)), R)
        by_src = ops.source_sorted(graph, R)
        E = graph.edge_count()
        X = torch.empty((2 * depth + 1, R, 64), dtype=torch.float32, device=dev)
        X[0].copy_(p["x0"])
        ea = G.place(batch.edge_attr.to(dev))
        h_img = ops.train_moment_fwd(X, graph, ea, [p[n] for n in ("w0", "b0", "w1", "b1", "w2", "b2")], p["root1"],
                                     p["bias1"], p["root2"], p["bias2"], depth, gemm_mode)
        outs = ops.train_moment_bwd(p["g_out"], X, h_img, graph, by_src, p["w2"], p["b2"], p["root1"], p["root2"], depth,
                                    gemm_mode)
        G.verify()
        res = [X.clone(), _h_rows(h_img, E, k)] + [o.clone() for o in outs]
    return res


COVERED = {"mdno_train_moment_fwd", "mdno_train_moment_bwd"}


@pytest.mark.parametrize("gemm_mode", GEMM_MODES)
def test_train_entry_points_stay_inside_their_buffers(dev, gemm_mode):
    """Both writing entry points of include/mdno_train.h inside guard bands under both fill bytes: every band intact,
    and the valid extent of every output bitwise equal under both fills (nothing unset is read)."""
    from pathlib import Path
    from guarded import FILLS, header_functions, writes_memory
    header = Path(__file__).resolve().parents[1] / "include" / "mdno_train.h"
    writing = {n for n, params in header_functions(header).items() if writes_memory(params)}
    assert writing == COVERED, writing ^ COVERED
    a, b = (_run_guarded(dev, fill, gemm_mode) for fill in FILLS)
    assert len(a) == len(b) == 7
    for i, (u, v) in enumerate(zip(a, b)):
        assert not torch.isnan(u).any() and torch.equal(u, v), i
    assert float(a[0][-1].abs().max()) > 0 and float(a[4].abs().max()) > 0 and float(a[5].abs().max()) > 0
