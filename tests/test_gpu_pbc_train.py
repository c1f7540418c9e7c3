"""Training under a periodic box (include/mdno_pbc_train.h, csrc/pbc_train.hip; training.DeviceTrajectory(box=),
training.unrolled_forward(box=), graph_kernel.recursive_propagation(box=)): the new kernel bit
for bit against the periodic radius graph's own attribute rows and against a numpy restatement, its autograd function
against the open adjoint, device batches against the host collation, one and several unrolled steps against fp64
autograd over the oracle's formulas with the device's edge lists AND their shifts as data, the training loop and the
propagation against the rollout engine.

The fixture wraps: every test that leans on the image asserts, with the numpy rule on the frames it actually uses (the
device's fed-back frames included), that at least 20 % of the edges carry a non-zero shift and that every periodic axis
has one (`assert_wraps`) — a fixture that stopped wrapping would let an implementation that forgets the image pass."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_BOX = 37
L_BOX = 17.0
CUT = 8.0
BOXES = {"cube": (L_BOX, L_BOX, L_BOX), "slab": (L_BOX, L_BOX, 0.0)}
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def bits(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ================================================================================================ the restatement
def shifts_of(pos, src, dst, box):
    """k * L per edge and axis, f64 [E, 3]: the header's rule on fp32 coordinates, every operation a separate array
    operation (nothing is contracted)."""
    p = np.ascontiguousarray(pos, dtype=np.float32).astype(np.float64)
    L = np.asarray(box, dtype=np.float64)
    periodic = L > 0.0
    inv = np.zeros(3)
    inv[periodic] = 1.0 / L[periodic]
    d = p[src] - p[dst]
    q = d * inv
    k = np.where(periodic, np.rint(q), 0.0)
    return k * L


def attr_rule(pos, src, dst, box):
    """edge_attr[p] = [(float)((double)x_s - shift), x_d] for any directed list."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    image = (pos[src].astype(np.float64) - shifts_of(pos, src, dst, box)).astype(np.float32)
    return np.concatenate([image, pos[dst]], axis=1)


def assert_wraps(pos, src, dst, box, what=""):
    sh = shifts_of(pos, src, dst, box)
    share = float((sh != 0.0).any(1).mean())
    per_axis = (sh != 0.0).sum(0)
    assert share >= 0.2, (what, share)
    for a in range(3):
        assert box[a] == 0.0 or per_axis[a] >= 1, (what, a, per_axis)
    return share


@functools.lru_cache(maxsize=None)
def box_trajectory():
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    frame, L = syn.periodic_box_frame(N_BOX, N_BOX / L_BOX ** 3, seed=1)
    assert abs(L - L_BOX) < 1e-9                 # (the cube root is 17 to the last bit or two; the box used is 17.0)
    return syn.ou_trajectory(frame, 40, sigma=0.3, theta=0.1, seed=2)


@functools.lru_cache(maxsize=None)
def box_dataset(window):
    import tempfile
    from pathlib import Path
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.dataset import ContactMapDataset, write_trajectory_npz
    traj = box_trajectory()
    cms = [syn.contact_map(f, CUT) for f in traj]                    # the OPEN maps: a periodic trajectory ignores them
    path = Path(tempfile.mkdtemp(prefix="mdno_pbc_train_")) / "box.npz"
    write_trajectory_npz(path, traj, cms, syn.amino_acids(N_BOX, seed=0))
    return ContactMapDataset(str(path), window_size=window, horizon=1)


def csr_of(dev, src, dst, R):
    """A CSRGraph over an arbitrary directed list (sorted by the library), its CSR-order endpoints on the host."""
    from molecular_dynamics_neural_operator_amd import ops
    ei = torch.from_numpy(np.stack([src, dst])).long()
    g = ops.coo_to_csr(ei.to(dev), R)
    E = ei.shape[1]
    return g, g.src[:E].cpu().numpy(), g.dst[:E].cpu().numpy()


def raw_entry(dev, pos, g, cap, box, ne=None, rows=None, fill=7.5):
    """mdnopbt_edge_attr_from_pos itself (an all-zero box included, which ops.edge_attr_from_pos sends the open way)."""
    from molecular_dynamics_neural_operator_amd import _lib
    lib = _lib.load()
    out = torch.full((max(cap, 1), 6), fill, dtype=torch.float32, device=dev)
    ne = g.num_edges if ne is None else torch.tensor([ne], dtype=torch.int32, device=dev)
    b = (C.c_double * 3)(*box)
    rc = lib.mdnopbt_edge_attr_from_pos(_lib.ptr(pos), _lib.ptr(g.src), _lib.ptr(g.dst), _lib.ptr(ne), cap,
                                        pos.shape[0] if rows is None else rows, CUT, b, _lib.ptr(out), _lib.stream_ptr(dev))
    assert rc == 0, lib.mdno_last_error()
    return out


# ================================================================================================ 1. the kernel
KERNEL_BOXES = {"cube": (17.0, 17.0, 17.0), "slab": (17.0, 17.0, 0.0), "wire": (0.0, 0.0, 17.0),
                "two_cutoffs": (16.0, 20.0, 40.0)}


@pytest.mark.parametrize("box", sorted(KERNEL_BOXES))
@pytest.mark.parametrize("M,N", [(1, 1), (1, 37), (3, 37), (2, 65)])
def test_rows_are_the_periodic_graph_s_own(dev, M, N, box):
    """Bit equality with ops.radius_graph_pbc's attribute rows, as stored and with every atom displaced by -3 .. 3 whole
    box vectors (frames are never wrapped): the same graph, and the source images move with their destinations.  The
    coordinates lie on a 1/64 grid, so that the displaced ones are exact in fp32 and every minimum-image difference is
    the stored frame's, bit for bit: the graph cannot change and the image moves by exactly its destination's vector."""
    from molecular_dynamics_neural_operator_amd import ops
    L = np.asarray(KERNEL_BOXES[box])
    rng = np.random.default_rng(100 * N + M + len(box))
    ext = np.where(L > 0, L, 12.0)
    base = (rng.integers(0, (ext * 64).astype(np.int64), size=(M * N, 3)) / 64.0).astype(np.float32)
    vec = rng.integers(-3, 4, size=(M * N, 3)) * L
    moved = (base.astype(np.float64) + vec).astype(np.float32)
    assert np.array_equal(moved.astype(np.float64), base.astype(np.float64) + vec)
    stored = {}
    for name, pos in (("stored", base), ("displaced", moved)):
        p = torch.from_numpy(pos).to(dev)
        g, attr = ops.radius_graph_pbc(p, N, CUT, tuple(L))
        E = g.edge_count()
        graph = ops.CSRGraph(g.row_ptr, g.src[:E], g.dst[:E], g.num_edges, E, None, g.status, n_edges=E)
        got = ops.edge_attr_from_pos(p, graph, tuple(L), CUT)
        assert np.array_equal(bits(got), bits(attr[:E])), (name, M, N, box)
        src, dst = g.src[:E].cpu().numpy(), g.dst[:E].cpu().numpy()
        assert np.array_equal(bits(got), bits(attr_rule(pos, src, dst, L)))
        if name == "stored":
            stored = dict(src=src, dst=dst, row_ptr=g.row_ptr.cpu().numpy(), attr=got.cpu().numpy().astype(np.float64))
            if N >= 37 and box in BOXES:
                assert_wraps(pos, src, dst, tuple(L), (M, N, box))
            elif N >= 37:
                assert (shifts_of(pos, src, dst, L) != 0.0).any(0)[L > 0].all()        # every periodic axis wraps
        else:
            assert np.array_equal(src, stored["src"]) and np.array_equal(dst, stored["dst"])
            assert np.array_equal(g.row_ptr.cpu().numpy(), stored["row_ptr"])
            want = stored["attr"] + np.concatenate([vec[dst], vec[dst]], axis=1)      # the image moves with its destination
            assert np.array_equal(got.cpu().numpy().astype(np.float64), want)


def arbitrary_list(R, seed):
    """Directed, not from a radius graph: random pairs (most beyond the cutoff under some image), self-loops, repeats."""
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, R, size=300), rng.integers(0, R, size=300)
    s = np.concatenate([s, [0, 0, 0, 5, 5, R - 1]])
    d = np.concatenate([d, [1, 1, 1, 5, 5, R - 1]])
    return s, d


@pytest.mark.parametrize("box", sorted(KERNEL_BOXES))
def test_arbitrary_directed_list(dev, box):
    from molecular_dynamics_neural_operator_amd import ops
    L = KERNEL_BOXES[box]
    R = 65
    rng = np.random.default_rng(7)
    pos = ((rng.random((R, 3)) - 0.5) * 90.0).astype(np.float32)                    # several box lengths wide
    s, d = arbitrary_list(R, 11)
    g, src, dst = csr_of(dev, s, d, R)
    p = torch.from_numpy(pos).to(dev)
    got = ops.edge_attr_from_pos(p, g, L, CUT)
    assert np.array_equal(bits(got), bits(attr_rule(pos, src, dst, L)))
    sh = shifts_of(pos, src, dst, L)
    assert (np.abs(sh).max(0)[np.asarray(L) > 0] >= 32.0).all()                     # shifts of more than one cutoff pair: far images
    zero = raw_entry(dev, p, g, len(s), (0.0, 0.0, 0.0))
    assert np.array_equal(bits(zero), bits(ops.edge_attr_from_pos(p, g)))
    assert np.array_equal(bits(ops.edge_attr_from_pos(p, g, (0.0, 0.0, 0.0), CUT)), bits(zero))


def test_buffer_behaviour_under_guard_bands(dev):
    """Rows past *num_edges untouched, edge_cap = 0 launches nothing, out-of-range endpoints clamped; the entry inside
    guard bands under both fills with bitwise equal results."""
    from pathlib import Path
    from guarded import FILLS, Guard
    from molecular_dynamics_neural_operator_amd import _lib, ops
    header = (Path(__file__).resolve().parents[1] / "include" / "mdno_pbc_train.h").read_text()
    assert header.count("mdnopbt_") >= 1 and set(_lib.PBC_TRAIN_SIGNATURES) == {"mdnopbt_edge_attr_from_pos"}
    L = KERNEL_BOXES["cube"]
    R = 37
    pos = box_trajectory()[0]
    s, d = arbitrary_list(R, 3)
    E = len(s)
    results = []
    for fill in FILLS:
        with Guard(fill, record_calls=False) as G:
            p = G.place(torch.from_numpy(pos).to(dev))
            g = ops.coo_to_csr(G.place(torch.from_numpy(np.stack([s, d])).long().to(dev)), R)
            full = ops.edge_attr_from_pos(p, g, L, CUT).clone()
            part = raw_entry(dev, p, g, E, L, ne=E - 50).clone()                    # the count below the capacity
            over = raw_entry(dev, p, g, E - 7, L, ne=E + 100).clone()               # the count above it: capacity rules
            none = raw_entry(dev, p, g, 0, L).clone()                               # edge_cap = 0
            bad = g.src.clone()
            bad[0], bad[1] = -5, R + 9
            gb = ops.CSRGraph(g.row_ptr, bad, g.dst, g.num_edges, g.edge_cap, None, g.status, n_edges=E)
            clamped = ops.edge_attr_from_pos(p, gb, L, CUT).clone()
            G.verify()
        src, dst = g.src[:E].cpu().numpy(), g.dst[:E].cpu().numpy()
        want = attr_rule(pos, src, dst, L)
        assert np.array_equal(bits(full), bits(want))
        assert np.array_equal(bits(part[:E - 50]), bits(want[:E - 50])) and bool((part[E - 50:] == 7.5).all())
        assert np.array_equal(bits(over), bits(want[:E - 7]))
        assert bool((none == 7.5).all())
        src_c = src.copy()
        src_c[0], src_c[1] = 0, R - 1
        assert np.array_equal(bits(clamped), bits(attr_rule(pos, src_c, dst, L)))
        results.append([full, part, over, clamped])
    for u, v in zip(*results):
        assert torch.equal(u, v) and not torch.isnan(u).any()


def test_autograd_is_the_open_adjoint(dev):
    """Backward bit-equal to the open function's for the same graph and incoming gradient, and equal to fp64 autograd of
    cat(pos[src] - shift, pos[dst]) with the shift as data within (terms + 2) eps sum |g| per entry."""
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd.training import EdgeAttrFromPositions
    L = BOXES["cube"]
    pos = torch.from_numpy(box_trajectory()[0])
    R = pos.shape[0]
    g, _ = ops.radius_graph_pbc(pos.to(dev), R, CUT, L, with_attr=False)
    E = g.edge_count()
    graph = ops.CSRGraph(g.row_ptr, g.src[:E], g.dst[:E], g.num_edges, E, None, g.status, n_edges=E)
    src, dst = graph.src.long().cpu(), graph.dst.long().cpu()
    assert_wraps(pos.numpy(), src.numpy(), dst.numpy(), L)
    gin = torch.randn(E, 6, generator=torch.Generator().manual_seed(5))
    grads = []
    for args in ((L, CUT), ()):
        p = pos.to(dev).requires_grad_(True)
        ea = EdgeAttrFromPositions.apply(p, graph, *args)
        ea.backward(gin.to(dev))
        grads.append(p.grad.cpu())
    assert torch.equal(grads[0], grads[1])
    shift = torch.from_numpy(shifts_of(pos.numpy(), src.numpy(), dst.numpy(), L))
    p64 = pos.double().requires_grad_(True)
    (torch.cat([p64[src] - shift, p64[dst]], dim=1) * gin.double()).sum().backward()
    mag = torch.zeros(R, 3, dtype=torch.float64).index_add_(0, src, gin[:, :3].double().abs()).index_add_(0, dst, gin[:, 3:].double().abs())
    terms = torch.bincount(src, minlength=R) + torch.bincount(dst, minlength=R)
    assert bool(((grads[0].double() - p64.grad).abs() <= (terms.double()[:, None] + 2) * EPS * mag).all())


# ================================================================================================ 2. batches
def host_batch(dset, idx, box, dev):
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    from molecular_dynamics_neural_operator_amd.graph_kernel import construct_pairdata
    from molecular_dynamics_neural_operator_amd.training import collate
    samples = []
    for i in idx:
        s = dset[i]
        pd = construct_pairdata(s.x_position[:1], s.x_aminoacid, CUT, box=box)
        samples.append(PairData(s.x_aminoacid.to(dev), s.x_position.to(dev), s.y.to(dev), pd.edge_attr, pd.edge_index))
    return collate(samples), samples


RAGGED = (3, 0, 17, 8, 8, 30, 1, 25, 12)


@pytest.mark.parametrize("box", sorted(BOXES))
def test_device_batches_are_the_host_collation(dev, box):
    from test_gpu_pbc import pbc_graph
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory
    B_ = BOXES[box]
    K = 3
    dset = box_dataset(4)
    traj = box_trajectory()
    dtraj = DeviceTrajectory(dset, dev, box=B_, cutoff=CUT)
    opn = DeviceTrajectory(dset, dev)
    want_counts = [pbc_graph(f, CUT, B_)["src"].size for f in traj]
    assert dtraj.counts.tolist() == want_counts and dtraj.counts.dtype == np.int64
    for idx in ((0,), (0, 5), RAGGED):
        got, ref = dtraj.batch(idx, unroll=K), opn.batch(idx, unroll=K)
        for f in ("x_position", "y", "y_unroll", "x_aminoacid"):
            assert torch.equal(getattr(got, f), getattr(ref, f)), (idx, f)
        want, _ = host_batch(dset, idx, B_, dev)
        assert got.edge_index.dtype == torch.long and torch.equal(got.edge_index, want.edge_index), idx
        assert np.array_equal(bits(got.edge_attr), bits(want.edge_attr)), idx
        assert got.box == B_ and got.cutoff == CUT and got.num_graphs == len(idx) and got.rows_per_sample == N_BOX
        assert got.sample_ids.tolist() == list(idx)
        assert len(idx) < 9 or len(set(dtraj.counts[list(idx)].tolist())) > 1       # ragged
        ei = got.edge_index.cpu().numpy()
        first = got.x_position[0].cpu().numpy()
        assert_wraps(first, ei[0], ei[1], B_, idx)
        assert np.array_equal(bits(got.edge_attr), bits(attr_rule(first, ei[0], ei[1], B_)))
        noisy = dtraj.batch(idx, noise_std=0.05, noise_seed=3, epoch=1, unroll=K)
        assert torch.equal(noisy.edge_index, got.edge_index) and np.array_equal(bits(noisy.edge_attr), bits(got.edge_attr))
        assert torch.equal(noisy.y, got.y) and torch.equal(noisy.y_unroll, got.y_unroll)
        assert not torch.equal(noisy.x_position, got.x_position)
        assert torch.equal(noisy.x_position, opn.batch(idx, noise_std=0.05, noise_seed=3, epoch=1, unroll=K).x_position)


def spy_new_entries(monkeypatch):
    from molecular_dynamics_neural_operator_amd import _lib
    lib = _lib.load()
    called = []
    for name in list(_lib.PBC_TRAIN_SIGNATURES) + ["mdno_radius_graph_pbc"]:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda real, name: lambda *a: (called.append(name), real(*a))[1])(real, name))
    return called


def test_no_box_calls_nothing_new(dev, monkeypatch):
    """DeviceTrajectory and unrolled_forward without a box: today's bits, and neither mdnopbt_ nor mdno_radius_graph_pbc
    is called (the same run without the spy gives the same tensors)."""
    from test_gpu_unroll import chain_dataset, live_model
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory, unrolled_forward
    dset, _ = chain_dataset(4)
    model = live_model(1, dev)

    def run(**kw):
        dtraj = DeviceTrajectory(dset, dev, **kw)
        b = dtraj.batch((0, 5), unroll=2)
        with torch.no_grad():
            outs, _ = unrolled_forward(model, b, 2, **({"box": None} if kw else {}))
        return [b.x_position, b.y, b.y_unroll, b.edge_index, b.edge_attr] + list(outs)
    plain = run()
    called = spy_new_entries(monkeypatch)
    spied = run(box=None, cutoff=8.0)
    zero = run(box=(0.0, 0.0, 0.0))
    assert called == [], called
    for u, v, w in zip(plain, spied, zero):
        assert torch.equal(u, v) and torch.equal(u, w)
    assert getattr(DeviceTrajectory(dset, dev).batch((0,)), "box", None) is None


# ================================================================================================ 3. training
def replica(sd, xp, aa, ys, depth, K, lists, shifts, ea0, dtype=torch.float64, detach_window=False, detach_edge=False,
            zero_shift=False):
    """The unrolled periodic step in `dtype` autograd over the oracle's formulas, every sample on its own.  Data: the
    windows xp [W, B N, 3], lists[k] [2, E_k] (sources; targets, batch-wide ids), shifts[k] f64 [E_k, 3] for every step,
    ea0 = the first step's attribute rows.  A fed-back step forms ea = cat(frame[src] - shift, frame[dst]).
    zero_shift: open attributes on the periodic topology (what an implementation that forgets the image computes)."""
    from oracle import graph_kernel_oracle as O
    params = {n: v.detach().cpu().to(dtype).clone().requires_grad_(True) for n, v in sd.items() if not n.startswith("conv2.net.")}
    N = aa.shape[0]
    B = xp.shape[1] // N
    outs = [[] for _ in range(K)]
    for b in range(B):
        win = xp[:, b * N:(b + 1) * N].to(dtype)
        for k in range(K):
            g = lists[k]
            mine = (g[1] >= b * N) & (g[1] < (b + 1) * N)
            ei = g[:, mine] - b * N
            assert int(ei.min()) >= 0 and int(ei.max()) < N
            if k == 0:
                ea = torch.cat([win[0][ei[0]], win[0][ei[1]]], dim=1) if zero_shift else ea0[mine].to(dtype)
            else:
                frame = outs[k - 1][b]
                fw = frame.detach() if detach_window else frame
                fe = frame.detach() if detach_edge else frame
                win = torch.cat([win[1:], fw[None]])
                sh = torch.zeros((int(mine.sum()), 3), dtype=dtype) if zero_shift else shifts[k][mine].to(dtype)
                ea = torch.cat([fe[ei[0]] - sh, fe[ei[1]]], dim=1)
            outs[k].append(O.kernelnn_forward_autograd(params, win, aa, ei, ea, depth))
    loss = sum(O.lp_loss_rel(torch.cat(outs[k]).view(B, -1), ys[k].to(dtype).view(B, -1), size_average=False)
               for k in range(K)) / K
    names = list(params)
    g = dict(zip(names, torch.autograd.grad(loss, [params[n] for n in names])))
    for n in list(g):
        if n.startswith("conv1.net."):
            g["conv2.net." + n[len("conv1.net."):]] = g[n]
    return float(loss.detach()), [torch.cat(o).detach() for o in outs], g


def worst_err(loss, grads, want_loss, want):
    from test_gpu_unroll import rel_err
    errs = {n: rel_err(g, want[n]) for n, g in grads.items() if float(want[n].norm()) > 0}
    errs["loss"] = abs(float(loss) - want_loss) / abs(want_loss)
    return max(errs.values()), max(errs, key=errs.get)


GEMM_MODES = ("f32", "split_bf16", "split_f16")


@pytest.mark.parametrize("conv_mode", ("materialized", "factored"))
@pytest.mark.parametrize("gemm_mode", GEMM_MODES)
@pytest.mark.parametrize("B,depth", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_one_step_on_a_periodic_batch_vs_fp64(dev, B, depth, gemm_mode, conv_mode):
    """k = 128: loss at 1e-5 and every parameter gradient at 1e-4 (the project's gates for one step against fp64, tests/
    test_gpu_unroll.py test 1) against fp64 autograd over the oracle's formulas with the batch's edges and attributes as
    data."""
    from test_gpu_unroll import live_model, rel_err
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory, train_forward
    box = BOXES["cube" if B == 1 else "slab"]
    dset = box_dataset(4)
    batch = DeviceTrajectory(dset, dev, box=box).batch((0, 5)[:B])
    model = live_model(depth, dev)
    model.gemm_mode, model.train_conv_mode = gemm_mode, conv_mode
    model.zero_grad(set_to_none=True)
    out = train_forward(model, batch)
    loss = LpLoss(size_average=False)(out.view(B, -1), batch.y.view(B, -1))
    loss.backward()
    grads = {n: p_.grad.clone() for n, p_ in model.named_parameters()}
    ei = batch.edge_index.cpu()
    first = batch.x_position[0].cpu().numpy()
    assert_wraps(first, ei[0].numpy(), ei[1].numpy(), box)
    sd = {n: v.detach().cpu() for n, v in model.state_dict().items()}
    want_loss, want_outs, want = replica(sd, batch.x_position.cpu(), dset.x_aminoacid, batch.y_unroll.cpu(), depth, 1, [ei],
                                         [None], batch.edge_attr.cpu())
    e, where = worst_err(loss, grads, want_loss, want)
    print("periodic step", B, depth, gemm_mode, conv_mode, "loss", abs(float(loss) - want_loss) / abs(want_loss), "out",
          rel_err(out, want_outs[0]), "worst", f"{e:.2e}", where)
    assert abs(float(loss) - want_loss) < 1e-5 * abs(want_loss) and rel_err(out, want_outs[0]) < 1e-5
    for n, g in grads.items():
        if float(want[n].norm()) > 0:
            assert rel_err(g, want[n]) < 1e-4, n


UNROLL_CONFIGS = {"d2w4k2_cube": (2, 4, 2, (0,), "cube"), "d1w2k3_b2_slab": (1, 2, 3, (0, 5), "slab")}


@pytest.mark.parametrize("conv_mode", ("materialized", "factored"))
@pytest.mark.parametrize("gemm_mode", GEMM_MODES)
@pytest.mark.parametrize("config", sorted(UNROLL_CONFIGS))
def test_unrolled_periodic_step_vs_fp64(dev, config, gemm_mode, conv_mode):
    """tests/test_gpu_unroll.py test_unrolled_step_vs_fp64 under a box: K = 2 (cube, one sample, depth 2) and K = 3 (slab,
    two samples): the loss and every parameter gradient against the fp64 replica that takes the device's per-step edge
    lists AND their shifts as data; the lists exactly against ops.radius_graph_pbc of the device's own frames and the
    numpy rule; detach=True against the replica with detached feedback.

    Gate per case: max(UNROLL_GATE, 4 x e32), e32 = the worst rel. L2 (loss, parameter gradients) between the same replica
    in fp32 on the CPU and in fp64 — the reference arithmetic's own error, not the device's.  Honesty, on the replica
    alone: cutting the window path moves the gradient by >= 0.1, cutting the edge path by >= 5e-3, and the replica with
    every shift set to zero differs from the right one by >= 10 x the gate.

    Measured on an MI355X over the 12 cases, full and detached: worst e32 8.56e-7 (d1w2k3_b2_slab detached; d2w4k2_cube
    7.25e-7), worst device error 8.60e-7 (d1w2k3_b2_slab, split_f16 materialised, detached; d2w4k2_cube 6.40e-7, split_f16
    materialised), always emb.weight's gradient; 4 x e32 < UNROLL_GATE in every case, so the gate is UNROLL_GATE =
    1.965e-5.  The zero-shift replica is 0.35 (slab) and 0.45 (cube) away; window path 0.34 / 0.51, edge path 3.3e-2 /
    2.5e-2."""
    from test_gpu_pbc import pbc_graph_members
    from test_gpu_unroll import UNROLL_GATE, live_model, max_change
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory, unrolled_forward
    depth, W, K, idxs, box_name = UNROLL_CONFIGS[config]
    box = BOXES[box_name]
    dset = box_dataset(W)
    B, N = len(idxs), N_BOX
    model = live_model(depth, dev)
    model.gemm_mode, model.train_conv_mode = gemm_mode, conv_mode
    batch = DeviceTrajectory(dset, dev, box=box).batch(idxs, unroll=K)
    ys = batch.y_unroll
    sd = {n: v.detach().cpu() for n, v in model.state_dict().items()}
    xp, aa, ea0 = batch.x_position.cpu(), dset.x_aminoacid, batch.edge_attr.cpu()
    for detach in (False, True):
        model.zero_grad(set_to_none=True)
        outs, graphs = unrolled_forward(model, batch, K, detach=detach)
        loss_fn = LpLoss(size_average=False)
        loss = sum(loss_fn(outs[k].view(B, -1), ys[k].view(B, -1)) for k in range(K)) / K
        loss.backward()
        grads = {n: p_.grad.clone() for n, p_ in model.named_parameters()}
        lists, shifts = [batch.edge_index.cpu()], [None]
        first = xp[0].numpy()
        shifts[0] = torch.from_numpy(shifts_of(first, lists[0][0].numpy(), lists[0][1].numpy(), box))
        assert_wraps(first, lists[0][0].numpy(), lists[0][1].numpy(), box, "step 0")
        for k in range(1, K):
            g, frame = graphs[k], outs[k - 1].detach()
            E = g.edge_count()
            fresh, _ = ops.radius_graph_pbc(frame, N, CUT, box, with_attr=False)
            assert fresh.edge_count() == E and torch.equal(fresh.row_ptr, g.row_ptr)
            assert torch.equal(fresh.src[:E], g.src[:E]) and torch.equal(fresh.dst[:E], g.dst[:E])
            f_np = frame.cpu().numpy()
            want_g = pbc_graph_members(f_np, N, CUT, box)
            src, dst = g.src[:E].cpu().numpy(), g.dst[:E].cpu().numpy()
            assert np.array_equal(src, want_g["src"]) and np.array_equal(dst, want_g["dst"])
            assert_wraps(f_np, src, dst, box, f"step {k}")
            lists.append(torch.from_numpy(np.stack([src, dst])).long())
            shifts.append(torch.from_numpy(shifts_of(f_np, src, dst, box)))
        args = (sd, xp, aa, ys.cpu(), depth, K, lists, shifts, ea0)
        want_loss, _, want = replica(*args, detach_window=detach, detach_edge=detach)
        l32, _, g32 = replica(*args, dtype=torch.float32, detach_window=detach, detach_edge=detach)
        e32, _ = worst_err(l32, g32, want_loss, want)
        gate = max(UNROLL_GATE, 4 * e32)
        if not detach:
            dw = max_change(replica(*args, detach_window=True)[2], want)
            de = max_change(replica(*args, detach_edge=True)[2], want)
            zl, _, zg = replica(*args, zero_shift=True)
            dz, _ = worst_err(zl, zg, want_loss, want)
            print(config, "edges per step", [int(l.shape[1]) for l in lists], "window path", f"{dw:.2e}", "edge path",
                  f"{de:.2e}", "zero shifts", f"{dz:.2e}", "gate", f"{gate:.2e}")
            assert dw >= 0.1 and de >= 5e-3, (dw, de)
            assert dz >= 10 * gate, (dz, gate)
        e, where = worst_err(loss, grads, want_loss, want)
        print("MEASURED", config, gemm_mode, conv_mode, "detach" if detach else "full", "e32", f"{e32:.3e}", "device",
              f"{e:.3e}", where, "gate", f"{gate:.3e}")
        assert set(grads) == set(n for n, _ in model.named_parameters())
        assert e < gate, (e, where, gate)


def test_path_equivalences_and_refusals(dev):
    from test_gpu_unroll import live_model
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory, train_forward, unrolled_forward
    box = BOXES["cube"]
    batch = DeviceTrajectory(box_dataset(4), dev, box=box).batch((0, 5), unroll=2)
    model = live_model(1, dev)
    with torch.no_grad():
        one, _ = unrolled_forward(model, batch, 1)
        assert torch.equal(one[0], train_forward(model, batch))
        same, _ = unrolled_forward(model, batch, 2, box=box)
        own, _ = unrolled_forward(model, batch, 2)
        assert torch.equal(same[1], own[1])
    for kw in (dict(box=(18.0, 17.0, 17.0)), dict(box=BOXES["slab"]), dict(cutoff=7.0), dict(box=(0.0, 0.0, 0.0))):
        with pytest.raises(MdnoError):
            unrolled_forward(model, batch, 2, **kw)


def _train_three(dev, **kw):
    from test_gpu_unroll import make_model
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import Adam, DeviceTrajectory, train_epoch
    dtraj = DeviceTrajectory(box_dataset(4), dev, box=BOXES["cube"])
    model = make_model(128, 1, dev)
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
    res = train_epoch(model, [dtraj.batch(range(s, s + 3), unroll=2) for s in (0, 4, 8)], opt, LpLoss(size_average=False),
                      unroll=2, **kw)
    return res, {n: p_.detach().clone() for n, p_ in model.named_parameters()}


@pytest.mark.parametrize("noise", (0.0, 0.05))
def test_training_loop_on_periodic_batches(dev, noise, monkeypatch):
    """train_epoch(unroll=2) on three periodic batches twice from the same state: the same parameters bit for bit, finite
    losses; with noise_std the rebuilt batch keeps y_unroll, box and cutoff (the periodic entries run)."""
    kw = dict(noise_std=noise, noise_seed=7, epoch=1) if noise else {}
    res_a, a = _train_three(dev, **kw)
    called = spy_new_entries(monkeypatch)
    res_b, b = _train_three(dev, **kw)
    assert "mdnopbt_edge_attr_from_pos" in called and "mdno_radius_graph_pbc" in called
    assert res_a == res_b and all(np.isfinite(v) for v in res_a)
    for n in a:
        assert torch.equal(a[n], b[n]) and bool(torch.isfinite(a[n]).all()), n


def test_data_parallel_world_size_one(dev):
    from test_gpu_unroll import make_model
    from molecular_dynamics_neural_operator_amd.data_parallel import DataParallelTrainer
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import Adam, DeviceTrajectory, train_epoch
    dtraj = DeviceTrajectory(box_dataset(4), dev, box=BOXES["cube"])
    runs = []
    for parallel in (False, True):
        model = make_model(128, 1, dev)
        opt = Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
        loss_fn = LpLoss(size_average=False)
        if parallel:
            res = DataParallelTrainer(model, opt, loss_fn).train_epoch([list(range(s, s + 4)) for s in (0, 4)], source=dtraj)
        else:
            res = train_epoch(model, [dtraj.batch(range(s, s + 4)) for s in (0, 4)], opt, loss_fn)
        runs.append((res, {n: p_.detach().clone() for n, p_ in model.named_parameters()}))
    assert runs[0][0] == runs[1][0] and all(np.isfinite(v) for v in runs[0][0])
    for n, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][n]), n


# ================================================================================================ 4. propagation
class PeriodicSamples:
    """dataset-like: sample i = the stored window with the periodic edges of construct_pairdata(window, aa, 8, box=)."""

    def __init__(self, dset, box):
        self.dset, self.box = dset, box

    def __len__(self):
        return len(self.dset)

    def __getitem__(self, i):
        from molecular_dynamics_neural_operator_amd.dataset import PairData
        from molecular_dynamics_neural_operator_amd.graph_kernel import construct_pairdata
        s = self.dset[i]
        pd = construct_pairdata(s.x_position, s.x_aminoacid, CUT, box=self.box)
        return PairData(s.x_aminoacid, s.x_position, s.y, pd.edge_attr.cpu(), pd.edge_index.cpu())


@pytest.mark.parametrize("box", sorted(BOXES))
def test_recursive_propagation_under_a_box(dev, box):
    from test_gpu_unroll import live_model
    from molecular_dynamics_neural_operator_amd.graph_kernel import construct_pairdata, propogate, recursive_propagation
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    B_ = BOXES[box]
    W, steps = 4, 4
    dlike = PeriodicSamples(box_dataset(W), B_)
    model = live_model(1, dev).eval()
    got = recursive_propagation(model, dlike, dev, steps, [0, 3], box=B_)
    assert len(got) == 2 * steps
    for j, start in enumerate((0, 3)):
        s = dlike[start]
        eng = RolloutEngine(model, members=1, n_atoms=N_BOX, window=W, threshold=CUT, max_steps=steps, device=dev, box=B_)
        eng.reset(s.x_position.unsqueeze(1), s.x_aminoacid)
        eng.first_step_from_sample(s.edge_index, s.edge_attr)
        eng.step(steps - 1)
        eng.synchronize()
        traj = eng.frames()[:, 0].cpu()
        for i in range(steps):
            f = got[j * steps + i]
            assert torch.equal(f.x_position[-1], traj[i]), (start, i)
            want = construct_pairdata(f.x_position, s.x_aminoacid, CUT, box=B_)
            assert torch.equal(f.edge_index, want.edge_index.cpu()) and np.array_equal(bits(f.edge_attr), bits(want.edge_attr))
            ei = f.edge_index.numpy()
            assert_wraps(f.x_position[-1].numpy(), ei[0], ei[1], B_, (start, i))
    fc, metrics = propogate(model, dlike, dev, steps, box=B_)
    assert len(metrics["mse"]) == steps
    for f, w in zip(fc, got[:steps]):
        assert torch.equal(f.x_position, w.x_position) and torch.equal(f.edge_index, w.edge_index)
        assert np.array_equal(bits(f.edge_attr), bits(w.edge_attr))


def test_open_propagation_is_untouched(dev, monkeypatch):
    from test_gpu_unroll import chain_dataset, live_model
    from molecular_dynamics_neural_operator_amd.graph_kernel import propogate, recursive_propagation
    dset, _ = chain_dataset(4)
    model = live_model(1, dev).eval()
    plain = recursive_propagation(model, dset, dev, 3, [0, 3])
    called = spy_new_entries(monkeypatch)
    keyword = recursive_propagation(model, dset, dev, 3, [0, 3], box=None)
    assert called == []
    for u, v in zip(plain, keyword):
        for f in ("x_position", "edge_index", "edge_attr"):
            assert torch.equal(getattr(u, f), getattr(v, f)), f
    a, ma = propogate(model, dset, dev, 3)
    b, mb = propogate(model, dset, dev, 3, box=None)
    assert ma == mb and all(torch.equal(u.x_position, v.x_position) for u, v in zip(a, b))
