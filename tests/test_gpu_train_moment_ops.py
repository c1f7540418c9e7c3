"""The two entry points of include/mdno_train.h called directly (`ops.train_moment_fwd`, `ops.train_moment_bwd`) at
ker_width 256 .. 1024, every one of their seven outputs against fp64 autograd over the formulas the header documents,
as whole tensors AND per slice of ownership: every destination row, every column block of 256 hidden units, every
edge row, every (i, column block) of d_w2, every i of d_b2.  A kernel that is wrong in one block of hidden units
(`blockIdx.x = cq > 0` of tm_edge_kernel, the cq sum of tm_gather_kernel), one chunk of destinations or one slice of
d_w2 shows in that slice at full size instead of diluted in a whole-tensor norm.

    err(slice) = |got - want|_slice / max(|want|_slice, |want|_tensor / sqrt(n_slices))

(the floor is for slices that cancel: a condition, not a tolerance).  The gates are the project's own, of
test_gpu_train_factored.py::test_factored_gradients_vs_fp64: 1e-5 for the forward (X, H), 1e-4 for the backward.

ReLU thresholds.  Margin = 1e-4 * rms of the fp64 pre-activation tensor (ten times the forward gate).  The node seeds
below are chosen so that NO node pre-activation p_a of the reference lies inside the margin (asserted: the device then
has to take the reference's branch everywhere); for z1 (E * k elements) that cannot be had: its elements inside the
margin are left out of gz2's comparison, of nothing else, and their share is asserted <= 1e-3.

Room under the gates, measured on the CPU: the same reference function in torch float32 against fp64 through the
same measure (largest figure over whole tensors and slices; the least room under a gate is 12x, X of k1024_edges),
and the share of z1 inside the margin:

    case            X        H        gz       g_in     gz2      d_w2     d_b2     z1 share
    k256_control    3.2e-07  2.1e-07  1.7e-07  2.2e-07  3.6e-07  2.3e-07  1.4e-07  9.0e-05
    k384            3.5e-07  2.5e-07  3.8e-07  4.3e-07  5.1e-07  3.0e-07  2.4e-07  9.9e-05
    k512            2.5e-07  2.2e-07  2.2e-07  2.9e-07  3.5e-07  2.2e-07  1.4e-07  1.0e-04
    k640            2.7e-07  2.4e-07  2.2e-07  3.1e-07  4.0e-07  2.0e-07  1.3e-07  7.6e-05
    k1024_edges     8.2e-07  2.4e-07  4.8e-07  6.9e-07  5.7e-07  5.4e-07  3.8e-07  8.9e-05
    k128_no_edges   3.5e-07  0        3.1e-07  3.4e-07  (empty)  0        0        (no z1)
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_train_factored import GEMM_MODES, _h_rows

pytestmark = pytest.mark.gpu

FWD_GATE, BWD_GATE = 1e-5, 1e-4
MARGIN = 1e-4                   # of the rms of a pre-activation tensor
Z1_SHARE = 1e-3

# name -> (ker_width, R, depth, graph, E asked for, node seed).  tm_nqc(k) = ceil(k / 256): 384 and 640 end in a half-live
# column block; R = 522 is two chunks of destinations, the second with 10; no R is a multiple of 64.  The node seed
# (x0, roots, biases, g_out) is the first from 0 at which no p_a of the fp64 reference lies inside the margin (the
# test asserts it).
CASES = {
    "k256_control": (256, 77, 1, "random", 1000, 1),
    "k384": (384, 150, 2, "random+", 2500, 3),
    "k512": (512, 77, 1, "random", 1000, 4),
    "k640": (640, 130, 1, "random", 2000, 8),
    "k1024_edges": (1024, 522, 1, "shaped", 3300, 2418),
    "k128_no_edges": (128, 70, 2, "none", 0, 6),
}

IN_DEGREES = (0, 1, 15, 16, 17, 32, 33)         # around tm_edge_kernel's stages of TE_EDGES = 16 in-edges
OUT_DEGREES = (0, 1, 3, 4, 5, 9)                # around tm_gather_kernel's four waves (stride 4)
HUB = 300


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def shaped_graph(R, rng):
    """In-degrees exactly IN_DEGREES and one hub of HUB, each small value also among the last 10 rows (the second chunk
    of destinations); out-degrees exactly OUT_DEGREES; row R - 10 has neither in- nor out-edges.  Stubs are matched at
    random: duplicate (src, dst) pairs and self-loops come with it (asserted)."""
    assert R == 522
    head = rng.permutation(np.repeat((33, 32, 17, 16, 15, 1, 0), (19, 19, 28, 28, 29, 258, 130)))
    din = np.concatenate([[HUB], head, [0, 1, 15, 16, 17, 32, 33, 1, 16, 17]])
    rest = rng.permutation(np.repeat((9, 5, 4, 3, 1, 0), (255, 101, 80, 50, 30, 5)))
    dout = np.concatenate([rest[:R - 10], [0], rest[R - 10:]])
    assert din.shape == dout.shape == (R,) and din.sum() == dout.sum() and din.sum() % 128
    assert din[R - 10] == 0 and dout[R - 10] == 0
    assert set(din) == set(IN_DEGREES) | {HUB} and set(dout) == set(OUT_DEGREES)
    src = rng.permutation(np.repeat(np.arange(R), dout))
    dst = np.repeat(np.arange(R), din)
    pairs = src * R + dst
    assert (src == dst).any() and len(np.unique(pairs)) < len(pairs)
    order = rng.permutation(len(src))               # the caller's order is not the CSR order
    return src[order], dst[order]


def make_graph(kind, R, E, rng):
    if kind == "none":
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if kind == "shaped":
        return shaped_graph(R, rng)
    src, dst = rng.integers(0, R, E), rng.integers(0, R, E)         # directed, with whatever repeats fall out
    if kind == "random+":                                           # and for certain: self-loops, repeated pairs
        loops = rng.integers(0, R, 20)
        again = rng.integers(0, E, 37)
        src, dst = np.concatenate([src, loops, src[again]]), np.concatenate([dst, loops, dst[again]])
        order = rng.permutation(len(src))
        src, dst = src[order], dst[order]
    return src, dst


@functools.lru_cache(maxsize=None)
def inputs(case):
    """Everything of a case on the host in fp32: edge_index [2, E] (source, destination) and edge_attr [E, 6] in the
    caller's order, x0, g_out and the weights, scaled as test_gpu_train_factored._bounds_inputs has them."""
    k, R, depth, kind, E, node_seed = CASES[case]
    rng = np.random.default_rng(1000 + sorted(CASES).index(case))
    src, dst = make_graph(kind, R, E, rng)
    E = len(src)
    g = torch.Generator().manual_seed(2000 + sorted(CASES).index(case))
    t = dict(ea=torch.randn(E, 6, generator=g),
             w0=torch.randn(k, 6, generator=g) * 0.3, b0=torch.randn(k, generator=g) * 0.1,
             w1=torch.randn(k, k, generator=g) / k ** 0.5, b1=torch.randn(k, generator=g) * 0.1,
             w2=torch.randn(4096, k, generator=g) * 0.02, b2=torch.randn(4096, generator=g) * 0.02)
    t.update(node_inputs(R, node_seed))
    t["edge_index"] = torch.from_numpy(np.stack([src, dst])).long()
    return t


def node_inputs(R, node_seed):
    g = torch.Generator().manual_seed(node_seed)
    return dict(x0=torch.rand(R, 64, generator=g), g_out=torch.randn(R, 64, generator=g),
                root1=torch.randn(64, 64, generator=g) / 8, bias1=torch.randn(64, generator=g) * 0.1,
                root2=torch.randn(64, 64, generator=g) / 8, bias2=torch.randn(64, generator=g) * 0.1)


def reference(t, depth, dtype=torch.float64):
    """What include/mdno_train.h documents, written out in torch on the CPU with autograd, edges in the caller's order:
    X [2 depth + 1, R, 64], H [E, k], the pre-activations p [2 depth, R, 64] and z1 [E, k], and the gradients of
    (x_L * g_out).sum(): gz = d/dp, g_in = d/dx0, gz2 = d/dz1, d_w2, d_b2."""
    from oracle import graph_kernel_oracle as O
    c = {n: (v.to(dtype) if v.is_floating_point() else v) for n, v in t.items()}
    x0, w2, b2 = (c[n].clone().requires_grad_() for n in ("x0", "w2", "b2"))
    z0 = c["ea"] @ c["w0"].T + c["b0"]
    z1 = (torch.relu(z0) @ c["w1"].T + c["b1"]).requires_grad_()
    H = torch.relu(z1)
    w_e = H @ w2.T + b2
    xs, ps = [x0], []
    for a in range(1, 2 * depth + 1):
        root, bias = (c["root1"], c["bias1"]) if a <= depth else (c["root2"], c["bias2"])
        ps.append(O.nnconv_apply(xs[-1], c["edge_index"], w_e, root, bias, "mean"))
        xs.append(torch.relu(ps[-1]))
    loss = (xs[-1] * c["g_out"]).sum()
    grads = torch.autograd.grad(loss, ps + [x0, z1, w2, b2], allow_unused=True)
    L = 2 * depth
    gz2 = grads[L + 1] if grads[L + 1] is not None else torch.zeros_like(z1)
    return dict(X=torch.stack(xs).detach(), H=H.detach(), p=torch.stack(ps).detach(), z1=z1.detach(),
                gz=torch.stack(grads[:L]), g_in=grads[L], gz2=gz2, d_w2=grads[L + 2], d_b2=grads[L + 3])


def inside_margin(pre):
    """Elements of a pre-activation tensor closer to zero than MARGIN * its rms."""
    if pre.numel() == 0:
        return torch.zeros_like(pre, dtype=torch.bool)
    return pre.abs() < MARGIN * pre.double().pow(2).mean().sqrt()


@functools.lru_cache(maxsize=None)
def want(case):
    """The fp64 reference of a case, once for the three GEMM modes; never modified."""
    ref = reference(inputs(case), CASES[case][2])
    ref["z1_near"] = inside_margin(ref["z1"])
    ref["p_near"] = int(sum(inside_margin(p).sum() for p in ref["p"]))
    return ref


# ------------------------------------------------------------------------------------------------ the measure
def col_blocks(t):
    """Sums per block of 256 along the last dimension (the last block may be half) -> [..., blocks]."""
    return torch.stack([b.sum(-1) for b in t.split(256, dim=-1)], dim=-1)


def measure(got, ref, sums=None):
    """The largest err(slice) over the slices that `sums` adds up (squares in, per-slice sums out); whole tensor: None."""
    got, ref = got.detach().cpu().double(), ref.double()
    d2, w2 = (got - ref) ** 2, ref ** 2
    total = w2.sum().sqrt()
    if sums is None:
        return float(d2.sum().sqrt() / total.clamp_min(1e-300))
    d, w = sums(d2).sqrt(), sums(w2).sqrt()
    if d.numel() == 0:
        return 0.0
    return float((d / torch.maximum(w, total / d.numel() ** 0.5).clamp_min(1e-300)).max())


def all_errors(got, ref, k):
    """name -> largest figure, whole tensors and slices, for one set of the seven outputs (gz2 and H in the same edge
    order as `ref`'s; gz2 without z1's elements inside the margin)."""
    rows = lambda t: t.sum(-1)                                                   # per destination (or edge) row
    keep = ~ref["z1_near"]
    gz2_got, gz2_ref = got["gz2"].detach().cpu() * keep, ref["gz2"] * keep
    L = ref["gz"].shape[0]
    e = {"X": measure(got["X"][1:], ref["X"][1:]), "H": measure(got["H"], ref["H"]),
         "gz": measure(got["gz"], ref["gz"]), "g_in": measure(got["g_in"], ref["g_in"]),
         "gz2": measure(gz2_got, gz2_ref), "d_w2": measure(got["d_w2"], ref["d_w2"]),
         "d_b2": measure(got["d_b2"], ref["d_b2"])}
    for a in range(L):
        e[f"X[{a + 1}] rows"] = measure(got["X"][a + 1], ref["X"][a + 1], rows)
        e[f"gz[{a}] rows"] = measure(got["gz"][a], ref["gz"][a], rows)
    e["g_in rows"] = measure(got["g_in"], ref["g_in"], rows)
    e["gz2 column blocks"] = measure(gz2_got, gz2_ref, lambda t: col_blocks(t.sum(0)))
    e["gz2 edge rows"] = measure(gz2_got, gz2_ref, rows)
    e["d_w2 (i, column block)"] = measure(got["d_w2"].view(64, 64, k), ref["d_w2"].view(64, 64, k),
                                          lambda t: col_blocks(t.sum(1)))
    e["d_b2 i"] = measure(got["d_b2"].view(64, 64), ref["d_b2"].view(64, 64), rows)
    return e


def gate(name):
    return FWD_GATE if name[0] in "XH" else BWD_GATE


def by_tensor(errs):
    """The largest figure per output tensor (its whole-tensor figure and its slices')."""
    out = {}
    for n, v in errs.items():
        key = n.split(" ")[0].split("[")[0]
        out[key] = max(out.get(key, 0.0), v)
    return out


# ------------------------------------------------------------------------------------------------ the device
def run_device(dev, case, gemm_mode, guard=None):
    """fwd + bwd through the two entry points -> the seven outputs on the host (H as rows, in CSR edge order) and
    graph.perm.  With a Guard: every input in an arena of its own, every band verified."""
    from molecular_dynamics_neural_operator_amd import ops
    k, R, depth = CASES[case][:3]
    t = inputs(case)
    put = (lambda v: guard.place(v.to(dev))) if guard is not None else (lambda v: v.to(dev))
    p = {n: put(v) for n, v in t.items()}
    graph = ops.coo_to_csr(p["edge_index"], R)
    by_src = ops.source_sorted(graph, R)
    E = graph.edge_count()
    assert E == t["edge_index"].shape[1]
    X = torch.empty((2 * depth + 1, R, 64), dtype=torch.float32, device=dev)
    X[0].copy_(p["x0"])
    h_img = ops.train_moment_fwd(X, graph, p["ea"], [p[n] for n in ("w0", "b0", "w1", "b1", "w2", "b2")], p["root1"],
                                 p["bias1"], p["root2"], p["bias2"], depth, gemm_mode)
    gz, g_in, gz2, d_w2, d_b2 = ops.train_moment_bwd(p["g_out"], X, h_img, graph, by_src, p["w2"], p["b2"], p["root1"],
                                                     p["root2"], depth, gemm_mode)
    if guard is not None:
        guard.verify()
    out = dict(X=X, H=_h_rows(h_img, E, k), gz=gz, g_in=g_in, gz2=gz2, d_w2=d_w2, d_b2=d_b2)
    return {n: v.cpu() for n, v in out.items()}, graph.perm[:E].cpu().long()


@pytest.mark.parametrize("gemm_mode", GEMM_MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_train_moment_ops_vs_fp64(dev, case, gemm_mode):
    """X[1:], H within 1e-5 and gz, g_in, gz2, d_w2, d_b2 within 1e-4 of fp64, whole and per slice of ownership; inside
    guard bands filled with NaN bytes; a second pass gives the same bits in all seven outputs."""
    from guarded import Guard
    k, R, depth = CASES[case][:3]
    ref = want(case)
    E = ref["H"].shape[0]
    near = float(ref["z1_near"].double().mean()) if E else 0.0
    print(case, gemm_mode, "E", E, "p_a inside the margin", ref["p_near"], "z1 share inside the margin", f"{near:.1e}")
    assert ref["p_near"] == 0
    assert near <= Z1_SHARE
    with Guard(0xFF) as G:
        got, perm = run_device(dev, case, gemm_mode, G)
    # graph.perm[p] = the caller's edge at CSR position p: a permutation that sorts by destination
    ei = inputs(case)["edge_index"]
    assert torch.equal(perm.sort().values, torch.arange(E))
    assert bool((ei[1][perm].diff() >= 0).all())
    in_csr = dict(ref)
    for n in ("H", "z1", "z1_near", "gz2"):
        in_csr[n] = ref[n][perm]
    errs = all_errors(got, in_csr, k)
    print(case, gemm_mode, "largest per tensor", {n: f"{v:.1e}" for n, v in by_tensor(errs).items()})
    print(case, gemm_mode, "all", {n: f"{v:.1e}" for n, v in errs.items()})
    for n, v in got.items():
        assert tuple(v.shape) == tuple(in_csr[n].shape), n
    bad = {n: v for n, v in errs.items() if not v < gate(n)}
    assert not bad, bad
    if E == 0:
        assert got["gz2"].numel() == 0
        assert torch.count_nonzero(got["d_w2"]) == 0 and torch.count_nonzero(got["d_b2"]) == 0
    again, _ = run_device(dev, case, gemm_mode)
    for n in got:
        assert torch.equal(got[n], again[n]), n
