"""Stand-alone NNConv_old / DenseNet at the shapes and edges where their kernels go wrong: channel counts past one
4,096-element chunk of bwd_x_edges and past one 64-lane pass of the row kernels, the VEC and scalar variants on the same
data, graphs without edges, with one node, with one huge in- or out-degree and with 200k edges, 1-D inputs, NaN / Inf
messages under every aggregation, and edge networks wide enough for the MFMA Linear kernels.  Every value and gradient
is compared with fp64 CPU autograd over the oracle (O.nnconv_apply), tolerances as test_gpu_layer_grad.py; each conv
case runs the inference forward (eval + no_grad) and the differentiable one (forward + backward, x and edge_attr
included).

fp32 and fp64 may take different sides of a ReLU whose input is within rounding of 0, or different argmaxes of a near
tie: at a few hundred thousand such decisions one of them flips and moves a whole term of a gradient.  The large inputs
are therefore conditioned (``conditioned``): edges and rows whose fp64 ReLU inputs lie within 1e-5 of their layer's
scale of 0, or whose destination has two messages within 1e-5 of the scale in some channel (max), are dropped before
the comparison.  Exact ties (duplicated edges) are kept where a test wants them."""
import math

import pytest
import torch
import torch.nn as nn

from test_gpu_layer_grad import check_grads, close, random_graph, ref_module, ref_params

pytestmark = pytest.mark.gpu

MARGIN = 1e-5


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def O():
    from oracle import graph_kernel_oracle
    return graph_kernel_oracle


@pytest.fixture(scope="module", autouse=True)
def _host_threads():
    # the fp64 references dominate this module: as many torch threads as the CPUs this process may use
    from conftest import host_cores
    old = torch.get_num_threads()
    torch.set_num_threads(host_cores())
    yield
    torch.set_num_threads(old)


# ------------------------------------------------------------------------------- helpers
def make_conv(dev, cin, cout, aggr, ker_in=5, hidden=(16, 16), seed=0, rb=True):
    from molecular_dynamics_neural_operator_amd.graph_kernel import DenseNet, NNConv_old
    torch.manual_seed(seed)
    net = DenseNet([ker_in, *hidden, cin * cout], nn.ReLU)
    return NNConv_old(cin, cout, net, aggr=aggr, root_weight=rb, bias=rb, differentiable=True).to(dev)


def relu_inputs_ok(net, h, P, prefix="net."):
    """Rows of h whose every ReLU input in ``net`` (fp64) is at least MARGIN * (that layer's max) away from 0."""
    from molecular_dynamics_neural_operator_amd.graph_kernel import DenseNet
    mods = list(net.layers) if isinstance(net, DenseNet) else list(net)
    pre = prefix + "layers." if isinstance(net, DenseNet) else prefix
    ok = torch.ones(h.shape[0], dtype=torch.bool)
    with torch.no_grad():
        h = h.double()
        for i, m in enumerate(mods):
            if isinstance(m, nn.ReLU) and h.numel():
                ok &= (h.abs() >= MARGIN * float(h.abs().max())).all(1)
            h = ref_module(h, m, P, f"{pre}{i}.")
    return ok


def messages(x, ei, w_e, cout):
    cin = x.shape[1]
    return (x[ei[0]].unsqueeze(1) @ w_e.view(-1, cin, cout)).squeeze(1)


def max_gap_ok(x, ei, w_e, cout):
    """Edges whose destination has, in every channel, a maximum message at least MARGIN * max|m| above the next one."""
    n, dst = x.shape[0], ei[1]
    with torch.no_grad():
        m = messages(x, ei, w_e, cout)
        ninf = torch.full((n, cout), -math.inf, dtype=m.dtype)
        top = ninf.clone().index_reduce_(0, dst, m, "amax")
        rest = m.masked_fill(m == top[dst], -math.inf)
        second = ninf.clone().index_reduce_(0, dst, rest, "amax")
        near = ((top - second) < MARGIN * float(m.abs().max())).any(1)
    return ~near[dst]


def conditioned(conv, x, ei, ea, aggr=None):
    """(ei, ea) without the edges whose fp64 ReLU inputs or max-aggregation argmax sit within rounding of a flip."""
    if ei.shape[1] == 0:
        return ei, ea
    P = {n: p.detach().cpu().double() for n, p in conv.named_parameters()}
    ea2 = ea.unsqueeze(-1) if ea.dim() == 1 else ea
    keep = relu_inputs_ok(conv.net, ea2, P)
    if (aggr or conv.aggr) == "max":
        x2 = x.unsqueeze(-1) if x.dim() == 1 else x
        with torch.no_grad():
            w_e = ref_module(ea2.double(), conv.net, P, "net.")
        keep &= max_gap_ok(x2.double(), ei, w_e, conv.out_channels)
    return ei[:, keep], ea[keep]


def canonical(t, canon):
    """t's values with every row replaced by row canon[row] (exactly), the gradient still reaching each row itself:
    duplicated edges get bitwise equal fp64 values whatever order a batched product rounds its rows in."""
    return t[canon].detach() + (t - t.detach())


def ref_forward(O, conv, P, xr, ei, ear, canon=None):
    x2 = xr.unsqueeze(-1) if xr.dim() == 1 else xr
    ea2 = ear.unsqueeze(-1) if ear.dim() == 1 else ear
    w_e = ref_module(ea2, conv.net, P, "net.")
    if canon is None:
        return O.nnconv_apply(x2, ei, w_e, P.get("root"), P.get("bias"), conv.aggr)
    # O.nnconv_apply with the messages of duplicated edges made exactly equal (see canonical)
    n, cout = x2.shape[0], conv.out_channels
    msg = canonical(messages(x2, ei, canonical(w_e, canon), cout), canon)
    if conv.aggr == "max":
        out = torch.zeros(n, cout, dtype=x2.dtype).index_reduce_(0, ei[1], msg, "amax", include_self=False)
    else:
        out = torch.zeros(n, cout, dtype=x2.dtype).index_add_(0, ei[1], msg)
        if conv.aggr == "mean":
            cnt = torch.zeros(n, dtype=x2.dtype).index_add_(0, ei[1], torch.ones(ei.shape[1], dtype=x2.dtype))
            out = out / cnt.clamp(min=1).unsqueeze(-1)
    return out + x2 @ P["root"] + P["bias"]


def check_conv(dev, O, conv, ei, x, ea, name, canon=None):
    """Inference and differentiable forward + backward of ``conv`` against fp64 autograd over the oracle."""
    P = ref_params(conv)
    xr, ear = x.double().requires_grad_(), ea.double().requires_grad_()
    yr = ref_forward(O, conv, P, xr, ei, ear, canon)
    gy = torch.randn(yr.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    (yr * gy).sum().backward()

    conv.eval()
    with torch.no_grad():
        y = conv(x.to(dev), ei.to(dev), ea.to(dev))
    conv.train()
    assert y.grad_fn is None
    close(y, yr, name=f"{name} inference y")

    xg, eag = x.to(dev).requires_grad_(), ea.to(dev).requires_grad_()
    y = conv(xg, ei.to(dev), eag)
    assert y.grad_fn is not None
    (y * gy.float().to(dev)).sum().backward()
    close(y, yr, name=f"{name} y")
    check_grads(conv, P, [(xg.grad, xr.grad, "x"), (eag.grad, ear.grad, "edge_attr")], name)
    return P


def graph_inputs(n, e, cin, ker_in, seed):
    ei = random_graph(n, e, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    return ei, torch.randn(n, cin, generator=g), torch.randn(e, ker_in, generator=g)


AGGRS = ("add", "mean", "max")


# ------------------------------------------------------------------------------- 1. channel grid
# bwd_x_edges holds kChunk = 4096 elements of [Cin, Cout] (kChunk / Cout whole rows) per pass; the row kernels put lanes
# on output channels with o += 64
CHANNELS = [
    (66, 63),       # scalar (Cout % 4), two chunks, the last one a single row
    (128, 64),      # VEC, exactly two chunks
    (96, 100),      # VEC, chunks of 40 / 40 / 16 rows, partial n, Cout > 64
    (3, 1500),      # one or two rows per chunk, many lane passes
    (1, 4096),      # Cout == kChunk
    (2, 4095),      # scalar, one row per chunk
    (200, 1),
    (64, 65),
    (65, 64),       # the neighbours of the tuned 64x64 path
]


@pytest.mark.parametrize("cin,cout", CHANNELS, ids=[f"{a}x{b}" for a, b in CHANNELS])
@pytest.mark.parametrize("aggr", AGGRS)
def test_channel_grid(dev, O, aggr, cin, cout):
    conv = make_conv(dev, cin, cout, aggr, seed=cin + cout)
    ei, x, ea = graph_inputs(40, 300, cin, 5, seed=cin * 1000 + cout)
    ei, ea = conditioned(conv, x, ei, ea)
    check_conv(dev, O, conv, ei, x, ea, f"{aggr} {cin}x{cout}")


def test_unequal_hidden_widths(dev, O):
    """A three-layer ReLU DenseNet with two different hidden widths is not the fused edge-MLP's shape (it has one
    ker_width): the inference forward must run it layer by layer."""
    conv = make_conv(dev, 8, 16, "mean", hidden=(16, 13), seed=5)
    assert not conv.net._fused
    ei, x, ea = graph_inputs(40, 300, 8, 5, seed=51)
    check_conv(dev, O, conv, ei, x, ea, "hidden 16/13")


def test_cout_past_one_chunk_refuses_backward(dev, O):
    """Cout = 4097 > kChunk: the forward is right, the backward raises MdnoError (no silent garbage)."""
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    conv = make_conv(dev, 1, 4097, "add", seed=6)
    ei, x, ea = graph_inputs(40, 300, 1, 5, seed=61)
    P = ref_params(conv)
    with torch.no_grad():
        yr = ref_forward(O, conv, P, x.double(), ei, ea.double())
        conv.eval()
        close(conv(x.to(dev), ei.to(dev), ea.to(dev)), yr, name="4097 inference y")
        conv.train()
    xg = x.to(dev).requires_grad_()
    y = conv(xg, ei.to(dev), ea.to(dev))
    close(y, yr, name="4097 y")
    with pytest.raises(MdnoError, match="Cout 4097"):
        y.sum().backward()


# ------------------------------------------------------------------------------- 2. VEC == scalar
def misaligned(t):
    """A contiguous copy of t that starts one float into a larger buffer: not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


@pytest.mark.parametrize("cin,cout", [(8, 16), (128, 64), (96, 100)], ids=["8x16", "128x64", "96x100"])
@pytest.mark.parametrize("aggr", AGGRS)
def test_vec_and_scalar_variants_agree(dev, aggr, cin, cout):
    """bwd_x_edges / bwd_we_edges pick their VEC kernel by Cout % 4 and 16-byte alignment; both add in the same order,
    so the same data through the scalar kernels (w_e, gm, root one float off) gives the same bits."""
    from molecular_dynamics_neural_operator_amd import ops
    n, e = 40, 300
    ei, x, _ = graph_inputs(n, e, cin, 1, seed=cin + 7 * cout)
    g = torch.Generator().manual_seed(8)
    w_e = torch.randn(e, cin * cout, generator=g).to(dev)
    root = torch.randn(cin, cout, generator=g).to(dev)
    gy = torch.randn(n, cout, generator=g).to(dev)
    x = x.to(dev)
    graph = ops.coo_to_csr(ei.to(dev), n)
    by_src = ops.source_sorted(graph, n)
    assert w_e.data_ptr() % 16 == 0 and root.data_ptr() % 16 == 0

    gm = ops.nnconv_msg_grad(x, graph, w_e, gy, aggr)
    gm_s = ops.nnconv_msg_grad(x, graph, misaligned(w_e), gy, aggr)
    assert torch.equal(gm, gm_s)
    assert gm.data_ptr() % 16 == 0
    dx = ops.nnconv_bwd_x_edges(gm, gy, by_src, w_e, root, cin)
    dx_s = ops.nnconv_bwd_x_edges(misaligned(gm), gy, by_src, misaligned(w_e), misaligned(root), cin)
    assert torch.equal(dx, dx_s)
    d_we = ops.nnconv_bwd_we_edges(x, gm, graph)
    d_we_s = ops.nnconv_bwd_we_edges(x, misaligned(gm), graph)
    assert torch.equal(d_we, d_we_s)
    # (and both are right: the same sums in fp64, CSR order)
    gmd, wd = gm.double().cpu(), w_e.double().cpu()
    src_s = by_src.row_ptr.cpu()
    eid = by_src.perm[:e].long().cpu()
    ref = gy.double().cpu() @ root.double().cpu().T
    per_edge = torch.einsum("eio,eo->ei", wd.view(e, cin, cout)[eid], gmd[eid])
    rows = torch.repeat_interleave(torch.arange(n), src_s[1:] - src_s[:-1])
    ref = ref.index_add(0, rows, per_edge)
    close(dx, ref, name=f"{aggr} {cin}x{cout} dx (ops)")


# ------------------------------------------------------------------------------- 3. degenerate and extreme graphs
@pytest.mark.parametrize("net_kind", ["densenet", "sequential"])
@pytest.mark.parametrize("aggr", AGGRS)
def test_no_edges(dev, O, aggr, net_kind):
    """E = 0: y = x.root + bias, dx = g.root^T, the edge network's gradients zero tensors (as torch gives)."""
    from molecular_dynamics_neural_operator_amd.graph_kernel import NNConv_old
    cin, cout, ker_in = 4, 6, 5
    if net_kind == "densenet":
        conv = make_conv(dev, cin, cout, aggr, ker_in=ker_in, seed=9)
    else:
        torch.manual_seed(9)
        net = nn.Sequential(nn.Linear(ker_in, 8), nn.Tanh(), nn.Linear(8, cin * cout))
        conv = NNConv_old(cin, cout, net, aggr=aggr, differentiable=True).to(dev)
    n = 12
    x = torch.randn(n, cin, generator=torch.Generator().manual_seed(10))
    ei, ea = torch.empty(2, 0, dtype=torch.long), torch.empty(0, ker_in)
    P = check_conv(dev, O, conv, ei, x, ea, f"E=0 {aggr} {net_kind}")
    gy = torch.randn(n, cout, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    torch.testing.assert_close(P["root"].grad, x.double().T @ gy)
    for name, p in conv.net.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and not p.grad.any(), name
    # the edge network alone on no rows (a DenseNet's inference forward: an empty product, not a kernel launch)
    with torch.no_grad():
        w_e = conv.net.eval()(ea.to(dev))
    assert w_e.shape == (0, cin * cout)


@pytest.mark.parametrize("cin,cout", [(3, 5), (64, 64)], ids=["3x5", "64x64"])
@pytest.mark.parametrize("aggr", AGGRS)
def test_single_node_self_loops(dev, O, aggr, cin, cout):
    conv = make_conv(dev, cin, cout, aggr, seed=11)
    ei = torch.zeros(2, 3, dtype=torch.long)
    g = torch.Generator().manual_seed(12)
    x, ea = torch.randn(1, cin, generator=g), torch.randn(3, 5, generator=g)
    ei, ea = conditioned(conv, x, ei, ea)
    check_conv(dev, O, conv, ei, x, ea, f"self-loops {aggr} {cin}x{cout}")


@pytest.mark.parametrize("cin,cout", [(3, 5), (8, 16)], ids=["3x5", "8x16"])
@pytest.mark.parametrize("aggr", AGGRS)
def test_star_into_one_node(dev, O, aggr, cin, cout):
    """5,000 in-edges of node 0; the second half duplicates the first (same source, same attributes), so under max
    every row maximum is an exact tie that the duplicates share."""
    n, half = 1500, 2500
    conv = make_conv(dev, cin, cout, aggr, seed=13)
    g = torch.Generator().manual_seed(14)
    src = torch.randint(1, n, (half,), generator=g).repeat(2)
    ei = torch.stack([src, torch.zeros_like(src)])
    ea = torch.randn(half, 5, generator=g).repeat(2, 1)
    x = torch.randn(n, cin, generator=g)
    keep = relu_inputs_ok(conv.net, ea[:half], {k: p.detach().cpu().double() for k, p in conv.named_parameters()})
    keep = keep.repeat(2)
    ei, ea = ei[:, keep], ea[keep]
    k = int(keep[:half].sum())
    canon = torch.cat([torch.arange(k), torch.arange(k)])
    check_conv(dev, O, conv, ei, x, ea, f"star-in {aggr} {cin}x{cout}", canon=canon)


@pytest.mark.parametrize("cin,cout", [(3, 5), (66, 63)], ids=["3x5", "66x63"])
@pytest.mark.parametrize("aggr", AGGRS)
def test_star_out_of_one_node(dev, O, aggr, cin, cout):
    """5,000 out-edges of node 0: bwd_x_edges runs all of them on one workgroup (two chunks at 66x63)."""
    n, e = 2000, 5000
    conv = make_conv(dev, cin, cout, aggr, seed=15)
    g = torch.Generator().manual_seed(16)
    ei = torch.stack([torch.zeros(e, dtype=torch.long), torch.randint(0, n, (e,), generator=g)])
    x, ea = torch.randn(n, cin, generator=g), torch.randn(e, 5, generator=g)
    ei, ea = conditioned(conv, x, ei, ea)
    check_conv(dev, O, conv, ei, x, ea, f"star-out {aggr} {cin}x{cout}")


@pytest.mark.parametrize("aggr", AGGRS)
def test_large_graph(dev, O, aggr):
    """~70k nodes, 200k edges: the edge-parallel kernels' grid-stride loops (4096 workgroups x 4 edges) go round."""
    conv = make_conv(dev, 3, 5, aggr, seed=17)
    ei, x, ea = graph_inputs(70000, 200000, 3, 5, seed=18)
    ei, ea = conditioned(conv, x, ei, ea)
    assert ei.shape[1] > 4096 * 4 * 10
    check_conv(dev, O, conv, ei, x, ea, f"large {aggr}")


@pytest.mark.parametrize("aggr", AGGRS)
def test_one_dimensional_inputs(dev, O, aggr):
    """x [N] and edge_attr [E] (Cin = 1, ker_in = 1): unsqueezed on the way in, gradients in the inputs' shapes."""
    conv = make_conv(dev, 1, 4, aggr, ker_in=1, seed=19)
    ei = random_graph(40, 300, seed=20)
    g = torch.Generator().manual_seed(21)
    x, ea = torch.randn(40, generator=g), torch.randn(300, generator=g)
    ei, ea = conditioned(conv, x, ei, ea)
    check_conv(dev, O, conv, ei, x, ea, f"1-D {aggr}")


# ------------------------------------------------------------------------------- 4. non-finite messages
# 64x64 with fewer and with more than 4096 rows (nnconv64_row_kernel with 16 and with 4 waves per row), and a generic
# shape; W_e is given directly (edge network nn.Identity), one element of one edge's matrix non-finite
NONFINITE_SHAPES = [(64, 64, 300, 1500), (64, 64, 4200, 4500), (5, 7, 40, 300)]


@pytest.mark.parametrize("shape", NONFINITE_SHAPES, ids=["64x64_few_rows", "64x64_many_rows", "5x7"])
@pytest.mark.parametrize("value", [math.nan, math.inf, -math.inf], ids=["nan", "posinf", "neginf"])
@pytest.mark.parametrize("aggr", AGGRS)
def test_nonfinite_message(dev, O, aggr, value, shape):
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd.graph_kernel import NNConv_old
    cin, cout, n, e = shape
    ei = random_graph(n, e, seed=22)
    ei[1, :3] = 5                                 # edges 0..2 meet at node 5; edge 1 carries the non-finite message
    g = torch.Generator().manual_seed(23)
    x = torch.randn(n, cin, generator=g)
    w_e = torch.randn(e, cin * cout, generator=g) / math.sqrt(cin)
    i0, o0 = cin // 2, cout - 2
    x[ei[0, 1], i0] = 1.0                         # (x > 0: W = +-inf gives a message of the same sign)
    w_e[1, i0 * cout + o0] = value
    torch.manual_seed(24)
    conv = NNConv_old(cin, cout, nn.Identity(), aggr=aggr).to(dev).eval()
    P = {k: p.detach().cpu().double() for k, p in conv.named_parameters()}
    ref = O.nnconv_apply(x.double(), ei, w_e.double(), P["root"], P["bias"], aggr)
    # (a -inf message loses every maximum it competes in)
    assert bool(ref[5, o0].isfinite()) == (aggr == "max" and value < 0)
    with torch.no_grad():
        y = conv(x.to(dev), ei.to(dev), w_e.to(dev)).cpu()
    for what in (torch.isnan, torch.isposinf, torch.isneginf):
        assert torch.equal(what(y), what(ref)), f"{what.__name__} pattern differs from the oracle"
    fin = ref.isfinite()
    close(y[fin], ref[fin], name=f"{aggr} {value} {cin}x{cout} finite y")

    if aggr == "max":     # the shares of every row whose messages are all finite still add up to g
        graph = ops.coo_to_csr(ei.to(dev), n)
        w_csr = ops.permute_rows(w_e.to(dev), graph.perm, e)
        gy = torch.randn(n, cout, generator=g)
        gm = ops.nnconv_msg_grad(x.to(dev), graph, w_csr, gy.to(dev), "max")[:e].cpu()
        dst = graph.dst[:e].long().cpu()
        sums = torch.zeros(n, cout).index_add_(0, dst, gm)
        msg_fin = messages(x.double(), ei, w_e.double(), cout).isfinite().all(1)
        row_fin = torch.zeros(n, dtype=torch.bool)
        row_fin[ei[1]] = True
        row_fin[ei[1][~msg_fin]] = False
        assert int(row_fin.sum()) > n // 4
        assert torch.equal(sums[row_fin], gy[row_fin]), "max shares of finite rows do not add up to g"


# ------------------------------------------------------------------------------- 5. wide DenseNets
DENSE_LAYERS = [[32, 128, 256, 128], [1, 129, 1], [10, 32, 32, 12], [5, 4099, 7]]
DENSE_CASES = [(layers, rows) for layers in DENSE_LAYERS for rows in (1, 127, 129, 70000)
               if not (layers[1] > 1024 and rows > 1024)]      # ([5, 4099, 7] at 70k rows: GBs of fp64 activations)


@pytest.mark.parametrize("layers,rows", DENSE_CASES, ids=[f"{'-'.join(map(str, l))}_rows{r}" for l, r in DENSE_CASES])
def test_wide_densenet(dev, layers, rows):
    """Both paths: the inference forward (layer by layer here, every one of these shapes — ker_in > 8 included — off
    the fused edge-MLP) and _DenseNetFn forward + backward."""
    from molecular_dynamics_neural_operator_amd.graph_kernel import DenseNet
    torch.manual_seed(25)
    net = DenseNet(layers, nn.ReLU, differentiable=True).to(dev)
    P = ref_params(net)
    x = torch.randn(2 * rows + 8, layers[0], generator=torch.Generator().manual_seed(26))
    x = x[relu_inputs_ok(net, x, P, prefix="")][:rows]
    assert x.shape[0] == rows
    xr = x.double().requires_grad_()
    yr = ref_module(xr, net, P, "")
    gy = torch.randn(yr.shape, generator=torch.Generator().manual_seed(27), dtype=torch.float64)
    (yr * gy).sum().backward()

    net.eval()
    with torch.no_grad():
        y = net(x.to(dev))
    net.train()
    close(y, yr, name=f"densenet {layers} x{rows} inference y")
    xg = x.to(dev).requires_grad_()
    y = net(xg)
    assert y.grad_fn is not None
    (y * gy.float().to(dev)).sum().backward()
    close(y, yr, name=f"densenet {layers} x{rows} y")
    check_grads(net, P, [(xg.grad, xr.grad, "x")], f"densenet {layers} x{rows}")


# ------------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("aggr,cin,cout", [("max", 96, 100), ("mean", 66, 63)])
def test_wide_backward_is_bitwise_reproducible(dev, aggr, cin, cout):
    conv = make_conv(dev, cin, cout, aggr, seed=28)
    ei, x, ea = graph_inputs(40, 300, cin, 5, seed=29)
    ei, x, ea = ei.to(dev), x.to(dev), ea.to(dev)
    gy = torch.randn(40, cout, generator=torch.Generator().manual_seed(30)).to(dev)
    runs = []
    for _ in range(2):
        conv.zero_grad()
        xg, eag = x.clone().requires_grad_(), ea.clone().requires_grad_()
        (conv(xg, ei, eag) * gy).sum().backward()
        runs.append([xg.grad.clone(), eag.grad.clone()] + [p.grad.clone() for p in conv.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
