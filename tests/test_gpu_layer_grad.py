"""Stand-alone NNConv_old / DenseNet with ``differentiable=True``: gradients of the HIP backward (csrc/layer_grad.hip and,
at 64x64 add / mean, the model's tuned training kernels) against fp64 torch autograd on the CPU over the oracle
(``O.nnconv_apply``, the torch_geometric stub's aggregation).  Tolerances as test_gpu_parity.py: rtol 1e-4 with
atol 1e-4 * max|ref|, relative L2 1e-5, unless noted."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RTOL = 1e-4
REL_L2 = 1e-5


def close(a, b, rtol=RTOL, scale=None, rel_l2=REL_L2, name=""):
    a = a.detach().cpu().double() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a)).double()
    b = b.detach().cpu().double() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b)).double()
    s = float(b.abs().max()) if (scale is None and b.numel()) else (scale or 0.0)
    err = (a - b).abs()
    l2 = float(err.norm() / b.norm().clamp_min(1e-300)) if b.numel() else 0.0
    big = b.abs() > 1e-2 * s
    max_rel = float((err[big] / b.abs()[big]).max()) if bool(big.any()) else 0.0
    print(f"close[{name}] rel_l2 {l2:.2e}  max rel err on |y|>1e-2*max {max_rel:.2e}  max abs err "
          f"{float(err.max()) if b.numel() else 0.0:.2e}  max|y| {s:.3e}")
    torch.testing.assert_close(a, b, rtol=rtol, atol=rtol * max(s, 1e-30))
    assert l2 <= rel_l2, f"{name}: relative L2 error {l2:.3e} > {rel_l2:.1e}"


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def O():
    from oracle import graph_kernel_oracle
    return graph_kernel_oracle


# ------------------------------------------------------------------------------- fp64 reference
def ref_module(h, mod, P, prefix):
    """``mod`` evaluated in fp64 on the CPU with the parameters P[prefix + name] (leaf tensors)."""
    if isinstance(mod, nn.Linear):
        return F.linear(h, P[prefix + "weight"], P.get(prefix + "bias"))
    if isinstance(mod, nn.BatchNorm1d):
        assert not mod.training
        rm, rv = mod.running_mean.detach().cpu().double(), mod.running_var.detach().cpu().double()
        return (h - rm) / torch.sqrt(rv + mod.eps) * P[prefix + "weight"] + P[prefix + "bias"]
    if isinstance(mod, nn.ReLU):
        return F.relu(h)
    if isinstance(mod, nn.Tanh):
        return torch.tanh(h)
    from molecular_dynamics_neural_operator_amd.graph_kernel import DenseNet
    if isinstance(mod, DenseNet):
        return ref_module(h, mod.layers, P, prefix + "layers.")
    assert isinstance(mod, (nn.Sequential, nn.ModuleList)), type(mod)
    for i, m in enumerate(mod):
        h = ref_module(h, m, P, f"{prefix}{i}.")
    return h


def ref_conv(O, conv, P, prefix, x, ei, ea, net_prefix=None):
    w_e = ref_module(ea, conv.net, P, net_prefix or prefix + "net.")
    return O.nnconv_apply(x, ei, w_e, P.get(prefix + "root"), P.get(prefix + "bias"), conv.aggr)


def ref_params(module):
    return {n: p.detach().cpu().double().requires_grad_() for n, p in module.named_parameters()}


def check_grads(module, P, extra=(), name=""):
    for n, p in module.named_parameters():
        assert p.grad is not None, f"{name}: no gradient for {n}"
        close(p.grad, P[n].grad, name=f"{name} d{n}")
    for got, ref, what in extra:
        close(got, ref, name=f"{name} d{what}")


def random_graph(n, e, seed):
    """Random edges with self-loops and repeated edges; nodes n-3.. have no in-edges, nodes 0..2 no out-edges."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(3, n, (e,), generator=g)
    dst = torch.randint(0, n - 3, (e,), generator=g)
    src[:6] = dst[:6] = torch.arange(3, 9)                 # self-loops
    src[6:12], dst[6:12] = src[12:18], dst[12:18]          # repeated edges
    return torch.stack([src, dst])


def make_conv(dev, cin, cout, aggr, rb, ker_in=5, hidden=(16, 13), seed=0):
    from molecular_dynamics_neural_operator_amd.graph_kernel import DenseNet, NNConv_old
    torch.manual_seed(seed)
    net = DenseNet([ker_in, *hidden, cin * cout], nn.ReLU)
    return NNConv_old(cin, cout, net, aggr=aggr, root_weight=rb, bias=rb, differentiable=True).to(dev)


def run_conv_case(dev, O, conv, ei, x, ea, name, generic=False):
    conv._generic_backward = generic
    xg, eag = x.to(dev).requires_grad_(), ea.to(dev).requires_grad_()
    y = conv(xg, ei.to(dev), eag)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    (y * gy.float().to(dev)).sum().backward()
    P = ref_params(conv)
    xr, ear = x.double().requires_grad_(), ea.double().requires_grad_()
    yr = ref_conv(O, conv, P, "", xr, ei, ear)
    (yr * gy).sum().backward()
    close(y, yr, name=f"{name} y")
    check_grads(conv, P, [(xg.grad, xr.grad, "x"), (eag.grad, ear.grad, "edge_attr")], name)


# ------------------------------------------------------------------------------- 1. conv gradients
# 64x64 add / mean run the tuned training kernels by default; "generic" sends them through csrc/layer_grad.hip
CONV_GRID = [(aggr, cin, cout, generic) for aggr in ("add", "mean", "max")
             for cin, cout in ((64, 64), (8, 16), (3, 5), (1, 1))
             for generic in ((False, True) if (cin, cout) == (64, 64) and aggr != "max" else (False,))]


@pytest.mark.parametrize("rb", [True, False], ids=["root_bias", "no_root_bias"])
@pytest.mark.parametrize("aggr,cin,cout,generic", CONV_GRID)
def test_conv_gradients(dev, O, aggr, cin, cout, generic, rb):
    n, e = 40, 300
    ei = random_graph(n, e, seed=cin * 100 + cout)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, cin, generator=g)
    ea = torch.randn(e, 5, generator=g)
    conv = make_conv(dev, cin, cout, aggr, rb)
    run_conv_case(dev, O, conv, ei, x, ea, f"{aggr} {cin}x{cout}", generic=generic)


# ------------------------------------------------------------------------------- 2. max ties
def test_max_ties_share_the_gradient(dev):
    """A duplicated edge (same source, destination, attributes) and a destination whose two in-edges carry equal
    messages: each tied edge gets g / ties, and the shares add up to g exactly."""
    from molecular_dynamics_neural_operator_amd import ops
    cin, cout = 3, 4
    conv = make_conv(dev, cin, cout, "max", True, ker_in=2, hidden=(8, 8))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, cin, generator=g)
    x[5] = x[4]
    # 0->2 twice (duplicate), 1->2; 4->3 and 5->3 (x[4] == x[5], same attributes); 2->0
    ei = torch.tensor([[0, 0, 1, 4, 5, 2], [2, 2, 2, 3, 3, 0]])
    ea = torch.randn(6, 2, generator=g)
    ea[1] = ea[0]
    ea[4] = ea[3]
    gy = torch.randn(6, cout, generator=g, dtype=torch.float64)

    xg, eag = x.to(dev).requires_grad_(), ea.to(dev).requires_grad_()
    y = conv(xg, ei.to(dev), eag)
    (y * gy.float().to(dev)).sum().backward()

    # the per-edge message gradient itself
    with torch.no_grad():
        graph = ops.coo_to_csr(ei.to(dev), 6)
        w_e = conv.net._forward_grad(ops.permute_rows(ea.to(dev), graph.perm, 6))     # (the forward's W_e)
        gm = ops.nnconv_msg_grad(x.to(dev), graph, w_e, gy.float().to(dev), "max")[:6].cpu()
    dst = graph.dst[:6].long().cpu()
    sums = torch.zeros(6, cout).index_add_(0, dst, gm)
    rows = torch.unique(dst)
    assert torch.equal(sums[rows], gy.float()[rows]), "edge shares do not add up to g"
    at3 = (dst == 3).nonzero().flatten()
    assert torch.equal(gm[at3[0]], gm[at3[1]]) and torch.equal(gm[at3[0]] * 2, gy.float()[3])

    # torch's scatter_reduce(amax) backward in fp64
    P = ref_params(conv)
    xr, ear = x.double().requires_grad_(), ea.double().requires_grad_()
    # one edge at a time: equal inputs give bitwise equal fp64 messages (a batched product may round its rows differently)
    msg = torch.cat([xr[ei[0, e]].unsqueeze(0) @ ref_module(ear[e:e + 1], conv.net, P, "net.").view(cin, cout)
                     for e in range(ei.shape[1])])
    agg = torch.zeros(6, cout, dtype=torch.float64).scatter_reduce(0, ei[1].unsqueeze(-1).expand_as(msg), msg,
                                                                    reduce="amax", include_self=False)
    yr = agg + xr @ P["root"] + P["bias"]
    (yr * gy).sum().backward()
    close(y, yr, name="ties y")
    check_grads(conv, P, [(xg.grad, xr.grad, "x"), (eag.grad, ear.grad, "edge_attr")], "ties")


# ------------------------------------------------------------------------------- 3. DenseNet alone
@pytest.mark.parametrize("layers,out_relu,normalize", [([5, 13, 7], False, False), ([6, 16, 18, 10], False, False),
                                                       ([4, 9, 14, 6, 5], True, False), ([5, 12, 8, 6], False, True)],
                         ids=["depth2", "depth3_fused", "depth4_relu_out", "depth3_bn_eval"])
def test_densenet_gradients(dev, layers, out_relu, normalize):
    from molecular_dynamics_neural_operator_amd.graph_kernel import DenseNet
    torch.manual_seed(2)
    net = DenseNet(layers, nn.ReLU, nn.ReLU if out_relu else None, normalize=normalize, differentiable=True).to(dev)
    if normalize:
        for m in net.layers:
            if isinstance(m, nn.BatchNorm1d):
                m.running_mean.uniform_(-0.5, 0.5)
                m.running_var.uniform_(0.5, 2.0)
                m.weight.data.uniform_(0.5, 1.5)
                m.bias.data.uniform_(-0.3, 0.3)
        net.eval()
    x = torch.randn(300, layers[0], generator=torch.Generator().manual_seed(4))
    xg = x.to(dev).requires_grad_()
    y = net(xg)
    assert y.grad_fn is not None
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    (y * gy.float().to(dev)).sum().backward()
    P = ref_params(net)
    xr = x.double().requires_grad_()
    yr = ref_module(xr, net, P, "")
    (yr * gy).sum().backward()
    close(y, yr, name="densenet y")
    check_grads(net, P, [(xg.grad, xr.grad, "x")], "densenet")


# ------------------------------------------------------------------------------- 4. composition
def test_shared_densenet_and_torch_net(dev, O):
    """Two convs share one DenseNet (gradients accumulate), a third has an nn.Sequential with a Tanh (run by torch)."""
    from molecular_dynamics_neural_operator_amd.graph_kernel import DenseNet, NNConv_old, enable_autograd
    torch.manual_seed(6)
    shared = DenseNet([5, 16, 16, 16], nn.ReLU)
    model = nn.ModuleDict({
        "c1": NNConv_old(4, 4, shared, aggr="mean"),
        "c2": NNConv_old(4, 4, shared, aggr="max"),
        "c3": NNConv_old(4, 2, nn.Sequential(nn.Linear(5, 8), nn.Tanh(), nn.Linear(8, 8)), aggr="add"),
    })
    enable_autograd(model)
    assert model.c1.differentiable and model.c3.differentiable and shared.differentiable
    model = model.to(dev)
    n, e = 30, 200
    ei = random_graph(n, e, seed=11)
    g = torch.Generator().manual_seed(8)
    x, ea = torch.randn(n, 4, generator=g), torch.randn(e, 5, generator=g)

    def fwd(c1, c2, c3, x, ei, ea):
        h = F.relu(c1(x, ei, ea))
        h = F.relu(c2(h, ei, ea))
        return c3(h, ei, ea)

    xg, eag = x.to(dev).requires_grad_(), ea.to(dev).requires_grad_()
    y = fwd(model.c1, model.c2, model.c3, xg, ei.to(dev), eag)
    (y ** 2).sum().backward()

    P = ref_params(model)
    xr, ear = x.double().requires_grad_(), ea.double().requires_grad_()
    h = F.relu(ref_conv(O, model.c1, P, "c1.", xr, ei, ear))
    h = F.relu(ref_conv(O, model.c2, P, "c2.", h, ei, ear, net_prefix="c1.net."))
    yr = ref_conv(O, model.c3, P, "c3.", h, ei, ear)
    (yr ** 2).sum().backward()
    close(y, yr, name="composition y")
    # named_parameters() lists the shared net once (under c1): its reference gradient holds both convs' shares
    check_grads(model, P, [(xg.grad, xr.grad, "x"), (eag.grad, ear.grad, "edge_attr")], "composition")


# ------------------------------------------------------------------------------- 5. training trajectory
class _Regressor(nn.Module):
    def __init__(self, width=8):
        super().__init__()
        from molecular_dynamics_neural_operator_amd.graph_kernel import DenseNet, NNConv_old
        self.fc1 = nn.Linear(3, width)
        self.convs = nn.ModuleList([NNConv_old(width, width, DenseNet([4, 16, 16, width * width], nn.ReLU), aggr=a,
                                               differentiable=True) for a in ("mean", "max", "mean")])
        self.fc2 = nn.Linear(width, 1)

    def forward(self, x, ei, ea):
        h = self.fc1(x)
        for c in self.convs:
            h = F.relu(c(h, ei, ea))
        return self.fc2(h)


def test_training_trajectory_matches_fp64(dev, O):
    from molecular_dynamics_neural_operator_amd import training
    torch.manual_seed(9)
    model = _Regressor()
    ref = {n: p.detach().double().clone().requires_grad_() for n, p in model.named_parameters()}
    model = model.to(dev)
    n, e = 48, 360
    ei = random_graph(n, e, seed=12)
    g = torch.Generator().manual_seed(10)
    x, ea, target = torch.randn(n, 3, generator=g), torch.randn(e, 4, generator=g), torch.randn(n, 1, generator=g)
    # (lr 3e-4 as test_adam_trajectory_vs_oracle: Adam's first steps move every weight by ~lr whatever the gradient's
    # size, so a gradient component near zero, where fp32 and fp64 may differ in sign, decides a whole step)
    opt = training.Adam(model.parameters(), lr=3e-4)
    ref_opt = torch.optim.Adam(list(ref.values()), lr=3e-4)
    xd, eid, ead, td = x.to(dev), ei.to(dev), ea.to(dev), target.to(dev)
    xr, ear, tr = x.double(), ea.double(), target.double()

    def ref_forward():
        h = F.linear(xr, ref["fc1.weight"], ref["fc1.bias"])
        for i, c in enumerate(model.convs):
            h = F.relu(ref_conv(O, c, ref, f"convs.{i}.", h, ei, ear))
        return F.linear(h, ref["fc2.weight"], ref["fc2.bias"])

    for step in range(20):
        opt.zero_grad()
        loss = F.mse_loss(model(xd, eid, ead), td)
        loss.backward()
        opt.step()
        ref_opt.zero_grad()
        ref_loss = F.mse_loss(ref_forward(), tr)
        ref_loss.backward()
        ref_opt.step()
        rel = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
        assert rel <= 1e-5, f"step {step}: loss {float(loss)} vs {float(ref_loss)} (rel {rel:.2e})"
    for name, p in model.named_parameters():
        close(p, ref[name], rtol=1e-4, rel_l2=1e-4, name=f"param {name}")


# ------------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("aggr,cin,cout", [("max", 64, 64), ("mean", 8, 16), ("add", 64, 64)])
def test_backward_is_bitwise_reproducible(dev, aggr, cin, cout):
    conv = make_conv(dev, cin, cout, aggr, True)
    n, e = 40, 300
    ei = random_graph(n, e, seed=13).to(dev)
    g = torch.Generator().manual_seed(14)
    x, ea = torch.randn(n, cin, generator=g).to(dev), torch.randn(e, 5, generator=g).to(dev)
    gy = torch.randn(n, cout, generator=g).to(dev)
    runs = []
    for _ in range(2):
        conv.zero_grad()
        xg, eag = x.clone().requires_grad_(), ea.clone().requires_grad_()
        (conv(xg, ei, eag) * gy).sum().backward()
        runs.append([xg.grad.clone(), eag.grad.clone()] + [p.grad.clone() for p in conv.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------- 7. size
@pytest.mark.parametrize("aggr,width,generic", [("mean", 64, False), ("mean", 64, True), ("max", 64, False),
                                                ("add", 32, False)])
def test_box_graph_gradients(dev, O, aggr, width, generic):
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    frame = syn.box_frame(220)
    ei = torch.from_numpy(O.radius_graph_coo(frame, 8.0)).long()
    assert ei.shape[1] >= 16000, ei.shape
    pos = torch.from_numpy(frame).float()
    ea = torch.cat([pos[ei[0]], pos[ei[1]]], dim=1) / 10.0
    x = torch.randn(pos.shape[0], width, generator=torch.Generator().manual_seed(15))
    conv = make_conv(dev, width, width, aggr, True, ker_in=6, hidden=(16, 16), seed=3)
    run_conv_case(dev, O, conv, ei, x, ea, f"box {aggr} {width}x{width}", generic=generic)


# ------------------------------------------------------------------------------- 8. opt-in and refusals
def test_flag_off_still_refuses_training(dev):
    from molecular_dynamics_neural_operator_amd.graph_kernel import DenseNet, NNConv_old
    conv = make_conv(dev, 4, 4, "mean", True)
    conv.differentiable = False
    conv.train()
    ei = random_graph(20, 60, seed=1).to(dev)
    x, ea = torch.randn(20, 4, device=dev), torch.randn(60, 5, device=dev)
    with pytest.raises(NotImplementedError):
        conv(x, ei, ea)
    net = DenseNet([5, 8, 3], nn.ReLU).to(dev).train()
    assert net.differentiable is False
    with pytest.raises(NotImplementedError):
        net(ea)
    # flag on, nothing needs a gradient: today's inference forward, same values
    conv.eval()
    with torch.no_grad():
        off = conv(x, ei, ea)
        conv.differentiable = True
        on = conv(x, ei, ea)
    assert torch.equal(off, on) and on.grad_fn is None


def test_flag_on_refusals(dev):
    from molecular_dynamics_neural_operator_amd.graph_kernel import DenseNet
    x = torch.randn(50, 5, device=dev)
    bn = DenseNet([5, 8, 3], nn.ReLU, normalize=True, differentiable=True).to(dev).train()
    with pytest.raises(NotImplementedError, match="batch statistics"):
        bn(x)
    tanh = DenseNet([5, 8, 3], nn.Tanh, differentiable=True).to(dev)
    with pytest.raises(NotImplementedError, match="Tanh"):
        tanh(x)
    conv = make_conv(dev, 4, 4, "max", True)
    ei = random_graph(20, 60, seed=2).to(dev)
    xg = torch.randn(20, 4, device=dev, requires_grad=True)
    y = conv(xg, ei, torch.randn(60, 5, device=dev))
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(y.sum(), xg, create_graph=True)
