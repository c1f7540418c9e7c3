"""fp64 replica of `train_precision="bf16"` (molecular_dynamics_neural_operator_amd/training.py
the bf16 branches of `KernelIntegralBlock`, csrc/train_bf16.hip, csrc/train_conv.hip) — TEST INFRASTRUCTURE.

The oracle's train step (oracle/graph_kernel_oracle.py `train_step`: the reference's forward, loss and
backward in fp64) with the bf16 path's STORAGE roundings put where the HIP path has them, so that what is
left between the two is fp32-vs-fp64 accumulation only:

  forward   h1 = bf16(relu(ea.W0^T + b0))                    (fp32 fmaf chains on the device, then one rounding)
            h2 = bf16(relu(h1.bf16(W1)^T + b1))              (bf16 x bf16 products, fp32 accumulation)
            W_e = bf16(h2.bf16(W2)^T + b2)
  backward  dW_e = bf16(sum over the 2*depth applications of x_src (x) gs_dst)
            gz2  = bf16(mask(h2) * (dW_e.bf16(W2)))          db2 = colsum(dW_e), dW2 = dW_e^T.h2
            gz1  = bf16(mask(h1) * (gz2.bf16(W1)))           db1 = colsum(gz2),  dW1 = gz2^T.h1
            db0 = colsum(gz1),  dW0 = gz1^T.ea               (one pass over gz1, fp32 attributes)

Everything else (per-atom prologue, conv applications on the rounded W_e, fc2, loss) is fp32 on the device and
fp64 here.  Rounding is round-to-nearest-even (torch's .to(bfloat16) == v_cvt_pk_bf16_f32)."""
import torch
import torch.nn.functional as F


def _r(x):
    return x.to(torch.bfloat16).to(x.dtype)


class _RoundForward(torch.autograd.Function):
    """y = bf16(x); gradient passes unchanged (the device differentiates through the rounded value)."""

    @staticmethod
    def forward(ctx, x):
        return _r(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBackward(torch.autograd.Function):
    """y = x; the gradient arriving here is what the device stores in bf16."""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return _r(g)


class _Layer0(torch.autograd.Function):
    """ea.W0^T + b0 with dW0 = g^T.ea (training.py: mdno_colsum_atb_bf16, fp32 attributes)."""

    @staticmethod
    def forward(ctx, ea, w0, b0):
        ctx.save_for_backward(ea)
        return ea @ w0.t() + b0

    @staticmethod
    def backward(ctx, g):
        (ea,) = ctx.saved_tensors
        return None, g.t() @ ea, g.sum(0)


def edge_mlp_bf16(edge_attr, p, prefix="conv1.net."):
    w0, b0 = p[prefix + "layers.0.weight"], p[prefix + "layers.0.bias"]
    w1, b1 = p[prefix + "layers.2.weight"], p[prefix + "layers.2.bias"]
    w2, b2 = p[prefix + "layers.4.weight"], p[prefix + "layers.4.bias"]
    h1 = _RoundForward.apply(F.relu(_RoundBackward.apply(_Layer0.apply(edge_attr, w0, b0))))
    h2 = _RoundForward.apply(F.relu(_RoundBackward.apply(h1 @ _RoundForward.apply(w1).t() + b1)))
    return _RoundBackward.apply(_RoundForward.apply(h2 @ _RoundForward.apply(w2).t() + b2))


def train_step_bf16(O, sd, samples, depth, dtype=torch.float64):
    """Same contract as O.train_step: (loss, out, {name: grad}); one block-diagonal batch like the device
    (a sample's rows only meet its own edges, so this equals sample-by-sample evaluation)."""
    shared = {k: v for k, v in sd.items() if not k.startswith("conv2.net.")}
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in shared.items()}
    outs, ys = [], []
    for s in samples:
        x = O.lstm_last_hidden_functional(s["x_position"], p)
        x = F.linear(x, p["lstm_fc.weight"], p["lstm_fc.bias"])
        x = F.relu(F.linear(torch.cat((F.embedding(s["x_aminoacid"], p["emb.weight"]), x), dim=1),
                            p["fc1.weight"], p["fc1.bias"]))
        w_e = edge_mlp_bf16(s["edge_attr"].to(dtype), p)
        for conv in ("conv1", "conv2"):
            for _ in range(depth):
                x = F.relu(O.nnconv_apply(x, s["edge_index"], w_e, p[conv + ".root"], p[conv + ".bias"], "mean"))
        outs.append(F.linear(x, p["fc2.weight"], p["fc2.bias"]))
        ys.append(s["y"].to(dtype))
    out, y = torch.cat(outs), torch.cat(ys)
    b = len(samples)
    loss = O.lp_loss_rel(out.view(b, -1), y.view(b, -1), size_average=False)
    names = list(p)
    g = dict(zip(names, torch.autograd.grad(loss, [p[n] for n in names])))
    for k in list(g):
        if k.startswith("conv1.net."):
            g["conv2.net." + k[len("conv1.net."):]] = g[k]
    return float(loss.detach()), out.detach(), g
