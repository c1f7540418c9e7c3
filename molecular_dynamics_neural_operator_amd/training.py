"""Training path (BASELINE.json configs[3]): the whole differentiable forward and
backward of `KernelNN` runs in libmdno's HIP kernels behind three `torch.autograd.Function`s — the node
prologue (LSTM(3,3) over the window, lstm_fc, Embedding, fc1, ReLU: graph_kernel.py:279-298), the
kernel-integral block (shared edge-MLP + 2*depth conv applications, :299-302) and fc2 (:305).  PyTorch
holds the parameters, chains the three functions and runs the optimizer; it computes nothing.

Replaces what autograd + torch_geometric do in `train()` (graph_kernel.py:445-474).  Members of a
batch are independent B=1 problems (block-diagonal graph); the reference's batched mode threads one
LSTM state through the batch axis and is not reproduced.

Two precisions (`model.train_precision`):
  "fp32" (default)  fp32 storage everywhere; the wide GEMMs per `model.gemm_mode` (bf16-split planes at
                    fp32-level accuracy, or fp32 MFMA); gradients match an fp64 replica to ~1e-6.
  "bf16"            BASELINE.json configs[3] ("bf16"): the block's large tensors (h1, h2, W_e, dW_e) are
                    stored in bf16 and every GEMM is one bf16 MFMA product with fp32 accumulation
                    (csrc/train_bf16.hip, csrc/train_conv.hip); parameters stay fp32 masters, reductions stay fp32.  Half the
                    memory of the two E x 16 KiB tensors, gradients match the fp64 replica to ~1e-2.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from ._args import INT_MAX
from ._lib import MdnoError
from .dataset import PairData
from .graph_kernel import LpLoss


class KernelIntegralBlock(torch.autograd.Function):
    """x_L = conv2^depth(conv1^depth(x_0)) with W_e = net(edge_attr) shared by every application
    (graph_kernel.py:271-273, :299-302), materialised formulation.  gemm_mode as for inference:
    "split_bf16" runs the four wide C = A.W^T products (two forward, two backward) on the bf16 matrix
    pipe with the exact 3-way split, "f32" on the fp32 MFMA; the weight-gradient products A^T.B are
    fp32 either way."""

    @staticmethod
    def forward(ctx, x0, edge_attr, graph, depth, gemm_mode, w0, b0, w1, b1, w2, b2, root1, bias1, root2, bias2):
        """graph.x_stack (optional): f32 [2*depth+1, R, 64] whose layer 0 IS x0 — train_forward lets the node prologue
        write there, so the block copies nothing in.  Returns layer 2*depth of the stack (a view: the stack is kept
        for the backward anyway)."""
        R = x0.shape[0]
        X = getattr(graph, "x_stack", None)
        E = graph.edge_count()
        ea = ops.permute_rows(edge_attr, graph.perm, E) if graph.perm is not None else ops.f32(edge_attr).contiguous()
        L = 2 * depth
        if X is None or X.data_ptr() != x0.data_ptr() or tuple(X.shape) != (L + 1, R, 64):
            X = torch.empty((L + 1, R, 64), dtype=torch.float32, device=x0.device)
            X[0].copy_(x0)
        ctx.bf16 = gemm_mode == "bf16"
        if ctx.bf16:
            h1 = ops.linear_smallk_bf16(ea, w0, b0, relu=True)               # K = 6: fp32 fmaf chains, stored bf16
            h2 = ops.linear_bf16(h1, w1, b1, relu=True, out_bf16=True)
            w_e = ops.linear_bf16(h2, w2, b2, relu=False, out_bf16=True)     # [E, 4096] bf16: 8 KiB per edge
        else:
            h1 = ops.linear(ea, w0, b0, relu=True)
            h2 = ops.linear(h1, w1, b1, relu=True, gemm_mode=gemm_mode)
            w_e = ops.linear(h2, w2, b2, relu=False, gemm_mode=gemm_mode)
        ops.nnconv_chain_fwd(X, graph, w_e, root1, bias1, root2, bias2, depth)        # the 2*depth applications, one call
        ctx.graph, ctx.depth, ctx.gemm_mode = graph, depth, gemm_mode
        ctx.save_for_backward(ea, h1, h2, w_e, X, w0, w1, w2, root1, root2)
        return X[L]

    @staticmethod
    def backward(ctx, g_out):
        ea, h1, h2, w_e, X, w0, w1, w2, root1, root2 = ctx.saved_tensors
        graph, depth, gemm_mode = ctx.graph, ctx.depth, ctx.gemm_mode
        L, R = 2 * depth, X.shape[1]
        # the conv applications: the same five steps in either precision (the ops pick the kernel by W_e's dtype)
        by_src = getattr(graph, "by_src", None) or ops.source_sorted(graph, R)
        inv = ops.inv_degree(graph, "mean")
        GZ, GS, g = ops.nnconv_chain_bwd(g_out, X, inv, by_src, w_e, root1, root2, depth)
        d_root1, d_bias1, d_root2, d_bias2 = ops.nnconv_bwd_root_pair(X[0:L], GZ[0:L])       # both convs, one launch
        bwd_we = ops.nnconv_bwd_we_bf16 if ctx.bf16 else ops.nnconv_bwd_we
        d_we, d_b2 = bwd_we(X[0:L], GS, graph, with_colsum=True)        # [E, 4096] and its column sums, one pass
        del GZ, GS
        # edge-MLP backward
        if ctx.bf16:
            d_w2 = ops.gemm_atb_bf16(d_we, h2)
            gz2 = ops.linear_bf16_relu_bwd(d_we, ops.transpose(w2), h2)        # bf16((h2 > 0) * (dW_e . W2))
            del d_we
            d_b1 = ops.colsum_bf16(gz2)
            d_w1 = ops.gemm_atb_bf16(gz2, h1)
            gz1 = ops.linear_bf16_relu_bwd(gz2, ops.transpose(w1), h1)
            # first layer: bias and weight gradient in ONE pass over gz1 (d_w0 = gz1^T . ea with the fp32 attributes)
            d_b0, d_w0 = ops.colsum_atb_bf16(gz1, ea)
        else:
            d_w2 = ops.gemm_atb(d_we, h2, gemm_mode=gemm_mode)
            gz2 = ops.relu_bwd(ops.linear(d_we, ops.transpose(w2), None, gemm_mode=gemm_mode), h2)
            del d_we
            d_b1 = ops.colsum(gz2)
            d_w1 = ops.gemm_atb(gz2, h1, gemm_mode=gemm_mode)
            gz1 = ops.relu_bwd(ops.linear(gz2, ops.transpose(w1), None, gemm_mode=gemm_mode), h1)
            d_b0 = ops.colsum(gz1)
            d_w0 = ops.gemm_atb(gz1, ea)
        d_ea = _edge_attr_grad(ctx, gz1, w0, graph) if ctx.needs_input_grad[1] else None
        return (g, d_ea, None, None, None, d_w0, d_b0, d_w1, d_b1, d_w2, d_b2, d_root1, d_bias1, d_root2, d_bias2)


def _edge_attr_grad(ctx, gz1, w0, graph):
    """dLoss/d edge_attr of a kernel-integral block, in the caller's edge order: gz1 . W0 in CSR order
    (mdno_edge_mlp_input_bwd), then `graph.perm` undone (mdno_scatter_rows)."""
    if getattr(ctx, "bf16", False):
        raise NotImplementedError('train_precision="bf16" has no gradient with respect to edge_attr (fp32 only)')
    d_ea = ops.edge_mlp_input_bwd(gz1, w0, graph.num_edges)
    if graph.perm is not None:
        d_ea = ops.scatter_rows(d_ea, graph.perm, d_ea.shape[0])
    return d_ea


class FactoredKernelIntegralBlock(torch.autograd.Function):
    """The same block in the factored formulation (`model.train_conv_mode`; csrc/train_moment.hip):
    per destination the sum over its in-edges is taken before the contraction with W2, so neither W_e nor dW_e
    [E, 4096] exists.  Kept for the backward: the feature stack and H = h2 as the k-tiled image (4 k bytes per edge).
    fp32 storage; the forward runs in `gemm_mode` (bitwise the eval-mode factored forward), the backward's own
    products are fp32 fmaf chains in every mode."""

    @staticmethod
    def forward(ctx, x0, edge_attr, graph, depth, gemm_mode, w0, b0, w1, b1, w2, b2, root1, bias1, root2, bias2):
        R = x0.shape[0]
        X = getattr(graph, "x_stack", None)
        L = 2 * depth
        if X is None or X.data_ptr() != x0.data_ptr() or tuple(X.shape) != (L + 1, R, 64):
            X = torch.empty((L + 1, R, 64), dtype=torch.float32, device=x0.device)
            X[0].copy_(x0)
        ea = ops.f32(edge_attr).contiguous()
        h_img = ops.train_moment_fwd(X, graph, ea, (w0, b0, w1, b1, w2, b2), root1, bias1, root2, bias2, depth, gemm_mode)
        ctx.graph, ctx.depth, ctx.gemm_mode = graph, depth, gemm_mode
        ctx.save_for_backward(ea, h_img, X, w0, b0, w1, w2, b2, root1, root2)
        return X[L]

    @staticmethod
    def backward(ctx, g_out):
        ea, h_img, X, w0, b0, w1, w2, b2, root1, root2 = ctx.saved_tensors
        graph, depth, gemm_mode = ctx.graph, ctx.depth, ctx.gemm_mode
        L, R = 2 * depth, X.shape[1]
        E = graph.edge_count()
        by_src = getattr(graph, "by_src", None) or ops.source_sorted(graph, R)
        gz, g, gz2, d_w2, d_b2 = ops.train_moment_bwd(g_out.contiguous(), X, h_img, graph, by_src, w2, b2, root1, root2,
                                                      depth, gemm_mode)
        d_root1, d_bias1, d_root2, d_bias2 = ops.nnconv_bwd_root_pair(X[0:L], gz)
        del gz
        # edge-MLP backward below H, with the existing ops; h1 is formed again from the attributes (K = ker_in: cheap)
        if graph.perm is not None:
            ea = ops.permute_rows(ea, graph.perm, E)
        h1 = ops.linear(ea, w0, b0, relu=True)
        d_b1 = ops.colsum(gz2)
        d_w1 = ops.gemm_atb(gz2, h1, gemm_mode=gemm_mode)
        gz1 = ops.relu_bwd(ops.linear(gz2, ops.transpose(w1), None, gemm_mode=gemm_mode), h1)
        del gz2, h1
        d_b0 = ops.colsum(gz1)
        d_w0 = ops.gemm_atb(gz1, ea)
        d_ea = _edge_attr_grad(ctx, gz1, w0, graph) if ctx.needs_input_grad[1] else None
        return (g, d_ea, None, None, None, d_w0, d_b0, d_w1, d_b1, d_w2, d_b2, d_root1, d_bias1, d_root2, d_bias2)


class NodePrologue(torch.autograd.Function):
    """x0 = relu(fc1([emb(aa), lstm_fc(LSTM over the window)]))  (graph_kernel.py:279-298), B=1 semantics per
    sample.  Parameters arrive as tensors (autograd tracks them) and as the model's ParamPack (device pointers)."""

    @staticmethod
    def forward(ctx, pack, frames, aa, *params):
        x0 = ops.node_prologue(pack, frames, aa, status=pack.train_status, out=getattr(pack, "prologue_out", None))
        ctx.pack, ctx.names = pack, pack.prologue_names
        ctx.save_for_backward(frames, aa, x0)
        return x0

    @staticmethod
    def backward(ctx, g0):
        frames, aa, x0 = ctx.saved_tensors
        need_frames = ctx.needs_input_grad[1]
        grads = ops.node_prologue_bwd(ctx.pack, frames, aa, x0, g0.contiguous(), need_frames=need_frames)
        return (None, grads["frames"] if need_frames else None, None) + tuple(grads[n] for n in ctx.names)


class FcOut(torch.autograd.Function):
    """fc2 (graph_kernel.py:305)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return ops.fc_out(x, w, b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        dx, d_w, d_b = ops.fc_out_bwd(x, w, g.contiguous())
        return dx, d_w, d_b


class EdgeAttrFromPositions(torch.autograd.Function):
    """edge_attr [E, 6] = [pos[src p], pos[dst p]] in `graph`'s CSR edge order, differentiable in `pos` [R, 3]
    (include/mdno_unroll.h mdno_edge_attr_from_pos / mdno_edge_attr_pos_bwd).  The graph is data: no gradient goes
    through its topology.  `graph.by_src` (ops.source_sorted) is used by the backward where it is already there.
    `box` (with `cutoff`, which only validates it): the source half of every row is the source's minimum image next to
    the destination, pos[src p] - k L (include/mdno_pbc_train.h).  The shift k L is a constant of the edge — k is
    piecewise constant in the positions, and no gradient goes through it, as none goes through the topology — so the
    backward is the open one, the same kernel on the same arguments."""

    @staticmethod
    def forward(ctx, pos, graph, box=None, cutoff=8.0):
        ctx.graph, ctx.rows = graph, pos.reshape(-1, 3).shape[0]
        ctx.shape = tuple(pos.shape)
        if box is None:
            return ops.edge_attr_from_pos(pos, graph)
        return ops.edge_attr_from_pos(pos, graph, box, cutoff)

    @staticmethod
    def backward(ctx, g):
        graph = ctx.graph
        by_src = getattr(graph, "by_src", None) or ops.source_sorted(graph, ctx.rows)
        return ops.edge_attr_pos_bwd(g.contiguous(), graph, by_src, ctx.rows).view(ctx.shape), None, None, None


_PROLOGUE_KEYS = ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "lstm_fc.weight",
                  "lstm_fc.bias", "emb.weight", "fc1.weight", "fc1.bias")


def collate(samples: Sequence[PairData]) -> PairData:
    """Block-diagonal batch; x_position stacked time-major [W, B*N, 3]."""
    if isinstance(samples, PairData):
        return samples
    b = PairData.collate(samples)
    W = samples[0].x_position.shape[0]
    b.x_position = torch.cat([s.x_position for s in samples], dim=1) if samples[0].x_position.dim() == 3 else \
        torch.cat([s.x_position.unsqueeze(0) for s in samples], dim=1)
    assert b.x_position.shape[0] == W or samples[0].x_position.dim() == 2
    b.num_graphs = len(samples)
    return b


class DeviceTrajectory:
    """A `ContactMapDataset` resident in HBM, handing out training batches built ON the device
    (include/mdno.h mdno_collate_samples).  Stands in for the reference's `DataListLoader` + torch_geometric
    collation (graph_kernel.py:513-519; `model(batch)` at :454 collates per step on the host): per batch the
    host only fills a 3*B+1 word table from the dataset's offsets — no per-sample Python, no per-sample H2D
    copies, no device->host read.  `batch(indices)` returns a collated `PairData` (time-major x_position
    [W,B*N,3], y, edge_index, edge_attr, x_aminoacid tiled) whose samples are `dataset[i]` for i in indices,
    in that order — the same tensors `collate([dataset[i] ...])` builds on the host (tested bitwise).

    `box` = (Lx, Ly, Lz) (with `cutoff`; include/mdno_pbc.h): the trajectory lies in a periodic cell.  The stored
    contact maps are then not used: a sample's edges are the minimum-image radius graph of its first window frame
    (frame idx, the frame whose stored map the open path uses) and its attributes that graph's imaged rows — what
    `construct_pairdata(window[:1], aa, cutoff, box=box)` gives per sample on the host, `edge_index[0]` = sources,
    sorted by target.  The edges of every stored frame are counted once, here (one read-back), so `batch()` sizes its
    buffers without reading the device, as on the open path; the batch carries `box` and `cutoff`, which
    `unrolled_forward` takes from it.  With box None (or all zero) every line below runs as it always has."""

    def __init__(self, dataset, device, box=None, cutoff: float = 8.0):
        self.box = ops.check_box(box, cutoff)
        self.cutoff = float(cutoff)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise MdnoError("DeviceTrajectory needs a GPU device (no CPU fallback)")
        self.W, self.horizon = int(dataset.window_size), int(dataset.horizon)
        self.length = len(dataset)
        pos = np.ascontiguousarray(dataset.edge_attrs, dtype=np.float32)                  # [T,N,3]
        self.N = int(pos.shape[1])
        self.pos = torch.from_numpy(pos).to(self.device)
        if self.box is None:
            cms = [np.asarray(c).reshape(2, -1) for c in dataset.edge_indices]
            counts = np.array([c.shape[1] for c in cms], dtype=np.int64)
            self.counts = counts
            self.offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            self.rows = torch.from_numpy(np.concatenate([c[0] for c in cms]).astype(np.int32)).to(self.device)
            self.cols = torch.from_numpy(np.concatenate([c[1] for c in cms]).astype(np.int32)).to(self.device)
        else:
            self.counts = self._count_periodic_edges()
            self.offsets = self.rows = self.cols = None
        self.x_aminoacid = dataset.x_aminoacid.to(self.device)
        self._aa_tiled = {}
        # the per-batch index table travels through a ring of PINNED host buffers: the upload is asynchronous, and a
        # slot is only rewritten once the copy that read it has passed (its event) — a pageable source would have to
        # be staged synchronously by the runtime to be safe
        self._meta_ring, self._meta_slot = [], 0

    _META_SLOTS = 4

    def _count_periodic_edges(self) -> np.ndarray:
        """Edges of the minimum-image radius graph of every stored frame, i64 [T] on the host: chunks of frames as the
        members of one topology-only graph call (at most 64M edge slots each, as graph_kernel._pairdata_of_windows),
        a frame's count = the difference of its first and the next frame's first row pointer."""
        T, N = int(self.pos.shape[0]), self.N
        chunk = max(1, min(T, (64 << 20) // max(N * N, 1)))
        counts = []
        for t0 in range(0, T, chunk):
            frames = self.pos[t0:t0 + chunk]
            g, _ = ops.radius_graph_pbc(frames.reshape(-1, 3), N, self.cutoff, self.box, with_attr=False)
            counts.append(torch.diff(g.row_ptr[::N]))
        return torch.cat(counts).cpu().numpy().astype(np.int64)           # the one read-back

    def _meta_buffer(self, words: int):
        if len(self._meta_ring) < self._META_SLOTS:
            self._meta_ring.append([torch.empty(max(words, 1024), dtype=torch.int64).pin_memory(), None])
            slot = self._meta_ring[-1]
        else:
            slot = self._meta_ring[self._meta_slot]
            self._meta_slot = (self._meta_slot + 1) % self._META_SLOTS
            if slot[1] is not None:
                slot[1].synchronize()
            if slot[0].numel() < words:
                slot[0] = torch.empty(words, dtype=torch.int64).pin_memory()
        return slot

    def __len__(self) -> int:
        return self.length

    def truth_frames(self, start: int, steps: int) -> torch.Tensor:
        """The `y` of samples start .. start + steps - 1 as ONE view [steps, N, 3] of the resident positions (no copy):
        frame start + k + window + horizon - 1 for sample start + k.  At horizon 1 these are the frames a free run from
        `dataset[start]` predicts step by step — what `graph_kernel.propogate` compares against — so they are the `truth`
        of `RolloutEngine.score` / `forecast.score_forecast`."""
        start, steps = int(start), int(steps)
        if start < 0 or steps < 0 or start + steps > self.length:
            raise IndexError(f"samples {start} .. {start + steps - 1} do not all lie in [0, {self.length})")
        first = start + self.W + self.horizon - 1
        return self.pos[first:first + steps]

    def batch(self, indices, noise_std: float = 0.0, noise_seed: int = 0, epoch: int = 0, unroll: int = 1,
              augment=None) -> PairData:
        """unroll = K > 1: the batch also carries `y_unroll` f32 [K, B*N, 3], the true frames an unrolled step of K
        model steps is scored against (frame idx + W + k of every sample, k < K; one more launch: include/mdno_unroll.h
        mdno_collate_targets); `y` stays `y_unroll[0]`.  Needs horizon 1 (the window slides one frame per step) and
        every sample index <= len - K.
        noise_std > 0: the input windows (`x_position` only — `y`, `edge_attr` and `edge_index` stay clean) get
        noise_std * z(noise_seed, sample index, epoch, frame, atom, component) added on the device (include/mdno_noise.h
        mdno_noise_add_window).  The key is the sample's index in the dataset: a sample's noise does not depend on the
        batch it is in, the batch size or the rank.  The batch carries `sample_ids` / `rows_per_sample` either way.
        augment = a `RigidAugment`: every sample is moved by its own random rigid motion, keyed by (augment.seed, sample
        index, epoch) — `augment_batch(batch, augment, epoch)`: windows, `y`, `y_unroll` moved, `edge_attr` gathered again,
        the batch carries `.motions`.  Noise, if asked for, is added after the motion with the values it always had.
        None: not one launch, allocation or bit differs.  Not under a box (`MdnoError`).
        Under a box (`DeviceTrajectory(box=)`): `edge_index` [2, E] holds the sources in row 0 (sorted by target, sources
        ascending), `edge_attr` the imaged rows, and the batch carries `box` and `cutoff` (`_periodic_batch`)."""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if idx.size == 0 or idx.min() < 0 or idx.max() >= self.length:
            raise IndexError(f"sample indices must lie in [0, {self.length})")
        K = int(unroll)
        if K < 1:
            raise MdnoError(f"unroll={unroll} (>= 1)")
        if K > 1 and self.horizon != 1:
            raise MdnoError(f"unroll={K} needs horizon 1 (got {self.horizon}): the window slides one frame per step")
        if idx.max() > self.length - K:
            raise IndexError(f"unroll={K}: sample indices must lie in [0, {self.length - K}] (the last target is frame "
                             f"index + window + {K - 1})")
        B = int(idx.size)
        if augment is not None and self.box is not None:
            raise MdnoError("rigid augmentation under a periodic box is not supported: an orthorhombic cell is not "
                            "rotation-invariant")
        if self.box is not None:
            return self._periodic_batch(idx, B, K, noise_std, noise_seed, epoch)
        cnt = self.counts[idx]
        slot = self._meta_buffer(3 * B + 1)
        meta = slot[0][:3 * B + 1].numpy()
        meta[:B] = idx
        meta[B:2 * B] = self.offsets[idx]
        meta[2 * B] = 0
        np.cumsum(cnt, out=meta[2 * B + 1:])
        E = int(meta[3 * B])
        meta_d = slot[0][:3 * B + 1].to(self.device, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(self.device))
        xp, y, ei, ea = ops.collate_samples(self.pos, self.rows, self.cols, meta_d, B, self.N, self.W, self.horizon, E,
                                            int(cnt.max()))
        if B not in self._aa_tiled:
            self._aa_tiled[B] = self.x_aminoacid.repeat(B)
        out = PairData(x_aminoacid=self._aa_tiled[B], x_position=xp, y=y, edge_attr=ea, edge_index=ei)
        out.num_graphs = B
        out.sample_ids, out.rows_per_sample = idx.copy(), self.N
        if K > 1:
            out.y_unroll = ops.collate_targets(self.pos, meta_d, B, self.N, self.W, self.horizon, K)
        else:
            out.y_unroll = y.unsqueeze(0)
        if augment is not None:
            out = augment_batch(out, augment, epoch)
        if float(noise_std) != 0.0:
            out.x_position = add_window_noise(out, noise_std, noise_seed, epoch)
        return out

    def _periodic_batch(self, idx: np.ndarray, B: int, K: int, noise_std: float, noise_seed: int, epoch: int) -> PairData:
        """`batch` under a box: positions and targets by the launches of the open path (mdno_collate_samples without its
        edge launch, mdno_collate_targets), the edges and their imaged attributes by ONE periodic radius graph of the B
        clean first frames (members of one call), sized by the counts taken at construction — nothing is read back.
        Noise perturbs `x_position` only, after the graph is built."""
        E = int(self.counts[idx].sum())
        slot = self._meta_buffer(3 * B + 1)
        meta = slot[0][:3 * B + 1].numpy()
        meta[:B] = idx
        meta[B:] = 0                      # (no stored edge list: offsets and cumulative counts are not read)
        meta_d = slot[0][:3 * B + 1].to(self.device, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(self.device))
        xp, y = ops.collate_positions(self.pos, meta_d, B, self.N, self.W, self.horizon)
        g, attr = ops.radius_graph_pbc(xp[0], self.N, self.cutoff, self.box, edge_cap=E)
        if B not in self._aa_tiled:
            self._aa_tiled[B] = self.x_aminoacid.repeat(B)
        out = PairData(x_aminoacid=self._aa_tiled[B], x_position=xp, y=y, edge_attr=attr[:E],
                       edge_index=torch.stack([g.src[:E], g.dst[:E]]).to(torch.long))
        out.num_graphs = B
        out.sample_ids, out.rows_per_sample = idx.copy(), self.N
        out.box, out.cutoff = self.box, self.cutoff
        out.y_unroll = ops.collate_targets(self.pos, meta_d, B, self.N, self.W, self.horizon, K) if K > 1 else y.unsqueeze(0)
        if float(noise_std) != 0.0:
            out.x_position = add_window_noise(out, noise_std, noise_seed, epoch)
        return out


def add_window_noise(batch: PairData, noise_std: float, noise_seed: int = 0, epoch: int = 0) -> torch.Tensor:
    """The noisy `x_position` [W, B*N, 3] of a collated batch made by `DeviceTrajectory.batch` (it knows which dataset
    sample every row belongs to): a new tensor, the batch itself is left as it is."""
    ids = getattr(batch, "sample_ids", None)
    if ids is None:
        raise MdnoError("window noise needs batches from DeviceTrajectory.batch (they carry their samples' dataset "
                        "indices); host-collated samples have none")
    if not (0.0 <= float(noise_std) < float("inf")):
        raise MdnoError(f"noise_std={noise_std} must be finite and >= 0")
    n, dev = int(batch.rows_per_sample), batch.x_position.device
    offs = torch.arange(0, (len(ids) + 1) * n, n, dtype=torch.int32, device=dev)
    return ops.noise_add_window(batch.x_position, ids, offs, n, noise_std, noise_seed, epoch)


# ------------------------------------------------------------------------------------------------
# Random rigid motions of training samples (include/mdno_augment.h; the rule: csrc/rigid_rule.h)
RIGID_PIVOTS = ("centroid", "origin")


class RigidAugment:
    """What `DeviceTrajectory.batch(augment=)`, `train_epoch(augment=)` and `augment_batch` draw a sample's motion
    from: a uniform rotation (`rotate`) about the `pivot` — the centroid of the sample's first window frame, or the
    origin — and a translation uniform in the cube [-translate, translate]^3 (Angstrom), keyed by (seed, the sample's
    index in its dataset, epoch) and nothing else."""

    def __init__(self, seed: int = 0, rotate: bool = True, translate: float = 0.0, pivot: str = "centroid"):
        self.seed = ops._noise_seed(seed)
        self.rotate = bool(rotate)
        self.translate = float(translate)
        if not 0.0 <= self.translate < float("inf"):
            raise MdnoError(f"translate={translate} must be finite and >= 0")
        if pivot not in RIGID_PIVOTS:
            raise MdnoError(f"pivot={pivot!r}: expected one of {list(RIGID_PIVOTS)}")
        self.pivot = pivot

    def __repr__(self) -> str:
        return f"RigidAugment(seed={self.seed}, rotate={self.rotate}, translate={self.translate}, pivot={self.pivot!r})"


class RigidMotions:
    """The motions of the B samples of one collated batch, on the batch's device: `quaternion` f64 [B,4] (w,x,y,z; not
    normalised), `pivot` f64 [B,3], `shift` f64 [B,3], `attempts` i32 [B,2] (the accepted elements of the rejection
    loop, -1 where the identity was taken instead) and `n_atoms`, the rows every sample owns."""

    def __init__(self, quaternion, pivot, shift, attempts, n_atoms: int):
        self.quaternion, self.pivot, self.shift, self.attempts = quaternion, pivot, shift, attempts
        self.n_atoms = int(n_atoms)

    def __len__(self) -> int:
        return int(self.quaternion.shape[0])

    @classmethod
    def identity(cls, B: int, n_atoms: int, device) -> "RigidMotions":
        q = torch.zeros((int(B), 4), dtype=torch.float64, device=device)
        q[:, 0] = 1.0
        zero = torch.zeros((int(B), 3), dtype=torch.float64, device=device)
        return cls(q, zero, zero.clone(), torch.full((int(B), 2), -1, dtype=torch.int32, device=device), n_atoms)

    def apply(self, rows: torch.Tensor, inverse: bool = False) -> torch.Tensor:
        """rows f32 [..., B*N, 3] -> the moved rows as a new tensor (mdnoaug_apply); inverse=True undoes `apply` up to
        the two fp32 roundings.  Works on a window [W, B*N, 3], on targets [B*N, 3] and on the `[S, M*N, 3]` view of
        an engine's frames alike."""
        return ops.rigid_apply(self.quaternion, self.pivot, self.shift, self.n_atoms, rows, inverse=inverse)

    def matrices(self) -> torch.Tensor:
        """fp64 [B,3,3], the rule's nine entries written in torch (for users; the kernels form them themselves)."""
        w, x, y, z = self.quaternion.unbind(1)
        g = 2.0 / (((w * w + x * x) + y * y) + z * z)
        rows = [1.0 - g * (y * y + z * z), g * (x * y - w * z), g * (x * z + w * y),
                g * (x * y + w * z), 1.0 - g * (x * x + z * z), g * (y * z - w * x),
                g * (x * z - w * y), g * (y * z + w * x), 1.0 - g * (x * x + y * y)]
        return torch.stack(rows, dim=1).view(-1, 3, 3)


def _augmentable(batch, what: str):
    """(sample_ids, rows per sample) of a batch a motion can be drawn for."""
    ids = getattr(batch, "sample_ids", None) if isinstance(batch, PairData) else None
    if ids is None:
        raise MdnoError(f"{what} needs batches from DeviceTrajectory.batch (they carry their samples' dataset "
                        "indices); host-collated samples have none")
    if getattr(batch, "box", None) is not None:
        raise MdnoError(f"{what} under a periodic box is not supported: an orthorhombic cell is not rotation-invariant")
    return ids, int(batch.rows_per_sample)


def draw_motions(batch: PairData, augment: RigidAugment, epoch: int = 0) -> RigidMotions:
    """The motions `augment` gives the samples of a `DeviceTrajectory.batch` at `epoch` (one launch: mdnoaug_motions)."""
    if not isinstance(augment, RigidAugment):
        raise MdnoError(f"augment must be a RigidAugment (got {type(augment).__name__})")
    ids, n = _augmentable(batch, "rigid augmentation")
    x = batch.x_position
    frame = x[0] if augment.pivot == "centroid" else None
    # the indices go up through pinned memory without blocking the host (a pageable source is copied synchronously:
    # measured, that stall cost a training step more than the five launches)
    ids = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids, dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() > INT_MAX):
        raise MdnoError("sample_ids must lie in [0, 2^31)")
    if x.is_cuda:
        ids = torch.from_numpy(ids.astype(np.int32)).pin_memory().to(x.device, non_blocking=True)
    q, c, t, att = ops.rigid_motions(augment.seed, ids, epoch, augment.rotate, augment.translate, first_frame=frame,
                                     n_atoms=n, device=x.device)
    return RigidMotions(q, c, t, att, n)


def move_batch(batch: PairData, motions: RigidMotions) -> PairData:
    """A new collated batch, every sample moved by its motion: all window frames, `y` and every step of `y_unroll` by
    `motions.apply`, `edge_attr` gathered again from the moved first window frame at `edge_index` (what collating the
    moved samples gives); `edge_index` and `x_aminoacid` are the caller's tensors.  The caller's batch is untouched.
    A batch put together by hand whose edge attributes hold the rows of another window frame (`construct_pairdata`
    takes the newest) says so with `batch.edge_frame` (-1 there); a batch without targets has `y` None."""
    _augmentable(batch, "rigid augmentation")
    xp = motions.apply(batch.x_position)
    edge_frame = int(getattr(batch, "edge_frame", 0))
    out = PairData(batch.x_aminoacid, xp, None if batch.y is None else motions.apply(batch.y),
                   ops.edge_attr_gather(xp[edge_frame], batch.edge_index), batch.edge_index)
    if edge_frame:
        out.edge_frame = edge_frame
    out.num_graphs = getattr(batch, "num_graphs", len(motions))
    out.sample_ids, out.rows_per_sample = batch.sample_ids, batch.rows_per_sample
    yu = getattr(batch, "y_unroll", None)
    if out.y is None:
        out.y_unroll = None
    elif yu is None or yu.shape[0] == 1:
        out.y_unroll = out.y.unsqueeze(0)
    else:
        out.y_unroll = motions.apply(yu)
    out.motions = motions
    return out


def augment_batch(batch: PairData, augment: RigidAugment, epoch: int = 0) -> PairData:
    """`move_batch(batch, draw_motions(batch, augment, epoch))`: the batch `collate` would build from the moved samples.
    It carries `.motions` (a `RigidMotions`: `motions.apply(out, inverse=True)` takes a prediction back)."""
    return move_batch(batch, draw_motions(batch, augment, epoch))


class EquivarianceError:
    """`rms` f64 [B]: per sample, the root mean square over atoms of |f(g x) - g f(x)| in Angstrom; `step_rms` f64 [B]: the
    same for |f(x) - x_last|, the size of the step the model takes, which sets the scale."""

    def __init__(self, rms: torch.Tensor, step_rms: torch.Tensor):
        self.rms, self.step_rms = rms, step_rms

    def relative(self) -> torch.Tensor:
        return self.rms / self.step_rms


def _rms_over_atoms(u: torch.Tensor, v: torch.Tensor, B: int) -> torch.Tensor:
    d = (u.double() - v.double()).view(B, -1, 3)          # (the difference is already an fp64 one)
    return (d * d).sum(dim=(1, 2)).div(d.shape[1]).sqrt()


def equivariance_error(model, batch: PairData, motions_or_augment, epoch: int = 0) -> EquivarianceError:
    """How far `model` is from commuting with rigid motions on this batch: the inference forward (`model.eval()`, no
    autograd) on the batch and on the moved batch, compared after moving the first prediction — f(g x) against g f(x).
    `motions_or_augment`: a `RigidMotions` (`RigidMotions.identity` gives exactly 0) or a `RigidAugment`, drawn at
    `epoch`.  A composition of the augmentation launches and two forwards; the reduction is fp64 torch."""
    motions = motions_or_augment if isinstance(motions_or_augment, RigidMotions) else draw_motions(batch, motions_or_augment, epoch)
    B = len(motions)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            out = model(batch)
            moved = model(move_batch(batch, motions))
            err = _rms_over_atoms(moved, motions.apply(out), B)
            step = _rms_over_atoms(out, batch.x_position[-1], B)
    finally:
        model.train(was_training)
    return EquivarianceError(err, step)


# Longest window the prologue backward keeps per atom (csrc/train_nodes.hip MAX_W), largest embedding it handles
MAX_TRAIN_WINDOW = 16
MAX_EMBEDDING_DIM = 16


# `model.train_conv_mode`: how the kernel-integral block runs in training.  "materialized" (default): W_e and dW_e
# [E, 4096] are formed (KernelIntegralBlock).  "factored": FactoredKernelIntegralBlock — for dense graphs, where 16 KiB
# per edge does not fit.  "auto": the library's rule on the batch's counted edge list (mdno_conv_mode_for_graph: mean
# degree >= 40 and >= 16,384 edges per member -> factored), materialized where the factored form does not apply.
# The rule is the inference one: a crossover of its own for training has not been measured yet.
TRAIN_CONV_MODES = ("materialized", "factored", "auto")


def factored_training_applies(model) -> bool:
    """Width 64, ker_width a multiple of 128 (csrc/moment.hip moment_supported), fp32 storage, mean aggregation."""
    k = model.conv1.net.hip_weights()[2].shape[0]
    convs = [model.conv1] + ([model.conv2] if getattr(model, "conv2", None) is not None else [])
    return (model.fc1.out_features == 64 and k >= 128 and k % 128 == 0 and
            getattr(model, "train_precision", "fp32") == "fp32" and all(getattr(c, "aggr", "mean") == "mean" for c in convs))


def resolve_train_conv_mode(model, members: int, n_atoms: int, n_edges: int) -> str:
    """The formulation a training step on this batch takes: "materialized" or "factored"."""
    mode = getattr(model, "train_conv_mode", "materialized")
    if mode == "materialized" or not factored_training_applies(model):
        return "materialized"
    if mode == "factored":
        return "factored"
    from . import _lib
    pack = model.param_pack(next(model.parameters()).device, conv_mode="materialized")
    rule = int(_lib.load().mdno_conv_mode_for_graph(pack.ref, int(members), int(n_atoms), int(n_edges)))
    return "factored" if rule == _lib.CONV_MODES["factored"] else "materialized"


def check_trainable(model, window: int, input_grad: bool = False) -> None:
    """Refuse, before any device work, a model or window the training kernels do not implement: the conv chain and
    its backward are 64x64 only (csrc/train_conv.hip), the prologue backward keeps at most 16 frames and 16 embedding
    channels per atom (csrc/train_nodes.hip), the edge-MLP's first layer reads at most 8 attributes
    (csrc/edge_mlp.hip), and bf16 training tiles k by 128.  `input_grad`: the step also wants gradients with respect to
    its inputs (an input that requires grad, an unrolled step that is not detached) — fp32 storage only."""
    conv2 = getattr(model, "conv2", None)
    if conv2 is not None and model.conv1.net is not conv2.net:
        raise NotImplementedError("training assumes the reference's single shared edge-MLP (graph_kernel.py:271-273)")
    if conv2 is None and model.depth % 2:
        raise NotImplementedError("notebook-era variant: training needs an even depth")
    width = model.fc1.out_features
    if width != 64:
        raise NotImplementedError(f"training needs width 64 (got {width}): the conv chain and its backward are 64x64 only")
    if not 1 <= window <= MAX_TRAIN_WINDOW:
        raise NotImplementedError(f"training window {window}: the prologue backward takes 1..{MAX_TRAIN_WINDOW} frames")
    emb = model.emb.embedding_dim
    if emb > MAX_EMBEDDING_DIM:
        raise NotImplementedError(f"embedding_dim={emb}: training takes 0..{MAX_EMBEDDING_DIM}")
    if model.fc1.in_features != emb + 3:
        raise MdnoError(f"in_width={model.fc1.in_features} must equal embedding_dim + 3 = {emb + 3} (graph_kernel.py:296)")
    w0, _, w1, _, _, _ = model.conv1.net.hip_weights()
    if w0.shape[1] > 8:
        raise NotImplementedError(f"ker_in={w0.shape[1]}: the edge-MLP reads 1..8 edge attributes")
    precision = getattr(model, "train_precision", "fp32")
    if precision not in ("fp32", "bf16"):
        raise MdnoError(f"train_precision={precision!r} (fp32, bf16)")
    if precision == "bf16" and (w1.shape[0] % 128 or w1.shape[1] % 32):
        raise NotImplementedError("bf16 training needs width 64 and ker_width a multiple of 128")
    if precision == "bf16" and input_grad:
        raise NotImplementedError('train_precision="bf16" has no gradients with respect to the inputs (x_position, '
                                  'edge_attr) and no unrolled step that feeds them back: bf16 storage for the input '
                                  'gradients is out of scope (use train_precision="fp32", or unroll with detach=True)')
    mode = getattr(model, "train_conv_mode", "materialized")
    if mode not in TRAIN_CONV_MODES:
        raise MdnoError(f"train_conv_mode={mode!r} {TRAIN_CONV_MODES}")
    if mode == "factored":
        if precision == "bf16":
            raise NotImplementedError('train_conv_mode="factored" keeps fp32 storage: bf16 storage for the factored '
                                      'training path is out of scope (use train_precision="fp32")')
        if not factored_training_applies(model):
            raise NotImplementedError(f'train_conv_mode="factored" needs width 64, ker_width a multiple of 128 (got '
                                      f'{w1.shape[0]}) and mean aggregation')


def _wants_grad(t) -> bool:
    return torch.is_tensor(t) and t.requires_grad and torch.is_grad_enabled()


def train_forward(model, data) -> torch.Tensor:
    """Differentiable forward of `KernelNN` for one sample, a list of samples, or an already collated batch
    (`collate`, `DeviceTrajectory.batch`) -> [B*N, out].  Nothing here waits for the device: index errors
    (amino-acid id or node id out of range — IndexError in the reference) are left in `model`'s training
    status word and raised by `check_train_status(model)`, which `train_epoch` calls once per epoch.
    `requires_grad` on `data.x_position` / `data.edge_attr` is honoured (fp32 training): their `.grad` is
    d out / d input through the LSTM prologue and through the edge-MLP (edge_attr in the caller's edge order);
    without it the backward launches and allocates exactly what it always has."""
    batch = collate(data) if not isinstance(data, PairData) else data
    check_trainable(model, batch.x_position.shape[0] if batch.x_position.dim() == 3 else 1,
                    input_grad=_wants_grad(batch.x_position) or _wants_grad(batch.edge_attr))
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise MdnoError("training needs the model on the GPU (model.to('cuda')); no CPU fallback")
    xp = batch.x_position.to(dev, torch.float32)
    if xp.dim() == 2:
        xp = xp.unsqueeze(0)
    B = max(int(getattr(batch, "num_graphs", 1) or 1), 1)
    return _forward_step(model, xp, batch.x_aminoacid.to(dev), B, edge_index=batch.edge_index,
                         edge_attr=batch.edge_attr)[0]


def _forward_step(model, xp, aa, B: int, edge_index=None, edge_attr=None, graph=None):
    """One differentiable forward on windows xp [W, R, 3] (on the model's device) -> (out [R, out_width], graph).  The
    edges: `edge_index` [2, E] with `edge_attr` in its order (sorted here), or an already sorted `graph` (a CSRGraph
    without `perm`) with `edge_attr` in ITS order — a fed-back step of `unrolled_forward`."""
    dev = xp.device
    W, R, _ = xp.shape
    # per-atom prologue (graph_kernel.py:279-298 with B=1 semantics per sample): HIP forward + backward.
    # The ParamPack holds device pointers to the parameters' CURRENT storage (fp32 contiguous parameters
    # are viewed, not copied), the tensors themselves are passed so that autograd routes their gradients.
    sd = dict(model.named_parameters())
    names = tuple(k for k in _PROLOGUE_KEYS if k in sd)
    pack = model.param_pack(dev, conv_mode="materialized")
    pack.prologue_names = names
    status = getattr(model, "_train_status", None)
    if status is None or status.device != dev:
        status = model._train_status = torch.zeros(1, dtype=torch.int32, device=dev)
    pack.train_status = status
    conv2 = getattr(model, "conv2", None)
    depth = model.depth if conv2 is not None else model.depth // 2
    # the feature stack of the kernel-integral block [2*depth+1, R, 64]: the prologue writes layer 0 in place and the
    # block returns its last layer as a view — no copy on either side
    X = torch.empty((2 * depth + 1, R, 64), dtype=torch.float32, device=dev)
    pack.prologue_out = X[0]
    x0 = NodePrologue.apply(pack, xp.unsqueeze(1).contiguous(), aa, *[sd[k] for k in names])
    pack.prologue_out = None
    if depth == 0:
        # no conv application (graph_kernel.py:299-302 loop zero times): fc2 reads x0, and the edge-MLP, root and
        # bias parameters take no part in the loss — their .grad stays None, as under torch autograd; the edge list
        # is not read, as in the reference
        return FcOut.apply(x0, model.fc2.weight, model.fc2.bias), graph
    if graph is None:
        graph = ops.coo_to_csr(edge_index.to(dev), R, validate=False, status=status)
    # the same edges grouped by source, for the input-gradient kernel: built now, next to the forward's sort
    # (ids already validated by it), so that the backward starts with everything in place
    graph.by_src = ops.source_sorted(graph, R, status=status) if torch.is_grad_enabled() else None
    graph.x_stack = X
    net = model.conv1.net
    w0, b0, w1, b1, w2, b2 = net.hip_weights()
    c2 = conv2 if conv2 is not None else model.conv1
    precision = getattr(model, "train_precision", "fp32")
    if resolve_train_conv_mode(model, B, max(R // B, 1), graph.edge_count()) == "factored":
        block = FactoredKernelIntegralBlock
    else:
        block = KernelIntegralBlock
    x = block.apply(x0, edge_attr.to(dev), graph, depth,
                    "bf16" if precision == "bf16" else getattr(model, "gemm_mode", "f32"),
                    w0, b0, w1, b1, w2, b2,
                    model.conv1.root, model.conv1.bias, c2.root, c2.bias)
    return FcOut.apply(x, model.fc2.weight, model.fc2.bias), graph


def _unroll_box(model, batch, cutoff: float, box):
    """The box an unrolled step on `batch` runs in — `box`, by default the one the batch was collated in
    (`DeviceTrajectory(box=)` batches carry it) — as ops.check_box returns it, or None for the open step.  Host checks
    only: a box or cutoff other than the batch's own, or a model that does not read six edge attributes
    (rollout.check_rollout_box's rule), raises MdnoError."""
    own = getattr(batch, "box", None)
    if box is None and own is None:
        return None
    from .rollout import check_rollout_box
    box = check_rollout_box(model, own if box is None else box, cutoff)
    if own is not None:
        if float(cutoff) != float(batch.cutoff):
            raise MdnoError(f"unrolled_forward: cutoff={cutoff}, but the batch was collated with cutoff={batch.cutoff} "
                            f"(its first step's edges were built with it)")
        if box != ops.check_box(own, batch.cutoff):
            raise MdnoError(f"unrolled_forward: box={box}, but the batch was collated in box={tuple(own)}")
    return box


def unrolled_forward(model, batch, steps: int, cutoff: float = 8.0, detach: bool = False, box=None):
    """`steps` model steps from a training window, each prediction fed back as `recursive_propagation` does
    (graph_kernel.py: the window slides by one frame, the new frame's radius graph and edge attributes replace the
    stored ones) -> (outs, graphs): `outs[k]` [B*N, 3] is the prediction of frame t + 1 + k, `graphs[k]` the CSRGraph
    step k ran on.  Gradients flow back through the fed-back frames — through the slid window (the LSTM prologue) and
    through the edge attributes `EdgeAttrFromPositions` forms from the predicted frame; the radius graph itself is
    data, built per sample on the detached frame, and no gradient goes through its topology.  `detach=True` cuts the
    gradient at every fed-back frame (the pushforward variant): none of the input-gradient kernels then runs.
    Step 1 is `train_forward(model, batch)` on the dataset's stored edge list and attributes; `train_conv_mode` is
    resolved per step on that step's edge count.  Every fed-back step reads its edge count back from the device
    (one device-to-host word: its buffers are sized by it) — the one place the training path waits for the device.
    The model predicts frames at horizon 1; `batch` is one sample, a list, or a collated batch of B samples.
    `box` (default: the box a `DeviceTrajectory(box=)` batch carries): a periodic cell.  Every fed-back step then runs
    on the minimum-image radius graph of its frame (`ops.radius_graph_pbc`, topology only) with the imaged attributes
    `EdgeAttrFromPositions.apply(frame, graph, box, cutoff)`; the shift of an edge is data, like the edge itself, so
    the backward launches what the open one does.  A box or cutoff other than the batch's own raises.  Without a box the
    function launches exactly what it always has."""
    steps = int(steps)
    if steps < 1:
        raise MdnoError(f"unrolled_forward: steps={steps} (>= 1)")
    batch = collate(batch) if not isinstance(batch, PairData) else batch
    box = _unroll_box(model, batch, cutoff, box)
    W = batch.x_position.shape[0] if batch.x_position.dim() == 3 else 1
    feeds_grad = steps > 1 and not detach and torch.is_grad_enabled()
    check_trainable(model, W, input_grad=feeds_grad or _wants_grad(batch.x_position) or _wants_grad(batch.edge_attr))
    if steps > 1 and model.fc2.out_features != 3:
        raise MdnoError(f"unrolled_forward: the model predicts {model.fc2.out_features} values per atom, a frame has 3")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise MdnoError("training needs the model on the GPU (model.to('cuda')); no CPU fallback")
    xp = batch.x_position.to(dev, torch.float32)
    if xp.dim() == 2:
        xp = xp.unsqueeze(0)
    aa = batch.x_aminoacid.to(dev)
    B = max(int(getattr(batch, "num_graphs", 1) or 1), 1)
    R = xp.shape[1]
    if R % B:
        raise MdnoError(f"unrolled_forward: {R} rows in {B} graphs")
    out, graph = _forward_step(model, xp, aa, B, edge_index=batch.edge_index, edge_attr=batch.edge_attr)
    outs, graphs = [out], [graph]
    for _ in range(1, steps):
        frame = out.detach() if detach else out
        xp = torch.cat([xp[1:], frame.unsqueeze(0)], dim=0)
        if box is None:
            rg = ops.radius_graph(frame.detach(), R // B, cutoff)
        else:
            rg, _ = ops.radius_graph_pbc(frame.detach(), R // B, cutoff, box, with_attr=False)
        E = rg.edge_count()                                # the device->host read of this step
        cap = max(E, 1)
        graph = ops.CSRGraph(rg.row_ptr, rg.src[:cap], rg.dst[:cap], rg.num_edges, cap, None, rg.status, n_edges=E)
        ea = EdgeAttrFromPositions.apply(frame, graph) if box is None else EdgeAttrFromPositions.apply(frame, graph, box, cutoff)
        out, graph = _forward_step(model, xp, aa, B, edge_attr=ea, graph=graph)
        outs.append(out)
        graphs.append(graph)
    return outs, graphs


def check_train_status(model) -> None:
    """Read (one device->host word) and clear the status the training forwards since the last call left
    behind; raises what the reference's nn.Embedding / index_select would have raised in that forward."""
    from ._lib import raise_on_status
    st = getattr(model, "_train_status", None)
    if st is None:
        return
    word = int(st.item())
    if word:                     # (cleared only when something was raised: no fill launch per epoch otherwise)
        st.zero_()
    raise_on_status(word, "training forward")


class Adam(torch.optim.Optimizer):
    """`torch.optim.Adam(params, lr, betas, eps, weight_decay)` — the optimiser of the reference's main()
    (graph_kernel.py:541-543) — with its step as ONE libmdno launch over all parameter tensors (`mdno_adam_step`: the same
    arithmetic in the same order; torch's fused form walks tensor lists through multi_tensor_apply).  A
    `torch.optim.Optimizer`: lr schedulers (StepLR, :544-546) drive `param_groups[i]["lr"]`, and `state_dict()` has
    torch.optim.Adam's layout (`step`, `exp_avg`, `exp_avg_sq` per parameter), so a checkpoint written with either
    (graph_kernel.py:633-639) loads into the other.  fp32 parameters on the GPU; no amsgrad / maximize."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError("Adam: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            by_step = {}      # parameters of one group normally share their step count: one launch per distinct count
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.zeros((), dtype=torch.float32)                     # (host tensor, as torch.optim.Adam keeps it)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                by_step.setdefault(int(st["step"]), []).append((p, g, st["exp_avg"], st["exp_avg_sq"]))
            b1, b2 = group["betas"]
            for t, items in by_step.items():
                ops.adam_step([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items],
                              group["lr"], b1, b2, group["eps"], group["weight_decay"], t)
        return loss


def train_epoch(model, batches, optimizer, loss_fn, batch_size: Optional[int] = None, noise_std: float = 0.0,
                noise_seed: int = 0, epoch: int = 0, unroll: int = 1, unroll_detach: bool = False, cutoff: float = 8.0,
                augment=None):
    """One pass over `batches` — an iterable of lists of PairData (as the reference's DataListLoader yields)
    or of collated batches (`DeviceTrajectory.batch`): returns (avg relative-L2 loss, avg MSE) like train()
    (graph_kernel.py:445-474).  The per-batch losses stay on the device until the pass is over (the
    reference's `l2.item()` per batch would stall the GPU once per step); they are then added on the host in
    double precision in batch order, which is what `avg_loss += l2.item()` does.
    noise_std > 0: every batch — collated by `DeviceTrajectory.batch` — trains on input windows perturbed by
    `add_window_noise(batch, noise_std, noise_seed, epoch)`; the caller's batches are left clean.  `validate_epoch`
    never adds noise.
    augment = a `RigidAugment`: every batch — collated by `DeviceTrajectory.batch`, not periodic — trains on
    `augment_batch(batch, augment, epoch)`, before any noise; the caller's batches are left as they are.  `validate_epoch`
    never augments.  None: the pass runs as it always has.
    unroll = K > 1: every batch — collated by `DeviceTrajectory.batch(indices, unroll=K)`, which adds the K true frames
    `y_unroll` — trains on `unrolled_forward(model, batch, K, cutoff, detach=unroll_detach)`: the loss is the mean over
    the K steps of `loss_fn(out_k, y_k)`, and the returned pair is that mean and the mean MSE of the K steps.  unroll = 1
    is the one-step path: the same launches, the same bits.
    Periodic batches (`DeviceTrajectory(box=)`) pass through as they are: a batch knows its box and cutoff, the noisy
    copy keeps them, and `cutoff` must be the batches' own when `unroll > 1`."""
    K = int(unroll)
    if K < 1:
        raise MdnoError(f"unroll={unroll} (>= 1)")
    if K > 1 and getattr(model, "train_precision", "fp32") == "bf16" and not unroll_detach:
        check_trainable(model, 1, input_grad=True)
    model.train()
    losses, mses = [], []
    one = None
    for batch in batches:
        if isinstance(batch, PairData):
            B = batch_size or getattr(batch, "num_graphs", 1)
        else:
            B = len(batch)
        optimizer.zero_grad()
        if augment is not None:
            batch = augment_batch(batch, augment, epoch)
        if float(noise_std) != 0.0:
            if not isinstance(batch, PairData):
                raise MdnoError("noise_std needs collated batches from DeviceTrajectory.batch")
            clean, batch = batch, PairData(batch.x_aminoacid, None, batch.y, batch.edge_attr, batch.edge_index)
            batch.num_graphs = getattr(clean, "num_graphs", 1)
            batch.x_position = add_window_noise(clean, noise_std, noise_seed, epoch)
            if K > 1:
                batch.y_unroll = getattr(clean, "y_unroll", None)
            if getattr(clean, "box", None) is not None:      # a periodic batch: the rebuilt one stays periodic
                batch.box, batch.cutoff = clean.box, clean.cutoff
                batch.y_unroll = getattr(clean, "y_unroll", None)
        if K > 1:
            l2, mse = _unrolled_loss(model, batch, B, K, loss_fn, cutoff, unroll_detach)
            if one is None or one.device != l2.device:
                one = torch.ones((), dtype=l2.dtype, device=l2.device)
            l2.backward(one)
            optimizer.step()
            losses.append(l2.detach())
            mses.append(mse)
            continue
        out = train_forward(model, batch)
        y = torch.cat([s.y for s in batch]).to(out.device) if not isinstance(batch, PairData) else batch.y.to(out.device)
        if hasattr(loss_fn, "rel_with_mse"):      # LpLoss: loss and the logged MSE from one pass (csrc/loss.hip)
            l2, mse = loss_fn.rel_with_mse(out.view(B, -1), y.view(B, -1))
        else:
            l2, mse = loss_fn(out.view(B, -1), y.view(B, -1)), F.mse_loss(out.detach(), y)
        if one is None or one.device != l2.device:
            one = torch.ones((), dtype=l2.dtype, device=l2.device)      # d loss / d loss, made once (not a fill per batch)
        l2.backward(one)
        optimizer.step()
        losses.append(l2.detach())
        mses.append(mse)
    check_train_status(model)
    n = len(losses)
    if n == 0:
        return 0.0, 0.0
    # ONE device->host copy once the pass is over (the values stacked on the device), added on the host in double
    # precision in batch order
    vals = torch.stack([v.reshape(()) for v in losses] + [v.detach().reshape(()) for v in mses]).double().cpu().tolist()
    tot, tot_mse = sum(vals[:n]), sum(vals[n:])
    return tot / n, tot_mse / n


def _unrolled_loss(model, batch, B: int, K: int, loss_fn, cutoff: float, detach: bool):
    """(mean over the K steps of loss_fn(out_k, y_k), mean MSE of the K steps) for one collated batch."""
    if not isinstance(batch, PairData):
        raise MdnoError("unroll > 1 needs collated batches from DeviceTrajectory.batch(indices, unroll=K): "
                        "host-collated lists carry no targets beyond the first step")
    ys = getattr(batch, "y_unroll", None)
    if ys is None or ys.shape[0] < K:
        raise MdnoError(f"unroll={K} needs batches from DeviceTrajectory.batch(indices, unroll={K}) (y_unroll "
                        f"{'missing' if ys is None else 'has %d steps' % ys.shape[0]})")
    outs, _ = unrolled_forward(model, batch, K, cutoff=cutoff, detach=detach)
    total, total_mse = None, None
    for k, out in enumerate(outs):
        y = ys[k].to(out.device)
        if hasattr(loss_fn, "rel_with_mse"):
            l2, mse = loss_fn.rel_with_mse(out.view(B, -1), y.view(B, -1))
        else:
            l2, mse = loss_fn(out.view(B, -1), y.view(B, -1)), F.mse_loss(out.detach(), y)
        total = l2 if total is None else total + l2
        total_mse = mse.detach() if total_mse is None else total_mse + mse.detach()
    return total / K, total_mse / K


def validate_epoch(model, batches, loss_fn, batch_size: Optional[int] = None):
    """One validation pass — `validate()` of the reference (graph_kernel.py:476-493): `model.eval()`, no autograd,
    `out = model(batch)` on every batch (lists of PairData or collated batches), returns (avg relative-L2 loss,
    avg MSE).  The forward is the inference path (B block-diagonal members of one `mdno_kernelnn_fwd`; nothing is
    kept for a backward, so a pass needs less memory than a training step); losses stay on the device until the
    pass is over and index errors are raised once, like `train_epoch`."""
    was_training = model.training
    model.eval()
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise MdnoError("validation needs the model on the GPU (model.to('cuda')); no CPU fallback")
    status = getattr(model, "_train_status", None)
    if status is None or status.device != dev:
        status = model._train_status = torch.zeros(1, dtype=torch.int32, device=dev)
    losses, mses = [], []
    try:
        with torch.no_grad():
            for batch in batches:
                if isinstance(batch, PairData):
                    B = batch_size or getattr(batch, "num_graphs", 1)
                    y = batch.y.to(dev)
                else:
                    B = len(batch)
                    y = torch.cat([s.y for s in batch]).to(dev)
                out = model(batch, _status=status)
                if hasattr(loss_fn, "rel_with_mse"):
                    l2, mse = loss_fn.rel_with_mse(out.view(B, -1), y.view(B, -1))
                else:
                    l2, mse = loss_fn(out.view(B, -1), y.view(B, -1)), F.mse_loss(out, y)
                losses.append(l2)
                mses.append(mse)
        check_train_status(model)
    finally:
        model.train(was_training)
    n = len(losses)
    if n == 0:
        return 0.0, 0.0
    vals = torch.stack([v.detach().reshape(()) for v in losses] + [v.detach().reshape(()) for v in mses]).double().cpu().tolist()
    tot, tot_mse = sum(vals[:n]), sum(vals[n:])      # (one copy; batch-order sums in double, as train_epoch)
    return tot / n, tot_mse / n


class StructureLoss(LpLoss):
    """A `loss_fn` for `train_epoch`, `validate_epoch`, unrolled training and `DataParallelTrainer` as they are, that puts a
    structure term beside the Cartesian one:

        loss(out, y) = base(out, y) + sum over kinds of w_kind * mean((ic(out) - ic(y)) ** 2)

    out, y [B, N * 3]; ic = `forecast.internal_coordinates(..., featurizer, box)` in its default mode (distances, angle
    cosines, dihedral (cos, sin)); the kinds are the featurizer's distance, angle and dihedral columns, and each mean runs
    over that kind's columns and the B frames.  `weight` is one number for all three or a (distances, angles, dihedrals)
    triple; a kind whose weight is 0 (or that has no column) is not evaluated, so weight = 0 IS `base`.  The features and
    their gradient are one hand-written kernel each (include/mdno_internal.h, include/mdno_internal_grad.h); the difference,
    the square and the weighted sum that is the mean are torch operations — a handful of small framework kernels per step
    on this opt-in path, which scripts/train_aten_audit.py --structure-weight lists.  `rel_with_mse` returns this loss and the MSE the base logs.
    It is an `LpLoss` that carries its base's `d`, `p`, `reduction` and `size_average` (p = None over any other base), which
    is what `DataParallelTrainer` asks of a loss; a rank's structure term is the mean over ITS shard of the batch, so under
    several ranks it is the global term where the base averages (`size_average=True`: shards weighted by their share) and
    the sum of the shards' means where the base sums.  The absolute form (`abs`) has no structure term and is refused."""

    def __init__(self, base, featurizer, weight=1.0, box=None):
        from .forecast import Featurizer
        if not callable(base):
            raise MdnoError(f"StructureLoss: base is a {type(base).__name__}, expected a loss function")
        if not isinstance(featurizer, Featurizer):
            raise MdnoError(f"StructureLoss: featurizer is a {type(featurizer).__name__}")
        if featurizer.n_atoms is None:
            raise MdnoError("StructureLoss: the featurizer has no n_atoms (build it with n_atoms=N): out [B, N * 3] does not say "
                            "how many atoms a frame has")
        try:
            w = [float(weight)] * 3 if not hasattr(weight, "__len__") else [float(v) for v in weight]
        except (TypeError, ValueError):
            w = []
        if len(w) != 3 or not all(np.isfinite(v) and v >= 0.0 for v in w):
            raise MdnoError(f"StructureLoss: weight = {weight!r}, expected a finite number >= 0 or three of them "
                            "(distances, angles, dihedrals)")
        if isinstance(base, LpLoss):
            super().__init__(base.d, base.p, base.size_average, base.reduction)
        else:
            self.d, self.p, self.reduction, self.size_average = 2, None, False, False
        self.base, self.featurizer, self.weight = base, featurizer, tuple(w)
        self.box = ops.check_box(box, 0.0)
        self._on = {}                   # device -> the featurizer's indices there
        self._wcol = {}                 # (device, B) -> the weight of every column, w_kind / (B columns of the kind)

    def _featurizer_on(self, device):
        ft = self._on.get(device)
        if ft is None:
            ft = self._on[device] = self.featurizer if self.featurizer.pairs.device == device else self.featurizer.to(device)
        return ft

    def structure(self, out, y):
        """The structure term alone (a 0-dim tensor), or None where every weight is 0."""
        from .forecast import internal_coordinates
        ft = self._featurizer_on(out.device)
        N = ft.n_atoms
        P, A, T = ft.pairs.shape[0], ft.triples.shape[0], ft.quads.shape[0]
        kinds = [(w, lo, hi) for w, lo, hi in zip(self.weight, (0, P, P + A), (P, P + A, P + A + 2 * T)) if w != 0.0 and hi > lo]
        if not kinds:
            return None
        B = out.shape[0]
        if out.dim() != 2 or out.shape[1] != 3 * N or tuple(y.shape) != tuple(out.shape):
            raise MdnoError(f"StructureLoss: out {tuple(out.shape)}, y {tuple(y.shape)}: expected [B, {3 * N}] both")
        f_out = internal_coordinates(out.reshape(B, N, 3), ft, box=self.box)
        with torch.no_grad():
            f_y = internal_coordinates(y.to(out.device).reshape(B, N, 3), ft, box=self.box)
        # one weighted sum per run of adjacent weighted kinds (w_kind / (B columns) per column IS w_kind times the kind's
        # mean): four small kernels forward where a mean per kind takes a dozen; a kind of weight 0 lies in no run
        key = (out.device, B)
        wcol = self._wcol.get(key)
        if wcol is None:
            wcol = torch.zeros(P + A + 2 * T, dtype=torch.float32)
            for w, lo, hi in kinds:
                wcol[lo:hi] = w / (B * (hi - lo))
            wcol = self._wcol[key] = wcol.to(out.device)
        runs = []
        for _, lo, hi in kinds:
            if runs and runs[-1][1] == lo:
                runs[-1][1] = hi
            else:
                runs.append([lo, hi])
        total = None
        for lo, hi in runs:
            whole = lo == 0 and hi == wcol.shape[0]
            d = f_out - f_y if whole else f_out[:, lo:hi] - f_y[:, lo:hi]
            term = torch.sum(d * d * (wcol if whole else wcol[lo:hi]))
            total = term if total is None else total + term
        return total

    def rel(self, out, y):
        loss, extra = self.base(out, y), self.structure(out, y)
        return loss if extra is None else loss + extra

    def __call__(self, out, y):
        return self.rel(out, y)

    def abs(self, out, y):
        raise MdnoError("StructureLoss wraps its base's relative form (call it, or rel / rel_with_mse); abs has no structure term")

    def rel_with_mse(self, out, y):
        if hasattr(self.base, "rel_with_mse"):
            loss, mse = self.base.rel_with_mse(out, y)
        else:
            loss, mse = self.base(out, y), F.mse_loss(out.detach(), y)
        extra = self.structure(out, y)
        return (loss if extra is None else loss + extra), mse
