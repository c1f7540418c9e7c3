"""Data-parallel training: what the reference's `torch_geometric.nn.DataParallel` (graph_kernel.py:528) does to train()
(:445-474) — every global batch split across the GPUs, the shards' gradients reduce-added before `optimizer.step()`
(:467) — with one process per GPU (torch.distributed; nccl = RCCL, gloo only to rehearse with ranks sharing a card).

Per step every rank runs the HIP forward and backward (`training.train_forward`) on its contiguous shard of the global
batch (`shard_range`), packs all gradients into one flat fp32 bucket in one launch (include/mdno.h mdno_pack_tensors),
reduces it with ONE all-reduce(SUM), points every `p.grad` at its slot of the reduced bucket (no copy back) and steps
the optimiser.  The backward seeds make the ranks' gradient sum the gradient of the global batch loss: 1 for
`LpLoss(size_average=False)` (a sum over samples), B_r / B for `size_average=True` (a mean).  Every rank applies the
same update to the same parameters (`broadcast_parameters` once at the start), so the replicas stay identical without
further traffic.  Per-batch losses stay on the device; an epoch ends with one all-reduce of the stacked values and one
of the training status word, so a bad sample on any rank raises on every rank.
"""
from __future__ import annotations

import hashlib
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .dataset import PairData
from .graph_kernel import LpLoss
from .training import check_train_status, train_forward


def shard_range(B: int, rank: int, world: int) -> Tuple[int, int]:
    """Rank `rank`'s contiguous shard [start, stop) of a global batch of B samples: shard sizes differ by at most one
    (the first B mod world ranks take one more), ranks in order, so the shards laid end to end are the batch — the
    split DataParallel's scatter makes.  A rank may get zero samples."""
    if world < 1 or not (0 <= rank < world) or B < 0:
        raise ValueError(f"shard_range: B={B}, rank={rank}, world={world}")
    q, r = divmod(B, world)
    start = rank * q + min(rank, r)
    return start, start + q + (1 if rank < r else 0)


def _dist(group):
    """(world, rank, backend) of the caller's process group; (1, 0, None) without torch.distributed."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 1, 0, None
    return dist.get_world_size(group), dist.get_rank(group), dist.get_backend(group)


def _slots(params) -> Tuple[List[int], int]:
    """Slot offsets (elements) of the parameters in `model.parameters()` order, each slot padded to 16 B."""
    offsets, off = [], 0
    for p in params:
        offsets.append(off)
        off += (p.numel() + 3) // 4 * 4
    return offsets, off


def _check_params(params) -> torch.device:
    if not params:
        raise ValueError("data parallel: the model has no parameters")
    dev = params[0].device
    for p in params:
        if p.device.type != "cuda" or p.device != dev:
            raise ValueError("data parallel: every parameter must be on the rank's GPU (model.to('cuda'))")
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError("data parallel: parameters must be fp32 and contiguous")
    return dev


class _Collectives:
    """The few collectives of this module on the caller's group; with gloo a device tensor is staged through host
    memory, as rollout.gather_trajectories does."""

    def __init__(self, group):
        self.group = group
        self.world, self.rank, self.backend = _dist(group)
        self.active = self.backend is not None

    def _run(self, t: torch.Tensor, fn):
        if self.backend == "gloo" and t.is_cuda:
            h = t.cpu()
            fn(h)
            t.copy_(h)
        else:
            fn(t)

    def all_reduce(self, t: torch.Tensor, op: str = "sum"):
        import torch.distributed as dist
        rop = {"sum": dist.ReduceOp.SUM, "max": dist.ReduceOp.MAX}[op]
        self._run(t, lambda x: dist.all_reduce(x, op=rop, group=self.group))

    def broadcast(self, t: torch.Tensor, src: int):
        import torch.distributed as dist
        self._run(t, lambda x: dist.broadcast(x, src=src, group=self.group))


def broadcast_parameters(model, group=None, src: int = 0) -> None:
    """Give every rank rank `src`'s parameters: pack them into one flat buffer, one broadcast, unpack.  Call it once,
    before the optimiser is built."""
    coll = _Collectives(group)
    if not coll.active or coll.world == 1:
        return
    params = list(model.parameters())
    dev = _check_params(params)
    offsets, total = _slots(params)
    flat = torch.zeros(total, dtype=torch.float32, device=dev)
    with torch.no_grad():
        ops.pack_tensors([p.detach() for p in params], flat, offsets)
        coll.broadcast(flat, src)
        ops.unpack_tensors(flat, [p.detach() for p in params], offsets)


def _is_index_batch(batch) -> bool:
    return not (len(batch) and isinstance(batch[0], PairData))


def batch_digest(batches) -> int:
    """A 62-bit digest of the structure of an epoch's batch list: the sample count of every batch and, for batches of
    sample indices, the indices.  Ranks that hold different lists would train different models."""
    h = hashlib.blake2b(digest_size=8)
    h.update(np.int64(len(batches)).tobytes())
    for b in batches:
        if _is_index_batch(b):
            idx = np.asarray(b, dtype=np.int64).reshape(-1)
            h.update(b"i" + np.int64(idx.size).tobytes() + idx.tobytes())
        else:
            h.update(b"s" + np.int64(len(b)).tobytes())
    return int.from_bytes(h.digest(), "little") & ((1 << 62) - 1)


def check_batch_lists(batches, group=None) -> None:
    """Raise ValueError on every rank unless all ranks of the group hold the same batch list (`batch_digest`): one
    all-reduce(MAX) of [digest, -digest] gives the group's largest and smallest digest at once."""
    coll = _Collectives(group)
    if not coll.active:
        return
    d = batch_digest(batches)
    dev = torch.device("cpu") if coll.backend == "gloo" else torch.device("cuda", torch.cuda.current_device())
    t = torch.tensor([d, -d], dtype=torch.int64, device=dev)
    coll.all_reduce(t, "max")
    hi, lo = int(t[0]), -int(t[1])
    if hi != d or lo != d:
        raise ValueError(f"rank {coll.rank}: the ranks hold different batch lists (digest {d:#x}, the group's range "
                         f"[{lo:#x}, {hi:#x}]); every rank must be given the same global batches")


def combine_losses(sums, sizes: Sequence[int], size_average: bool) -> Tuple[float, float]:
    """(avg loss, avg MSE) of an epoch from the ranks' reduced per-batch values: sums[k] = the sum over ranks of
    [loss_r * B_r (size_average) or loss_r (sum), mse_r * B_r] for batch k of B = sizes[k] samples, in float64.  Batch
    k's loss is sums[k][0] / B or sums[k][0], its MSE sums[k][1] / B; both are added on the host in batch order and
    divided by the batch count — train_epoch's arithmetic, bit for bit at one rank."""
    n = len(sizes)
    if n == 0:
        return 0.0, 0.0
    losses = [(float(s[0]) / B if size_average else float(s[0])) for s, B in zip(sums, sizes)]
    mses = [float(s[1]) / B for s, B in zip(sums, sizes)]
    return sum(losses) / n, sum(mses) / n


class DataParallelTrainer:
    """train()'s epoch (graph_kernel.py:445-474) under DataParallel (:528): `train_epoch(batches)` shards every global
    batch across the group's ranks and reduces the gradients with one all-reduce per step; `validate_epoch(batches)`
    shards validate() (:476-493) the same way.  At world size 1, or without torch.distributed, the results are bitwise
    those of `training.train_epoch` / `validate_epoch`.

    model: on the rank's GPU, fp32 contiguous parameters, identical on every rank (`broadcast_parameters`).
    optimizer: any optimiser that reads `p.grad` (`training.Adam`, `torch.optim.Adam`).
    loss_fn: `LpLoss` with p = 2 and a reduction (either `size_average`).
    Every parameter receives its slot of the reduced bucket as gradient, also one no rank computed a gradient for
    (a zero gradient then)."""

    def __init__(self, model, optimizer, loss_fn, group=None):
        if not isinstance(loss_fn, LpLoss) or loss_fn.p != 2 or not loss_fn.reduction:
            raise NotImplementedError("DataParallelTrainer: LpLoss with p = 2 and a reduction only")
        self.model, self.optimizer, self.loss_fn = model, optimizer, loss_fn
        self.params = list(model.parameters())
        self.device = _check_params(self.params)
        self.coll = _Collectives(group)
        self.world, self.rank = self.coll.world, self.coll.rank
        self.offsets, total = _slots(self.params)
        self.bucket = torch.zeros(total, dtype=torch.float32, device=self.device)        # allocated once
        self.grad_views = [self.bucket[o:o + p.numel()].view_as(p) for p, o in zip(self.params, self.offsets)]
        st = getattr(model, "_train_status", None)
        if st is None or st.device != self.device:       # a rank without samples still joins the status reduction
            model._train_status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._seeds = {}
        self._zero2 = torch.zeros(2, dtype=torch.float32, device=self.device)
        # per-step device events (forward+backward, pack, all-reduce, optimiser) when `timing` is set
        self.timing = False
        self._events = []

    @property
    def bucket_bytes(self) -> int:
        return self.bucket.numel() * 4

    # ------------------------------------------------------------------------------------------ epoch structure
    def _check_batches(self, batches, source) -> None:
        for b in batches:
            if _is_index_batch(b) and len(b) and source is None:
                raise ValueError("batches of sample indices need `source` (a DeviceTrajectory)")
            if not _is_index_batch(b) and source is not None:
                raise ValueError("`source` is given, but a batch holds PairData samples")
        check_batch_lists(batches, self.coll.group)

    def _shard(self, batch, source, noise=None):
        B = len(batch)
        s, e = shard_range(B, self.rank, self.world)
        if e == s:
            return B, 0, None, None
        if source is not None:
            data = source.batch(np.asarray(batch, dtype=np.int64).reshape(-1)[s:e], **(noise or {}))
            return B, e - s, data, data.y
        part = list(batch[s:e])
        return B, e - s, part, torch.cat([x.y for x in part])

    def _seed(self, value: float) -> torch.Tensor:
        t = self._seeds.get(value)
        if t is None:                                    # made once per distinct value (not a fill per batch)
            t = self._seeds[value] = torch.full((), value, dtype=torch.float32, device=self.device)
        return t

    def _event(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    # ------------------------------------------------------------------------------------------ one step
    def _reduce_gradients(self):
        """Pack every parameter's gradient into the bucket (a parameter without one sends zeros), all-reduce(SUM) the
        bucket and make each `p.grad` a view of its slot.  Returns the event recorded after the pack (timing), or None."""
        grads = [p.numel() if p.grad is None else p.grad.contiguous() for p in self.params]
        ops.pack_tensors(grads, self.bucket, self.offsets)
        ev = self._event() if self.timing else None
        if self.coll.active:
            self.coll.all_reduce(self.bucket, "sum")
        for p, v in zip(self.params, self.grad_views):
            p.grad = v
        return ev

    def _finish(self, per, weights, sizes, size_average: bool) -> Tuple[float, float]:
        model = self.model
        if per:
            vals = torch.stack(per).double() * torch.tensor(weights, dtype=torch.float64).to(self.device)
            if self.coll.active:
                self.coll.all_reduce(vals, "sum")
        if self.coll.active:
            self.coll.all_reduce(model._train_status, "max")
        check_train_status(model)
        return combine_losses(vals.cpu().tolist() if per else [], sizes, size_average)

    def train_epoch(self, batches, source=None, noise_std: float = 0.0, noise_seed: int = 0, epoch: int = 0,
                    augment=None) -> Tuple[float, float]:
        """One training pass over the global batch list (lists of PairData, or lists of sample indices into `source`,
        a DeviceTrajectory) -> (avg relative-L2 loss, avg MSE), the same numbers on every rank.
        noise_std > 0 (index batches only): `source.batch(..., noise_std, noise_seed, epoch)` — keyed by dataset index,
        so a sample's noise is the same on whichever rank its shard falls.
        augment = a `training.RigidAugment` (index batches only): `source.batch(..., augment=augment, epoch=epoch)` — the
        motion is keyed by dataset index too, so a sample moves the same way on whichever rank it lands."""
        batches = list(batches)
        self._check_batches(batches, source)
        noise = None
        if float(noise_std) != 0.0:
            if source is None:
                raise ValueError("noise_std needs batches of sample indices and `source` (a DeviceTrajectory)")
            noise = dict(noise_std=float(noise_std), noise_seed=int(noise_seed), epoch=int(epoch))
        if augment is not None:
            if source is None:
                raise ValueError("augment needs batches of sample indices and `source` (a DeviceTrajectory)")
            noise = dict(noise or {}, augment=augment, epoch=int(epoch))
        model, opt = self.model, self.optimizer
        sa = bool(self.loss_fn.size_average)
        model.train()
        per, weights, sizes = [], [], []
        for batch in batches:
            B, Br, data, y = self._shard(batch, source, noise)
            opt.zero_grad(set_to_none=True)
            e0 = self._event() if self.timing else None
            if Br:
                out = train_forward(model, data)
                l2, mse = self.loss_fn.rel_with_mse(out.view(Br, -1), y.to(out.device).view(Br, -1))
                l2.backward(self._seed(Br / B if sa else 1.0))
                per.append(torch.stack([l2.detach().reshape(()), mse.detach().reshape(())]))
            else:
                per.append(self._zero2)
            weights.append((float(Br) if sa else 1.0, float(Br)))
            sizes.append(B)
            e1 = self._event() if self.timing else None
            e2 = self._reduce_gradients()
            e3 = self._event() if self.timing else None
            opt.step()
            if self.timing:
                self._events.append((e0, e1, e2, e3, self._event()))
        return self._finish(per, weights, sizes, sa)

    def validate_epoch(self, batches, source=None) -> Tuple[float, float]:
        """validate() (graph_kernel.py:476-493) with the same sharding: eval mode, no autograd, the inference forward
        `model(batch)` on every rank's shard; one reduction of the per-batch values when the pass is over."""
        batches = list(batches)
        self._check_batches(batches, source)
        model = self.model
        was_training = model.training
        model.eval()
        status = model._train_status
        per, weights, sizes = [], [], []
        try:
            with torch.no_grad():
                for batch in batches:
                    B, Br, data, y = self._shard(batch, source)
                    if Br:
                        out = model(data, _status=status)
                        l2, mse = self.loss_fn.rel_with_mse(out.view(Br, -1), y.to(out.device).view(Br, -1))
                        per.append(torch.stack([l2.reshape(()), mse.reshape(())]))
                    else:
                        per.append(self._zero2)
                    weights.append((float(Br) if self.loss_fn.size_average else 1.0, float(Br)))
                    sizes.append(B)
            return self._finish(per, weights, sizes, bool(self.loss_fn.size_average))
        finally:
            model.train(was_training)

    # ------------------------------------------------------------------------------------------ timing
    def step_times_ms(self, reset: bool = True) -> dict:
        """Mean device time per step of each phase since the last reset (needs `timing = True` during the epochs):
        forward+backward, pack, all-reduce (with gloo: including the host staging), optimiser step."""
        if not self._events:
            return {}
        self._events[-1][-1].synchronize()
        keys = ("forward_backward", "pack", "all_reduce", "optimizer")
        out = {k: float(np.mean([ev[i].elapsed_time(ev[i + 1]) for ev in self._events])) for i, k in enumerate(keys)}
        out["steps"] = len(self._events)
        if reset:
            self._events = []
        return out
