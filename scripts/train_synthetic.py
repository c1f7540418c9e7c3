"""BASELINE.json configs[3]: graph-kernel operator training on a synthetic preprocessed-BBA-layout
trajectory (N=28 C-alpha chain, Ornstein-Uhlenbeck jitter, contact maps at 8 A), 1 GPU.

  python scripts/train_synthetic.py [--frames 2000] [--batch-size 128] [--epochs 1] [--cpu-batches 1]
                                    [--augment-rotate] [--augment-translate A] [--augment-seed S]

Model, optimiser and loss as the reference's main() (graph_kernel.py:528-547): KernelNN(64, 1024, 6, 6, 7, 3,
20, 4), Adam(lr, weight_decay=5e-4), StepLR(50, 0.8), LpLoss(size_average=False), partition split 0.8,
drop_last.  Prints the reference's epoch line format and a JSON summary with samples/s; `--cpu-batches`
times the same step in plain torch autograd on the host (oracle formulas, fp32) as a baseline.
"""
import argparse
import copy
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from molecular_dynamics_neural_operator_amd import synthetic as syn  # noqa: E402
from molecular_dynamics_neural_operator_amd.dataset import ContactMapDataset, write_trajectory_npz  # noqa: E402
from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN, LpLoss  # noqa: E402
from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory, collate, train_epoch, validate_epoch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=2000)
ap.add_argument("--batch-size", type=int, default=128)
ap.add_argument("--epochs", type=int, default=1)
ap.add_argument("--kernel-width", type=int, default=1024)
ap.add_argument("--depth", type=int, default=6)
ap.add_argument("--lr", type=float, default=1e-4)
ap.add_argument("--cpu-batches", type=int, default=0)
ap.add_argument("--precision", choices=["fp32", "bf16"], default="bf16",
                help="bf16 (BASELINE configs[3]): h1, h2, W_e, dW_e stored in bf16, single-product bf16 GEMMs with "
                     "fp32 accumulation, fp32 master weights; fp32: split-bf16 GEMMs at fp32-level accuracy")
ap.add_argument("--train-conv-mode", choices=["materialized", "factored", "auto"], default="materialized",
                help="kernel-integral block in training: W_e formed, factored per destination (dense graphs; needs "
                     "--precision fp32), or by the counted-graph rule")
ap.add_argument("--torch-adam", action="store_true", help="torch.optim.Adam(fused=True) instead of training.Adam (mdno_adam_step)")
ap.add_argument("--host-collate", action="store_true",
                help="collate every batch on the host from ContactMapDataset samples (what the reference's "
                     "DataListLoader does) instead of on the device from the resident trajectory")
ap.add_argument("--noise-std", type=float, default=0.0,
                help="Gaussian noise on the input windows of every training batch (device-collated batches only)")
ap.add_argument("--noise-seed", type=int, default=0)
ap.add_argument("--unroll", type=int, default=1,
                help="train on K model steps per window, each prediction fed back (training.unrolled_forward; "
                     "device-collated batches, --precision fp32 unless --unroll-detach)")
ap.add_argument("--unroll-detach", action="store_true",
                help="cut the gradient at every fed-back frame (the pushforward variant)")
ap.add_argument("--structure-weight", type=float, default=0.0,
                help="W > 0: train and validate on LpLoss + W * (mean squared difference of the internal coordinates, per "
                     "kind: training.StructureLoss over Featurizer.backbone(N, K, S)); 0: the loss is not wrapped")
ap.add_argument("--structure-min-sep", type=int, default=3, help="K: the least sequence separation of a non-bonded pair")
ap.add_argument("--structure-stride", type=int, default=1, help="S: non-bonded pairs among every S-th atom")
ap.add_argument("--box", type=float, nargs=3, metavar=("LX", "LY", "LZ"), default=None,
                help="train on a synthetic PERIODIC trajectory in this orthorhombic cell (0 = an open axis; every periodic "
                     "axis >= 16 A): synthetic.periodic_box_frame scaled to the cell plus ou_trajectory, batches from "
                     "DeviceTrajectory(box=); composes with --unroll, --noise-std and --structure-weight")
ap.add_argument("--augment-rotate", action="store_true",
                help="train every sample under a random rotation about its first frame's centroid, drawn anew every epoch "
                     "(training.RigidAugment; device-collated batches, not under --box)")
ap.add_argument("--augment-translate", type=float, default=0.0, metavar="A",
                help="and / or under a random translation, uniform in [-A, A]^3 Angstrom")
ap.add_argument("--augment-seed", type=int, default=0)
ap.add_argument("--workdir", default="/tmp/mdno_train")
a = ap.parse_args()
dev = torch.device("cuda:0")
Path(a.workdir).mkdir(parents=True, exist_ok=True)

N, W = 28, 10
box = None
if a.box is not None:
    from molecular_dynamics_neural_operator_amd import ops  # noqa: E402
    box = ops.check_box(a.box, 8.0)
if box is not None:
    if a.host_collate or a.cpu_batches:
        ap.error("--box trains on device-collated periodic batches (drop --host-collate and --cpu-batches)")
    side = max(box)                                               # a cube of the longest axis, scaled to the cell; an open
    base, _ = syn.periodic_box_frame(N, N / side ** 3, seed=1)    # axis keeps that extent
    base = (base * np.array([L / side if L > 0 else 1.0 for L in box])).astype(np.float32)
else:
    base = syn.chain_frame(N, seed=0)
traj = syn.ou_trajectory(base, a.frames, sigma=0.3, theta=0.1, seed=2)
cms = [syn.contact_map(f, 8.0) for f in traj]
path = Path(a.workdir) / "synthetic_bba.npz"
write_trajectory_npz(path, traj, cms, syn.amino_acids(N, seed=0))
dset = ContactMapDataset(str(path), window_size=W, horizon=1)
n_train = int(len(dset) * 0.8)                                    # partition split (graph_kernel.py:509-520)
train_idx, valid_idx = list(range(n_train)), list(range(n_train, len(dset)))
if a.unroll > 1 and a.host_collate:
    ap.error("--unroll needs device-collated batches (drop --host-collate)")
augment = None
if a.augment_rotate or a.augment_translate != 0.0:
    from molecular_dynamics_neural_operator_amd.training import RigidAugment  # noqa: E402
    if a.host_collate or a.cpu_batches or box is not None:
        ap.error("--augment-rotate / --augment-translate move device-collated batches of an open system (drop --host-collate, "
                 "--cpu-batches and --box)")
    augment = RigidAugment(seed=a.augment_seed, rotate=a.augment_rotate, translate=a.augment_translate)
B = a.batch_size
traj_dev = None if a.host_collate else (DeviceTrajectory(dset, dev) if box is None else DeviceTrajectory(dset, dev, box=box))


class Batches:
    """drop_last batches over an index list; device mode builds each batch on the GPU when it is asked for
    (as a loader would), host mode hands out lists of samples for `collate`."""

    def __init__(self, idx):
        self.idx = [idx[s:s + B] for s in range(0, len(idx) - B + 1, B)]
        self.host = [[dset[i] for i in b] for b in self.idx] if traj_dev is None else None
        self.unroll = 1

    def __len__(self):
        return len(self.idx)

    def __getitem__(self, k):
        if isinstance(k, slice):
            out = Batches([])
            out.idx, out.host = self.idx[k], (self.host[k] if self.host is not None else None)
            out.unroll = self.unroll
            return out
        return self.host[k] if self.host is not None else traj_dev.batch(self.idx[k], unroll=self.unroll)

    def __iter__(self):
        return (self[k] for k in range(len(self)))


batches, vbatches = Batches(train_idx), Batches(valid_idx)
batches.unroll = a.unroll          # (the training indices end n_valid samples before the data does: every target exists)

torch.manual_seed(0)
model = KernelNN(64, a.kernel_width, a.depth, 6, 7, 3, 20, 4)
with torch.no_grad():     # the reference's init makes activations explode through 12 layers at k=1024 (outputs ~1e5);
    for p_ in model.conv1.net.layers[4].parameters():   # damp the kernel's last layer so Adam starts from O(1) values
        p_.mul_(0.05)
cpu_model = copy.deepcopy(model)
model.to(dev)
model.train_precision = a.precision
model.train_conv_mode = a.train_conv_mode
from molecular_dynamics_neural_operator_amd.training import Adam  # noqa: E402
if a.torch_adam:      # torch's own (its single-kernel form where the build has it): the same update rule (graph_kernel.py:541-543)
    try:
        opt = torch.optim.Adam(model.parameters(), lr=a.lr, weight_decay=5e-4, fused=True)
    except (RuntimeError, TypeError):
        opt = torch.optim.Adam(model.parameters(), lr=a.lr, weight_decay=5e-4)
else:                 # training.Adam: torch.optim.Adam's arithmetic and state as ONE libmdno launch over the 27 tensors
    opt = Adam(model.parameters(), lr=a.lr, weight_decay=5e-4)
sched = torch.optim.lr_scheduler.StepLR(opt, step_size=50, gamma=0.8)
loss_fn = LpLoss(size_average=False)
step_loss = loss_fn                # what the device path trains and validates on (the CPU baseline leg keeps the plain loss)
if a.structure_weight != 0.0:
    from molecular_dynamics_neural_operator_amd.forecast import Featurizer  # noqa: E402
    from molecular_dynamics_neural_operator_amd.training import StructureLoss  # noqa: E402
    if a.host_collate or a.cpu_batches:
        ap.error("--structure-weight runs on the device (drop --host-collate and --cpu-batches)")
    step_loss = StructureLoss(loss_fn, Featurizer.backbone(N, a.structure_min_sep, a.structure_stride), weight=a.structure_weight,
                              box=box)


def validate():
    """The reference's validate() (graph_kernel.py:476-493): eval mode, no autograd, model(batch) per batch."""
    return validate_epoch(model, vbatches, step_loss)[0]


summary = {"frames": a.frames, "batch_size": B, "train_batches": len(batches), "edges_per_batch":
           int(sum(dset[i].edge_index.shape[1] for i in batches.idx[0]) if box is None else traj_dev.counts[batches.idx[0]].sum()),
           "kernel_width": a.kernel_width,
           "depth": a.depth, "collate": "host" if a.host_collate else "device"}
summary["precision"] = a.precision
if box is not None:
    summary["box"] = list(box)
summary["unroll"], summary["unroll_detach"] = a.unroll, a.unroll_detach
if augment is not None:
    summary["augment"] = repr(augment)
if step_loss is not loss_fn:
    summary.update(structure_weight=a.structure_weight, structure_min_sep=a.structure_min_sep, structure_stride=a.structure_stride,
                   structure_features=step_loss.featurizer.dim())
train_epoch(model, batches[:1], opt, step_loss)        # warm-up (allocator, kernels)
torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats()
for ep in range(a.epochs):
    t0 = time.perf_counter()
    tl, mse = train_epoch(model, batches, opt, step_loss, noise_std=a.noise_std, noise_seed=a.noise_seed, epoch=ep,
                          unroll=a.unroll, unroll_detach=a.unroll_detach, augment=augment)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    vl = validate()
    sched.step()
    print(f"Epoch: {ep}\tTime: {dt}\ttrain_loss: {tl}\tvalid_loss: {vl}")
    summary.update(epoch_seconds=dt, samples_per_s=len(batches) * B / dt, train_loss=tl, valid_loss=vl, train_mse=mse,
                   peak_memory_MiB=torch.cuda.max_memory_allocated() / 2**20)

if a.cpu_batches:
    # same step in plain torch autograd on the host (oracle formulas, edge-MLP evaluated once per forward):
    # the CPU baseline leg, the only place this script touches oracle/
    from oracle import graph_kernel_oracle as O
    ref = cpu_model
    ref.train()
    sd = dict(ref.named_parameters())
    copt = torch.optim.Adam(ref.parameters(), lr=a.lr, weight_decay=5e-4)
    t0 = time.perf_counter()
    for bi in batches.idx[:a.cpu_batches]:
        cb = collate([dset[i] for i in bi])
        copt.zero_grad()
        xp = cb.x_position
        R = xp.shape[1]
        hidden = (torch.zeros(1, R, 3), torch.zeros(1, R, 3))
        out = None
        for t in range(W):
            out, hidden = ref.lstm(xp[t].unsqueeze(0), hidden)
        x = F.relu(ref.fc1(torch.cat((ref.emb(cb.x_aminoacid), ref.lstm_fc(out.reshape(R, 3))), dim=1)))
        w_e = O.edge_mlp(cb.edge_attr, sd, "conv1.net.")
        for conv in ("conv1", "conv2"):
            for _ in range(ref.depth):
                x = F.relu(O.nnconv_apply(x, cb.edge_index, w_e, sd[conv + ".root"], sd[conv + ".bias"], "mean"))
        l2 = loss_fn(ref.fc2(x).view(B, -1), cb.y.view(B, -1))
        l2.backward()
        copt.step()
    dt = time.perf_counter() - t0
    summary["cpu_baseline"] = {"samples_per_s": a.cpu_batches * B / dt, "threads": torch.get_num_threads(),
                               "batches": a.cpu_batches, "note": "plain torch autograd, edge-MLP hoisted (the reference "
                               "re-evaluates it in all 12 conv applications)"}
print(json.dumps(summary))
