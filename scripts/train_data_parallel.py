"""BASELINE.json configs[3] trained data-parallel: every global batch split across the ranks, one gradient all-reduce per
step (data_parallel.DataParallelTrainer) — the reference's main() under torch_geometric.nn.DataParallel
(graph_kernel.py:528), one process per GPU.

  python -m torch.distributed.run --nproc-per-node 8 scripts/train_data_parallel.py [--batch-size 128] [--epochs 1]
  python scripts/train_data_parallel.py --force-dist          # alone: a one-rank nccl (RCCL) group

The cfg4 set-up of scripts/train_synthetic.py: the synthetic N=28 trajectory, KernelNN(64, 1024, 6, 6, 7, 3, 20, 4)
with its kernel's last layer damped, training.Adam(lr, weight_decay=5e-4), StepLR(50, 0.8), LpLoss(size_average=False),
partition split 0.8, drop_last; batches built on the device.  Rank 0 prints the reference's epoch line and a JSON
summary: global samples/s, world size and backend, and the per-step device time of forward+backward, pack, all-reduce
and optimiser step.
"""
import argparse
import json
import os
import socket
import sys
import time
from pathlib import Path

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC only on this driver (RCCL needs it)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from molecular_dynamics_neural_operator_amd import synthetic as syn  # noqa: E402
from molecular_dynamics_neural_operator_amd.data_parallel import DataParallelTrainer, broadcast_parameters  # noqa: E402
from molecular_dynamics_neural_operator_amd.dataset import ContactMapDataset, write_trajectory_npz  # noqa: E402
from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN, LpLoss  # noqa: E402
from molecular_dynamics_neural_operator_amd.training import Adam, DeviceTrajectory  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=2000)
ap.add_argument("--batch-size", type=int, default=128, help="global batch (split across the ranks)")
ap.add_argument("--epochs", type=int, default=1)
ap.add_argument("--kernel-width", type=int, default=1024)
ap.add_argument("--depth", type=int, default=6)
ap.add_argument("--lr", type=float, default=1e-4)
ap.add_argument("--precision", choices=["fp32", "bf16"], default="bf16")
ap.add_argument("--train-conv-mode", choices=["materialized", "factored", "auto"], default="materialized",
                help="kernel-integral block in training: W_e formed, factored per destination (dense graphs; needs "
                     "--precision fp32), or by the counted-graph rule")
ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                help="nccl (RCCL), one GPU per rank; gloo only to rehearse with ranks sharing a card")
ap.add_argument("--force-dist", action="store_true", help="run alone as a one-rank process group")
ap.add_argument("--noise-std", type=float, default=0.0, help="Gaussian noise on the input windows of every training batch")
ap.add_argument("--noise-seed", type=int, default=0)
ap.add_argument("--workdir", default="/tmp/mdno_train_dp")
a = ap.parse_args()

if a.force_dist and "WORLD_SIZE" not in os.environ:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
if "WORLD_SIZE" not in os.environ:
    ap.error("run under torch.distributed.run, or alone with --force-dist")
local = int(os.environ.get("LOCAL_RANK", "0"))
gpu = local if a.backend == "nccl" else 0
torch.cuda.set_device(gpu)
dev = torch.device("cuda", gpu)
t_init = time.perf_counter()
if a.backend == "nccl":
    dist.init_process_group("nccl", device_id=dev)
else:
    dist.init_process_group("gloo")
init_s = time.perf_counter() - t_init
rank, world = dist.get_rank(), dist.get_world_size()

workdir = Path(a.workdir) / f"rank{rank}"
workdir.mkdir(parents=True, exist_ok=True)
N, W = 28, 10
base = syn.chain_frame(N, seed=0)
traj = syn.ou_trajectory(base, a.frames, sigma=0.3, theta=0.1, seed=2)
path = workdir / "synthetic_bba.npz"
write_trajectory_npz(path, traj, [syn.contact_map(f, 8.0) for f in traj], syn.amino_acids(N, seed=0))
dset = ContactMapDataset(str(path), window_size=W, horizon=1)
n_train = int(len(dset) * 0.8)                                    # partition split (graph_kernel.py:509-520)
train_idx, valid_idx = list(range(n_train)), list(range(n_train, len(dset)))
B = a.batch_size
batches = [train_idx[s:s + B] for s in range(0, len(train_idx) - B + 1, B)]          # drop_last
vbatches = [valid_idx[s:s + B] for s in range(0, len(valid_idx) - B + 1, B)]
src = DeviceTrajectory(dset, dev)

torch.manual_seed(0)
model = KernelNN(64, a.kernel_width, a.depth, 6, 7, 3, 20, 4)
with torch.no_grad():     # as train_synthetic.py: damp the kernel's last layer so Adam starts from O(1) values
    for p_ in model.conv1.net.layers[4].parameters():
        p_.mul_(0.05)
model.to(dev)
model.train_precision = a.precision
model.train_conv_mode = a.train_conv_mode
broadcast_parameters(model)                                       # every replica starts from rank 0's parameters
opt = Adam(model.parameters(), lr=a.lr, weight_decay=5e-4)
sched = torch.optim.lr_scheduler.StepLR(opt, step_size=50, gamma=0.8)
loss_fn = LpLoss(size_average=False)
trainer = DataParallelTrainer(model, opt, loss_fn)

summary = {"frames": a.frames, "batch_size": B, "train_batches": len(batches), "kernel_width": a.kernel_width,
           "depth": a.depth, "precision": a.precision, "world_size": world, "backend": dist.get_backend(),
           "forced_one_rank_group": bool(a.force_dist), "init_process_group_s": init_s,
           "bucket_bytes": trainer.bucket_bytes}
trainer.train_epoch(batches[:1], src)                             # warm-up (allocator, kernels, communicator)
torch.cuda.synchronize()
trainer.step_times_ms()
torch.cuda.reset_peak_memory_stats()
trainer.timing = True
for ep in range(a.epochs):
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tl, mse = trainer.train_epoch(batches, src, noise_std=a.noise_std, noise_seed=a.noise_seed, epoch=ep)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    vl = trainer.validate_epoch(vbatches, src)[0]
    sched.step()
    if rank == 0:
        print(f"Epoch: {ep}\tTime: {dt}\ttrain_loss: {tl}\tvalid_loss: {vl}")
    summary.update(epoch_seconds=dt, samples_per_s=len(batches) * B / dt, train_loss=tl, valid_loss=vl, train_mse=mse,
                   peak_memory_MiB=torch.cuda.max_memory_allocated() / 2**20)
st = trainer.step_times_ms()
summary["step_us"] = {k: v * 1e3 for k, v in st.items() if k != "steps"}
summary["timed_steps"] = st.get("steps", 0)
if rank == 0:
    print(json.dumps(summary))
dist.barrier()
dist.destroy_process_group()
