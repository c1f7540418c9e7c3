"""Data-parallel training (data_parallel.py) on the MI355X: the gradient bucket's pack / unpack kernels
(include/mdno.h mdno_pack_tensors / mdno_unpack_tensors), a world-size-1 RCCL group bitwise against
training.train_epoch, and two gloo ranks sharing the card (the rehearsal backend: RCCL refuses two ranks on one GPU)
against single-process training.  Every distributed run is a fresh child process under a timeout; at most two children
run at a time."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

pytestmark = pytest.mark.gpu

# the set-up both the children and the in-process reference run: a synthetic 28-atom trajectory, index batches into
# its device-resident copy, KernelNN(64, 128, 2, ...) from a fixed seed, training.Adam
SETUP = r"""
import hashlib, numpy as np, torch
from molecular_dynamics_neural_operator_amd import synthetic as syn
from molecular_dynamics_neural_operator_amd.dataset import ContactMapDataset, write_trajectory_npz
from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN, LpLoss
from molecular_dynamics_neural_operator_amd.training import Adam, DeviceTrajectory


def make_dataset(workdir):
    N, W = 28, 10
    base = syn.chain_frame(N, seed=0)
    traj = syn.ou_trajectory(base, 60, sigma=0.3, theta=0.1, seed=2)
    path = workdir + "/traj.npz"
    write_trajectory_npz(path, traj, [syn.contact_map(f, 8.0) for f in traj], syn.amino_acids(N, seed=0))
    return ContactMapDataset(path, window_size=W, horizon=1)


def make_model(dev, precision):
    torch.manual_seed(0)
    model = KernelNN(64, 128, 2, 6, 7, 3, 20, 4).to(dev)
    model.train_precision = precision
    return model, Adam(model.parameters(), lr=1e-4, weight_decay=5e-4)


def param_hash(model):
    h = hashlib.sha256()
    for p in model.parameters():
        h.update(p.detach().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def state_of(model, opt):
    params = [p.detach().cpu().clone() for p in model.parameters()]
    st = [opt.state[p] for p in model.parameters()]
    return {"params": params, "exp_avg": [s["exp_avg"].cpu().clone() if s else None for s in st],
            "exp_avg_sq": [s["exp_avg_sq"].cpu().clone() if s else None for s in st]}
"""

CHILD = SETUP + r"""
import json, os, sys, time
import torch.distributed as dist
from molecular_dynamics_neural_operator_amd.data_parallel import DataParallelTrainer, broadcast_parameters
cfg = json.loads(sys.argv[1])
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
if cfg["backend"] == "nccl":
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
else:
    dist.init_process_group("gloo", rank=rank, world_size=world)
try:
    os.makedirs(cfg["workdir"] + f"/rank{rank}", exist_ok=True)
    dset = make_dataset(cfg["workdir"] + f"/rank{rank}")
    model, opt = make_model(dev, cfg["precision"])
    broadcast_parameters(model)
    loss_fn = LpLoss(size_average=cfg["size_average"])
    tr = DataParallelTrainer(model, opt, loss_fn)
    res = {"rank": rank}
    if cfg.get("bad"):
        bad = dset[1]
        bad.x_aminoacid = bad.x_aminoacid.clone()
        bad.x_aminoacid[3] = 20
        t0 = time.time()
        try:
            tr.train_epoch([[dset[0], bad], [dset[2], dset[3]]])
            res["raised"] = None
        except IndexError as e:
            res["raised"] = type(e).__name__
        res["seconds"] = time.time() - t0
    else:
        src = DeviceTrajectory(dset, dev)
        if cfg.get("validate"):
            res["valid"] = tr.validate_epoch(cfg["validate"], src)
        res["epochs"] = []
        for ep in range(cfg["epochs"]):
            loss, mse = tr.train_epoch(cfg["batches"], src)
            res["epochs"].append({"loss": loss, "mse": mse, "hash": param_hash(model)})
        torch.save(state_of(model, opt), cfg["workdir"] + f"/state{rank}.pt")
    print("RESULT " + json.dumps(res), flush=True)
finally:
    dist.destroy_process_group()
"""


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_children(tmp_path, world, cfg, timeout=180):
    script = tmp_path / "dp_child.py"
    script.write_text(CHILD)
    cfg = dict(cfg, workdir=str(tmp_path))
    port = _port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), PYTHONPATH=str(REPO))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, str(script), json.dumps(cfg)], env=env, cwd=str(REPO),
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    results = []
    try:
        for p in procs:
            out, err = p.communicate(timeout=timeout)
            assert p.returncode == 0, (p.returncode, out[-1000:], err[-3000:])
            line = [ln for ln in out.splitlines() if ln.startswith("RESULT ")]
            assert line, (out[-1000:], err[-3000:])
            results.append(json.loads(line[-1][len("RESULT "):]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    return results


def _setup_ns():
    ns = {}
    exec(SETUP, ns)
    return ns


def _reference(tmp_path, batches, epochs, precision="fp32", size_average=False, validate=None):
    """Single-process training.train_epoch (and validate_epoch) on the same global batches."""
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory, train_epoch, validate_epoch
    ns = _setup_ns()
    dev = torch.device("cuda", 0)
    ref_dir = tmp_path / "ref"
    ref_dir.mkdir(exist_ok=True)
    dset = ns["make_dataset"](str(ref_dir))
    src = DeviceTrajectory(dset, dev)
    model, opt = ns["make_model"](dev, precision)
    loss_fn = LpLoss(size_average=size_average)
    res = {}
    if validate:
        res["valid"] = validate_epoch(model, [src.batch(b) for b in validate], loss_fn)
    res["epochs"] = []
    for _ in range(epochs):
        res["epochs"].append(train_epoch(model, [src.batch(b) for b in batches], opt, loss_fn))
    res["state"] = ns["state_of"](model, opt)
    return res


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


def _state_rel_l2(got, want):
    worst = 0.0
    for k in ("params", "exp_avg", "exp_avg_sq"):
        for g, w in zip(got[k], want[k]):
            assert (g is None) == (w is None)
            if g is not None and k == "params":
                worst = max(worst, float((g.double() - w.double()).norm() / max(float(w.double().norm()), 1e-30)))
    return worst


# ------------------------------------------------------------------------------------------------ 1. pack / unpack
def test_pack_unpack_bucket(tmp_path):
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.data_parallel import _slots
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    dev = torch.device("cuda", 0)
    m = KernelNN(64, 1024, 6, 6, 7, 3, 20, 4)
    # the 27 state_dict tensors (conv2 shares conv1's edge-MLP: 21 distinct parameters, 5,264,383 values)
    shapes = [tuple(v.shape) for v in m.state_dict().values()]
    assert len(shapes) == 27 and sum(p.numel() for p in m.parameters()) == 5_264_383
    gen = torch.Generator().manual_seed(0)
    tensors = [torch.randn(s, generator=gen).to(dev) for s in shapes + [(1,), (3,), (5,), (4097,)]]
    store = torch.randn(1001, generator=gen).to(dev)
    tensors.append(store[1:])                                         # starts 4 B into its storage: scalar path
    assert tensors[-1].data_ptr() % 16 == 4
    offsets, total = _slots(tensors)
    flat = torch.full((total,), float("nan"), device=dev)
    ops.pack_tensors(tensors, flat, offsets)
    got = torch.cat([flat[o:o + t.numel()] for t, o in zip(tensors, offsets)])
    assert torch.equal(got, torch.cat([t.reshape(-1) for t in tensors]))
    back = [torch.full_like(t, float("nan")) for t in tensors]
    ops.unpack_tensors(flat, back, offsets)
    assert all(torch.equal(a, b) for a, b in zip(back, tensors))
    # an entry without data zero-fills its slot (the others are untouched)
    entries = list(tensors)
    entries[3] = tensors[3].numel()
    entries[-2] = tensors[-2].numel()
    flat2 = torch.full((total,), float("nan"), device=dev)
    ops.pack_tensors(entries, flat2, offsets)
    for i, (t, o) in enumerate(zip(tensors, offsets)):
        want = torch.zeros_like(t).reshape(-1) if i in (3, len(tensors) - 2) else t.reshape(-1)
        assert torch.equal(flat2[o:o + t.numel()], want), i
    # a list longer than one kernel argument holds: several launches, same result
    many = [torch.randn(n % 37 + 1, generator=gen).to(dev) for n in range(150)]
    moff, mtot = _slots(many)
    mflat = torch.zeros(mtot, device=dev)
    ops.pack_tensors(many, mflat, moff)
    assert torch.equal(torch.cat([mflat[o:o + t.numel()] for t, o in zip(many, moff)]), torch.cat(many))
    torch.cuda.synchronize()
    # bad arguments, all refused before any device work
    with pytest.raises(MdnoError):
        ops.pack_tensors(tensors[:2], None, offsets[:2])                                    # null flat
    with pytest.raises(MdnoError):
        ops.pack_tensors([tensors[0], -1], flat, offsets[:2])                              # negative numel
    with pytest.raises(MdnoError):
        ops.pack_tensors(tensors[:2], flat, [0, 1])                                         # overlapping slots
    with pytest.raises(MdnoError):
        ops.unpack_tensors(flat, tensors[:2], [offsets[0], offsets[0] + 2])                # overlapping slots
    with pytest.raises(MdnoError):
        ops.unpack_tensors(flat, [tensors[0], 5], offsets[:2])                             # unpack into nothing
    with pytest.raises(MdnoError):
        ops.pack_tensors(tensors[:1], flat, [total - 1])                                   # slot outside flat
    assert torch.equal(back[0], tensors[0])


# ------------------------------------------------------------------------------------------------ 2. world 1 over RCCL
def test_world1_rccl_bitwise_equals_train_epoch(tmp_path):
    batches = [list(range(8 * k, 8 * k + 8)) for k in range(4)]
    res = _run_children(tmp_path, 1, dict(backend="nccl", precision="fp32", size_average=False, epochs=3,
                                          batches=batches))[0]
    ref = _reference(tmp_path, batches, 3)
    assert [(e["loss"], e["mse"]) for e in res["epochs"]] == [tuple(e) for e in ref["epochs"]]
    got = torch.load(tmp_path / "state0.pt")
    for k in ("params", "exp_avg", "exp_avg_sq"):
        for i, (g, w) in enumerate(zip(got[k], ref["state"][k])):
            assert w is not None and torch.equal(g, w), (k, i)


# ------------------------------------------------------------------------------------------------ 3 + 8. world 2, gloo, fp32
GLOO_BATCHES = [list(range(0, 8)), list(range(8, 15)), list(range(15, 23)), list(range(23, 30))]   # 8 = 4 + 4, 7 = 4 + 3
VALID_BATCHES = [list(range(30, 38)), list(range(38, 45))]


@pytest.fixture(scope="module")
def gloo_fp32(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dp_gloo_fp32")
    res = _run_children(tmp, 2, dict(backend="gloo", precision="fp32", size_average=False, epochs=3,
                                     batches=GLOO_BATCHES, validate=VALID_BATCHES))
    ref = _reference(tmp, GLOO_BATCHES, 3, validate=VALID_BATCHES)
    return tmp, res, ref


def test_world2_gloo_fp32_replicas_identical_and_match_single_process(gloo_fp32):
    tmp, (r0, r1), ref = gloo_fp32
    for e0, e1, (rl, rm) in zip(r0["epochs"], r1["epochs"], ref["epochs"]):
        assert e0 == e1                                              # same hash, same (loss, mse) on both ranks
        assert _rel(e0["loss"], rl) < 1e-6 and _rel(e0["mse"], rm) < 1e-6, (e0, rl, rm)
    worst = _state_rel_l2(torch.load(tmp / "state0.pt"), ref["state"])
    assert worst < 1e-5, worst


def test_world2_validate_epoch_matches_single_process(gloo_fp32):
    _, (r0, r1), ref = gloo_fp32
    assert r0["valid"] == r1["valid"]
    assert _rel(r0["valid"][0], ref["valid"][0]) < 1e-6 and _rel(r0["valid"][1], ref["valid"][1]) < 1e-6, \
        (r0["valid"], ref["valid"])


# ------------------------------------------------------------------------------------------------ 4. world 2, gloo, bf16
def test_world2_gloo_bf16(tmp_path):
    r0, r1 = _run_children(tmp_path, 2, dict(backend="gloo", precision="bf16", size_average=False, epochs=3,
                                             batches=GLOO_BATCHES))
    ref = _reference(tmp_path, GLOO_BATCHES, 3, precision="bf16")
    for e0, e1, (rl, _) in zip(r0["epochs"], r1["epochs"], ref["epochs"]):
        assert e0 == e1
        assert _rel(e0["loss"], rl) < 3e-2, (e0, rl)


# ------------------------------------------------------------------------------------------------ 5. a rank without samples
def test_world2_global_batch_of_one(tmp_path):
    batches = [[k] for k in range(4)]
    r0, r1 = _run_children(tmp_path, 2, dict(backend="gloo", precision="fp32", size_average=False, epochs=3,
                                             batches=batches))
    ref = _reference(tmp_path, batches, 3)
    assert r0["epochs"] == r1["epochs"]
    assert [(e["loss"], e["mse"]) for e in r0["epochs"]] == [tuple(e) for e in ref["epochs"]]
    got = torch.load(tmp_path / "state0.pt")
    for k in ("params", "exp_avg", "exp_avg_sq"):
        for i, (g, w) in enumerate(zip(got[k], ref["state"][k])):
            assert torch.equal(g, w), (k, i)


# ------------------------------------------------------------------------------------------------ 6. size_average=True
def test_world2_size_average_loss(tmp_path):
    r0, r1 = _run_children(tmp_path, 2, dict(backend="gloo", precision="fp32", size_average=True, epochs=3,
                                             batches=GLOO_BATCHES))
    ref = _reference(tmp_path, GLOO_BATCHES, 3, size_average=True)
    for e0, e1, (rl, rm) in zip(r0["epochs"], r1["epochs"], ref["epochs"]):
        assert e0 == e1
        assert _rel(e0["loss"], rl) < 1e-6 and _rel(e0["mse"], rm) < 1e-6, (e0, rl, rm)
    worst = _state_rel_l2(torch.load(tmp_path / "state0.pt"), ref["state"])
    assert worst < 1e-5, worst


# ------------------------------------------------------------------------------------------------ 7. bad sample on rank 1
def test_world2_bad_sample_raises_on_every_rank(tmp_path):
    """Rank 1's shard holds an amino-acid id outside the embedding table: the status word is reduced at the end of the
    epoch, so both ranks raise IndexError (neither waits in a collective for the other)."""
    res = _run_children(tmp_path, 2, dict(backend="gloo", precision="fp32", size_average=False, bad=True), timeout=60)
    for r in res:
        assert r["raised"] == "MdnoIndexError" and r["seconds"] < 60, r
