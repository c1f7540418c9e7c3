"""Host side of data-parallel training (data_parallel.py), no GPU: how a global batch is split across ranks, the
batch-list check between two gloo ranks, and how the ranks' per-batch values become train_epoch's epoch averages."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from molecular_dynamics_neural_operator_amd.data_parallel import batch_digest, combine_losses, shard_range


@pytest.mark.parametrize("world", range(1, 9))
def test_shard_range_partitions_in_rank_order(world):
    for B in range(1, 21):
        shards = [shard_range(B, r, world) for r in range(world)]
        assert shards[0][0] == 0 and shards[-1][1] == B
        assert all(shards[r][1] == shards[r + 1][0] for r in range(world - 1))       # laid end to end: the batch
        sizes = [e - s for s, e in shards]
        assert min(sizes) >= 0 and max(sizes) - min(sizes) <= 1
        assert sizes == sorted(sizes, reverse=True)                                    # the first B mod world take one more
    with pytest.raises(ValueError):
        shard_range(4, world, world)


def test_batch_digest_sees_counts_and_indices():
    a = [[0, 1, 2, 3], [4, 5, 6]]
    assert batch_digest(a) == batch_digest([np.arange(4), np.array([4, 5, 6])])
    assert batch_digest(a) != batch_digest([[0, 1, 2, 3], [4, 5, 7]])
    assert batch_digest(a) != batch_digest([[0, 1, 2, 3]])
    assert 0 <= batch_digest(a) < 2 ** 62


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _digest_worker(rank, world, port, differ, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from molecular_dynamics_neural_operator_amd.data_parallel import check_batch_lists
        batches = [list(range(8)), list(range(8, 15))]
        if differ and rank == 1:
            batches[1] = list(range(8, 14)) + [20]
        try:
            check_batch_lists(batches)
            q.put((rank, "ok"))
        except ValueError:
            q.put((rank, "ValueError"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("differ", [False, True])
def test_batch_list_check_over_two_gloo_ranks(differ):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_digest_worker, args=(r, 2, port, differ, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(0, "ValueError"), (1, "ValueError")] if differ else [(0, "ok"), (1, "ok")]


def _train_epoch_arithmetic(l2s, mses):
    """training.train_epoch's end of epoch: fp32 per-batch values, summed as doubles in batch order."""
    vals = torch.stack([torch.tensor(v, dtype=torch.float32) for v in l2s + mses]).double().tolist()
    n = len(l2s)
    return sum(vals[:n]) / n, sum(vals[n:]) / n


@pytest.mark.parametrize("size_average", [False, True])
def test_loss_combination_is_train_epochs_arithmetic(size_average):
    gen = torch.Generator().manual_seed(1)
    sizes = [8, 7, 128, 1, 3]
    # one rank: [loss, mse * B] per batch reproduces train_epoch bit for bit
    l2 = (torch.rand(len(sizes), generator=gen) * 50).float()
    mse = (torch.rand(len(sizes), generator=gen) * 1e-2).float()
    sums = [[float(l) * (B if size_average else 1), float(m) * B] for l, m, B in zip(l2.tolist(), mse.tolist(), sizes)]
    assert combine_losses(sums, sizes, size_average) == _train_epoch_arithmetic(l2.tolist(), mse.tolist())
    # two ranks on per-sample values: the combination is the global batch's loss and MSE
    got_l, got_m, want_l, want_m = [], [], [], []
    for B in sizes:
        rel = torch.rand(B, generator=gen, dtype=torch.float64)
        sq = torch.rand(B, generator=gen, dtype=torch.float64)                 # per-sample mean squared error
        tot = [0.0, 0.0]
        for r in range(2):
            s, e = shard_range(B, r, 2)
            if e == s:
                continue
            loss_r = float(rel[s:e].mean() if size_average else rel[s:e].sum())
            tot[0] += loss_r * ((e - s) if size_average else 1)
            tot[1] += float(sq[s:e].mean()) * (e - s)
        got_l.append(tot)
        want_l.append(float(rel.mean() if size_average else rel.sum()))
        want_m.append(float(sq.mean()))
    loss, m = combine_losses(got_l, sizes, size_average)
    assert loss == pytest.approx(sum(want_l) / len(sizes), rel=1e-13)
    assert m == pytest.approx(sum(want_m) / len(sizes), rel=1e-13)
    assert combine_losses([], [], size_average) == (0.0, 0.0)
