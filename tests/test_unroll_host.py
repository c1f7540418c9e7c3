"""include/mdno_unroll.h without a GPU: the names of its ctypes table (`_lib.UNROLL_SIGNATURES`) are pinned (that
header, table and exports agree is tests/test_cabi_tables.py's); every new entry point validates its arguments before any device work; the Python layer refuses what
an unrolled step cannot do (horizon != 1, targets past the data, bf16 storage, host-collated lists) on the host."""
import numpy as np
import pytest
import torch

from cabi import CSRC, lib  # noqa: F401  (lib: the fixture)

NAMES = {"mdno_edge_mlp_input_bwd", "mdno_edge_attr_from_pos", "mdno_edge_attr_pos_bwd", "mdno_node_prologue_bwd_frames",
         "mdno_collate_targets"}


def test_unroll_header_table_and_exports_agree(lib):
    """What is particular to this header; that header, table and exports agree is tests/test_cabi_tables.py's."""
    from molecular_dynamics_neural_operator_amd import _lib
    assert set(_lib.UNROLL_SIGNATURES) == NAMES
    assert lib.mdno_abi_version() == 15 and lib.mdno_train_abi_version() == 1          # additive: both stay
    assert (CSRC / "input_grad.hip").exists()                                          # inside the library's content hash


def test_unroll_entry_points_validate_before_device_work(lib):
    from molecular_dynamics_neural_operator_amd import _lib
    E = _lib.EINVAL
    err = lib.mdno_last_error
    # mdno_edge_mlp_input_bwd(gz1, w0, num_edges, edge_cap, ker_width, ker_in, d_edge_attr, stream)
    assert lib.mdno_edge_mlp_input_bwd(None, None, None, 5, 16, 6, None, None) == E and b"null pointer" in err()
    assert lib.mdno_edge_mlp_input_bwd(None, None, None, 5, 16, 0, None, None) == E and b"ker_in=0" in err()
    assert lib.mdno_edge_mlp_input_bwd(None, None, None, 5, 16, 9, None, None) == E and b"ker_in=9" in err()
    assert lib.mdno_edge_mlp_input_bwd(None, None, None, 5, 0, 6, None, None) == E and b"ker_width=0" in err()
    assert lib.mdno_edge_mlp_input_bwd(None, None, None, -1, 16, 6, None, None) == E
    assert lib.mdno_edge_mlp_input_bwd(None, None, None, 0, 16, 6, None, None) == 0          # E = 0 is legal: nothing to do
    # mdno_edge_attr_from_pos(pos, src, dst, num_edges, edge_cap, num_rows, edge_attr, stream)
    assert lib.mdno_edge_attr_from_pos(None, None, None, None, 5, 4, None, None) == E and b"null pointer" in err()
    assert lib.mdno_edge_attr_from_pos(None, None, None, None, 5, 0, None, None) == E and b"num_rows=0" in err()
    assert lib.mdno_edge_attr_from_pos(None, None, None, None, -1, 4, None, None) == E
    assert lib.mdno_edge_attr_from_pos(None, None, None, None, 0, 4, None, None) == 0
    # mdno_edge_attr_pos_bwd(d_edge_attr, row_ptr, row_ptr_s, eid_s, num_rows, d_pos, stream)
    assert lib.mdno_edge_attr_pos_bwd(None, None, None, None, 4, None, None) == E and b"null pointer" in err()
    assert lib.mdno_edge_attr_pos_bwd(None, None, None, None, 0, None, None) == E and b"num_rows=0" in err()
    # mdno_node_prologue_bwd_frames(p, frames, M, W, N, aa, aa_per_member, x0, g0, d_lstm, d_emb, d_fc1_w, d_fc1_b,
    #                               d_frames, workspace, workspace_bytes, stream)
    nul = (None,) * 7
    assert lib.mdno_node_prologue_bwd_frames(None, None, 1, 17, 5, None, 0, *nul, None, 0, None) == E and b"window 17" in err()
    assert lib.mdno_node_prologue_bwd_frames(None, None, 1, 0, 5, None, 0, *nul, None, 0, None) == E and b"window 0" in err()
    assert lib.mdno_node_prologue_bwd_frames(None, None, 1, 4, 5, None, 0, *nul, None, 0, None) == E and b"null pointer" in err()
    # mdno_collate_targets(pos, num_frames, meta, B, N, W, horizon, K, y, stream)
    assert lib.mdno_collate_targets(None, 10, None, 2, 5, 3, 1, 0, None, None) == E and b"K=0" in err()
    assert lib.mdno_collate_targets(None, 10, None, 0, 5, 3, 1, 2, None, None) == E and b"B=0" in err()
    assert lib.mdno_collate_targets(None, 10, None, 2, 5, 3, 1, 2, None, None) == E and b"null pointer" in err()


class _Dataset:
    """The four things DeviceTrajectory reads, and a device type check before them."""

    def __init__(self, frames=12, n=5, window=3, horizon=1):
        self.window_size, self.horizon = window, horizon
        self.edge_attrs = np.zeros((frames, n, 3), dtype=np.float32)
        self.edge_indices = [np.zeros((2, n), dtype=np.int64) for _ in range(frames)]
        self.x_aminoacid = torch.zeros(n, dtype=torch.long)

    def __len__(self):
        return len(self.edge_indices) - self.window_size - self.horizon + 1


def _host_trajectory(**kw):
    """A DeviceTrajectory's host-side state without a device (its constructor copies the data to one): what batch()
    checks before it touches anything."""
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory
    d = _Dataset(**kw)
    t = DeviceTrajectory.__new__(DeviceTrajectory)
    t.device, t.W, t.horizon, t.length, t.N = torch.device("cpu"), d.window_size, d.horizon, len(d), 5
    t.counts = np.full(len(d.edge_indices), 5, dtype=np.int64)
    t.offsets = np.concatenate([[0], np.cumsum(t.counts)]).astype(np.int64)
    return t


def test_batch_refuses_horizon_and_late_indices_without_a_device():
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    t = _host_trajectory()                       # 12 frames, window 3: 9 samples
    assert len(t) == 9
    with pytest.raises(IndexError, match="unroll=3"):
        t.batch([0, 7], unroll=3)                # sample 7 needs frames up to 7 + 3 + 2 = 12
    with pytest.raises(IndexError):
        t.batch([9], unroll=1)
    with pytest.raises(MdnoError, match="unroll=0"):
        t.batch([0], unroll=0)
    with pytest.raises(MdnoError, match="horizon 1"):
        _host_trajectory(horizon=2).batch([0], unroll=2)


def _model(k=128):
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    torch.manual_seed(0)
    return KernelNN(64, k, 1, 6, 7, 3, 20, 4)


def _sample(n=5, w=3, requires_grad=False):
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    ei = torch.stack([torch.arange(n), torch.arange(n)])
    s = PairData(torch.zeros(n, dtype=torch.long), torch.zeros(w, n, 3), torch.zeros(n, 3), torch.zeros(n, 6), ei)
    s.num_graphs = 1
    if requires_grad:
        s.x_position.requires_grad_()
    return s


def test_bf16_and_lists_are_refused_without_a_device():
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import check_trainable, train_epoch, train_forward, unrolled_forward
    model = _model()                             # on the host: anything that got as far as the device check raises MdnoError
    model.train_precision = "bf16"
    check_trainable(model, 3)                    # bf16 training itself stays
    with pytest.raises(NotImplementedError, match="bf16"):
        check_trainable(model, 3, input_grad=True)
    with pytest.raises(NotImplementedError, match="bf16"):
        train_forward(model, _sample(requires_grad=True))
    ea = _sample()
    ea.edge_attr.requires_grad_()
    with pytest.raises(NotImplementedError, match="bf16"):
        train_forward(model, ea)
    with pytest.raises(NotImplementedError, match="bf16"):
        unrolled_forward(model, _sample(), 2)
    with pytest.raises(MdnoError, match="GPU"):                      # detached: bf16 is allowed, the next check is the device
        unrolled_forward(model, _sample(), 2, detach=True)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    with pytest.raises(NotImplementedError, match="bf16"):
        train_epoch(model, [_sample()], opt, LpLoss(size_average=False), unroll=2)
    model.train_precision = "fp32"
    with pytest.raises(MdnoError, match="steps=0"):
        unrolled_forward(model, _sample(), 0)
    with pytest.raises(MdnoError, match="DeviceTrajectory"):         # a host-collated list of samples
        train_epoch(model, [[_sample(), _sample()]], opt, LpLoss(size_average=False), unroll=2)
    with pytest.raises(MdnoError, match="y_unroll"):                 # a collated batch without the K targets
        train_epoch(model, [_sample()], opt, LpLoss(size_average=False), unroll=2)
    with pytest.raises(MdnoError, match="unroll=0"):
        train_epoch(model, [], opt, LpLoss(size_average=False), unroll=0)
