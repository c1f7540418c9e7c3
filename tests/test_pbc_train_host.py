"""Training under a periodic box without a GPU: what is particular to include/mdno_pbc_train.h and its ctypes table (that
header, table and exports agree is tests/test_cabi_tables.py's); the entry refuses what the other periodic entries refuse, before any
launch; the Python layers raise MdnoError on the same boxes and on ker_in != 6 without touching a device; and the numpy
restatement of the attribute rule, and the fp64 replica the GPU tests compare with (tests/test_gpu_pbc_train.py), have the
properties those tests lean on."""
import ctypes as C

import numpy as np
import pytest
import torch

from cabi import CSRC, lib  # noqa: F401  (lib: the fixture)
from test_pbc_host import BAD_BOXES

NAMES = {"mdnopbt_edge_attr_from_pos"}


def box3(*v):
    return (C.c_double * 3)(*v)


def test_header_table_and_exports_agree(lib):
    """What is particular to this header; that header, table and exports agree is tests/test_cabi_tables.py's."""
    from molecular_dynamics_neural_operator_amd import _lib
    assert set(_lib.PBC_TRAIN_SIGNATURES) == NAMES
    assert lib.mdno_abi_version() == 15 and lib.mdno_train_abi_version() == 1          # additive: both stay
    assert (CSRC / "pbc_train.hip").exists()                                           # inside the library's content hash
    assert '#include "pbc.h"' in (CSRC / "pbc_train.hip").read_text()                  # the rule is included, not restated


def test_entry_refuses_before_any_launch(lib):
    """No pointer below is a device pointer: a call that got as far as a launch would fault, not return EINVAL."""
    from molecular_dynamics_neural_operator_amd import _lib
    E = _lib.EINVAL
    f = lib.mdnopbt_edge_attr_from_pos
    for bad in BAD_BOXES:
        for cap in (25, 0):
            assert f(None, None, None, None, cap, 5, 8.0, box3(*bad), None, None) == E and b"box[" in lib.mdno_last_error(), bad
    assert f(None, None, None, None, 25, 5, 8.0, None, None, None) == E and b"null box" in lib.mdno_last_error()
    assert f(None, None, None, None, 25, 5, float("nan"), box3(20, 20, 20), None, None) == E
    for ok in ((16.0, 16.0, 16.0), (16.0, 0.0, 40.0), (0.0, 0.0, 0.0)):
        assert f(None, None, None, None, 25, 5, 8.0, box3(*ok), None, None) == E and b"null pointer" in lib.mdno_last_error()
        assert f(None, None, None, None, 0, 5, 8.0, box3(*ok), None, None) == 0            # edge_cap = 0: nothing to do
        assert f(None, None, None, None, -1, 5, 8.0, box3(*ok), None, None) == E
        assert f(None, None, None, None, 25, 0, 8.0, box3(*ok), None, None) == E and b"num_rows=0" in lib.mdno_last_error()
    assert f(0x1000, 0x1000, 0x1000, 0x1000, 25, 5, 8.0, box3(16, 16, 16), 0x1004, None) == E
    assert b"aligned" in lib.mdno_last_error()


class _Dataset:
    window_size, horizon = 2, 1
    edge_attrs = np.zeros((6, 5, 3), np.float32)
    edge_indices = [np.zeros((2, 0), np.int64)] * 6
    x_aminoacid = torch.zeros(5, dtype=torch.long)

    def __len__(self):
        return 4

    def __getitem__(self, i):
        raise AssertionError("the box is checked before the dataset is read")


def test_python_arguments_are_checked_without_a_device():
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN, propogate, recursive_propagation
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory, EdgeAttrFromPositions, unrolled_forward
    model6 = KernelNN(64, 128, 1, 6, 7, 3, 20, 4)
    model5 = KernelNN(64, 128, 1, 5, 7, 3, 20, 4)
    batch = PairData(torch.zeros(5, dtype=torch.long), torch.zeros(2, 5, 3), torch.zeros(5, 3), torch.zeros(5, 6),
                     torch.arange(5).repeat(2, 1))
    graph = ops.CSRGraph(None, None, None, None, 0, n_edges=0)
    for bad in BAD_BOXES + [(20.0, 20.0), "abc"]:
        for call in (lambda: DeviceTrajectory(_Dataset(), "cuda", box=bad),
                     lambda: DeviceTrajectory(_Dataset(), "cpu", box=bad),
                     lambda: unrolled_forward(model6, batch, 2, box=bad),
                     lambda: recursive_propagation(model6, _Dataset(), "cuda", 2, [0], box=bad),
                     lambda: propogate(model6, _Dataset(), "cuda", 2, box=bad),
                     lambda: ops.edge_attr_from_pos(torch.zeros(5, 3), graph, bad),
                     lambda: EdgeAttrFromPositions.apply(torch.zeros(5, 3), graph, bad, 8.0)):
            with pytest.raises(MdnoError, match="box"):
                call()
    good = (16.0, 16.0, 0.0)
    with pytest.raises(MdnoError, match="ker_in=5"):
        unrolled_forward(model5, batch, 2, box=good)
    with pytest.raises(MdnoError, match="ker_in=5"):
        recursive_propagation(model5, _Dataset(), "cuda", 2, [0], box=good)
    # a batch knows its box and cutoff: another one is refused
    batch.box, batch.cutoff = good, 8.0
    for kw in (dict(box=(16.0, 16.0, 16.0)), dict(cutoff=7.5), dict(box=(0.0, 0.0, 0.0))):
        with pytest.raises(MdnoError, match="collated"):
            unrolled_forward(model6, batch, 2, **kw)
    with pytest.raises(MdnoError, match="ker_in=5"):
        unrolled_forward(model5, batch, 2)


def test_restatement_properties():
    """Translating all atoms by a whole box vector changes no shift; translating ONE atom by a box vector changes its
    edges' shifts by exactly that vector and leaves every imaged row's distance unchanged.  (Coordinates on a 1/64 grid:
    the translated ones are exact in fp32.)"""
    from test_gpu_pbc_train import attr_rule, shifts_of
    rng = np.random.default_rng(0)
    L = np.array([17.0, 17.0, 0.0])
    n = 40
    pos = (rng.integers(0, 17 * 64, size=(n, 3)) / 64.0).astype(np.float32)
    src, dst = rng.integers(0, n, size=400), rng.integers(0, n, size=400)
    d = pos[src].astype(np.float64) - pos[dst].astype(np.float64)
    tie = (np.abs(d[:, :2]) == 8.5).any(1)           # exactly half a box apart (possible on a grid): never an edge, and
    src, dst = src[~tie], dst[~tie]                   # round-half-even there depends on the parity of the translation
    sh = shifts_of(pos, src, dst, L)
    assert (sh != 0).any(0).tolist() == [True, True, False] and set(np.unique(sh / 17.0)) <= {-1.0, 0.0, 1.0}
    assert np.array_equal(shifts_of((pos + np.array([2, -1, 0]) * L).astype(np.float32), src, dst, L), sh)
    one = pos.copy()
    vec = np.array([-2.0, 1.0, 0.0]) * L
    one[7] = (one[7].astype(np.float64) + vec).astype(np.float32)
    sh1 = shifts_of(one, src, dst, L)
    want = sh + np.where((src == 7)[:, None], vec, 0.0) - np.where((dst == 7)[:, None], vec, 0.0)
    assert (src == 7).sum() > 3 and (dst == 7).sum() > 3 and np.array_equal(sh1, want)
    a0, a1 = attr_rule(pos, src, dst, L).astype(np.float64), attr_rule(one, src, dst, L).astype(np.float64)
    assert np.array_equal(a0[:, :3] - a0[:, 3:], a1[:, :3] - a1[:, 3:])
    d = a0[:, :2] - a0[:, 3:5]
    assert float(np.abs(d).max()) <= 8.5                                               # the minimum image on the periodic axes


@pytest.mark.parametrize("config", ["d2w4k2_cube", "d1w2k3_b2_slab"])
def test_replica_is_sensitive_to_both_paths_and_to_the_image(config):
    """What keeps tests/test_gpu_pbc_train.py test_unrolled_periodic_step_vs_fp64 honest, on the CPU replica alone (its
    fed-back frames' edge lists from the numpy rule on its own frames): cutting the window path moves the gradient by
    >= 0.1, cutting the edge path by >= 5e-3, and the replica with every shift zero differs from the right one by at
    least 10 x the gate max(UNROLL_GATE, 4 e32)."""
    from test_gpu_pbc import pbc_graph_members
    from test_gpu_pbc_train import (BOXES, CUT, N_BOX, UNROLL_CONFIGS, assert_wraps, attr_rule, box_dataset, replica,
                                    shifts_of, worst_err)
    from test_gpu_unroll import UNROLL_GATE, live_model, max_change
    depth, W, K, idxs, box_name = UNROLL_CONFIGS[config]
    box = BOXES[box_name]
    dset = box_dataset(W)
    samples = [dset[i] for i in idxs]
    B, N = len(idxs), N_BOX
    xp = torch.cat([s.x_position for s in samples], dim=1)
    ys = torch.stack([torch.cat([torch.from_numpy(dset.edge_attrs[i + W + k]) for i in idxs]) for k in range(K)])
    sd = {n: v.detach() for n, v in live_model(depth, "cpu").state_dict().items()}
    first = xp[0].numpy()
    g0 = pbc_graph_members(first, N, CUT, box)
    lists = [torch.from_numpy(np.stack([g0["src"], g0["dst"]])).long()]
    shifts = [torch.from_numpy(shifts_of(first, g0["src"], g0["dst"], box))]
    ea0 = torch.from_numpy(attr_rule(first, g0["src"], g0["dst"], box))
    assert_wraps(first, g0["src"], g0["dst"], box)
    for k in range(1, K):           # the replica's own frames, step by step
        outs = replica(sd, xp, dset.x_aminoacid, ys, depth, k, lists, shifts, ea0)[1]
        f = outs[-1].float().numpy()
        g = pbc_graph_members(f, N, CUT, box)
        assert_wraps(f, g["src"], g["dst"], box, k)
        lists.append(torch.from_numpy(np.stack([g["src"], g["dst"]])).long())
        shifts.append(torch.from_numpy(shifts_of(f, g["src"], g["dst"], box)))
    args = (sd, xp, dset.x_aminoacid, ys, depth, K, lists, shifts, ea0)
    want_loss, _, want = replica(*args)
    l32, _, g32 = replica(*args, dtype=torch.float32)
    e32, where = worst_err(l32, g32, want_loss, want)
    gate = max(UNROLL_GATE, 4 * e32)
    dw = max_change(replica(*args, detach_window=True)[2], want)
    de = max_change(replica(*args, detach_edge=True)[2], want)
    zl, _, zg = replica(*args, zero_shift=True)
    dz, _ = worst_err(zl, zg, want_loss, want)
    print(config, "e32", f"{e32:.3e}", where, "gate", f"{gate:.3e}", "window path", f"{dw:.2e}", "edge path", f"{de:.2e}",
          "zero shifts", f"{dz:.2e}")
    assert dw >= 0.1 and de >= 5e-3, (dw, de)
    assert dz >= 10 * gate, (dz, gate)
