"""Periodic boxes without a GPU: what is particular to include/mdno_pbc.h and its ctypes table (that header, table and
exports agree is tests/test_cabi_tables.py's); every refusal of the rule (a periodic axis shorter than 2 * cutoff, a negative, NaN or Inf
length, a null plan, a null attribute buffer with a periodic axis, ker_in != 6) comes back as MDNO_EINVAL, or is raised
as MdnoError, before any device work; and the numpy restatement of the rule (tests/test_gpu_pbc.py) has the properties
the GPU tests lean on."""
import ctypes as C

import numpy as np
import pytest
import torch

from cabi import CSRC, lib  # noqa: F401  (lib: the fixture)

NAMES = {"mdno_radius_graph_pbc", "mdno_rollout_plan_set_box", "mdno_forecast_score_pbc", "mdno_contact_maps_pbc"}
BAD_BOXES = [(15.9, 20.0, 20.0), (20.0, 20.0, 1e-3), (-1.0, 20.0, 20.0), (20.0, float("nan"), 20.0),
             (20.0, 20.0, float("inf")), (-0.5, 0.0, 0.0)]


def box3(*v):
    return (C.c_double * 3)(*v)


def test_pbc_header_table_and_exports_agree(lib):
    """What is particular to this header; that header, table and exports agree is tests/test_cabi_tables.py's."""
    from molecular_dynamics_neural_operator_amd import _lib
    assert set(_lib.PBC_SIGNATURES) == NAMES
    assert lib.mdno_abi_version() == 15 and lib.mdno_train_abi_version() == 1          # additive: both stay
    assert (CSRC / "pbc.h").exists() and (CSRC / "pbc.hip").exists()                   # inside the library's content hash


def test_entry_points_refuse_bad_boxes_before_device_work(lib):
    """No pointer below is a device pointer: a call that got as far as a launch would fault, not return EINVAL."""
    from molecular_dynamics_neural_operator_amd import _lib
    E = _lib.EINVAL
    for bad in BAD_BOXES:
        b = box3(*bad)
        assert lib.mdno_radius_graph_pbc(None, 1, 5, 8.0, b, None, None, None, None, 25, None, None, None) == E, bad
        assert b"box[" in lib.mdno_last_error(), bad
        assert lib.mdno_contact_maps_pbc(None, 2, 5, 8.0, b, None, None) == E and b"box[" in lib.mdno_last_error(), bad
        assert lib.mdno_forecast_score_pbc(None, None, 0, 2, 1, 5, 8.0, b, None, None, None, None, 0, None, 0, None) == E
        assert b"box[" in lib.mdno_last_error(), bad
    # a null box, and a cutoff that is no number
    assert lib.mdno_radius_graph_pbc(None, 1, 5, 8.0, None, None, None, None, None, 25, None, None, None) == E
    assert b"null box" in lib.mdno_last_error()
    assert lib.mdno_contact_maps_pbc(None, 2, 5, 8.0, None, None, None) == E
    assert lib.mdno_forecast_score_pbc(None, None, 0, 2, 1, 5, 8.0, None, None, None, None, None, 0, None, 0, None) == E
    assert lib.mdno_radius_graph_pbc(None, 1, 5, float("nan"), box3(20, 20, 20), None, None, None, None, 25, None, None, None) == E
    # L == 2 * cutoff exactly, an open axis and the all-open box pass the box check (and stop at the null pointers)
    for ok in ((16.0, 16.0, 16.0), (16.0, 0.0, 40.0), (0.0, 0.0, 0.0)):
        assert lib.mdno_radius_graph_pbc(None, 1, 5, 8.0, box3(*ok), None, None, None, None, 25, None, None, None) == E
        assert b"null pointer" in lib.mdno_last_error(), ok
    assert lib.mdno_contact_maps_pbc(None, 0, 5, 8.0, box3(16, 16, 16), None, None) == 0          # nothing to do


def _host_plan(lib, ker_in):
    """A rollout plan made of host arithmetic alone (use_graph = 0: creation touches no device): the pointers are
    made-up addresses that nothing dereferences before a run."""
    from molecular_dynamics_neural_operator_amd import _lib
    p = _lib.KernelNNParams()
    p.width, p.ker_width, p.depth, p.ker_in, p.in_width, p.out_width = 64, 128, 1, ker_in, 7, 3
    p.num_embeddings, p.embedding_dim, p.x_position_dim = 20, 4, 3
    for name in _lib.KernelNNParams._PTRS:
        setattr(p, name, 0x10000)
    M, W, N, cap = 1, 3, 10, 100
    nbytes = lib.mdno_rollout_workspace_bytes(C.byref(p), M, N, cap)
    assert nbytes > 0
    plan = C.c_void_p()
    rc = lib.mdno_rollout_plan_create(C.byref(plan), C.byref(p), 0x10000, M, W, N, 4, 0x10000, 0, 8.0, cap, 0x100000, nbytes,
                                      0x10000, 0x10000, 0, None)
    assert rc == 0 and plan, lib.mdno_last_error()
    return plan


def test_set_box_refusals(lib):
    from molecular_dynamics_neural_operator_amd import _lib
    E = _lib.EINVAL
    good = box3(16.0, 20.0, 0.0)
    assert lib.mdno_rollout_plan_set_box(None, good, 0x10000) == E and b"null plan" in lib.mdno_last_error()
    plan = _host_plan(lib, 6)
    try:
        for bad in BAD_BOXES:
            assert lib.mdno_rollout_plan_set_box(plan, box3(*bad), 0x10000) == E and b"box[" in lib.mdno_last_error(), bad
        assert lib.mdno_rollout_plan_set_box(plan, good, None) == E and b"null edge_attr" in lib.mdno_last_error()
        assert lib.mdno_rollout_plan_steps_per_launch(plan) == 0
        assert lib.mdno_rollout_plan_set_box(plan, good, 0x10000) == 0          # no captured graph: nothing to redo
        assert lib.mdno_rollout_plan_set_box(plan, good, 0x10000) == 0
        assert lib.mdno_rollout_plan_set_box(plan, None, None) == 0             # back to the plain step
        assert lib.mdno_rollout_plan_set_box(plan, box3(0, 0, 0), None) == 0    # all open = no box
    finally:
        lib.mdno_rollout_plan_destroy(plan)
    plan = _host_plan(lib, 5)
    try:
        assert lib.mdno_rollout_plan_set_box(plan, good, 0x10000) == E and b"ker_in=5" in lib.mdno_last_error()
        assert lib.mdno_rollout_plan_set_box(plan, box3(0, 0, 0), None) == 0    # no periodic axis: nothing asked of the model
    finally:
        lib.mdno_rollout_plan_destroy(plan)


def test_python_arguments_are_checked_without_a_device():
    """MdnoError with the box named, whether or not a GPU is visible: validation comes first."""
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN, construct_pairdata
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine, RolloutEngine
    pos = torch.zeros(3, 5, 3)
    model6 = KernelNN(8, 16, 1, 6, 7, 3, 20, 4)
    model5 = KernelNN(8, 16, 1, 5, 7, 3, 20, 4)
    for bad in BAD_BOXES + [(20.0, 20.0), (1.0, 2.0, 3.0, 4.0), "abc"]:
        for call in (lambda: ops.radius_graph_pbc(pos[0], 5, 8.0, bad),
                     lambda: construct_pairdata(pos, torch.zeros(5, dtype=torch.long), 8.0, box=bad),
                     lambda: forecast.contact_maps(pos, 8.0, box=bad),
                     lambda: forecast.score_forecast(pos.unsqueeze(1), pos, 8.0, box=bad),
                     lambda: RolloutEngine(model6, 1, 5, 3, 8.0, max_steps=2, box=bad),
                     lambda: GroupedRolloutEngine(model6, 2, 5, 3, 8.0, max_steps=2, box=bad)):
            with pytest.raises(MdnoError, match="box"):
                call()
    for cls in (RolloutEngine, GroupedRolloutEngine):
        with pytest.raises(MdnoError, match="ker_in=5"):
            cls(model5, 2, 5, 3, 8.0, max_steps=2, box=(16.0, 16.0, 16.0))
    assert ops.check_box(None, 8.0) is None and ops.check_box((0, 0, 0), 8.0) is None          # no periodic axis: open
    assert ops.check_box((16, 0, 40.5), 8.0) == (16.0, 0.0, 40.5)
    assert ops.check_box(torch.tensor([16.0, 17.0, 18.0]), 8.0) == (16.0, 17.0, 18.0)
    assert ops.check_box(np.array([16.0, 17.0, 18.0]), 8.0) == (16.0, 17.0, 18.0)


def test_periodic_box_frame():
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    frame, L = syn.periodic_box_frame(504, 0.1, seed=1)
    assert frame.dtype == np.float32 and frame.shape == (504, 3) and abs(L - 17.145) < 1e-3
    assert float(frame.min()) >= 0.0 and float(frame.max()) <= L
    assert np.array_equal(frame, syn.periodic_box_frame(504, 0.1, seed=1)[0])
    assert not np.array_equal(frame, syn.periodic_box_frame(504, 0.1, seed=2)[0])


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_properties():
    """What the GPU tests take from the rule, checked on the restatement alone: symmetry, bulk degree, the exact tie,
    and the large box equal to the open graph with attributes cat(pos[src], pos[dst])."""
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from test_gpu_pbc import check_condition, pbc_graph, random_frame
    pos = random_frame(65, 13.0, seed=4)
    g = pbc_graph(pos, 6.5, (13.0, 13.0, 13.0))
    check_condition(g)
    keep = np.zeros((65, 65), bool)
    keep[g["dst"], g["src"]] = True
    assert np.array_equal(keep, keep.T) and keep.diagonal().all()
    assert np.array_equal(g["dst"], np.sort(g["dst"])) and g["row_ptr"][-1] == g["src"].size
    # the source's image lies within the cutoff of the destination as stored
    d = g["attr"][:, :3].astype(np.float64) - g["attr"][:, 3:].astype(np.float64)
    assert float(np.sqrt((d * d).sum(1)).max()) < 6.5 + 1e-5
    frame, L = syn.periodic_box_frame(504, 0.1, seed=1)
    deg = pbc_graph(frame, 8.0, (L, L, L))["src"].size / 504.0
    open_deg = pbc_graph(frame, 8.0, (0.0, 0.0, 0.0))["src"].size / 504.0
    print("mean degree at 504 atoms: periodic", deg, "open", open_deg)
    assert 200.0 < deg < 230.0 and 100.0 < open_deg < 140.0          # bulk: 4/3 pi 8^3 x 0.1 + 1 = 215
    # the exact tie: x = 0.5 and 8.5, L = 16, cutoff 8 -> no edge from either side
    tie = np.array([[0.5, 1.0, 1.0], [8.5, 1.0, 1.0]], dtype=np.float32)
    t = pbc_graph(tie, 8.0, (16.0, 16.0, 16.0))
    assert t["src"].tolist() == [0, 1] and t["dst"].tolist() == [0, 1]
    # nothing wraps in a large box
    big = pbc_graph(pos, 6.5, (1e6, 1e6, 1e6))
    opn = pbc_graph(pos, 6.5, (0.0, 0.0, 0.0))
    for k in ("row_ptr", "src", "dst"):
        assert np.array_equal(big[k], opn[k])
    assert np.array_equal(big["attr"].view(np.uint32), np.concatenate([pos[big["src"]], pos[big["dst"]]], 1).view(np.uint32))
    assert big["src"].size < g["src"].size
