"""Distance-constraint projection without a GPU (include/mdno_constrain.h): the greedy colouring of
the package against the restatement's (tests/constrain_ref.py) and the colour counts it must give; what is particular
to the header and its ctypes table (that header, table and exports agree is tests/test_cabi_tables.py's); the entry points and the Python layer validate before any device work; and the
properties the restatement itself must have, since the device is held to it bit for bit (tests/test_gpu_constrain.py)."""
import re

import numpy as np
import pytest
import torch

import constrain_ref as R
from cabi import CSRC, INCLUDE, lib  # noqa: F401  (lib: the fixture)

HEADER = INCLUDE / "mdno_constrain.h"
NAMES = {"mdnocst_project", "mdnocst_rollout_plan_set_constraints"}


# ------------------------------------------------------------------------------------------------ colouring
def _valid(pairs, colours):
    seen = set()
    for (i, j), c in zip(np.asarray(pairs).tolist(), list(colours)):
        assert (i, c) not in seen and (j, c) not in seen
        seen.add((i, c))
        seen.add((j, c))


def _cases():
    from molecular_dynamics_neural_operator_amd.forecast import Featurizer
    hub = np.stack([np.zeros(70, dtype=np.int64), np.arange(1, 71)], 1)
    return [("chain", R.chain_pairs(28, second=False), 2), ("chain + (i, i+2)", R.chain_pairs(28), 4),
            ("backbone(28,3,1)", Featurizer.backbone(28, 3, 1).pairs.numpy(), 35),
            ("backbone(504,3,4)", Featurizer.backbone(504, 3, 4).pairs.numpy(), 129), ("hub", hub, 70),
            ("two atoms", np.array([[0, 1]]), 1), ("none", np.zeros((0, 2), dtype=np.int64), 0)]


def test_colouring_is_valid_deterministic_and_counts_as_stated():
    from molecular_dynamics_neural_operator_amd.forecast import DistanceConstraints, greedy_colours
    for name, pairs, n_colours in _cases():
        want = R.greedy_colours(pairs)
        got = greedy_colours(np.asarray(pairs).tolist())
        assert got == want.tolist() == greedy_colours(np.asarray(pairs).tolist()), name
        _valid(pairs, got)
        assert (max(got) + 1 if got else 0) == n_colours, name
        if len(pairs) == 0:
            continue
        dc = DistanceConstraints.of(pairs, np.arange(len(pairs)) * 0.5, np.arange(len(pairs)) * 0.5 + 1.0)
        t = dc.coloured()
        rp, rlo, rhi, rptr, order = R.colour_table(pairs, dc.lo.numpy(), dc.hi.numpy())
        assert t.n_colours == n_colours and np.array_equal(t.colour_ptr.numpy(), rptr), name
        assert t.pairs.dtype == torch.int32 and np.array_equal(t.pairs.numpy(), rp), name
        assert np.array_equal(t.lo.numpy(), rlo) and np.array_equal(t.hi.numpy(), rhi) and np.array_equal(t.order.numpy(), order)
        assert dc.coloured() is t                                        # coloured once
        for c in range(n_colours):                                       # within a colour, list order is kept
            seg = order[rptr[c]:rptr[c + 1]]
            assert np.all(np.diff(seg) > 0)


def test_constructors_concatenation_and_device_moves():
    from molecular_dynamics_neural_operator_amd.forecast import DistanceConstraints
    a = DistanceConstraints.chain(5, 3.7, 3.9)
    assert a.pairs.tolist() == [[0, 1], [1, 2], [2, 3], [3, 4]] and a.lo.tolist() == [3.7] * 4 and a.hi.tolist() == [3.9] * 4
    b = DistanceConstraints.of([[0, 2], [1, 3]], [5.0, 5.5], [float("inf"), 6.0], n_atoms=5)
    c = a + b
    assert len(c) == 6 and c.n_atoms == 5 and c.top == 4 and c.hi[4] == float("inf")
    assert c.to("cpu").pairs.tolist() == c.pairs.tolist()
    assert DistanceConstraints.chain(1, 1.0, 2.0).pairs.shape == (0, 2) and DistanceConstraints.chain(0, 1.0, 2.0).coloured().n_colours == 0
    w = DistanceConstraints.chain(3, 1.0, 1.0, weights=[1.0, 0.0, 2.0])
    assert w.weights.dtype == torch.float32 and w.coloured().weights.tolist() == [1.0, 0.0, 2.0]


def test_host_validation_raises():
    from molecular_dynamics_neural_operator_amd import forecast as F, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    DC = F.DistanceConstraints
    for bad in (lambda: DC.of([[0, 5]], 1.0, 2.0, n_atoms=5),                       # index range
                lambda: DC.of([[-1, 2]], 1.0, 2.0),
                lambda: DC.of([[2, 2]], 1.0, 2.0),                                  # i == j
                lambda: DC.of([[0, 1]], 2.0, 1.0),                                  # lo > hi
                lambda: DC.of([[0, 1]], -0.5, 1.0),                                 # negative
                lambda: DC.of([[0, 1]], float("nan"), 1.0),                         # NaN
                lambda: DC.of([[0, 1]], 1.0, float("nan")),
                lambda: DC.of([[0, 1]], float("inf"), float("inf")),
                lambda: DC.of([[0, 1], [1, 2]], [1.0, 1.0, 1.0], 2.0),              # three bounds for two pairs
                lambda: DC.of([[0.5, 1.0]], 1.0, 2.0),                              # not integers
                lambda: DC.of([[0, 1]], 1.0, 2.0, weights=[1.0, -1.0]),
                lambda: DC.of([[0, 1]], 1.0, 2.0, weights=[1.0, float("nan")]),
                lambda: DC.of([[0, 3]], 1.0, 2.0, weights=[1.0, 1.0]),              # fewer weights than atoms
                lambda: DC.chain(-1, 1.0, 2.0),
                lambda: DC.chain(4, 1.0, 2.0) + DC.chain(5, 1.0, 2.0),
                lambda: DC.chain(3, 1.0, 2.0) + DC.chain(3, 1.0, 2.0, weights=[1, 1, 1]),
                lambda: DC.from_frames(torch.zeros(2, 3, 3), [[0, 1]], margin=-1.0),
                lambda: F.project_constraints(torch.zeros(2, 4, 3), DC.chain(4, 1.0, 2.0)),          # CPU frames
                lambda: F.project_constraints(torch.zeros(2, 5, 3), DC.chain(4, 1.0, 2.0)),          # other N
                lambda: F.project_constraints(torch.zeros(2, 4, 3), [[0, 1]]),
                lambda: ops.check_projection_args(-1, 0.0), lambda: ops.check_projection_args(1.5, 0.0),
                lambda: ops.check_projection_args(8, -1e-9), lambda: ops.check_projection_args(8, float("nan"))):
        with pytest.raises(MdnoError):
            bad()
    assert ops.check_projection_args(0, 0) == (0, 0.0)


# ------------------------------------------------------------------------------------------------ header, table, exports
def test_constrain_header_table_and_exports_agree(lib):
    """What is particular to this header; that header, table and exports agree is tests/test_cabi_tables.py's."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    assert set(_lib.CONSTRAIN_SIGNATURES) == NAMES
    assert lib.mdno_abi_version() == _lib.ABI_VERSION == 15 and lib.mdno_train_abi_version() == _lib.TRAIN_ABI_VERSION == 1
    assert (CSRC / "constrain.hip").exists()                                                  # inside the library's content hash
    text = HEADER.read_text()
    const = lambda name: int(eval(re.search(rf"#define {name} (\([^)]*\)|\d+)", text).group(1)))
    assert const("MDNOCST_MAX_ATOMS") == ops.CST_MAX_ATOMS == _lib.CONSTRAIN_MAX_ATOMS >= 4096
    assert const("MDNOCST_MAX_ATOMS") * 24 + 2 * const("MDNOCST_MAX_GROUP_FRAMES") * 8 <= 160 * 1024     # the LDS of a compute unit
    assert const("MDNOCST_MAX_CONSTRAINTS") == ops.CST_MAX_CONSTRAINTS
    assert const("MDNOCST_GROUP_ATOMS") == ops.CST_GROUP_ATOMS and const("MDNOCST_MAX_GROUP_FRAMES") == ops.CST_MAX_GROUP_FRAMES
    assert [ops.cst_frames_per_group(n) for n in (0, 1, 28, 64, 65, 504, 1024, 1025, 6144)] == [1, 16, 16, 16, 15, 2, 1, 1, 1]


def test_constrain_entry_points_validate_before_device_work(lib):
    from molecular_dynamics_neural_operator_amd import _lib
    E = _lib.EINVAL
    proj = lib.mdnocst_project
    assert proj(None, None, 1, _lib.CONSTRAIN_MAX_ATOMS + 1, None, None, None, 0, None, 0, None, None, 8, 0.0, None, None, None, None) == E
    assert b"at most" in lib.mdno_last_error()
    assert proj(None, None, -1, 4, None, None, None, 0, None, 0, None, None, 8, 0.0, None, None, None, None) == E
    assert proj(None, None, 1, 4, None, None, None, 0, None, 0, None, None, -1, 0.0, None, None, None, None) == E
    assert proj(None, None, 1, 4, None, None, None, 0, None, 0, None, None, 8, -1.0, None, None, None, None) == E
    assert proj(None, None, 1, 4, None, None, None, 0, None, 0, None, None, 8, float("nan"), None, None, None, None) == E
    assert proj(None, None, 1, 4, None, None, None, 3, None, 1, None, None, 8, 0.0, None, None, None, None) == E
    assert b"null pointer" in lib.mdno_last_error()
    assert proj(None, None, 1, 4, None, None, None, _lib.CONSTRAIN_MAX_CONSTRAINTS + 1, None, 1, None, None, 8, 0.0, None, None, None, None) == E
    import ctypes as C
    bad_box = (C.c_double * 3)(-1.0, 0.0, 0.0)
    assert proj(None, None, 1, 4, None, None, None, 0, None, 0, None, bad_box, 8, 0.0, None, None, None, None) == E
    assert proj(None, None, 1, 4, None, None, None, 0, None, 0, None, None, 8, 0.0, None, None, None, None) == E      # frames, no pointer
    assert proj(None, None, 0, 4, None, None, None, 0, None, 0, None, None, 8, 0.0, None, None, None, None) == 0      # nothing to do
    assert lib.mdnocst_rollout_plan_set_constraints(None, None, None, None, 0, None, 0, None, 8, 0.0, None, None, None) == E
    assert b"null plan" in lib.mdno_last_error()


# ------------------------------------------------------------------------------------------------ the restatement
def noisy_chain(n, sigma=0.3, band=0.05):
    clean, rng = R.random_walk_chain(n, 3.8, seed=0)
    pairs = R.chain_pairs(n)
    d = R.lengths(clean, pairs)
    table = R.colour_table(pairs, d - band, d + band)
    frame = (clean + rng.normal(scale=sigma, size=clean.shape)).astype(np.float32)
    return clean, frame, table


def test_restatement_in_band_frames_come_back_bit_identical():
    clean, _, (pairs, lo, hi, ptr, _) = noisy_chain(28)
    frames = np.stack([clean.astype(np.float32), (clean + 100.0).astype(np.float32)])
    d32 = np.stack([R.lengths(f.astype(np.float64), pairs) for f in frames])
    lo, hi = d32.min(0) - 1e-3, d32.max(0) + 1e-3
    out, sweeps, vin, vout, _ = R.project(frames, pairs, lo, hi, ptr, iterations=8)
    assert np.array_equal(out.view(np.int32), frames.view(np.int32)) and not sweeps.any() and not vin.any() and not vout.any()
    # iterations = 0 measures only
    _, noisy, (pairs, lo, hi, ptr, _) = noisy_chain(28)
    out, sweeps, vin, vout, _ = R.project(noisy[None], pairs, lo, hi, ptr, iterations=0)
    assert np.array_equal(out[0].view(np.int32), noisy.view(np.int32)) and sweeps[0] == 0 and vin[0] == vout[0] > 0.1


def test_restatement_moves_the_centre_of_mass_by_rounding_only():
    _, noisy, (pairs, lo, hi, ptr, _) = noisy_chain(28)
    _, sweeps, _, _, state = R.project(noisy[None], pairs, lo, hi, ptr, iterations=8)
    shift = np.abs(state[0].mean(0) - noisy.astype(np.float64).mean(0)).max()
    print("centre of mass moved by", shift)
    # every update adds +g r to one atom and -g r to another: the sum changes by the rounding of 2 x 3 additions of
    # magnitude <= |x| ~ 60 A per constraint and sweep, ulp(64) = 1.4e-14 each, 53 constraints, 8 sweeps, mean of 28
    assert sweeps[0] == 8 and shift <= 53 * 8 * 2 * 1.5e-14


def test_restatement_keeps_a_pinned_atoms_bits():
    _, noisy, (pairs, lo, hi, ptr, _) = noisy_chain(28)
    w = np.ones(28, dtype=np.float32)
    w[[5, 6, 20]] = 0.0                                   # 5 and 6 are bonded: that constraint is skipped
    w[9] = 3.0
    out, sweeps, vin, vout, state = R.project(noisy[None], pairs, lo, hi, ptr, weights=w, iterations=8)
    assert np.array_equal(out[0][[5, 6, 20]].view(np.int32), noisy[[5, 6, 20]].view(np.int32))
    assert np.array_equal(state[0][[5, 6, 20]], noisy[[5, 6, 20]].astype(np.float64))
    assert sweeps[0] == 8 and vout[0] < vin[0]
    free, *_ = R.project(noisy[None], pairs, lo, hi, ptr, iterations=8)
    assert not np.array_equal(free[0][[5, 6, 20]], noisy[[5, 6, 20]])


def test_restatement_confines_nan_and_inf_to_their_atoms():
    _, noisy, (pairs, lo, hi, ptr, _) = noisy_chain(28)
    bad = noisy.copy()
    bad[7, 1] = np.nan
    bad[19, 0] = np.inf
    out, _, vin, vout, _ = R.project(bad[None], pairs, lo, hi, ptr, iterations=8)
    finite = np.isfinite(out[0]).all(1)
    assert not finite[7] and not finite[19] and finite.sum() == 26 and np.isfinite([vin[0], vout[0]]).all()
    assert np.array_equal(out[0][[7, 19]].view(np.int32), bad[[7, 19]].view(np.int32))


def test_restatement_converges():
    """The condition the device inherits: chain + (i, i + 2) of a 28-atom random walk with 3.8 A bonds, bands of +-0.05 A
    around the clean lengths, Gaussian noise of 0.3 A: within 256 sweeps every distance is inside its band to 1e-6, and 8
    sweeps already reduce the violation; the 3-atom chain likewise."""
    for n in (28, 3):
        _, noisy, (pairs, lo, hi, ptr, _) = noisy_chain(n)
        _, sweeps, vin, vout, state = R.project(noisy[None], pairs, lo, hi, ptr, iterations=256, tol=1e-6)
        print(f"N={n}: {int(sweeps[0])} sweeps, viol_in {vin[0]:.3g}, viol_out {vout[0]:.3g}")
        assert vout[0] <= 1e-6 and sweeps[0] < 256 and vin[0] > 0.05
        d = R.lengths(state[0], pairs.astype(np.int64))
        assert np.all(d >= lo - 1e-6) and np.all(d <= hi + 1e-6)
        _, sweeps8, vin8, vout8, _ = R.project(noisy[None], pairs, lo, hi, ptr, iterations=8, tol=1e-6)
        print(f"N={n}: after {int(sweeps8[0])} sweeps viol_out {vout8[0]:.3g}")
        assert vout8[0] < vin8[0] and sweeps8[0] <= 8


def test_restatement_under_a_box_takes_the_minimum_image():
    x = np.array([[0.5, 1.0, 1.0], [9.6, 1.0, 1.0], [9.6, 1.0, 4.0]], dtype=np.float32)      # 0-1 across the x boundary: 0.9 apart
    pairs, lo, hi, ptr, _ = R.colour_table([[0, 1], [1, 2]], [1.5, 3.0], [1.5, 3.0])
    out, sweeps, vin, vout, state = R.project(x[None], pairs, lo, hi, ptr, box=(10.0, 10.0, 0.0), iterations=50, tol=1e-9)
    assert abs(vin[0] - 0.6) < 1e-6 and vout[0] <= 1e-9 and sweeps[0] < 50
    assert state[0][0, 0] > 0.5 and state[0][1, 0] < 9.6                                       # pushed apart THROUGH the boundary
    open_, _, vin_open, _, _ = R.project(x[None], pairs, lo, hi, ptr, iterations=1)
    assert abs(vin_open[0] - 7.6) < 1e-5                                                       # without the box: 9.1 apart
