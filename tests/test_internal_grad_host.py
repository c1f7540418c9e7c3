"""The gradient of the internal coordinates without a GPU: what is particular to include/mdno_internal_grad.h and its ctypes
table (that header, table and exports agree is tests/test_cabi_tables.py's); every refusal of the header comes back before any device work;
forecast.Featurizer.incidence builds the table the header describes; the numpy restatement (tests/internal_grad_ref.py) is
held to an independent formulation — torch autograd in fp64 of a plain restatement of the FEATURES — and keeps the skip rules;
training.StructureLoss validates on the host.

THE GATE of the autograd comparison is |restatement - autograd| <= K * 2^-53 * S_abs per element, S_abs = the sum of the
absolute contributions to that element (what the rounding of a chain scales with).  K is not taken from that difference: both
sides are measured against the restatement run in long double (64-bit significand) on the SEEDS below, and K is twice the
larger of the two distances, per kind.  Measured on the CPU, in units of 2^-53 S_abs, over the seeds, open and under a box:
    distances   restatement 2.68   autograd 2.63   -> K = 5.4
    angles      restatement 31.6   autograd 152.5  -> K = 305
    dihedrals   restatement 97.3   autograd 365.3  -> K = 731
(the two against each other, for orientation: 3.1, 167.3 and 365.4; all kinds in one chain: 5.2).  S_abs counts the
contributions as they are added, not the terms inside one: next to |c| = 0.995 the two terms of di cancel to a tenth of
their size, which is where the angles' and dihedrals' figures come from.  All kinds together are held to the largest K: an
atom's chain mixes them.  The chains keep internal_ref.conditioning >= 0.05 for h and <= 0.995 for |c| (asserted); the
seeds are the first six of 0, 1, 2, ... that do, open and under the box."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import internal_grad_ref as gref
import internal_ref as ref
from cabi import CSRC, INCLUDE, lib  # noqa: F401  (lib: the fixture)

HEADER = INCLUDE / "mdno_internal_grad.h"
NAMES = {"mdnoicg_features_bwd"}
FAKE = 0x10000          # a made-up address: nothing may dereference it
SEEDS = (0, 1, 3, 6, 7, 8)
K_GATE = {"distances": 5.4, "angles": 305.0, "dihedrals": 731.0}
BOX = (7.0, 0.0, 9.5)


def test_header_table_and_exports_agree(lib):
    """What is particular to this header; that header, table and exports agree is tests/test_cabi_tables.py's."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    assert set(_lib.INTERNAL_GRAD_SIGNATURES) == NAMES
    assert len(_lib.INTERNAL_GRAD_SIGNATURES["mdnoicg_features_bwd"][1]) == 20
    assert set(_lib.INTERNAL_SIGNATURES) == {"mdnoic_features", "mdnoic_column_histogram"}    # that table stays as it is
    assert lib.mdno_abi_version() == _lib.ABI_VERSION and lib.mdno_train_abi_version() == _lib.TRAIN_ABI_VERSION
    head = (INCLUDE / "mdno.h").read_text() + (INCLUDE / "mdno_train.h").read_text()
    assert f"#define MDNO_ABI_VERSION {_lib.ABI_VERSION}" in head and f"#define MDNO_TRAIN_ABI_VERSION {_lib.TRAIN_ABI_VERSION}" in head
    assert (CSRC / "internal_grad.hip").exists() and (CSRC / "internal_rule.h").exists()      # inside the library's content hash
    text = HEADER.read_text()
    for name, value in (("MAX_ITEMS", None), ("TARGET_GROUPS", ops.ICG_TARGET_GROUPS), ("MIN_THREADS", ops.ICG_MIN_THREADS)):
        m = re.search(rf"#define MDNO_ICG_{name} (\S.*)", text)
        assert m and (value is None or int(m.group(1)) == value), name
    assert "(1 << 29)" in text and ops.ICG_MAX_ITEMS == 1 << 29 == _lib.INTERNAL_GRAD_MAX_ITEMS
    assert "mdnoicg_" in text and "THE PREFIX" in text and "is ABI" in text                  # the header says why the names differ
    assert '#include "mdno_internal.h"' in text                                               # dtypes, forms and G are that header's
    src = (CSRC / "internal_grad.hip").read_text()
    assert '#include "../../include/mdno_internal_grad.h"' in src and '#include "internal_rule.h"' in src
    assert '#include "internal_rule.h"' in (CSRC / "internal.hip").read_text()                # ONE bond / dot / cross
    assert "atomic" not in src.replace("no atomics", "")                                      # a gather: nothing is summed across threads
    # the atom chunk of the header: a training batch is not eight workgroups, a long run stages no frame twice
    assert ops.icg_atom_chunk(128, 28) == 4 and -(-28 // 4) * (128 // 16) == 56
    assert ops.icg_atom_chunk(8, 504) == 16 and ops.icg_atom_chunk(8000, 504) == 504 and ops.icg_atom_chunk(1, 1) == 1
    assert ops.icg_atom_chunk(1, 5000) == 40 and ops.icg_atom_chunk(5000, 5000) == 5000


def bwd(lib, frames=FAKE, F=3, N=5, pairs=FAKE, P=2, triples=FAKE, A=1, quads=FAKE, T=1, atom_ptr=FAKE, inc=FAKE, n_inc=7, box=None,
        flags=0, g=FAKE, g_dtype=0, grad=FAKE, grad_dtype=0, form=0):
    arr = None if box is None else (C.c_double * 3)(*box)
    return lib.mdnoicg_features_bwd(frames, F, N, pairs, P, triples, A, quads, T, atom_ptr, inc, n_inc, arr, flags, g, g_dtype, grad,
                                    grad_dtype, form, None)


def test_the_entry_point_refuses_before_device_work(lib):
    """No device pointer below is a device pointer: a call that got as far as a launch would fault, not return a code."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    E, U = _lib.EINVAL, _lib.EUNSUPPORTED
    err = lib.mdno_last_error
    for kw in ({"F": -1}, {"N": -1}, {"P": -1}, {"A": -1}, {"T": -1}, {"n_inc": -1}, {"g_dtype": 2}, {"g_dtype": -1}, {"grad_dtype": 2},
               {"grad_dtype": -1}, {"form": 3}, {"form": -1}, {"flags": 1}, {"flags": 2}, {"flags": 3}, {"flags": -1},
               {"form": 1, "N": ops.IC_LDS_ATOMS + 1}, {"P": 1 << 29, "A": 0, "T": 0}, {"P": (1 << 29) - 2, "A": 1, "T": 1},
               {"P": 2 ** 31 - 1, "A": 2 ** 31 - 1, "T": 2 ** 31 - 1}, {"box": (1.0, -1.0, 0.0)}, {"box": (float("nan"), 0.0, 0.0)},
               {"box": (float("inf"), 1.0, 1.0)}):
        assert bwd(lib, **kw) == E, kw
    assert bwd(lib, g_dtype=7) == E and b"g_dtype" in err()
    assert bwd(lib, grad_dtype=7) == E and b"grad_dtype" in err()
    assert bwd(lib, flags=1) == E and b"radians" in err() and b"not differentiable" in err()
    assert bwd(lib, flags=4) == E and b"unknown bit" in err()
    assert bwd(lib, form=1, N=ops.IC_LDS_ATOMS + 1) == E and b"lds form" in err()
    assert bwd(lib, P=1 << 29) == E and b"2^29" in err()
    for kw in ({"pairs": None}, {"triples": None}, {"quads": None}, {"atom_ptr": None}, {"inc": None}, {"frames": None}, {"g": None},
               {"grad": None}):
        assert bwd(lib, **kw) == E and b"null pointer" in err(), kw
    assert bwd(lib, P=0, A=0, T=0, pairs=None, triples=None, quads=None, g=None, inc=None, n_inc=0, grad=None) == E    # D == 0 zeros grad
    assert bwd(lib, F=ops.ic_frames_per_group(5) * (1 << 31)) == U and b"grid" in err()
    assert bwd(lib, F=ops.ic_frames_per_group(5) * (1 << 31), g_dtype=3) == E                 # (the argument checks come first)
    assert bwd(lib, F=0, frames=None, g=None, grad=None, atom_ptr=None, inc=None) == 0        # F == 0 touches nothing
    assert bwd(lib, N=0, frames=None, g=None, grad=None, atom_ptr=None, inc=None) == 0        # N == 0 likewise
    assert bwd(lib, F=0, flags=1) == E and bwd(lib, N=0, form=9) == E                         # (but is refused like any call)


# ================================================================================================ the incidence table
def test_featurizer_incidence():
    from molecular_dynamics_neural_operator_amd.forecast import Featurizer
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    # N = 1: no tuple of distinct atoms; (0, 0) names atom 0 twice
    ft = Featurizer.distances([(0, 0)], n_atoms=1)
    ptr, inc = ft.incidence(1)
    assert ptr.tolist() == [0, 2] and inc.tolist() == [0, 1] and ptr.dtype == inc.dtype == torch.int32
    assert [t.tolist() for t in Featurizer.backbone(1).incidence(1)] == [[0, 0], []]
    assert [t.tolist() for t in Featurizer.backbone(0).incidence(0)] == [[0], []]
    # N = 4: every kind, an atom (3) in the quad only, an angle that names atom 0 twice
    ft = Featurizer.of(pairs=[(0, 1), (1, 1), (2, 0)], triples=[(0, 1, 0)], quads=[(0, 1, 2, 3)], n_atoms=4)
    ptr, inc = ft.incidence(4)
    assert ptr.tolist() == [0, 5, 10, 12, 13]
    assert inc.tolist() == [0, 9, 12, 14, 16, 1, 4, 5, 13, 17, 8, 18, 19]
    want = gref.incidence(ft.pairs.tolist(), ft.triples.tolist(), ft.quads.tolist(), 4)
    assert ptr.tolist() == want[0].tolist() and inc.tolist() == want[1].tolist()
    # N = 12: the backbone set against the loop of the restatement; ascending (item, slot) within every atom; an atom in no item
    ft = Featurizer.backbone(12)
    ptr, inc = ft.incidence(12)
    want = gref.incidence(ft.pairs.tolist(), ft.triples.tolist(), ft.quads.tolist(), 12)
    assert ptr.tolist() == want[0].tolist() and inc.tolist() == want[1].tolist()
    assert int(ptr[-1]) == inc.numel() == 2 * ft.pairs.shape[0] + 3 * ft.triples.shape[0] + 4 * ft.quads.shape[0]
    for a in range(12):
        row = inc[int(ptr[a]):int(ptr[a + 1])].tolist()
        assert row == sorted(row) and len(set(row)) == len(row) and row
    lone = Featurizer.distances([(0, 2), (2, 5)])                               # (no n_atoms: any frame with more than 5 atoms)
    ptr, inc = lone.incidence(12)
    assert ptr.tolist() == [0, 1, 1, 3, 3, 3] + [4] * 7 and inc.tolist() == [0, 1, 4, 5]
    # entries whose atom is outside the frame are dropped; the rest of their tuple stays
    ptr, inc = lone.incidence(4)
    assert ptr.tolist() == [0, 1, 1, 3, 3] and inc.tolist() == [0, 1, 4]
    # cached per (n_atoms, device) on the instance; .to and + make instances without a cache
    assert lone.incidence(4)[0] is ptr and lone.incidence(4)[1] is inc and lone.incidence(12)[0] is not ptr
    assert lone.incidence(4, "cpu")[1] is inc and set(lone._incidence) == {(12, "cpu"), (4, "cpu")}
    assert lone.to("cpu")._incidence == {} and (lone + lone)._incidence == {} and lone._incidence
    for bad in (-1, 2.0, True):
        with pytest.raises(MdnoError, match="incidence"):
            lone.incidence(bad)


# ================================================================================================ the restatement
def chain(seed, N=12, F=4, box=None):
    """A seeded random-walk chain: f32 [F, N, 3]."""
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.normal(size=(F, N, 3)) * 2.0, 1).astype(np.float32)


def torch_features(x, pairs, triples, quads, box=None):
    """The FEATURES of include/mdno_internal.h as plain differentiable torch fp64 (sums of products and sqrt; no norm, cross,
    atan or clamp), x f64 [F, N, 3] -> [F, D]."""
    L = None if box is None else torch.tensor(box, dtype=torch.float64)

    def bond(a, b):
        d = x[:, b] - x[:, a]
        if L is not None:
            d = d - torch.where(L > 0, torch.round(d / torch.where(L > 0, L, torch.ones_like(L))) * L, torch.zeros_like(d))
        return d

    dot = lambda p, q: (p * q).sum(-1)
    cross = lambda p, q: torch.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2],
                                      p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], -1)
    cols = []
    for i, j in pairs:
        v = bond(i, j)
        cols.append(torch.sqrt(dot(v, v)))
    for i, j, k in triples:
        u, w = bond(j, i), bond(j, k)
        cols.append(dot(u, w) / torch.sqrt(dot(u, u) * dot(w, w)))
    for i, j, k, l in quads:
        b1, b2, b3 = bond(i, j), bond(j, k), bond(k, l)
        n1, n2 = cross(b1, b2), cross(b2, b3)
        xx, yy = dot(n1, n2), torch.sqrt(dot(b2, b2)) * dot(b1, n2)
        h = torch.sqrt(xx * xx + yy * yy)
        cols += [xx / h, yy / h]
    return torch.stack(cols, 1)


def autograd_gradient(frames, g, pairs, triples, quads, box=None):
    x = torch.from_numpy(frames.astype(np.float64)).requires_grad_()
    torch_features(x, pairs, triples, quads, box).backward(torch.from_numpy(g.astype(np.float64)))
    return x.grad.numpy()


def backbone_case(seed, kind, box=None):
    from molecular_dynamics_neural_operator_amd.forecast import Featurizer
    ft = Featurizer.backbone(12)
    pairs, triples, quads = (ft.pairs.tolist() if kind in ("distances", "all") else [], ft.triples.tolist() if kind in ("angles", "all") else [],
                             ft.quads.tolist() if kind in ("dihedrals", "all") else [])
    frames = chain(seed)
    if box is not None:
        for c, l in enumerate(box):                                                     # atoms wrapped into the periodic axes
            if l > 0:
                frames[..., c] = np.mod(frames[..., c], np.float32(l))
    g = np.random.default_rng(seed + 1000).normal(size=(frames.shape[0], len(pairs) + len(triples) + 2 * len(quads)))
    return frames, g, pairs, triples, quads


def distances_from_long_double(seed, kind, box=None):
    """(restatement, autograd) against the restatement in long double, largest over the elements, in units of 2^-53 S_abs."""
    frames, g, pairs, triples, quads = backbone_case(seed, kind, box)
    h_min, c_max = ref.conditioning(frames, triples, quads, box)
    assert h_min >= 0.05 and c_max <= 0.995, (seed, kind, h_min, c_max)
    got, s_abs = gref.features_bwd(frames, g, pairs, triples, quads, box)
    wide, _ = gref.features_bwd(frames, g, pairs, triples, quads, box, real=np.longdouble)
    auto = autograd_gradient(frames, g, pairs, triples, quads, box)
    unit = np.longdouble(2.0) ** -53 * s_abs.astype(np.longdouble)
    assert float(s_abs.min()) > 0.0
    return (float((np.abs(got - wide) / unit).max()), float((np.abs(auto - wide) / unit).max()),
            float((np.abs(got - auto) / unit.astype(np.float64)).max()))


@pytest.mark.parametrize("kind", ["distances", "angles", "dihedrals", "all"])
def test_the_restatement_equals_autograd_of_the_features(kind):
    """See the module docstring for the gate and where K comes from."""
    K = max(K_GATE.values()) if kind == "all" else K_GATE[kind]
    worst = [0.0, 0.0, 0.0]
    for seed in SEEDS:
        for box in (None, BOX):
            worst = [max(a, b) for a, b in zip(worst, distances_from_long_double(seed, kind, box))]
    print(f"{kind}: restatement {worst[0]:.3g}, autograd {worst[1]:.3g} from long double; against each other {worst[2]:.3g}; "
          f"K = {K} (units of 2^-53 S_abs)")
    assert worst[2] <= K


def test_a_wrong_sign_or_a_swapped_slot_is_far_outside_the_gate():
    """The gate has teeth: the gradient with two atoms' rows exchanged, or one negated, misses it by many orders."""
    frames, g, pairs, triples, quads = backbone_case(SEEDS[0], "all")
    got, s_abs = gref.features_bwd(frames, g, pairs, triples, quads)
    auto = autograd_gradient(frames, g, pairs, triples, quads)
    unit = 2.0 ** -53 * s_abs
    for wrong in (got[:, ::-1], -got, got * (1 + 1e-9)):
        assert float((np.abs(wrong - auto) / unit).max()) > 1e4 * max(K_GATE.values())
    assert float(np.abs(got).max()) > 1.0


def test_the_skip_rules():
    # a collinear quad (j, k, l on a line: n2 = 0 exactly): g = 0 gives 0, anything else a non-finite value on all four atoms
    step = np.array([0.5, 1.25, -0.75], np.float32)
    x = np.zeros((2, 5, 3), np.float32)
    x[:, 0] = (0.0, 1.0, 0.0)
    x[:, 1] = (1.0, -2.0, 0.5)
    x[:, 2], x[:, 3] = x[:, 1] + step, x[:, 1] + 2 * step
    x[:, 4] = (3.0, 3.0, 3.0)
    quads = [(0, 1, 2, 3)]
    assert np.isnan(ref.features(x, quads=quads)).all()
    g = np.array([[0.0, -0.0], [0.5, 0.0]])
    grad, s_abs = gref.features_bwd(x, g, quads=quads)
    assert (grad[0] == 0.0).all() and not np.signbit(grad[0]).any() and (s_abs[0] == 0.0).all()
    assert not np.isfinite(grad[1, :4]).any() and (grad[1, 4] == 0.0).all()
    g[1] = (0.0, np.nan)                                                                 # a NaN g is not zero
    assert np.isnan(gref.features_bwd(x, g, quads=quads)[0][1, :4]).all()
    # a straight angle's gradient is finite (c = -1, di = dk = 0 up to rounding); a zero-length bond is 0 / 0
    grad, _ = gref.features_bwd(x, np.array([[1.0, 1.0]] * 2), triples=[(1, 2, 3), (1, 1, 4)])
    assert np.isnan(grad[:, 1]).all() and np.isnan(grad[:, 4]).all() and np.isfinite(grad[:, [2, 3]]).all()
    # r == 0: the pair (i, i) and two atoms at one place contribute nothing; the other pair of the same atoms counts
    x[:, 4] = x[:, 0]
    g = np.array([[2.0, 3.0, 1.0]] * 2)
    grad, s_abs = gref.features_bwd(x, g, pairs=[(2, 2), (0, 4), (0, 1)])
    assert (grad[:, [2, 3, 4]] == 0.0).all() and (s_abs[:, [2, 3, 4]] == 0.0).all()
    want = (x[0, 1].astype(np.float64) - x[0, 0]) / np.linalg.norm(x[0, 1].astype(np.float64) - x[0, 0])
    assert np.allclose(grad[0, 1], want, rtol=1e-15, atol=0) and np.array_equal(grad[:, 0], -grad[:, 1])
    # an index outside the frame: the item contributes nothing, to the atoms inside it either
    grad, _ = gref.features_bwd(x, np.ones((2, 2)), pairs=[(0, 5)], triples=[(0, 1, -1)])
    assert (grad == 0.0).all()
    # f32 g is converted on load: the same as its f64 value
    g32 = np.random.default_rng(3).normal(size=(2, 2)).astype(np.float32)
    a, _ = gref.features_bwd(x, g32, quads=[(4, 1, 2, 0)])
    b, _ = gref.features_bwd(x, g32.astype(np.float64), quads=[(4, 1, 2, 0)])
    assert np.array_equal(a, b)


def test_a_wrong_table_is_walked_as_the_header_says():
    frames, g, pairs, triples, quads = backbone_case(SEEDS[1], "all")
    good = gref.incidence(pairs, triples, quads, 12)
    base, _ = gref.features_bwd(frames, g, pairs, triples, quads)
    assert np.array_equal(gref.features_bwd(frames, g, pairs, triples, quads, table=good)[0], base)
    items = len(pairs) + len(triples) + len(quads)
    ptr, inc = good[0].copy(), good[1].copy()
    lo0, hi0 = int(ptr[0]), int(ptr[1])
    inc[lo0] = 4 * items                                                               # an item out of range
    inc[lo0 + 1] = -3                                                                  # a negative entry
    inc[lo0 + 2] = int(good[1][int(ptr[5])])                                           # a slot that names another atom
    ptr[-1] = len(inc) + 1000                                                          # a range past the table
    ptr[3] = -7                                                                        # (atom 2 ends, atom 3 starts, before it)
    got, _ = gref.features_bwd(frames, g, pairs, triples, quads, table=(ptr, inc))
    keep = [a for a in range(12) if a not in (0, 2, 3)]
    assert np.array_equal(got[:, keep], base[:, keep])                                  # the entries that are right still count
    assert not np.array_equal(got[:, 0], base[:, 0]) and np.isfinite(got).all() and (got[:, 2] == 0.0).all()
    assert hi0 - lo0 > 3


# ================================================================================================ StructureLoss on the host
def test_structure_loss_refusals_on_the_host():
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import StructureLoss
    base = LpLoss(size_average=False)
    ft = forecast.Featurizer.backbone(5)
    with pytest.raises(MdnoError, match="no n_atoms"):
        StructureLoss(base, forecast.Featurizer.distances([(0, 1)]))
    with pytest.raises(MdnoError, match="featurizer is a"):
        StructureLoss(base, ft.pairs)
    with pytest.raises(MdnoError, match="base is a"):
        StructureLoss(None, ft)
    for bad in (-1.0, float("nan"), (1.0, 2.0), (1.0, 2.0, -3.0), "much"):
        with pytest.raises(MdnoError, match="weight"):
            StructureLoss(base, ft, weight=bad)
    with pytest.raises(MdnoError):
        StructureLoss(base, ft, box=(1.0, -1.0, 0.0))
    loss = StructureLoss(base, ft, weight=(1.0, 0.0, 2.5), box=(0.0, 0.0, 0.0))
    assert loss.weight == (1.0, 0.0, 2.5) and loss.box is None and hasattr(loss, "rel_with_mse")
    # an LpLoss with its base's reduction (what DataParallelTrainer asks of a loss); p = None over any other base
    assert isinstance(loss, LpLoss) and (loss.d, loss.p, loss.reduction, loss.size_average) == (2, 2, True, False)
    assert StructureLoss(LpLoss(size_average=True), ft).size_average is True and StructureLoss(lambda a, b: a, ft).p is None
    with pytest.raises(MdnoError, match="abs"):
        loss.abs(torch.zeros(2, 15), torch.zeros(2, 15))
    with pytest.raises(MdnoError, match=r"expected \[B, 15\]"):
        loss(torch.zeros(2, 18), torch.zeros(2, 18))
    with pytest.raises(MdnoError, match="CPU tensor"):                                  # no CPU fallback
        loss.structure(torch.zeros(2, 15), torch.zeros(2, 15))
    # weight 0 IS the base: nothing else is evaluated (these are CPU tensors)
    zero = StructureLoss(lambda out, y: (out - y).abs().sum(), ft, weight=0.0)
    out, y = torch.ones(2, 15, requires_grad=True), torch.zeros(2, 15)
    assert float(zero(out, y).detach()) == 30.0 and zero.structure(out, y) is None
    l, mse = zero.rel_with_mse(out, y)
    assert float(l.detach()) == 30.0 and float(mse) == 1.0
    # radians has no gradient: refused where the frames require grad, before the device is looked at
    with pytest.raises(MdnoError, match="not differentiable"):
        forecast.internal_coordinates(torch.zeros(2, 5, 3, requires_grad=True), ft, radians=True)
    with torch.no_grad(), pytest.raises(MdnoError, match="CPU tensor"):                 # (grad mode off: the old path, the old refusal)
        forecast.internal_coordinates(torch.zeros(2, 5, 3, requires_grad=True), ft, radians=True)
    for args in ((torch.zeros(2, 5, 3), torch.zeros(2, 4), ft.pairs, None, None, torch.zeros(6, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)),):
        with pytest.raises(MdnoError, match="CPU tensor"):
            from molecular_dynamics_neural_operator_amd import ops
            ops.internal_features_bwd(*args)
