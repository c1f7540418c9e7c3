"""Internal coordinates without a GPU: what is particular to include/mdno_internal.h and its ctypes table (that header,
table and exports agree is tests/test_cabi_tables.py's); every refusal of the header comes back before any device work; the numpy restatement
(tests/internal_ref.py) gives the known values on known geometry and is invariant under rigid motion to first order;
forecast.Featurizer counts, names and validates on the host; discretize(featurizer=None) takes the path it always took."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import internal_ref as ref
from cabi import CSRC, INCLUDE, lib  # noqa: F401  (lib: the fixture)

HEADER = INCLUDE / "mdno_internal.h"
NAMES = {"mdnoic_features", "mdnoic_column_histogram"}
FAKE = 0x10000          # a made-up address: nothing may dereference it


def test_internal_header_table_and_exports_agree(lib):
    """What is particular to this header; that header, table and exports agree is tests/test_cabi_tables.py's."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    assert set(_lib.INTERNAL_SIGNATURES) == NAMES
    assert lib.mdno_abi_version() == _lib.ABI_VERSION and lib.mdno_train_abi_version() == _lib.TRAIN_ABI_VERSION
    assert (CSRC / "internal.hip").exists()                                                   # inside the library's content hash
    text = HEADER.read_text()
    for name, value in (("WORKGROUP", ops.IC_WORKGROUP), ("LDS_ATOMS", ops.IC_LDS_ATOMS), ("MAX_GROUP_FRAMES", ops.IC_MAX_GROUP_FRAMES),
                        ("FEATURE_CHUNK", ops.IC_FEATURE_CHUNK), ("MAX_BINS", ops.IC_MAX_BINS), ("HIST_ROWS", ops.IC_HIST_ROWS),
                        ("HIST_TABLE", ops.IC_HIST_TABLE), ("HIST_COLUMNS", ops.IC_HIST_COLUMNS)):
        assert int(re.search(rf"#define MDNO_IC_{name} (\d+)", text).group(1)) == value, name
    for name, table in (("F32", _lib.INTERNAL_DTYPES["float32"]), ("F64", _lib.INTERNAL_DTYPES["float64"]), ("RADIANS", _lib.INTERNAL_RADIANS),
                        ("FORM_AUTO", ops.IC_FORMS["auto"]), ("FORM_LDS", ops.IC_FORMS["lds"]), ("FORM_GLOBAL", ops.IC_FORMS["global"])):
        assert int(re.search(rf"#define MDNO_IC_{name} (\d+)", text).group(1)) == table, name
    # MDNO_IC_FRAMES_PER_GROUP(N) and its mirror: whole frames within IC_LDS_ATOMS atoms, 1 .. IC_MAX_GROUP_FRAMES
    assert "MDNO_IC_FRAMES_PER_GROUP(N)" in text
    top, cap = ops.IC_LDS_ATOMS, ops.IC_MAX_GROUP_FRAMES
    for n in (0, 1, 28, 63, 64, 65, 504, top // cap, top // cap + 1, top // 2, top // 2 + 1, top, top + 1, 50000):
        want = 1 if n <= 0 or top // n < 1 else min(top // n, cap)
        assert ops.ic_frames_per_group(n) == want and want * n <= max(top, n), n
    assert ops.ic_frames_per_group(28) == cap > 1                                             # a 336-byte frame is not a workgroup's work
    assert 12 * ops.IC_LDS_ATOMS <= 64 * 1024 and 4 * ops.IC_HIST_TABLE <= 64 * 1024          # static LDS of either kernel
    assert ops.IC_MAX_BINS + 2 <= ops.IC_HIST_TABLE and ops.IC_MAX_BINS == ops.MAX_HISTOGRAM_BINS
    assert "mdnoic_" in text and "prefix" in text.lower()                                     # the header says why the names differ
    src = (CSRC / "internal.hip").read_text()
    assert '#include "../../include/mdno_internal.h"' in src
    assert not re.search(r"atomicAdd\([^;]*\b(double|float)\b", src)                          # integer atomics only


def feat(lib, frames=FAKE, F=3, N=5, pairs=FAKE, P=2, triples=FAKE, A=1, quads=FAKE, T=1, box=None, flags=0, dtype=0, out=FAKE,
         form=0):
    arr = None if box is None else (C.c_double * 3)(*box)
    return lib.mdnoic_features(frames, F, N, pairs, P, triples, A, quads, T, arr, flags, dtype, out, form, None)


def hist(lib, x=FAKE, R=9, D=2, groups=1, dtype=0, lo=(0.0, 0.0), hi=(1.0, 2.0), shared=0, n_bins=4, counts=FAKE, n_nan=FAKE):
    lo = None if lo is None else (C.c_double * len(lo))(*lo)
    hi = None if hi is None else (C.c_double * len(hi))(*hi)
    return lib.mdnoic_column_histogram(x, R, D, groups, dtype, lo, hi, shared, n_bins, counts, n_nan, None)


def test_entry_points_refuse_before_device_work(lib):
    """No device pointer below is a device pointer: a call that got as far as a launch would fault, not return a code."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    E, U = _lib.EINVAL, _lib.EUNSUPPORTED
    err = lib.mdno_last_error
    for kw in ({"F": -1}, {"N": -1}, {"P": -1}, {"A": -1}, {"T": -1}, {"dtype": 2}, {"dtype": -1}, {"form": 3}, {"form": -1}, {"flags": 2},
               {"flags": -1}, {"form": 1, "N": ops.IC_LDS_ATOMS + 1}, {"box": (1.0, -1.0, 0.0)}, {"box": (float("nan"), 0.0, 0.0)},
               {"box": (float("inf"), 1.0, 1.0)}, {"P": 2 ** 31 - 1, "T": 1}):
        assert feat(lib, **kw) == E, kw
    assert feat(lib, dtype=7) == E and b"out_dtype" in err()
    assert feat(lib, form=1, N=ops.IC_LDS_ATOMS + 1) == E and b"lds form" in err()
    for kw in ({"pairs": None}, {"triples": None}, {"quads": None}, {"frames": None}, {"out": None}):
        assert feat(lib, **kw) == E and b"null pointer" in err(), kw
    assert feat(lib, F=ops.ic_frames_per_group(5) * (1 << 31)) == U and b"grid" in err()
    assert feat(lib, F=ops.ic_frames_per_group(5) * (1 << 31), dtype=3) == E                 # (the argument checks come first)
    assert feat(lib, F=0, frames=None, out=None) == 0                                         # F == 0 touches nothing
    assert feat(lib, P=0, A=0, T=0, pairs=None, triples=None, quads=None, out=None) == 0      # D == 0 likewise
    # column histogram
    for kw in ({"R": -1}, {"D": -1}, {"groups": -1}, {"D": 2 ** 30, "groups": 2}, {"dtype": 2}, {"n_bins": 0}, {"n_bins": ops.IC_MAX_BINS + 1}, {"hi": (1.0, 0.0)}, {"hi": (0.0, 1.0)},
               {"lo": (float("nan"), 0.0)}, {"hi": (1.0, float("inf"))}, {"lo": (-1e308, 0.0), "hi": (1e308, 1.0)},
               {"lo": (0.0, 0.0), "hi": (5e-324, 1.0)}):
        assert hist(lib, **kw) == E, kw
    assert hist(lib, hi=(1.0, 0.0)) == E and b"column 1" in err()
    # (a shared range reads entry 0 alone: the complaint is the missing output, which R == 0 still needs)
    assert hist(lib, R=0, x=None, hi=(1.0, 0.0), shared=1, counts=None) == E and b"null pointer" in err()
    for kw in ({"x": None}, {"lo": None}, {"hi": None}, {"counts": None}, {"n_nan": None}):
        assert hist(lib, **kw) == E and b"null pointer" in err(), kw
    assert hist(lib, R=ops.IC_HIST_ROWS * (1 << 31)) == U and b"grid" in err()
    assert hist(lib, groups=65536) == U and b"grid" in err()
    assert hist(lib, groups=0, x=None, lo=None, hi=None, counts=None, n_nan=None) == 0        # no group: touches nothing
    assert hist(lib, D=0, x=None, lo=None, hi=None, counts=None, n_nan=None) == 0             # D == 0 touches nothing


def test_the_restatement_on_known_geometry():
    f32 = lambda rows: np.array([rows], np.float32)
    # IUPAC sign: looking along j -> k, i at twelve o'clock; l at three o'clock is +90 degrees
    for l_atom, want in (((0, 1, 1), (1.0, 0.0)),      # cis: l above i
                         ((0, -1, 1), (-1.0, 0.0)),    # trans
                         ((-1, 0, 1), (0.0, 1.0)),     # +90: seen from j towards k (+z), with +y up, -x lies to the right
                         ((1, 0, 1), (0.0, -1.0))):
        x = f32([(0, 1, 0), (0, 0, 0), (0, 0, 1), l_atom])
        got = ref.features(x, quads=[(0, 1, 2, 3)])[0]
        assert got.tolist() == list(want), (l_atom, got)
        ang = float(ref.radians_longdouble(x, quads=[(0, 1, 2, 3)])[0, 0])
        assert abs(ang - math.atan2(want[1], want[0])) < 1e-15
    x = f32([(3, 0, 0), (0, 0, 0), (0, 4, 0), (0, 4, 12)])
    assert ref.features(x, pairs=[(0, 2), (2, 0), (0, 3), (1, 1)])[0].tolist() == [5.0, 5.0, 13.0, 0.0]       # 3-4-5, 5-12-13, i == j
    assert ref.features(x, triples=[(0, 1, 2), (1, 0, 2)])[0].tolist() == [0.0, 0.6]                          # a right angle; cos = 3/5
    assert float(ref.radians_longdouble(x, triples=[(0, 1, 2)])[0, 0]) == pytest.approx(math.pi / 2, abs=1e-15)
    assert ref.features(x, pairs=[(0, 1)], triples=[(0, 1, 2)], quads=[(0, 1, 2, 3)]).shape == (1, 4)
    # across a periodic face: 0.5 and 9.5 in a box of 10 are 1 apart, the vector points DOWN the axis; an open axis does not wrap
    x = f32([(0.5, 0, 0), (9.5, 0, 0), (0.5, 9.5, 0)])
    assert ref.features(x, pairs=[(0, 1)], box=(10.0, 0.0, 0.0))[0, 0] == 1.0
    assert ref.bond(x, 0, 1, *ref._box((10.0, 0.0, 0.0)))[0][0] == -1.0
    assert ref.features(x, pairs=[(0, 1), (0, 2)], box=(0.0, 0.0, 10.0))[0].tolist() == [9.0, 9.5]
    assert ref.features(x, pairs=[(0, 2)], box=(10.0, 4.0, 0.0))[0, 0] == 1.5                                 # 9.5 - 2 * 4: a non-cubic box
    # the degenerate cases of the header
    x = f32([(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 1, 0), (0, 0, 0)])
    got = ref.features(x, pairs=[(0, 5), (-1, 0)], triples=[(0, 4, 1), (0, 1, 2)], quads=[(0, 1, 2, 3), (4, 1, 2, 7)])[0]
    assert np.isnan(got[[0, 1, 2, 4, 5, 6, 7]]).all() and got[3] == -1.0
    assert np.isnan(ref.radians_longdouble(x, quads=[(0, 1, 2, 3)])[0, 0])                                    # h == 0: NaN, not atan2(0, 0)
    x = f32([(0, 0, 0), (np.nan, 0, 0), (0, 1, 0), (np.inf, 0, 0)])
    got = ref.features(x, pairs=[(0, 2), (0, 1), (0, 3), (2, 3)])[0]
    assert got[0] == 1.0 and np.isnan(got[1]) and got[2] == np.inf and got[3] == np.inf
    assert ref.features(np.zeros((0, 4, 3), np.float32), pairs=[(0, 1)]).shape == (0, 1)
    assert ref.features(np.zeros((2, 4, 3), np.float32)).shape == (2, 0)


def test_the_restatement_is_invariant_under_rigid_motion_to_first_order():
    from molecular_dynamics_neural_operator_amd.forecast import Featurizer
    rng = np.random.default_rng(5)
    N = 12
    x = np.cumsum(rng.normal(size=(6, N, 3)) * 2.0, 1).astype(np.float32)
    ft = Featurizer.backbone(N)
    args = dict(pairs=ft.pairs.tolist(), triples=ft.triples.tolist(), quads=ft.quads.tolist())
    assert ref.conditioning(x, args["triples"], args["quads"])[0] > 1e-3
    base = ref.features(x, **args)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.linalg.det(q))                                               # a proper rotation
    moved = (x.astype(np.float64) @ q.T + np.array([3.0, -2.0, 1.0])).astype(np.float32)
    got = ref.features(moved, **args)
    # the moved coordinates are rounded to fp32 (relative 2^-24 of |x| <= 64): distances move by ~1e-5 absolute at the most,
    # cosines and sines by that over the shortest bond length involved (>= ~0.1 here)
    scale = float(np.abs(moved).max())
    assert scale < 64.0
    P = len(args["pairs"])
    assert np.abs(got[:, :P] - base[:, :P]).max() < 8 * scale * 2.0 ** -24
    assert np.abs(got[:, P:] - base[:, P:]).max() < 1e-3
    mirrored = x * np.array([1, 1, -1], np.float32)                                 # a reflection flips the sine of every dihedral, exactly
    got = ref.features(mirrored, **args)
    sin_cols = [i for i, n in enumerate(ft.names()) if n.startswith("sin")]
    flip = np.ones(base.shape[1])
    flip[sin_cols] = -1.0
    assert len(sin_cols) == N - 3 and np.array_equal(got, base * flip)


@pytest.mark.parametrize("n", [4, 5, 28])
def test_backbone_counts_and_names(n):
    from molecular_dynamics_neural_operator_amd.forecast import Featurizer
    ft = Featurizer.backbone(n)
    far = sum(1 for i in range(n) for j in range(i + 3, n))
    assert ft.n_atoms == n and ft.top == n - 1 and ft.n_bonds == n - 1
    assert (ft.pairs.shape[0], ft.triples.shape[0], ft.quads.shape[0]) == (n - 1 + far, n - 2, n - 3)
    assert ft.dim() == n - 1 + far + n - 2 + 2 * (n - 3) and ft.dim(radians=True) == ft.dim() - (n - 3)
    assert all(t.dtype == torch.int32 and t.is_contiguous() for t in (ft.pairs, ft.triples, ft.quads))
    names = ft.names()
    assert len(names) == ft.dim() == len(set(names)) and len(ft.names(radians=True)) == ft.dim(radians=True)
    assert names[0] == "d 0-1" and names[n - 2] == f"d {n - 2}-{n - 1}" and names[n - 1] == "d 0-3"
    assert names[n - 1 + far] == "cos a 0-1-2" and names[-2:] == [f"cos t {n - 4}-{n - 3}-{n - 2}-{n - 1}", f"sin t {n - 4}-{n - 3}-{n - 2}-{n - 1}"]
    assert ft.names(radians=True)[-1] == f"t {n - 4}-{n - 3}-{n - 2}-{n - 1}"
    if n == 28:
        assert ft.dim() == 428
        s = Featurizer.backbone(28, 3, 4)                                          # bonds + the pairs of atoms 0, 4, ..., 24
        assert s.pairs.shape[0] == 27 + 21 and s.names()[27] == "d 0-4" and s.n_bonds == 27
        assert Featurizer.backbone(28, 5, 4).pairs.shape[0] == 27 + 21 - 6         # (0, 4), (4, 8), ... fall below 5
    two = Featurizer.distances([(3, 17)]) + Featurizer.angles(np.array([[4, 5, 6]])) + Featurizer.dihedrals(torch.tensor([[1, 2, 3, 4]]))
    assert two.names() == ["d 3-17", "cos a 4-5-6", "cos t 1-2-3-4", "sin t 1-2-3-4"] and two.n_atoms is None and two.top == 17
    both = ft + Featurizer.distances([(0, 2)], n_atoms=n)
    assert both.dim() == ft.dim() + 1 and both.names()[ft.pairs.shape[0]] == "d 0-2" and both.n_atoms == n
    assert Featurizer.backbone(3).dim() == 3 and Featurizer.backbone(1).dim() == 0 and Featurizer.backbone(0).dim() == 0


def test_featurizer_refusals_on_the_host():
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    F = forecast.Featurizer
    with pytest.raises(MdnoError, match="outside 0 .. 9"):
        F.distances([(0, 10)], n_atoms=10)
    with pytest.raises(MdnoError, match="outside 0 .. 9"):
        F.of(quads=[(0, 1, 2, 10)], n_atoms=10)
    with pytest.raises(MdnoError, match="negative"):
        F.angles([(0, -1, 2)])
    with pytest.raises(MdnoError, match="integer array"):
        F.distances(np.array([[0.0, 1.0]]))
    with pytest.raises(MdnoError, match="integer array"):
        F.dihedrals(torch.tensor([[0.0, 1.0, 2.0, 3.0]]))
    for bad, make in (([(0, 1, 2)], F.distances), ([(0, 1)], F.angles), ([(0, 1, 2)], F.dihedrals), ([0, 1], F.distances)):
        with pytest.raises(MdnoError, match="expected \\[n, "):
            make(bad)
    with pytest.raises(MdnoError, match="n_atoms 5 \\+ n_atoms 6"):
        F.backbone(5) + F.backbone(6)
    for kw in ({"n_atoms": -1}, {"n_atoms": 2.0}, {"n_atoms": 5, "min_separation": 0}, {"n_atoms": 5, "stride": 0}):
        with pytest.raises(MdnoError, match="backbone"):
            F.backbone(**kw)
    # frames of another N, before anything else is looked at (these are CPU tensors)
    ft = F.backbone(5)
    with pytest.raises(MdnoError, match="built for frames of 5 atoms, these have 6"):
        forecast.internal_coordinates(torch.zeros(2, 6, 3), ft)
    with pytest.raises(MdnoError, match="more than 17 atoms, these have 17"):
        forecast.internal_coordinates(torch.zeros(2, 1, 17, 3), F.distances([(3, 17)]))
    with pytest.raises(MdnoError, match="CPU tensor"):
        forecast.internal_coordinates(torch.zeros(2, 5, 3), ft)
    with pytest.raises(MdnoError, match="frames must be"):
        forecast.internal_coordinates(torch.zeros(5, 3), ft)
    with pytest.raises(MdnoError, match="featurizer is a"):
        forecast.internal_coordinates(torch.zeros(2, 5, 3), ft.pairs)
    with pytest.raises(MdnoError, match="CPU tensor"):
        ops.internal_features(torch.zeros(2, 5, 3), ft.pairs)
    with pytest.raises(MdnoError, match="CPU tensor"):
        forecast.feature_histograms(torch.zeros(4, 3), 0.0, 1.0, 4)
    for lo, hi, bins in ((0.0, 0.0, 4), (0.0, float("inf"), 4), ([0.0, 0.0], [1.0, 1.0], 4), (0.0, 1.0, 0), (0.0, 1.0, ops.IC_MAX_BINS + 1),
                         (0.0, 1.0, 2.5)):
        with pytest.raises(MdnoError, match="column_histogram"):
            ops.check_column_ranges(lo, hi, bins, 3)
    assert ops.check_column_ranges(0, 1, 4, 3) == ([0.0], [1.0], 4)
    assert ops.check_column_ranges(torch.tensor([0.0, 1.0, 2.0]), [1, 2, 3], 4, 3) == ([0.0, 1.0, 2.0], [1.0, 2.0, 3.0], 4)
    for form, dtype in (("tiled", torch.float32), ("auto", torch.float16)):
        with pytest.raises(MdnoError, match="expected"):
            ops.internal_features(torch.zeros(2, 5, 3), ft.pairs, form=form, dtype=dtype)


def test_feature_histograms_on_cpu_tensors():
    from molecular_dynamics_neural_operator_amd.forecast import FeatureHistograms
    x = np.array([[0.0, 5.0], [0.25, np.nan], [0.5, -1.0], [1.0, 0.0], [0.999, 0.5]])
    counts, n_nan = ref.column_histogram(x, 0.0, 1.0, 4)
    assert counts.tolist() == [[0, 1, 1, 1, 1, 1], [1, 1, 0, 1, 0, 1]] and n_nan.tolist() == [0, 1]
    assert (counts.sum(1) + n_nan == 5).all()
    a = FeatureHistograms(torch.from_numpy(counts), torch.from_numpy(n_nan), [0.0], [1.0])
    assert a.outside().tolist() == [0.2, 0.5] and a.total_variation(a).tolist() == [0.0, 0.0]
    b = FeatureHistograms(torch.tensor([[0, 5, 0, 0, 0, 0], [0, 0, 4, 0, 0, 0]]), torch.zeros(2, dtype=torch.int64), [0.0], [1.0])
    assert torch.allclose(a.total_variation(b), torch.tensor([0.8, 1.0], dtype=torch.float64), atol=1e-15)
    run = FeatureHistograms(torch.stack([a.counts, b.counts]), torch.zeros(2, 2, dtype=torch.int64), [0.0], [1.0])   # [M, D, bins + 2]
    assert run.total_variation(a).shape == (2, 2) and run.total_variation(a)[0].tolist() == [0.0, 0.0]
    assert torch.allclose(a.distribution().sum(-1), torch.ones(2, dtype=torch.float64))


def test_discretize_without_a_featurizer_takes_the_old_path(monkeypatch):
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    calls = []

    class Reached(Exception):
        pass

    def fake_superpose(frames, reference):
        calls.append(("superpose", tuple(frames.shape), tuple(reference.shape)))
        raise Reached()

    def fake_internal(frames, featurizer, box=None, radians=False, dtype=torch.float32):
        calls.append(("internal", tuple(frames.shape), featurizer.dim(), box))
        raise Reached()

    monkeypatch.setattr(forecast, "superpose", fake_superpose)
    monkeypatch.setattr(forecast, "internal_coordinates", fake_internal)
    frames = torch.zeros(6, 2, 5, 3)
    with pytest.raises(Reached):
        forecast.discretize(frames, 2)
    with pytest.raises(Reached):
        forecast.discretize(frames, 2, featurizer=None, reference=torch.ones(5, 3))
    assert calls == [("superpose", (6, 2, 5, 3), (5, 3))] * 2
    ft = forecast.Featurizer.backbone(5)
    with pytest.raises(Reached):
        forecast.discretize(frames, 2, featurizer=ft, box=(10.0, 0.0, 0.0))
    assert calls[-1] == ("internal", (6, 2, 5, 3), ft.dim(), (10.0, 0.0, 0.0))
    with pytest.raises(MdnoError, match="both given"):
        forecast.discretize(frames, 2, featurizer=ft, reference=torch.ones(5, 3))
    with pytest.raises(MdnoError, match="only used with a featurizer"):
        forecast.discretize(frames, 2, box=(10.0, 0.0, 0.0))
    d = forecast.Discretization(torch.ones(5, 3), None, torch.zeros(2, 15), torch.zeros(()))      # the four fields it always had
    assert d.featurizer is None and d.box is None and d.n_states == 2
