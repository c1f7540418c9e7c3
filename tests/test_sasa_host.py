"""The solvent-accessible surface without a GPU: the numpy restatement of include/mdno_surface.h (tests/sasa_ref.py) against
the closed form for two spheres and against cases known by hand, `forecast.Spheres` and the arithmetic of
`forecast.SurfaceArea` on CPU tensors, and every refusal that happens before the library is loaded."""
import math

import numpy as np
import pytest
import torch

import sasa_ref as R
from molecular_dynamics_neural_operator_amd import _lib
from molecular_dynamics_neural_operator_amd import forecast as F
from molecular_dynamics_neural_operator_amd import ops
from molecular_dynamics_neural_operator_amd._lib import MdnoError

NAMES = {"mdnosa_workspace_bytes", "mdnosa_exposed_points"}


def test_the_table_of_the_header_is_pinned():
    assert set(_lib.SURFACE_SIGNATURES) == NAMES
    assert ("mdno_surface.h", _lib.SURFACE_SIGNATURES) in _lib.TABLES
    assert (ops.SA_MAX_POINTS, ops.SA_STAGED_ATOMS, ops.SA_TILE, ops.SA_CHUNK) == (1024, 2048, 256, 64)


# ================================================================================================ the closed form
DIRECTIONS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (2.0 / 3.0, -1.0 / 3.0, 2.0 / 3.0))
RADII = ((3.0, 3.0), (2.6, 3.4), (3.4, 2.6))          # (R_i, R_j): equal, the smaller and the larger sphere looked at
SWEEP = 41                                            # distances per pair of radii and direction


def worst_cap_error(P):
    """The largest |count - P * exposed fraction| of sphere i, in points, over the sweep: for every pair of radii and every
    direction, SWEEP distances evenly spaced strictly inside the overlapping range |R_i - R_j| < d < R_i + R_j."""
    U = F.golden_spiral(P).numpy()
    assert np.array_equal(U, R.golden_spiral(P))
    worst = 0.0
    for Ri, Rj in RADII:
        lo, hi = abs(Ri - Rj), Ri + Rj
        for d in lo + (hi - lo) * (np.arange(SWEEP) + 0.5) / SWEEP:
            for u in DIRECTIONS:
                x = np.array([[0.0, 0.0, 0.0], [d * u[0], d * u[1], d * u[2]]], dtype=np.float32)
                dd = float(np.sqrt((x[1].astype(np.float64) ** 2).sum()))          # the distance the fp32 frame holds
                counts, _, _ = R.frame_counts(x, np.array([Ri, Rj]), U)
                worst = max(worst, abs(counts[0] - P * R.cap_exposed_fraction(dd, Ri, Rj)))
    return worst


MEASURED = {96: 2.87, 960: 5.71}          # worst_cap_error(P) with the shipped golden spiral, rounded up to 0.01


@pytest.mark.parametrize("P", [96, 960])
def test_the_restatement_against_the_analytic_cap(P):
    """Two spheres at distance d: the buried fraction of sphere i is h / (2 R_i), h = R_i - (d^2 + R_i^2 - R_j^2) / (2 d);
    for equal radii the exposed fraction is (1 + d / 2R) / 2.  The count of the restatement with the shipped golden-section
    spiral stays within the error MEASURED against that formula — 2.87 points of 96 and 5.71 of 960 over 3 pairs of radii
    x 5 directions x 41 distances — plus one point; the computation is deterministic, the extra point only covers a libm
    whose sin / cos differ in the table's last bit."""
    assert R.cap_exposed_fraction(3.0, 3.0, 3.0) == (1.0 + 3.0 / 6.0) / 2.0
    worst = worst_cap_error(P)
    print(f"P={P}: worst cap error {worst:.4f} points")
    assert worst <= MEASURED[P] + 1.0


# ================================================================================================ known cases
def test_an_isolated_atom_is_fully_exposed_and_a_contained_one_fully_buried():
    sp = F.Spheres([1.6, 1.6], probe=1.4)
    assert sp.R.tolist() == [1.6 + 1.4] * 2 and sp.n_points == 96
    far = np.array([[0.0, 0.0, 0.0], [100.0, 0.0, 0.0]], dtype=np.float32)
    counts, m_point, m_pair = R.frame_counts(far, sp.R.numpy(), sp.points.numpy())
    assert counts.tolist() == [96, 96] and m_point == np.inf and m_pair == 100.0 - 6.0
    area = F.SurfaceArea(torch.from_numpy(counts)[None], sp.R, 96)
    assert area.per_atom().tolist() == [[4.0 * math.pi * (3.0 * 3.0)] * 2]
    inside = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]], dtype=np.float32)
    counts, _, _ = R.frame_counts(inside, np.array([1.0, 4.0]), sp.points.numpy())
    assert counts[0] == 0 and counts[1] == 96          # |q - d| <= 1.5 < 4 everywhere; the large one sticks out all round
    one, _, _ = R.frame_counts(far[:1], np.array([3.0]), sp.points.numpy())
    assert one.tolist() == [96]
    nan = far.copy()
    nan[1, 1] = np.nan
    counts, _, _ = R.frame_counts(nan, sp.R.numpy(), sp.points.numpy())
    assert counts.tolist() == [96, -1]


def test_the_restatement_under_a_box_takes_the_minimum_image():
    U = R.golden_spiral(64)
    x = np.array([[1.0, 5.0, 5.0], [19.0, 5.0, 5.0]], dtype=np.float32)          # 18 apart, 2 through the wall of a 20 box
    Rr = np.array([3.0, 3.0])
    assert R.frame_counts(x, Rr, U)[0].tolist() == [64, 64]
    wrapped, _, _ = R.frame_counts(x, Rr, U, (20.0, 0.0, 0.0))
    near, _, _ = R.frame_counts(np.array([[1.0, 5.0, 5.0], [-1.0, 5.0, 5.0]], dtype=np.float32), Rr, U)
    assert wrapped.tolist() == near.tolist() and 0 < wrapped[0] < 64


# ================================================================================================ Spheres
def test_spheres_hold_expanded_radii_the_table_and_the_reach():
    sp = F.Spheres([1.2, 2.0, 1.7], probe=1.4, n_points=64)
    assert sp.R.dtype == torch.float64 and sp.R.tolist() == [1.2 + 1.4, 2.0 + 1.4, 1.7 + 1.4]
    assert sp.reach == 2.0 * (2.0 + 1.4) and sp.n_atoms == 3 and sp.points.shape == (64, 3) and sp.points.dtype == torch.float64
    assert np.array_equal(sp.points.numpy(), R.golden_spiral(64))
    assert np.allclose(np.linalg.norm(R.golden_spiral(96), axis=1), 1.0, atol=1e-15)
    same = F.Spheres(1.5, probe=0.0, n_atoms=4)
    assert same.R.tolist() == [1.5] * 4 and same.reach == 3.0 and same.probe == 0.0
    assert F.Spheres(torch.tensor([1.0, 2.0], dtype=torch.float32)).R.tolist() == [2.4, 3.4]
    table = [[1.0, 0.0, 0.0], [0.0, 2.0, 0.0]]
    custom = F.Spheres([1.0], points=table)
    assert custom.points.tolist() == table and custom.n_points == 2
    assert sp.to("cpu") is sp
    sp.check_frames(3)
    with pytest.raises(MdnoError, match="built for frames of 3"):
        sp.check_frames(4)
    assert F.Spheres([], probe=1.4).reach == 0.0


@pytest.mark.parametrize("kw", [dict(radii=[1.0, 0.0]), dict(radii=[1.0, -1.0]), dict(radii=[float("nan")]), dict(radii=[float("inf")]),
                                dict(radii="a"), dict(radii=1.5), dict(radii=[[1.0]]), dict(radii=[1.0], n_atoms=2),
                                dict(radii=[1.0], probe=-0.1), dict(radii=[1.0], probe=float("nan")), dict(radii=[1.0], probe=float("inf")),
                                dict(radii=[1.0], probe="x"), dict(radii=[1.0], n_points=0), dict(radii=[1.0], n_points=1025),
                                dict(radii=[1.0], n_points=9.5), dict(radii=[1.0], points=[[1.0, 0.0]]), dict(radii=[1.0], points=[]),
                                dict(radii=[1.0], points=[[0.0, 0.0, float("nan")]]), dict(radii=[1.0], points=[[0.0, 0.0, 1.0]] * 1025),
                                dict(radii=[1e308], probe=1e308)])
def test_spheres_refuse(kw):
    with pytest.raises(MdnoError):
        F.Spheres(**kw)


# ================================================================================================ SurfaceArea, by hand
def hand_area():
    counts = torch.tensor([[[4, 2, 0], [4, 4, -1]], [[2, 2, 2], [0, 4, 4]]], dtype=torch.int32)          # [S=2, M=2, N=3], P = 4
    return F.SurfaceArea(counts, torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64), 4)


def test_per_atom_total_and_burial_with_nan_for_minus_one():
    a = hand_area()
    pa = a.per_atom()
    k = 4.0 * math.pi
    assert pa.shape == (2, 2, 3) and pa[0, 0].tolist() == [k * 1.0, k * 4.0 * 0.5, 0.0] and pa[1, 1].tolist() == [0.0, k * 4.0, k * 0.25]
    assert torch.isnan(pa[0, 1, 2]) and int(torch.isnan(pa).sum()) == 1
    tot = a.total()
    assert tot.shape == (2, 2) and tot[0, 0] == k * 1.0 + k * 2.0 and torch.isnan(tot[0, 1]) and not torch.isnan(tot[1]).any()
    b = a.burial()
    assert b[0, 0].tolist() == [0.0, 0.5, 1.0] and torch.isnan(b[0, 1, 2]) and b[1, 1].tolist() == [1.0, 0.0, 0.0]
    m = a.mean()
    assert m.shape == (2, 3) and m[0].tolist() == [k * 0.75, k * 4.0 * 0.5, k * 0.25 * 0.25] and torch.isnan(m[1, 2])
    assert a.mean_burial()[0].tolist() == [0.25, 0.5, 0.75]


def test_per_group_sums_the_atoms_of_a_residue():
    a = hand_area()
    g = a.per_group([1, 1, 0], 3)
    k = 4.0 * math.pi
    assert g.shape == (2, 2, 3) and g[0, 0].tolist() == [0.0, k * 1.0 + k * 2.0, 0.0]
    assert torch.isnan(g[0, 1, 0]) and g[0, 1, 1] == k * 1.0 + k * 4.0 and g[0, 1, 2] == 0.0
    assert torch.equal(a.per_group(torch.tensor([0, 0, 0]), 1)[1], a.total()[1, :, None])
    for index, n in (([0, 1], 2), ([0, 1, 2], 2), ([0, -1, 0], 2), ([0.0, 1.0, 0.0], 2), ([0, 1, 0], -1)):
        with pytest.raises(MdnoError):
            a.per_group(index, n)


def test_cat_cpu_and_difference():
    a = hand_area()
    two = F.SurfaceArea.cat([a, a])
    assert two.counts.shape == (2, 4, 3) and torch.equal(two.counts[:, 2:], a.counts) and two.n_points == 4 and two.R is a.R
    assert torch.equal(two.cpu().counts, two.counts)
    run = F.SurfaceArea(torch.tensor([[[4, 0, 2]], [[4, 0, 2]]], dtype=torch.int32), a.R, 4)          # burial 0, 1, 0.5
    truth = F.SurfaceArea(torch.tensor([[[4, 4, 4]], [[4, 0, 0]]], dtype=torch.int32), a.R, 4)        # mean burial 0, 0.5, 0.5
    d = run.difference(truth)
    assert d.shape == (1,) and d[0] == math.sqrt((0.0 + 0.25 + 0.0) / 3.0)
    assert run.difference(run).tolist() == [0.0]
    both = F.SurfaceArea.cat([run, truth]).difference(truth)
    assert both.tolist() == [d[0].item(), 0.0]
    assert torch.isnan(a.difference(a)[1]) and a.difference(a)[0] == 0.0
    with pytest.raises(MdnoError, match="other is a"):
        run.difference(truth.counts)
    with pytest.raises(MdnoError, match="mean burials of shape"):
        run.difference(F.SurfaceArea(torch.zeros((2, 1, 2), dtype=torch.int32), a.R[:2], 4))


# ================================================================================================ refusals, library not loaded
def test_every_refusal_happens_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were refused")
    monkeypatch.setattr(_lib, "load", no_load)
    sp = F.Spheres([1.6, 1.6, 1.6])
    x = torch.zeros((4, 2, 3, 3))
    with pytest.raises(MdnoError, match=r"frames is a CPU tensor: the kernels run on the GPU only \(no CPU fallback exists\)"):
        F.surface_area(x, sp)
    with pytest.raises(MdnoError, match=r"frames is a CPU tensor: the kernels run on the GPU only \(no CPU fallback exists\)"):
        ops.exposed_points(x, sp.R, sp.points, reach=sp.reach)
    for box in ((11.9, 0.0, 0.0), (12.0, 12.0), (12.0, -1.0, 0.0), (float("nan"), 0.0, 0.0)):          # reach = 6: 12 is the least
        with pytest.raises(MdnoError):
            F.surface_area(x, sp, box=box)
        with pytest.raises(MdnoError):
            ops.check_surface_args(sp.reach, box)
    assert ops.check_surface_args(6, (12.0, 0.0, 0.0), "tiled") == (6.0, (12.0, 0.0, 0.0), 2)
    with pytest.raises(MdnoError, match="form 'staged'"):
        F.surface_area(x, sp, form="staged")
    for reach in (0.0, -1.0, float("inf"), float("nan"), "a"):
        with pytest.raises(MdnoError, match="reach"):
            ops.check_surface_args(reach)
    with pytest.raises(MdnoError, match="built for frames of 3 atoms, these have 4"):
        F.surface_area(torch.zeros((4, 2, 4, 3)), sp)
    with pytest.raises(MdnoError, match="spheres is a"):
        F.surface_area(x, [1.6, 1.6, 1.6])
    for bad in (torch.zeros(3), torch.zeros((2, 3, 2)), "frames"):
        with pytest.raises(MdnoError):
            F.surface_area(bad, sp)
    with pytest.raises(MdnoError):                                # P outside 1 .. 1,024 is refused where the table is given
        F.Spheres([1.6] * 3, points=np.zeros((1025, 3)))


def test_the_engines_refuse_before_a_view_is_handed_out():
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine, RolloutEngine, _ProducedFrames

    class NoFrames(_ProducedFrames):
        box, threshold, M = (13.0, 0.0, 0.0), 8.0, 3

        def _member_views(self, first_step, steps):
            raise AssertionError("the frames were asked for before the arguments were checked")

    eng = NoFrames()
    with pytest.raises(MdnoError, match="spheres is a"):
        eng.surface_area([1.6])
    with pytest.raises(MdnoError, match="2 \\* cutoff"):
        eng.surface_area(F.Spheres([2.0], probe=1.4))             # reach 6.8: the engine's box of 13 < 13.6
    with pytest.raises(AssertionError, match="before the arguments"):
        eng.surface_area(F.Spheres([1.8], probe=1.4))             # reach 6.4
    assert RolloutEngine.surface_area is GroupedRolloutEngine.surface_area
    assert "surface_area" not in vars(RolloutEngine) and "surface_area" not in vars(GroupedRolloutEngine)
    assert (RolloutEngine.surface_area.__doc__ or "").strip()
