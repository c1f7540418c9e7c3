"""Distributional scoring without a GPU: what is particular to include/mdno_observe.h and its ctypes table (that
header, table and exports agree is tests/test_cabi_tables.py's); every refusal of the header comes back as MDNO_EINVAL (the LDS form with too
many atoms as MDNO_EUNSUPPORTED), or is raised as MdnoError, before any device work; the numpy restatement of the rule
(tests/observe_ref.py) has the properties the GPU tests lean on; and the arithmetic of forecast.PairHistogram holds
against closed forms."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import observe_ref as ref
from cabi import CSRC, lib  # noqa: F401  (lib: the fixture)

NAMES = {"mdno_pair_histogram_workspace_bytes", "mdno_pair_histogram", "mdno_radius_of_gyration"}
BAD_BOXES = [(15.9, 20.0, 20.0), (20.0, 20.0, 1e-3), (-1.0, 20.0, 20.0), (20.0, float("nan"), 20.0),
             (20.0, 20.0, float("inf")), (-0.5, 0.0, 0.0)]
FAKE = 0x10000          # a made-up address: nothing may dereference it


def box3(*v):
    return (C.c_double * 3)(*v)


def test_observe_header_table_and_exports_agree(lib):
    """What is particular to this header; that header, table and exports agree is tests/test_cabi_tables.py's."""
    from molecular_dynamics_neural_operator_amd import _lib
    assert set(_lib.OBSERVE_SIGNATURES) == NAMES
    assert lib.mdno_abi_version() == 15 == _lib.ABI_VERSION and lib.mdno_train_abi_version() == 1          # additive: both stay
    assert (CSRC / "observe.hip").exists()                                             # inside the library's content hash


def hist(lib, frames=FAKE, F=2, N=5, r_max=8.0, n_bins=7, box=None, counts=FAKE, form=0, ws=None, ws_bytes=0):
    return lib.mdno_pair_histogram(frames, F, N, r_max, n_bins, box, counts, form, ws, ws_bytes, None)


def test_entry_points_refuse_before_device_work(lib):
    """No pointer below is a device pointer: a call that got as far as a launch would fault, not return a code."""
    from molecular_dynamics_neural_operator_amd import _lib
    E = _lib.EINVAL
    for n_bins in (0, -1, 4097, 1 << 20):
        assert hist(lib, n_bins=n_bins) == E and b"n_bins" in lib.mdno_last_error(), n_bins
    for r_max in (0.0, -8.0, float("nan"), float("inf"), -float("inf")):
        assert hist(lib, r_max=r_max) == E and b"r_max" in lib.mdno_last_error(), r_max
    for bad in BAD_BOXES:
        assert hist(lib, box=box3(*bad)) == E and b"box[" in lib.mdno_last_error(), bad
    assert hist(lib, r_max=8.5, box=box3(16.9, 17.0, 17.0)) == E and b"box[0]" in lib.mdno_last_error()   # L < 2 * r_max
    assert hist(lib, frames=None) == E and b"null pointer" in lib.mdno_last_error()
    assert hist(lib, counts=None) == E and b"null pointer" in lib.mdno_last_error()
    assert hist(lib, counts=None, N=0) == E                                    # rows of zeros still need somewhere to go
    for form in (-1, 3):
        assert hist(lib, form=form) == E and b"form" in lib.mdno_last_error()
    assert hist(lib, F=-1) == E and hist(lib, N=-1) == E
    # a workspace smaller than stated (today neither form states any: the refusal cannot arise, the size is consistent)
    for form in (0, 1, 2):
        need = lib.mdno_pair_histogram_workspace_bytes(2, 5, 7, form)
        assert need == lib.mdno_pair_histogram_workspace_bytes(2, 50000, 4096, form) == 0
        if need:
            assert hist(lib, form=form, ws=FAKE, ws_bytes=need - 1) == E and b"workspace" in lib.mdno_last_error()
    # the LDS form holds 2,048 atoms
    assert hist(lib, N=2049, form=1) == _lib.EUNSUPPORTED and b"2048" in lib.mdno_last_error()
    # nothing to do: no frame is looked at, whatever the pointers
    assert hist(lib, F=0) == 0 and hist(lib, F=0, frames=None, counts=None) == 0
    assert hist(lib, F=0, box=box3(16.0, 16.0, 0.0)) == 0 and hist(lib, F=0, form=2) == 0
    assert hist(lib, F=0, n_bins=0) == E                                       # (arguments are checked first)
    assert lib.mdno_radius_of_gyration(FAKE, 0, 5, FAKE, None) == 0
    assert lib.mdno_radius_of_gyration(None, 0, 5, None, None) == 0
    assert lib.mdno_radius_of_gyration(None, 2, 5, FAKE, None) == E and b"null pointer" in lib.mdno_last_error()
    assert lib.mdno_radius_of_gyration(FAKE, 2, 5, None, None) == E
    assert lib.mdno_radius_of_gyration(FAKE, -1, 5, FAKE, None) == E


def test_python_arguments_are_checked_without_a_device():
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    x = torch.zeros(3, 5, 3)
    with pytest.raises(MdnoError, match="CPU tensor"):
        ops.pair_histogram(x, 8.0, 7)
    with pytest.raises(MdnoError, match="CPU tensor"):
        forecast.pair_histogram(x, 8.0, 7, box=(16.0, 16.0, 16.0))
    with pytest.raises(MdnoError, match="CPU tensor"):
        ops.radius_of_gyration(x)
    with pytest.raises(MdnoError, match="CPU tensor"):
        forecast.radius_of_gyration(x)
    for n_bins in (0, -3, 4097, 2.5):
        with pytest.raises(MdnoError, match="n_bins"):
            ops.pair_histogram(x, 8.0, n_bins)
        with pytest.raises(MdnoError, match="n_bins"):
            forecast.pair_histogram(x, 8.0, n_bins)
    for r_max in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(MdnoError, match="r_max"):
            ops.pair_histogram(x, r_max, 7)
    for bad in BAD_BOXES + [(20.0, 20.0), "abc"]:
        with pytest.raises(MdnoError, match="box"):
            ops.pair_histogram(x, 8.0, 7, box=bad)
    with pytest.raises(MdnoError, match="form"):
        ops.pair_histogram(x, 8.0, 7, form="fast")
    assert ops.check_histogram_args(8, 7, (0, 0, 0)) == (8.0, 7, None)
    assert ops.check_histogram_args(8.55, 4096, (17.1, 17.1, 0)) == (8.55, 4096, (17.1, 17.1, 0.0))
    # g(r) needs a bulk density: a slab or an open system has none
    counts = torch.ones(4, dtype=torch.int64)
    for box in (None, (17.1, 17.1, 0.0)):
        with pytest.raises(MdnoError, match=r"distribution\(\)"):
            forecast.PairHistogram(counts, 8.0, 4, 10, box).rdf()


# ------------------------------------------------------------------------------------------------ the restatement
def frames(N, seed=1, F=1):
    rng = np.random.default_rng(seed)
    return ((rng.random((F, N, 3)) * 1.5 - 0.2) * 17.1).astype(np.float32)


def test_restatement_properties():
    """Symmetry under swapping i and j bit for bit, the contact identity against a numpy contact count, rows that
    count every pair below r_max once, and the hand-made edge cases."""
    x = frames(65)[0]
    for box in (None, (17.1, 17.1, 17.1), (17.1, 17.1, 0.0)):
        r = ref.pair_distances(x, box)
        assert np.array_equal(r.view(np.int64), r.T.view(np.int64))
        assert np.array_equal(ref.histogram(x, 8.0, 7, box), ref.histogram(x[::-1], 8.0, 7, box))      # any order of atoms
        contacts = int((r < 8.0).sum())                                        # ordered pairs, diagonal included
        h = ref.histogram(x, 8.0, 7, box)
        assert 2 * int(h.sum()) + 65 == contacts == ref.contact_count(x, 8.0, box)
        assert int(ref.histogram(x, 8.0, 1, box)[0]) == int(h.sum())
        fine = ref.histogram(x, 8.0, 7 * 16, box)
        assert np.array_equal(fine.reshape(7, 16).sum(1), h) or ref.margin(x, 8.0, 7, box) < 1e-12
    # faces add pairs
    assert ref.histogram(x, 8.0, 7, (17.1,) * 3).sum() > ref.histogram(x, 8.0, 7).sum()
    # exact distances: 5 lands in bin 5, r == r_max is not counted, coincident atoms land in bin 0
    t = np.array([[0, 0, 0], [3, 4, 0], [0, 0, 0], [5, 12, 0]], dtype=np.float32)
    h = ref.histogram(t, 13.0, 13)
    assert h[0] == 1 and h[5] == 2 and h.sum() == 4 and h[8] == 1          # 1-3: sqrt(4 + 64) = 8.2
    assert ref.margin(t, 13.0, 13) == 0.0 and ref.margin(t, 13.0, 13, ignore_zero=True) > 0.2
    # a NaN or an Inf is in no pair; one atom or none has no pair
    bad = x.copy()
    bad[3, 0], bad[9, 2] = np.nan, np.inf
    keep = np.ones(65, bool)
    keep[[3, 9]] = False
    for box in (None, (17.1, 17.1, 17.1)):
        assert np.array_equal(ref.histogram(bad, 8.0, 7, box), ref.histogram(x[keep], 8.0, 7, box))
    assert not ref.histogram(x[:1], 8.0, 7).any() and not ref.histogram(x[:0], 8.0, 7).any()
    assert math.isnan(ref.radius_of_gyration(bad)) and math.isnan(ref.radius_of_gyration(x[:0]))
    assert ref.radius_of_gyration(x[:1]) == 0.0
    two = np.array([[0, 0, 0], [6, 8, 0]], dtype=np.float32)
    assert ref.radius_of_gyration(two) == 5.0


def test_gpu_cases_meet_their_condition():
    """The shapes, seeds and (n_bins, r_max, box) combinations tests/test_gpu_observe.py compares exactly: no pair
    within 1e-9 bins of an edge, in the restatement alone."""
    import test_gpu_observe as T
    worst = min(T.expected(N, combo)[1] for N in T.SIZES for combo in T.COMBOS)
    print("smallest margin over the GPU cases:", worst, "bins")
    assert worst >= 1e-9


# ------------------------------------------------------------------------------------------------ PairHistogram
def close(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool((np.abs(a - b) <= rel * np.abs(b)).all())


def test_pair_histogram_arithmetic():
    from molecular_dynamics_neural_operator_amd.forecast import PairHistogram
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    L, N, r_max, nb = 20.0, 10, 8.0, 4
    counts = torch.tensor([[[1, 2, 3, 4], [0, 0, 0, 0]], [[4, 3, 2, 1], [0, 5, 0, 5]], [[1, 1, 1, 1], [2, 0, 0, 0]]])   # [3, 2, 4]
    h = PairHistogram(counts, r_max, nb, N, (L, L, L))
    assert h.edges().dtype == torch.float64 and h.edges().tolist() == [0.0, 2.0, 4.0, 6.0, 8.0]
    assert h.centers().tolist() == [1.0, 3.0, 5.0, 7.0]
    p = h.distribution()
    assert p.dtype == torch.float64 and close(p[0, 0], [0.1, 0.2, 0.3, 0.4]) and close(p[1, 1], [0, 0.5, 0, 0.5])
    assert torch.isnan(p[0, 1]).all()                                          # an empty row has no distribution
    s = h.sum((0,))
    assert s.n_frames == 3 and s.counts.tolist() == [[6, 6, 6, 6], [2, 5, 0, 5]] and s.box == h.box and s.n_atoms == N
    both = h.sum((0, 1))
    assert both.n_frames == 6 and both.counts.tolist() == [8, 11, 6, 11] and h.sum((1, 0)).counts.tolist() == both.counts.tolist()
    assert h.sum(-1).counts.shape == (3, 4) and h.sum(()).n_frames == 1
    for bad in ((2,), (0, 0), (5,)):
        with pytest.raises(MdnoError, match="dims"):
            h.sum(bad)
    # g(r): counts over the ideal gas's share of the shell
    shell = 4.0 * math.pi / 3.0 * (np.array([2.0, 4.0, 6.0, 8.0]) ** 3 - np.array([0.0, 2.0, 4.0, 6.0]) ** 3)
    ideal = (N * (N - 1) / 2.0) * shell / L ** 3
    assert close(h.rdf()[1, 0], np.array([4, 3, 2, 1]) / ideal)
    assert close(s.rdf()[0], np.array([6, 6, 6, 6]) / (3 * ideal)) and close(both.rdf(), np.array([8, 11, 6, 11]) / (6 * ideal))
    # an ideal gas has g = 1: counts equal to the expectation give exactly that
    gas = PairHistogram(torch.tensor([1, 7, 19, 37]), r_max, nb, N, (L, L, L), n_frames=1)
    g = gas.rdf()
    assert close(g / g[0], [1.0, 1.0, 1.0, 1.0])
    # total variation: 0 for equal, 1 for disjoint, symmetric, the closed form between
    a = PairHistogram(torch.tensor([1, 2, 3, 4]), r_max, nb, N)
    b = PairHistogram(torch.tensor([40, 30, 20, 10]), r_max, nb, N)
    assert float(a.total_variation(a)) == 0.0 and close(a.total_variation(b), 0.4) and close(b.total_variation(a), 0.4)
    c = PairHistogram(torch.tensor([[5, 0, 0, 0], [0, 0, 7, 7]]), r_max, nb, N)
    d = PairHistogram(torch.tensor([0, 9, 0, 0]), r_max, nb, N)
    assert c.total_variation(d).tolist() == [1.0, 1.0]                          # broadcast over the leading shape
    assert close(s.total_variation(both), [0.5 * (abs(6 / 24 - 8 / 36) + abs(6 / 24 - 11 / 36) * 2 + abs(6 / 24 - 6 / 36)),
                                           0.5 * (abs(2 / 12 - 8 / 36) + abs(5 / 12 - 11 / 36) * 2 + 6 / 36)])
    for other in (PairHistogram(counts, 8.5, nb, N), PairHistogram(torch.ones(5, dtype=torch.int64), r_max, 5, N), counts):
        with pytest.raises(MdnoError, match="r_max and n_bins"):
            a.total_variation(other)
    k = h.cpu()
    assert torch.equal(k.counts, counts) and (k.r_max, k.n_bins, k.n_atoms, k.box, k.n_frames) == (r_max, nb, N, (L, L, L), 1)
