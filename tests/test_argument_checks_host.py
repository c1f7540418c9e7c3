"""The host-side argument checks of ops.py and forecast.py, held to one table: which values every public validator takes
(and what it returns) and which it refuses, and that every analysis wrapper refuses a CPU tensor, a non-tensor, a wrong
rank and a wrong last dimension with MdnoError before the library is loaded.  No device, no library."""
import re

import numpy as np
import pytest
import torch

from molecular_dynamics_neural_operator_amd import _lib, ops
from molecular_dynamics_neural_operator_amd import forecast as F
from molecular_dynamics_neural_operator_amd._lib import MdnoError

R = "raises MdnoError"
I31 = 2 ** 31
T0, T1 = torch.tensor(3), torch.tensor([3, 4])           # a 0-d tensor, an int64 tensor


def outcome(fn, *args):
    try:
        return fn(*args)
    except MdnoError:
        return R


def run_table(fn, table):
    wrong = [(args, want, got) for args, want in table for got in [outcome(fn, *args)] if type(got) is not type(want) or got != want]
    assert not wrong, "\n".join(f"{fn.__name__}{args!r}: expected {want!r}, got {got!r}" for args, want, got in wrong)


# ================================================================================================ lag lists
def test_check_lags_table():
    S = 6
    run_table(ops.check_lags, [
        (([], S), R), (([0], S), [0]), (([0] * ops.MAX_LAGS, S), [0] * ops.MAX_LAGS), (([0] * (ops.MAX_LAGS + 1), S), R),
        (([-1], S), R), (([5], S), [5]), (([6], S), R), (([4], S, 1), [4]), (([5], S, 1), R), (([0, 5, 2], S), [0, 5, 2]),
        (([True], S), [1]), (([3.0], S), [3]), (([3.5], S), R), (([np.int64(3)], S), [3]), ((["3"], S), R), (([T0], S), [3]),
        ((T1, S), [3, 4]), ((T0, S), [3]), ((torch.tensor([3.0, 4.0]), S), [3, 4]), ((torch.tensor([3.5]), S), R),
        ((range(3), S), [0, 1, 2]), ((np.array([1, 2]), S), [1, 2]), ((3, S), R), (("34", S), R), ((None, S), R), (([None], S), R),
    ])


def test_check_msm_lags_table():
    n = ops.MSM_MAX_LAGS
    run_table(ops.check_msm_lags, [
        (([],), R), (([1],), [1]), (([1] * n,), [1] * n), (([1] * (n + 1),), R),
        (([0],), R), (([I31 - 1],), [I31 - 1]), (([I31],), R), (([-1],), R),
        (([True],), [1]), (([3.0],), [3]), (([3.5],), R), (([np.int64(3)],), [3]), ((["3"],), R), (([T0],), [3]),
        ((T1,), [3, 4]), ((T0,), [3]), ((3,), R), ((None,), R),
    ])


def test_check_contact_lags_table():
    S, n = 4, ops.CM_MAX_LAGS
    run_table(ops.check_contact_lags, [
        (([], S), []), (([0], S), [0]), (([0] * n, S), [0] * n), (([0] * (n + 1), S), R),
        (([-1], S), R), (([3], S), [3]), (([4], S), R), (([0], 0), R),
        (([True], S), [1]), (([3.0], S), [3]), (([3.5], S), R), (([np.int64(3)], S), [3]), ((["3"], S), R), (([T0], S), [3]),
        ((torch.tensor([0, 3]), S), [0, 3]), ((T0, S), [3]), ((3, S), R), ((None, S), R),
    ])


# ================================================================================================ scalar integers
def test_exact_integers_table():
    """`exact`: anything with int(v) == v."""
    run_table(ops.check_origin_stride, [
        ((0,), R), ((1,), 1), ((I31 - 1,), I31 - 1), ((I31,), R), ((-1,), R),
        ((True,), 1), ((3.0,), 3), ((3.5,), R), ((np.int64(3),), 3), (("3",), R), ((T0,), 3), ((T1,), R), ((None,), R),
    ])
    top = ops.MAX_HISTOGRAM_BINS
    run_table(ops.check_histogram_args, [
        ((8.0, 0), R), ((8.0, 1), (8.0, 1, None)), ((8.0, top), (8.0, top, None)), ((8.0, top + 1), R),
        ((8.0, True), (8.0, 1, None)), ((8.0, 3.0), (8.0, 3, None)), ((8.0, 3.5), R), ((8.0, np.int64(3)), (8.0, 3, None)),
        ((8.0, "3"), R), ((8.0, T0), (8.0, 3, None)), ((8.0, T1), R), ((8.0, None), R),
        ((0.0, 4), R), ((-1.0, 4), R), ((float("inf"), 4), R), ((float("nan"), 4), R), (("a", 4), R), ((None, 4), R),
        ((8, 4), (8.0, 4, None)), (("8", 4), (8.0, 4, None)), ((True, 4), (1.0, 4, None)), ((torch.tensor(8.0), 4), (8.0, 4, None)),
        ((8.0, 4, (16.0, 0.0, 0.0)), (8.0, 4, (16.0, 0.0, 0.0))), ((8.0, 4, (15.9, 0.0, 0.0)), R), ((8.0, 4, (0, 0, 0)), (8.0, 4, None)),
    ])


def test_strict_integers_table():
    """`strict`: int only, never bool."""
    top = ops.IC_MAX_BINS
    ok = ([0.0], [1.0])
    run_table(ops.check_column_ranges, [
        ((0, 1, 0, 3), R), ((0, 1, 1, 3), ok + (1,)), ((0, 1, top, 3), ok + (top,)), ((0, 1, top + 1, 3), R),
        ((0, 1, True, 3), R), ((0, 1, 3.0, 3), R), ((0, 1, 3.5, 3), R), ((0, 1, np.int64(3), 3), R), ((0, 1, "3", 3), R),
        ((0, 1, T0, 3), R), ((0, 1, T1, 3), R),
        (([0, 1, 2], [1, 2, 3], 4, 3), ([0.0, 1.0, 2.0], [1.0, 2.0, 3.0], 4)), (([0, 1], [1, 2], 4, 3), R), (([0], [1, 2, 3], 4, 3), R),
        ((torch.tensor([0.0, 1.0, 2.0]), np.array([1, 2, 3]), 4, 3), ([0.0, 1.0, 2.0], [1.0, 2.0, 3.0], 4)),
        ((1, 1, 4, 3), R), ((2, 1, 4, 3), R), ((0, float("inf"), 4, 3), R), ((float("nan"), 1, 4, 3), R), ((-1e308, 1e308, 4, 3), R),
        (("a", 1, 4, 3), R), ((None, 1, 4, 3), R), (([], [], 4, 0), ([], [], 4)),
    ])
    run_table(ops.check_contact_args, [
        ((8.0, None, 0), R), ((8.0, None, 1), (8.0, None, 1)), ((8.0, None, I31 - 1), (8.0, None, I31 - 1)), ((8.0, None, I31), R),
        ((8.0, None, True), R), ((8.0, None, 3.0), R), ((8.0, None, 3.5), R), ((8.0, None, np.int64(3)), R), ((8.0, None, "3"), R),
        ((8.0, None, T0), R), ((8.0, None, T1), R),
        ((0.0,), R), ((-1.0,), R), ((float("inf"),), R), ((float("nan"),), R), (("a",), R), ((None,), R),
        ((8,), (8.0, None, 1)), ((8, (16.0, 0.0, 0.0), 64), (8.0, (16.0, 0.0, 0.0), 64)), ((8.0, (15.9, 0.0, 0.0)), R),
    ])
    run_table(ops.check_projection_args, [
        ((-1, 0.0), R), ((0, 0.0), (0, 0.0)), ((I31 - 1, 0.0), (I31 - 1, 0.0)), ((I31, 0.0), R),
        ((True, 0.0), R), ((3.0, 0.0), R), ((3.5, 0.0), R), ((np.int64(3), 0.0), R), (("3", 0.0), R), ((T0, 0.0), R), ((T1, 0.0), R),
        ((8, -1e-9), R), ((8, float("nan")), R), ((8, 0), (8, 0.0)), ((8, float("inf")), (8, float("inf"))), ((8, "1.5"), (8, 1.5)),
    ])


def test_state_and_component_counts_table():
    """`_msm_states` under its callers' names, `_check_k` through pca (both strict)."""
    top = ops.MSM_MAX_STATES
    for what in ("kcenters: k", "centroid_sums: k", "transition_counts: n_states"):
        run_table(lambda k: ops._msm_states(k, what), [
            ((0,), R), ((1,), 1), ((top,), top), ((top + 1,), R),
            ((True,), R), ((3.0,), R), ((3.5,), R), ((np.int64(3),), R), (("3",), R), ((T0,), R), ((T1,), R), ((None,), R)])
        with pytest.raises(MdnoError, match=what.split(": ")[1]):
            ops._msm_states(0, what)
    cov = F.Covariance(mean=torch.zeros(4, dtype=torch.float64), sums=torch.eye(4, dtype=torch.float64), n=10, lag=0)

    def n_components(k):
        return F.pca(cov, k).vectors.shape[1]
    run_table(n_components, [
        ((0,), R), ((1,), 1), ((4,), 4), ((5,), R),
        ((True,), R), ((3.0,), R), ((3.5,), R), ((np.int64(3),), R), (("3",), R), ((T0,), R), ((T1,), R), ((None,), R)])
    with pytest.raises(MdnoError, match="k ="):
        F.pca(cov, 5)


# ================================================================================================ boxes
def test_check_box_table():
    run_table(ops.check_box, [
        ((None, 8.0), None), (((0, 0, 0), 8.0), None), (((0.0, 0.0, 0.0), 8.0), None), ((torch.zeros(3), 8.0), None),
        (((16, 0, 40.5), 8.0), (16.0, 0.0, 40.5)), (((15.999, 0, 0), 8.0), R), (((16.0, 16.0, 16.0), 8.0), (16.0, 16.0, 16.0)),
        ((torch.tensor([16.0, 17.0, 18.0]), 8.0), (16.0, 17.0, 18.0)), ((np.array([16.0, 17.0, 18.0]), 8.0), (16.0, 17.0, 18.0)),
        ((["16", "17", "18"], 8.0), (16.0, 17.0, 18.0)), ((iter([16.0, 17.0, 18.0]), 8.0), (16.0, 17.0, 18.0)),
        (((16.0, 16.0), 8.0), R), (((16.0, 16.0, 16.0, 16.0), 8.0), R), (((), 8.0), R), ((torch.zeros(1, 3), 8.0), None),
        (((-1.0, 0, 0), 0.0), R), (((float("nan"), 0, 0), 0.0), R), (((float("inf"), 0, 0), 0.0), R),
        (("abc", 8.0), R), ((5, 8.0), R), (((None, 0, 0), 8.0), R),
        (((16.0, 0, 0), -1.0), R), (((16.0, 0, 0), float("nan")), R), (((16.0, 0, 0), float("inf")), R), (((1e-3, 0, 0), 0.0), (1e-3, 0.0, 0.0)),
    ])


# ================================================================================================ wrappers: no library, no device
FR4, FR3, X2 = torch.zeros(4, 2, 5, 3), torch.zeros(4, 5, 3), torch.zeros(6, 4)
PAIRS = torch.tensor([[0, 1]], dtype=torch.int32)
F64V, I32V = torch.zeros(1, dtype=torch.float64), torch.zeros(2, dtype=torch.int32)
BOX = (20.0, 20.0, 20.0)

# (the name the refusal gives the argument under test, whatever its letter case; the call with that argument as `t`)
WRAPPERS = {
    "ops.forecast_score": ("frames", lambda t: ops.forecast_score(t, FR3)),
    "ops.contact_maps": ("frames", lambda t: ops.contact_maps(t)),
    "ops.pair_histogram": ("frames", lambda t: ops.pair_histogram(t, 8.0, 4)),
    "ops.radius_of_gyration": ("frames", lambda t: ops.radius_of_gyration(t)),
    "ops.displacement_stats": ("frames", lambda t: ops.displacement_stats(t, [0])),
    "ops.velocity_autocorrelation": ("frames", lambda t: ops.velocity_autocorrelation(t, [0])),
    "ops.unwrap_frames": ("frames", lambda t: ops.unwrap_frames(t, BOX)),
    "ops.ensemble_score": ("frames", lambda t: ops.ensemble_score(t, FR3)),
    "ops.cross_rmsd": ("frames", lambda t: ops.cross_rmsd(t, FR3)),
    "ops.superpose_frames": ("frames", lambda t: ops.superpose_frames(t, FR3[0])),
    "ops.feature_sums": ("x", lambda t: ops.feature_sums(t)),
    "ops.feature_covariance": ("x", lambda t: ops.feature_covariance(t, F64V)),
    "ops.project_features": ("x", lambda t: ops.project_features(t, F64V, F64V)),
    "ops.assign_features": ("x", lambda t: ops.assign_features(t, X2)),
    "ops.kcenters": ("x", lambda t: ops.kcenters(t, 2)),
    "ops.centroid_sums": ("x", lambda t: ops.centroid_sums(t, I32V, 2)),
    "ops.transition_counts": ("label", lambda t: ops.transition_counts(t, 2, [1])),
    "ops.internal_features": ("frames", lambda t: ops.internal_features(t, PAIRS)),
    "ops.internal_features_bwd": ("frames", lambda t: ops.internal_features_bwd(t, X2, PAIRS, None, None, I32V, I32V)),
    "ops.column_histogram": ("x", lambda t: ops.column_histogram(t, 0.0, 1.0, 4)),
    "ops.project_constraints": ("frames", lambda t: ops.project_constraints(t, PAIRS, F64V, F64V, I32V)),
    "ops.pair_statistics": ("frames", lambda t: ops.pair_statistics(t)),
    "ops.contact_bits": ("frames", lambda t: ops.contact_bits(t, PAIRS, F64V, 8.0)),
    "ops.contact_correlation": ("bits", lambda t: ops.contact_correlation(t, 4, [0])),
    "ops.radius_graph_pbc": ("pos", lambda t: ops.radius_graph_pbc(t, 5, 8.0, BOX)),
    "forecast.score_forecast": ("frames", lambda t: F.score_forecast(t, FR3)),
    "forecast.contact_maps": ("frames", lambda t: F.contact_maps(t)),
    "forecast.pair_histogram": ("frames", lambda t: F.pair_histogram(t, 8.0, 4)),
    "forecast.radius_of_gyration": ("frames", lambda t: F.radius_of_gyration(t)),
    "forecast.displacement_stats": ("frames", lambda t: F.displacement_stats(t)),
    "forecast.velocity_autocorrelation": ("frames", lambda t: F.velocity_autocorrelation(t)),
    "forecast.unwrap": ("frames", lambda t: F.unwrap(t, BOX)),
    "forecast.ensemble_score": ("frames", lambda t: F.ensemble_score(t, FR3)),
    "forecast.cross_rmsd": ("frames", lambda t: F.cross_rmsd(t, FR3)),
    "forecast.superpose": ("frames", lambda t: F.superpose(t, FR3[0])),
    "forecast.covariance": ("X", lambda t: F.covariance(t)),
    "forecast.assign": ("X", lambda t: F.assign(t, X2)),
    "forecast.kcenters": ("X", lambda t: F.kcenters(t, 2)),
    "forecast.kmeans": ("X", lambda t: F.kmeans(t, 2)),
    "forecast.transition_counts": ("label", lambda t: F.transition_counts(t, 2, [1])),
    "forecast.internal_coordinates": ("frames", lambda t: F.internal_coordinates(t, F.Featurizer.of(pairs=[[0, 1]]))),
    "forecast.feature_histograms": ("features|x", lambda t: F.feature_histograms(t, 0.0, 1.0)),
    "forecast.project_constraints": ("frames", lambda t: F.project_constraints(t, F.DistanceConstraints.chain(5, 1.0, 2.0))),
    "forecast.pair_statistics": ("frames", lambda t: F.pair_statistics(t)),
    "forecast.contact_series": ("frames", lambda t: F.contact_series(t, F.ContactPairs.of([[0, 1]], 8.0))),
}
# a CPU tensor of every rank a wrapper takes, non-tensors, ranks nobody takes, and last dimensions that are not 3
INPUTS = {"cpu [S,M,N,3]": FR4, "cpu [F,N,3]": FR3, "cpu [R,D]": X2, "cpu int32 [S,M]": torch.zeros(6, 2, dtype=torch.int32),
          "cpu int64 [M,P,W]": torch.zeros(2, 1, 1, dtype=torch.int64),
          "list": [[0.0, 0.0, 0.0]], "None": None, "ndarray": np.zeros((4, 2, 5, 3), np.float32),
          "rank 0": torch.zeros(()), "rank 9": torch.zeros((1,) * 8 + (3,)), "last 2 of 4": torch.zeros(4, 2, 5, 2),
          "last 2 of 3": torch.zeros(4, 5, 2)}


@pytest.mark.parametrize("entry", sorted(WRAPPERS))
def test_wrappers_refuse_on_the_host(entry, monkeypatch):
    def no_library():
        pytest.fail(f"{entry} loaded the library before it refused its arguments")
    monkeypatch.setattr(_lib, "load", no_library)
    name, call = WRAPPERS[entry]
    for label, t in INPUTS.items():
        with pytest.raises(MdnoError) as err:
            call(t)
        msg = str(err.value)
        said = [type(t).__name__, "CPU tensor", "no CPU fallback", "must be"] + ([str(tuple(t.shape))] if torch.is_tensor(t) else [])
        assert re.search(rf"\b({name})\b", msg, re.I) and any(s in msg for s in said), f"{entry} <- {label}: {msg!r}"
        if torch.is_tensor(t) and "CPU tensor" in msg:
            assert "no CPU fallback" in msg, msg


def test_second_operands_are_refused_on_the_host(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    for call in (lambda: ops.contact_correlation(torch.zeros(2, 1, 1, dtype=torch.int64), True, [0]),
                 lambda: ops.unwrap_frames(FR4, None), lambda: ops.pair_histogram(FR4, 8.0, 4, form="fast"),
                 lambda: ops.internal_features(FR4, PAIRS, form="fast"), lambda: ops.internal_features(FR4, PAIRS, dtype=torch.float16),
                 lambda: ops.displacement_stats(FR4, [0], 0), lambda: ops.rigid_motions(0, [0], 0, translate=-1.0),
                 lambda: ops.rigid_motions(0, [0], 0, translate=float("inf")), lambda: ops.rigid_motions(0, [0], 0, last_element=1),
                 lambda: ops.rigid_motions(0, [0], 2 ** 48), lambda: ops.rigid_motions(-1, [0], 0),
                 lambda: ops.rigid_apply(torch.zeros(2, 4), torch.zeros(2, 3), torch.zeros(2, 3), 5, torch.zeros(10, 3)),
                 lambda: ops.rigid_apply(*(torch.zeros(2, n, dtype=torch.float64) for n in (4, 3, 3)), 5, torch.zeros(9, 3)),
                 lambda: F.kmeans(X2, 2, iters=-1), lambda: F.kmeans(X2, 2, iters=True), lambda: F.free_energy(torch.zeros(4, 2), bins=0),
                 lambda: F.free_energy(torch.zeros(4, 2), bins=2.0), lambda: F.Featurizer.of(pairs=[[0, 1]], n_atoms=True),
                 lambda: F.Featurizer.of(pairs=[[0, 5]], n_atoms=5), lambda: F.Featurizer.of(pairs=[[0, 2 ** 31 - 1]]),
                 lambda: F.Featurizer.backbone(5, 0), lambda: F.Featurizer.backbone(5, 3, True),
                 lambda: F.DistanceConstraints.chain(3.0, 1.0, 2.0), lambda: F.ContactPairs.of([[0, 1]], 8.0, n_atoms=-1)):
        with pytest.raises(MdnoError):
            call()
    assert F.Featurizer.of(pairs=[[0, 2 ** 31 - 2]]).top == 2 ** 31 - 2 and F.Featurizer.of(pairs=[[0, 4]], n_atoms=5).n_atoms == 5
    assert F.ForecastScore._ratio(torch.tensor([1, 2]), torch.tensor([0, 4])).tolist()[1] == 0.5


def test_check_constraint_table_on_host_tensors():
    """The table check compares with the device it is given, so host tensors exercise every operand rule."""
    dev = torch.device("cpu")
    pairs, lo, hi = torch.tensor([[0, 1], [1, 2]], dtype=torch.int32), torch.ones(2, dtype=torch.float64), torch.full((2,), 2.0, dtype=torch.float64)
    cp, w = torch.tensor([0, 1, 2], dtype=torch.int32), torch.ones(3)

    def ok(*args):
        got = ops.check_constraint_table(*args, 3, dev)
        return [None if t is None else (t.dtype, tuple(t.shape), t.is_contiguous()) for t in got]
    i32, f64, f32 = torch.int32, torch.float64, torch.float32
    full = [(i32, (2, 2), True), (f64, (2,), True), (f64, (2,), True), (i32, (3,), True), (f32, (3,), True)]
    strided = torch.zeros(4, dtype=torch.float64)[::2]
    run_table(ok, [
        ((pairs, lo, hi, cp, w), full), ((pairs, lo, hi, cp, None), full[:4] + [None]), ((pairs, strided, hi, cp, w), full),
        ((pairs[:0], lo[:0], hi[:0], cp[:1], None), [(i32, (0, 2), True), (f64, (0,), True), (f64, (0,), True), (i32, (1,), True), None]),
        ((pairs.long(), lo, hi, cp, w), R), ((pairs.reshape(-1), lo, hi, cp, w), R), ((pairs.tolist(), lo, hi, cp, w), R),
        ((torch.zeros((2, 3), dtype=i32), lo, hi, cp, w), R), ((pairs, lo.float(), hi, cp, w), R), ((pairs, lo[:1], hi, cp, w), R),
        ((pairs, lo, hi[None], cp, w), R), ((pairs, lo, None, cp, w), R), ((pairs, lo, hi, cp.long(), w), R), ((pairs, lo, hi, cp[:0], w), R),
        ((pairs, lo, hi, cp[None], w), R), ((pairs, lo, hi, cp, w.double()), R), ((pairs, lo, hi, cp, w[:2]), R), ((pairs, lo, hi, cp, [1.0] * 3), R),
        ((pairs, lo, hi, cp, w.to("meta")), R), ((pairs.to("meta"), lo, hi, cp, w), R),
    ])


# ================================================================================================ the helpers themselves
class OnDevice(torch.Tensor):
    """A host tensor that says it lives on the GPU: the rank and dtype rules behind the device check, without a device."""
    is_cuda = True


def test_device_tensor_rules():
    A = pytest.importorskip("molecular_dynamics_neural_operator_amd._args")
    for bad, said in (([1.0], "list"), (None, "NoneType"), (np.zeros(3), "ndarray")):
        with pytest.raises(MdnoError, match=rf"frames must be a torch tensor, got {said}"):
            A.device_tensor(bad, "frames", (3, 4), last=3)
    with pytest.raises(MdnoError, match=r"truth is a CPU tensor.*no CPU fallback"):
        A.device_tensor(torch.zeros(2, 5, 3), "truth", (3,), last=3)
    dev = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype).as_subclass(OnDevice)
    for t, ranks, last in ((dev(5, 3), (3, 4), 3), (dev(1, 1, 1, 5, 3), (3, 4), 3), (dev(2, 5, 2), (3, 4), 3), (dev(), (1,), None),
                           (dev(), None, 3), (dev(4), range(2, 9), None)):
        with pytest.raises(MdnoError, match=re.escape(str(tuple(t.shape)))):
            A.device_tensor(t, "frames", ranks, last=last)
    assert A.device_tensor(dev(2, 5, 3), "frames", (3, 4), last=3).shape == (2, 5, 3)
    assert A.device_tensor(dev(7), "x", None).shape == (7,) and A.device_tensor(dev(0, 3), "x", range(2, 9), last=3).shape == (0, 3)
    f16, f32, f64, i32, i64 = torch.float16, torch.float32, torch.float64, torch.int32, torch.int64
    for given, asked, got in ((f64, f32, f32), (f16, f32, f32), (i64, f32, f32), (f32, f64, f64), (f64, "float", f64), (f32, "float", f32),
                              (f16, "float", f32), (i32, "float", f32), (i32, None, i32), (i64, None, i64), (f16, None, f16)):
        out = A.device_tensor(dev(4, 6, dtype=given)[:, ::2], "x", (2,), dtype=asked)
        assert out.dtype == got and out.is_contiguous() and out.shape == (4, 3)
    same = dev(4, 3)
    assert A.device_tensor(same, "x", (2,)) is same          # nothing to convert: no copy


def test_operand_rules():
    A = pytest.importorskip("molecular_dynamics_neural_operator_amd._args")
    cpu, f32, f64, i32 = torch.device("cpu"), torch.float32, torch.float64, torch.int32
    t = torch.zeros(4, 2, dtype=i32)
    assert A.operand(t, "pairs", i32, (4, 2), cpu) is t and A.operand(t, "pairs", (i32, torch.int64), (None, 2), cpu) is t
    assert A.operand(t, "pairs", i32, (None, None), cpu) is t and A.operand(t[:0], "pairs", i32, (None, 2), cpu).shape == (0, 2)
    assert A.operand(t.t(), "pairs", i32, (2, None), cpu).is_contiguous()
    assert A.operand(None, "weights", f32, (3,), cpu, optional=True) is None
    for bad, dtypes, shape, dev, optional in ((None, f32, (3,), cpu, False), (t, f32, (4, 2), cpu, False), (t, (f32, f64), (4, 2), cpu, False),
                                              (t, i32, (4, 3), cpu, False), (t, i32, (None, 3), cpu, False), (t, i32, (4,), cpu, False),
                                              (t, i32, (4, 2, None), cpu, False), (t, i32, (4, 2), torch.device("meta"), False),
                                              ([[0, 1]], i32, (None, 2), cpu, True), (t, i32, (), cpu, True)):
        with pytest.raises(MdnoError, match="pairs is .*expected"):
            A.operand(bad, "pairs", dtypes, shape, dev, optional)
    with pytest.raises(MdnoError, match=r"int32 \(4, 2\) on cpu: expected float32 or float64 \[n, 2\] on cpu or None"):
        A.operand(t, "pairs", (f32, f64), (None, 2), cpu, optional=True)


def test_scalar_and_list_rules():
    A = pytest.importorskip("molecular_dynamics_neural_operator_amd._args")
    assert A.integer(5, "n", 0, None) == 5 and A.integer(2 ** 40, "n", 0, None) == 2 ** 40 and A.integer(3.0, "n", 3, 3, exact=True) == 3
    assert type(A.integer(np.int64(3), "n", 0, exact=True)) is int and type(A.integer(True, "n", 0, exact=True)) is int
    for v, kw in ((2 ** 31, {}), (-1, {}), (True, {}), (3.0, {}), (np.int64(3), {}), ("3", dict(exact=True)), (3.5, dict(exact=True))):
        with pytest.raises(MdnoError, match=r"n = .*expected an integer >= 0"):
            A.integer(v, "n", 0, **kw)
    with pytest.raises(MdnoError, match=r"k = 5: expected an integer in 1 \.\. 4"):
        A.integer(5, "k", 1, 4)
    inf, nan = float("inf"), float("nan")
    assert A.real("2", "r") == 2.0 and A.real(0, "r", positive=False) == 0.0 and A.real(inf, "tol", positive=False, finite=False) == inf
    for v, kw in ((0.0, {}), (-1.0, {}), (inf, {}), (nan, {}), ("a", {}), (None, {}), (-1e-9, dict(positive=False)), (inf, dict(positive=False)),
                  (nan, dict(positive=False, finite=False)), (-inf, dict(positive=False, finite=False))):
        with pytest.raises(MdnoError, match="r = .*expected a"):
            A.real(v, "r", **kw)
    assert A.int_list(torch.tensor([[1, 2], [3, 4]]), "f", "lag", (0, 4), 1, 4) == [1, 2, 3, 4]
    assert A.form_code("lds", {"auto": 0, "lds": 1}) == 1
    with pytest.raises(MdnoError, match=r"form 'fast': expected one of \['auto', 'lds'\]"):
        A.form_code("fast", {"auto": 0, "lds": 1})
    A.check_dims("x", (2 ** 31 - 1, 3))
    A.check_dims("x", (2 ** 31, 3), (3,))
    with pytest.raises(MdnoError, match=r"x has shape \(2147483648, 3\): a dimension exceeds 2\^31 - 1"):
        A.check_dims("x", (2 ** 31, 3))
