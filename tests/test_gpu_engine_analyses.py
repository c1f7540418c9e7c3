"""Every analysis the rollout engines offer on their produced frames, under UNEVEN grouping.  The per-module engine tests
group their members evenly (1 + 1 or 4 + 4); here three members run as one engine, as groups of 2 + 1 and as three groups of
one, and each of the thirteen methods must give the bits of the corresponding `forecast` / `ops` call on
`eng.produced(first, n).contiguous()`, in the engine's own box and at its own threshold.  Public methods only."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M, N, W, STEPS, THRESHOLD = 3, 28, 3, 4, 8.0
ENGINES = {"single": None, "groups_2_1": 2, "groups_1_1_1": 3}


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def same(a, b):
    """Two results with the same bits: tensors of one dtype and shape compared as integers (so NaN equals NaN and -0 is not
    0), records field by field, tuples element by element, anything else with ==."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        if not (torch.is_tensor(a) and torch.is_tensor(b)) or a.dtype != b.dtype or a.shape != b.shape or a.device != b.device:
            return False
        if a.is_floating_point():
            as_int = {4: torch.int32, 8: torch.int64, 2: torch.int16}[a.element_size()]
            a, b = a.contiguous().view(as_int), b.contiguous().view(as_int)
        return bool(torch.equal(a, b))
    if dataclasses.is_dataclass(a):
        return type(a) is type(b) and all(same(getattr(a, f.name), getattr(b, f.name)) for f in dataclasses.fields(a))
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


@pytest.fixture(scope="module")
def inputs(dev):
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    traj = syn.ou_trajectory(syn.chain_frame(N, seed=1), W + 6, seed=2)
    wins = torch.from_numpy(np.ascontiguousarray(syn.ensemble_windows(traj[:W], M, sigma=0.1, seed0=100).transpose(1, 0, 2, 3)))
    model = KernelNN(64, 128, 2, 6, 7, 3, 20, 4)
    model.load_state_dict(near_identity_state_dict(64, 128, seed=0, kernel_gain=1e-3, feature_gain=0.1))
    truth = torch.from_numpy(np.ascontiguousarray(traj[W:W + 6]).astype(np.float32)).to(dev)          # [6, N, 3]
    rng = np.random.default_rng(5)                                       # a truth of its own per member: a wrong slice shows
    per_member = truth[:STEPS, None] + torch.from_numpy(rng.normal(0.0, 0.3, (STEPS, M, N, 3)).astype(np.float32)).to(dev)
    return dict(wins=wins, aa=torch.from_numpy(syn.amino_acids(N, seed=1)), model=model.eval().to(dev), truth=truth,
                per_member=per_member.contiguous(), reference=truth[0].contiguous(),
                featurizer=forecast.Featurizer.backbone(N).to(dev),
                native=forecast.ContactPairs.native(torch.from_numpy(traj[0]), THRESHOLD, min_separation=3))


@pytest.mark.parametrize("kind", list(ENGINES))
def test_every_analysis_equals_the_free_function_on_the_produced_frames(dev, inputs, kind):
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine, RolloutEngine
    groups = ENGINES[kind]
    args = (inputs["model"], M, N, W, THRESHOLD)
    kw = dict(max_steps=STEPS, device=dev, noise_sigma=0.05, noise_seed=7)
    eng = RolloutEngine(*args, **kw) if groups is None else GroupedRolloutEngine(*args, groups=groups, **kw)
    if groups is not None:
        assert [e.M for e in eng.engines] == {2: [2, 1], 3: [1, 1, 1]}[groups]
    eng.run(inputs["wins"], inputs["aa"], STEPS)
    before = eng.frames().clone()
    assert not same(before[:, 0], before[:, 1]) and not same(before[:, 1], before[:, 2])       # the members differ
    truth, reference, ft, native = inputs["truth"], inputs["reference"], inputs["featurizer"], inputs["native"]
    box, thr = eng.box, THRESHOLD                      # (the threshold the engine was built with)
    disc = forecast.discretize(before, 5, reference=reference)
    for first, steps in ((0, None), (1, 2)):
        n = STEPS - first if steps is None else steps
        x = eng.produced(first, n).contiguous()
        rng = dict(first_step=first, steps=steps)
        shared, own = truth[first:first + n].contiguous(), inputs["per_member"][first:first + n].contiguous()
        lags, vlags = sorted({0, 1, n - 1}), sorted({0, n - 2})
        aligned = forecast.superpose(x, reference)
        checks = {
            "score": (eng.score(shared, **rng), forecast.score_forecast(x, shared, thr, box=box)),
            "score, a truth per member": (eng.score(own, **rng), forecast.score_forecast(x, own, thr, box=box)),
            "pair_histogram": (eng.pair_histogram(12.0, 50, **rng), forecast.pair_histogram(x, 12.0, 50, box=box)),
            "radius_of_gyration": (eng.radius_of_gyration(**rng), ops.radius_of_gyration(x)),
            "displacement_stats": (eng.displacement_stats(lags, 1, True, 2.0, 16, **rng),
                                   forecast.displacement_stats(x, lags, 1, True, 2.0, 16)),
            "velocity_autocorrelation": (eng.velocity_autocorrelation(vlags, **rng), forecast.velocity_autocorrelation(x, vlags)),
            "ensemble_score": (eng.ensemble_score(shared, **rng), forecast.ensemble_score(x, shared)),
            "cross_rmsd": (eng.cross_rmsd(truth, **rng), forecast.cross_rmsd(x, truth)),
            "cross_rmsd, no matrix": (eng.cross_rmsd(truth, matrix=False, **rng), forecast.cross_rmsd(x, truth, False)),
            "superpose": (eng.superpose(reference, **rng), aligned),
            "assign": (eng.assign(disc, **rng), disc.assign(x)),
            "internal_coordinates": (eng.internal_coordinates(ft, **rng), forecast.internal_coordinates(x, ft, box=box)),
            "internal_coordinates, radians f64": (eng.internal_coordinates(ft, True, torch.float64, **rng),
                                                  forecast.internal_coordinates(x, ft, box=box, radians=True, dtype=torch.float64)),
            "pair_statistics": (eng.pair_statistics(block_len=3, **rng), forecast.pair_statistics(x, thr, box=box, block_len=3)),
            "pair_statistics, counts only": (eng.pair_statistics(7.0, 64, False, **rng),
                                             forecast.pair_statistics(x, 7.0, box=box, block_len=64, moments=False)),
            "contact_series": (eng.contact_series(native, **rng), forecast.contact_series(x, native, box=box)),
            "covariance": (eng.covariance(reference, **rng), forecast.covariance(aligned[0], None, 0)),
            "covariance, lagged": (eng.covariance(reference, lag=1, **rng), forecast.covariance(aligned[0], None, 1)),
        }
        for name, (got, want) in checks.items():
            assert same(got, want), (kind, first, steps, name)
        assert tuple(checks["score"][0].mse.shape) == (n, M) and tuple(checks["superpose"][0][0].shape) == (n, M, N, 3)
        assert not same(checks["score"][0].mse, checks["score, a truth per member"][0].mse)
    assert torch.equal(eng.frames(), before)
    eng.close()
