"""Roll an ensemble out and score it on the device: 64 members of a 504-atom box start from perturbed copies of the first
window of a synthetic Ornstein-Uhlenbeck trajectory (synthetic.ou_trajectory) and are scored, step by step, against the
frames of that trajectory they forecast (forecast.py).  Prints ONE JSON line: per-step ensemble means, the first
non-finite step per member, and the cost of the scoring call (HIP events) beside the time the rollout took.  With
`--rdf R_MAX N_BINS` also the distributional score (forecast.PairHistogram): per member the total-variation distance
between the forecast's and the truth's pair-distance distributions summed over the steps, and the radius of gyration at
the first and the last step.  With `--msd [R_MAX N_BINS]` also the dynamical score (forecast.DisplacementStats): per lag the
ensemble mean of MSD(tau) and of the non-Gaussian parameter alpha_2(tau) beside the truth's, and (with R_MAX N_BINS) the
total-variation distance between the forecast's and the truth's displacement distributions per lag.  With `--ensemble` also
the verification of the members AS AN ENSEMBLE (forecast.EnsembleScore): every `--every`-th step the RMSE of the ensemble mean,
the spread, the spread-skill ratio, the CRPS and the fair CRPS, and the flatness of the rank histogram pooled over the steps
(INTEGRATION.md "Is the ensemble calibrated?" reads them).  `--noise-sigma` gives the members their per-step kicks; without
it they differ only by their starting windows.  With `--coverage RADIUS` also the structural coverage
(forecast.CrossRmsd): every produced frame against every frame of the truth, per member the precision (the share of its
frames within RADIUS of some true frame), the coverage (the share of the true frames it comes within RADIUS of) and the
median nearest-frame RMSD (INTEGRATION.md "Does the run visit the right structures?" reads them).  With `--pca K` also the
essential dynamics (forecast.pca): the truth, superposed on its first frame, gives K principal components; printed are its
explained-variance ratios, per member the RMSIP of the member's own top-K subspace with the truth's and the total variation
between the member's and the truth's PC1/PC2 histograms, both projected on the TRUTH's components; with `--tica LAG` also
the leading implied timescales of the truth and of the pooled members (INTEGRATION.md "Does the run move along the right
coordinates?" reads them).  With `--msm N_STATES LAG` (and `--pca K`) also a Markov state model (forecast.discretize,
forecast.markov_model): the truth is cut into N_STATES states in its own TICA space (with `--tica`, else its PCA space), truth
and members are assigned to the truth's centres, and printed per member are the total variation of the state populations
against the truth's, the share of its frames outside the truth's covering radius and the leading implied timescales at LAG
beside the truth's (INTEGRATION.md "Does the run hop between the right states?" reads them).  With `--internal [MIN_SEP STRIDE]`
also the internal coordinates (forecast.Featurizer.backbone(atoms, MIN_SEP, STRIDE), default 3 4: pseudo-bonds, the pairs of
every STRIDE-th atom at least MIN_SEP apart, pseudo-angles and pseudo-dihedrals): per member the largest and the median
per-column total variation of its feature histograms against the truth's over the truth's own ranges, and the share of its
bond lengths outside the truth's range; `--pca`, `--tica` and `--msm` then work on these features instead of the superposed
Cartesian coordinates (INTEGRATION.md "Features that do not depend on a reference frame" reads them).  With
`--constrain [MARGIN]` the free run is made a second time with distance constraints on the pseudo-bonds
(forecast.DistanceConstraints.from_frames: each inside the truth's own range widened by MARGIN), projected at the end of every
step (include/mdno_constrain.h), and "constrained" holds, as [free run, constrained run], the diverged members, the RMSD,
native-fraction and Jaccard series and the share of bond lengths outside the truth's range, with the mean violation before and
after the projection and the mean sweep count per step (INTEGRATION.md "Keeping a rollout on the chain manifold" reads them).
With `--contacts [MIN_SEP]` also the contact statistics over the run (forecast.PairStatistics, ContactSeries, ContactCorrelation;
pairs at least MIN_SEP apart in sequence, default 3): per member the mean |dP| between its contact-probability map and the
truth's, the share of the native contacts (truth P >= 0.5) it keeps at P >= 0.5 and the share of its own P >= 0.5 contacts that
are not native, the mean Q over the run beside the truth's own, and the contact survival at a few lags beside the truth's
(INTEGRATION.md "Contact maps over time" reads them).  With `--equivariance K` also how far the model is from commuting with
rigid motions on the start windows (training.equivariance_error): K seeded motions (a uniform rotation about every member's
centroid, plus `--equivariance-translate A`), the mean and the largest per-member RMS of |f(g x) - g f(x)| in Angstrom and the
same relative to the size of the step |f(x) - x_last| (INTEGRATION.md "Training on rigid motions / how equivariant is the
model?" reads them).  With `--sasa [RADIUS PROBE N_POINTS]` also the solvent-accessible surface of the run
(forecast.surface_area: Shrake-Rupley counts, one RADIUS for every atom, default 1.9 1.4 96): per member the mean and the
standard deviation over the steps of the total area beside the truth's, and the RMS over the atoms of the difference between
its per-atom mean burial and the truth's (INTEGRATION.md "Does the run keep its core buried?" reads them).

    python scripts/score_rollout.py [--members 64] [--atoms 504] [--steps 1000] [--window 10] [--reps 5] [--rdf 8.0 200]
                                    [--msd 4.0 64] [--ensemble] [--noise-sigma 0.05] [--coverage 2.0]
                                    [--pca 10] [--tica 10] [--msm 100 10] [--internal 3 4] [--constrain 0.1] [--contacts 3]
                                    [--equivariance 8] [--sasa 1.9 1.4 96]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--atoms", type=int, default=504)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--threshold", type=float, default=8.0)
    ap.add_argument("--kernel-width", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions of the scoring call (after one warm-up)")
    ap.add_argument("--every", type=int, default=50, help="print every n-th step of the per-step series")
    ap.add_argument("--rdf", nargs=2, metavar=("R_MAX", "N_BINS"), default=None,
                    help="also score the distribution of pair distances below R_MAX in N_BINS bins, and the radius of gyration")
    ap.add_argument("--msd", nargs="*", metavar="R_MAX N_BINS", default=None,
                    help="also score the dynamics: MSD and alpha_2 per lag against the truth's; with R_MAX N_BINS the total "
                         "variation of the displacement histograms per lag as well")
    ap.add_argument("--ensemble", action="store_true",
                    help="also verify the members as one ensemble: RMSE of the mean, spread, spread-skill, CRPS, rank histogram")
    ap.add_argument("--noise-sigma", type=float, default=0.0, help="per-step Gaussian kick of every member (0: none)")
    ap.add_argument("--noise-seed", type=int, default=0)
    ap.add_argument("--coverage", type=float, metavar="RADIUS", default=None,
                    help="also score the structural coverage: per member the precision, the coverage and the median "
                         "nearest-frame RMSD against the truth, at this radius")
    ap.add_argument("--pca", type=int, metavar="K", default=None,
                    help="also score the essential dynamics: K principal components of the superposed truth, per member the "
                         "RMSIP with them and the total variation of the PC1/PC2 histograms")
    ap.add_argument("--tica", type=int, metavar="LAG", default=None,
                    help="with --pca: also the K leading implied timescales at this lag, of the truth and of the pooled members")
    ap.add_argument("--msm", type=int, nargs=2, metavar=("N_STATES", "LAG"), default=None,
                    help="with --pca: also a Markov state model: the truth is cut into N_STATES states in its TICA space (with "
                         "--tica, else its PCA space); per member the total variation of the state populations, the share of "
                         "frames outside the truth's covering radius and the leading implied timescales at LAG beside the truth's")
    ap.add_argument("--internal", type=int, nargs="*", metavar="MIN_SEP STRIDE", default=None,
                    help="also score the internal coordinates of the backbone feature set (default 3 4): per member the largest "
                         "and median per-column total variation of the feature histograms against the truth's and the share of "
                         "bond lengths outside the truth's range; --pca/--tica/--msm then run on these features")
    ap.add_argument("--constrain", type=float, nargs="?", const=0.0, metavar="MARGIN", default=None,
                    help="run the free run a second time with distance constraints on the pseudo-bonds, each held inside the "
                         "truth's own range widened by MARGIN (default 0), and print the scores of both runs side by side")
    ap.add_argument("--constrain-iterations", type=int, default=8, help="with --constrain: sweeps per step at most")
    ap.add_argument("--contacts", type=int, nargs="?", const=3, metavar="MIN_SEP", default=None,
                    help="also the contact statistics over the run: per member the error of its contact-probability map against "
                         "the truth's over pairs at least MIN_SEP apart (default 3), the share of native contacts it keeps and "
                         "of its own contacts that are not native, the mean Q beside the truth's and the contact survival at a "
                         "few lags beside the truth's")
    ap.add_argument("--equivariance", type=int, metavar="K", default=None,
                    help="also the equivariance error of the model on the start windows: mean and max over K seeded rigid "
                         "motions (and over the members) of the RMS of |f(g x) - g f(x)|, absolute and relative to the step")
    ap.add_argument("--equivariance-translate", type=float, default=0.0, metavar="A",
                    help="with --equivariance: also translate by up to A Angstrom per axis")
    ap.add_argument("--sasa", nargs="*", metavar="RADIUS PROBE N_POINTS", default=None,
                    help="also the solvent-accessible surface area of the run (Shrake-Rupley, one RADIUS for every atom; default "
                         "1.9 1.4 96): per member the mean and standard deviation of the total area beside the truth's, and the "
                         "per-atom RMS of its mean burial against the truth's")
    a = ap.parse_args()
    if a.sasa is not None and len(a.sasa) not in (0, 3):
        ap.error("--sasa takes no values or RADIUS PROBE N_POINTS")
    if a.equivariance is not None and (a.equivariance < 1 or not a.equivariance_translate >= 0.0):
        ap.error("--equivariance takes K >= 1 (and --equivariance-translate A >= 0)")
    if a.contacts is not None and a.contacts < 0:
        ap.error("--contacts takes a MIN_SEP >= 0")
    if a.constrain is not None and not (a.constrain >= 0.0 and a.constrain_iterations >= 0):
        ap.error("--constrain takes a MARGIN >= 0 and --constrain-iterations a number >= 0")
    if a.internal is not None and (len(a.internal) not in (0, 2) or any(v < 1 for v in a.internal)):
        ap.error("--internal takes no values or MIN_SEP STRIDE, both >= 1")
    if a.tica is not None and a.pca is None:
        ap.error("--tica needs --pca K")
    if a.msm is not None and (a.pca is None or a.msm[0] < 1 or a.msm[1] < 1):
        ap.error("--msm needs --pca K, N_STATES >= 1 and LAG >= 1")
    if a.msd is not None and len(a.msd) not in (0, 2):
        ap.error("--msd takes no values or R_MAX N_BINS")

    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("score_rollout.py needs a GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    M, N, W, S = a.members, a.atoms, a.window, a.steps
    base = syn.box_frame(N, seed=1) if N > 128 else syn.chain_frame(N, seed=1)
    traj = syn.ou_trajectory(base, W + S, seed=2)                                    # [W+S, N, 3]: window, then the truth
    wins = syn.ensemble_windows(traj[:W], M, sigma=0.1, seed0=100)                   # [M, W, N, 3]
    model = KernelNN(64, a.kernel_width, 6, 6, 7, 3, 20, 4)
    model.load_state_dict(near_identity_state_dict(64, a.kernel_width, seed=0, kernel_gain=1e-3, feature_gain=0.1))
    model.eval().to(dev)
    eng = RolloutEngine(model, M, N, W, a.threshold, max_steps=S, device=dev, noise_sigma=a.noise_sigma,
                        noise_seed=a.noise_seed)
    truth = torch.from_numpy(traj[W:]).to(dev)                                       # [S, N, 3]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.run(torch.from_numpy(np.ascontiguousarray(wins.transpose(1, 0, 2, 3))), torch.from_numpy(syn.amino_acids(N, seed=1)), S)
    torch.cuda.synchronize()
    produce_s = time.perf_counter() - t0                                             # (includes reset: graph probe + capture)

    score = eng.score(truth)                                                         # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        score = eng.score(truth)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    c = score.cpu()
    pair_tests = S * M * N * (N + 1)                                                 # i <= j, forecast and truth
    best = min(ms)

    def series(x):
        return [None if not np.isfinite(v) else float(v) for v in x[::a.every].tolist()]

    def finite(x):
        return [None if not np.isfinite(v) else float(v) for v in x.tolist()]

    dist = {}
    if a.rdf is not None and S > 0:
        from molecular_dynamics_neural_operator_amd.forecast import pair_histogram, radius_of_gyration
        r_max, n_bins = float(a.rdf[0]), int(a.rdf[1])
        fh = eng.pair_histogram(r_max, n_bins).sum((0,))                             # counts [M, n_bins] over the steps
        th = pair_histogram(truth, r_max, n_bins, box=eng.box).sum((0,))             # counts [n_bins]
        rg, rg_truth = eng.radius_of_gyration(), radius_of_gyration(truth)
        dist = {"rdf_r_max": r_max, "rdf_bins": n_bins,
                "pair_distance_total_variation": finite(fh.total_variation(th).cpu()),
                "rg_first_step": finite(rg[0].cpu()), "rg_last_step": finite(rg[-1].cpu()),
                "rg_truth_first_last": finite(rg_truth[[0, -1]].cpu())}

    if a.msd is not None and S > 1:
        from molecular_dynamics_neural_operator_amd.forecast import displacement_stats
        r_max, n_bins = (float(a.msd[0]), int(a.msd[1])) if a.msd else (None, 0)
        fd = eng.displacement_stats(r_max=r_max, n_bins=n_bins)                      # [M, L] over the default lags
        td = displacement_stats(truth, fd.lags.tolist(), r_max=r_max, n_bins=n_bins) # [1, L]
        dist.update({"msd_lags": fd.lags.tolist(), "msd_forecast_mean": finite(fd.msd().nanmean(0).cpu()),
                     "msd_truth": finite(td.msd()[0].cpu()),
                     "alpha2_forecast_mean": finite(fd.non_gaussian().nanmean(0).cpu()),
                     "alpha2_truth": finite(td.non_gaussian()[0].cpu())})
        if n_bins:
            dist.update({"msd_r_max": r_max, "msd_bins": n_bins,
                         "displacement_total_variation_mean": finite(fd.total_variation(td).nanmean(0).cpu())})

    if a.ensemble and S > 0:
        es = eng.ensemble_score(truth)                                               # one row per step
        pooled = es.sum()
        spread = es.spread().cpu()
        dist.update({"ensemble_rmse_of_mean": series(es.rmse().cpu()), "ensemble_spread": series(spread),
                     "ensemble_spread_skill": series(es.spread_skill().cpu()), "ensemble_crps": series(es.crps().cpu()),
                     "ensemble_crps_fair": series(es.crps(fair=True).cpu()),
                     "ensemble_spread_skill_pooled": finite(pooled.spread_skill().cpu())[0],
                     "ensemble_rank_flatness_pooled": finite(pooled.rank_flatness().cpu())[0],
                     "ensemble_invalid_samples": int(es.n_invalid.sum()), "noise_sigma": a.noise_sigma})
        if not bool(spread.nan_to_num(1.0).any()):
            dist["ensemble_note"] = ("spread 0: the members coincide bit for bit (noise_sigma = 0 and one starting window), so "
                                     "they carry no uncertainty, the spread-skill ratio is 0 and the CRPS is the mean absolute "
                                     "error; run with --noise-sigma")
        elif a.noise_sigma == 0.0:
            dist["ensemble_note"] = ("noise_sigma = 0: the members differ only by their perturbed starting windows, the spread "
                                     "is what the model keeps of that; run with --noise-sigma for a stochastic ensemble")

    if a.coverage is not None and S > 0:
        cr = eng.cross_rmsd(truth, matrix=False)                                     # nearest [S, M], cover [M, S]
        dist.update({"coverage_radius": a.coverage, "coverage_precision": finite(cr.precision(a.coverage).cpu()),
                     "coverage": finite(cr.coverage(a.coverage).cpu()),
                     "nearest_true_frame_rmsd_median": finite(cr.nearest.nanmedian(0).values.cpu())})

    if a.contacts is not None and S > 0:
        from molecular_dynamics_neural_operator_amd import forecast as fc
        run = eng.pair_statistics(moments=False).total()                             # count i32 [M, N, N] over the run
        tru = fc.pair_statistics(truth[:, None], a.threshold, box=eng.box, moments=False).total()
        far = (torch.arange(N, device=dev)[:, None] - torch.arange(N, device=dev)[None, :]).abs() >= a.contacts
        native_map = (tru.probability() >= 0.5) & far                                # [1, N, N]
        own_map = (run.probability() >= 0.5) & far                                   # [M, N, N]
        kept = fc._ratio((own_map & native_map).sum((1, 2)), native_map.sum((1, 2)).expand(M))
        spurious = fc._ratio((own_map & ~native_map).sum((1, 2)), own_map.sum((1, 2)))
        native = fc.ContactPairs.from_statistics(tru, 0.5, a.contacts)              # the one read-back
        q_run, q_truth = eng.contact_series(native), fc.contact_series(truth[:, None], native, box=eng.box)
        some = [l for l in (0, 1, 2, 5, 10, 20, 50, 100, 200, 500) if l < S]
        s_run, s_truth = q_run.correlation(some).survival(), q_truth.correlation(some).survival()
        dist.update({"contacts_min_separation": a.contacts, "contacts_native_pairs": len(native),
                     "contact_map_error": finite(run.map_error(tru, a.contacts).cpu()),
                     "native_contacts_kept": finite(kept.cpu()), "contacts_not_native": finite(spurious.cpu()),
                     "q_mean": finite(q_run.fraction().mean(0).cpu()), "q_mean_truth": finite(q_truth.fraction().mean(0).cpu())[0],
                     "contact_survival_lags": some, "contact_survival_mean": finite(s_run.nanmean(0).cpu()),
                     "contact_survival_truth": finite(s_truth[0].cpu())})

    if a.sasa is not None and S > 0:
        from molecular_dynamics_neural_operator_amd import forecast as fs
        radius, probe, n_points = (float(a.sasa[0]), float(a.sasa[1]), int(a.sasa[2])) if a.sasa else (1.9, 1.4, 96)
        spheres = fs.Spheres(radius, probe=probe, n_points=n_points, n_atoms=N)
        run, tru = eng.surface_area(spheres), fs.surface_area(truth[:, None], spheres, box=eng.box)
        total, total_truth = run.total(), tru.total()                                # f64 [S, M], [S, 1]
        dist.update({"sasa_radius_probe_points": [radius, probe, n_points],
                     "sasa_total_mean": finite(total.mean(0).cpu()), "sasa_total_std": finite(total.std(0, unbiased=False).cpu()),
                     "sasa_total_mean_truth": finite(total_truth.mean(0).cpu())[0],
                     "sasa_total_std_truth": finite(total_truth.std(0, unbiased=False).cpu())[0],
                     "sasa_burial_rms_difference": finite(run.difference(tru).cpu())})

    if a.equivariance is not None:
        from molecular_dynamics_neural_operator_amd import ops
        from molecular_dynamics_neural_operator_amd.dataset import PairData
        from molecular_dynamics_neural_operator_amd.training import RigidAugment, equivariance_error
        # the start windows as ONE collated batch of M samples, graph and attributes of the newest frame (construct_pairdata)
        xw = torch.from_numpy(np.ascontiguousarray(wins.transpose(1, 0, 2, 3))).to(dev).reshape(W, M * N, 3)
        ei = ops.radius_graph(xw[-1].contiguous(), N, a.threshold).to_edge_index()
        start = PairData(torch.from_numpy(syn.amino_acids(N, seed=1)).to(dev).repeat(M), xw, None,
                         torch.cat([xw[-1][ei[0]], xw[-1][ei[1]]], dim=1), ei)
        start.num_graphs, start.sample_ids, start.rows_per_sample, start.edge_frame = M, np.arange(M), N, -1
        aug = RigidAugment(seed=a.noise_seed, translate=a.equivariance_translate)
        errs = [equivariance_error(model, start, aug, epoch=k) for k in range(a.equivariance)]
        rms, rel = torch.stack([e_.rms for e_ in errs]), torch.stack([e_.relative() for e_ in errs])      # [K, M]
        dist.update({"equivariance_motions": a.equivariance, "equivariance_translate": a.equivariance_translate,
                     "equivariance_rms_mean": float(rms.mean()), "equivariance_rms_max": float(rms.max()),
                     "equivariance_relative_mean": float(rel.mean()), "equivariance_relative_max": float(rel.max()),
                     "equivariance_step_rms_mean": float(errs[0].step_rms.mean())})

    internal = None
    if a.internal is not None and S > 0:
        from molecular_dynamics_neural_operator_amd import forecast as fc
        min_sep, stride = a.internal or (3, 4)
        ft = fc.Featurizer.backbone(N, min_sep, stride).to(dev)
        t_feat = fc.internal_coordinates(truth, ft, box=eng.box)                     # [S, D]
        f_feat = eng.internal_coordinates(ft)                                        # [S, M, D]
        lo, hi = fc.feature_ranges(t_feat)                                           # the truth's own range per column
        ic_bins, nb = 32, ft.n_bonds
        tv = fc.feature_histograms(f_feat, lo, hi, ic_bins).total_variation(fc.feature_histograms(t_feat, lo, hi, ic_bins))
        bonds = fc.feature_histograms(f_feat[..., :nb].contiguous(), min(lo[:nb]), max(hi[:nb]), 1) if nb else None
        dist.update({"internal_min_separation": min_sep, "internal_stride": stride, "internal_features": ft.dim(),
                     "internal_bins": ic_bins, "internal_total_variation_max": finite(tv.max(1).values.cpu()),
                     "internal_total_variation_median": finite(tv.nanmedian(1).values.cpu()),
                     "internal_bond_fraction_outside_truth_range": finite(bonds.outside().mean(1).cpu()) if nb else []})
        internal = (ft, t_feat[:, None].contiguous(), f_feat)

    if a.pca is not None and S > 2:
        from molecular_dynamics_neural_operator_amd import forecast as fc
        K, bins = a.pca, 32
        reference = truth[0].contiguous()
        if internal is not None:                                                     # rows of internal coordinates, no reference
            t_al, f_al = internal[1], internal[2]                                    # [S, 1, D], [S, M, D]
        else:
            t_al = fc.superpose(truth, reference)[0]                                 # [S, 1, N, 3]
            f_al = eng.superpose(reference)[0]                                       # [S, M, N, 3]
        t_cov = fc.covariance(t_al)
        t_pc = fc.pca(t_cov, K)
        t_proj, f_proj = fc.project(t_al, t_pc), fc.project(f_al, t_pc)              # [S, 1, K], [S, M, K]
        lo = torch.minimum(t_proj.amin((0, 1)), f_proj.nan_to_num(posinf=0.0, neginf=0.0).amin((0, 1))).cpu()
        hi = torch.maximum(t_proj.amax((0, 1)), f_proj.nan_to_num(posinf=0.0, neginf=0.0).amax((0, 1))).cpu()
        j = 1 if K > 1 else 0
        rng = ((float(lo[0]), float(hi[0])), (float(lo[j]), float(hi[j])))
        t_hist = fc.free_energy(t_proj, 0, j, bins, rng)[1]
        rmsip, tv = [], []
        for m in range(M):                                                           # per member: slice and copy (forecast.covariance pools)
            own = f_al[:, m].contiguous()
            ok = bool(torch.isfinite(own).all())
            rmsip.append(fc.pca(fc.covariance(own), K).rmsip(t_pc) if ok else float("nan"))
            tv.append(float(fc.histogram_total_variation(fc.free_energy(f_proj[:, m], 0, j, bins, rng)[1], t_hist)))
        dist.update({"pca_k": K, "pca_truth_explained_ratio": finite(t_pc.explained_ratio().cpu()),
                     "pca_rmsip_with_truth": finite(np.asarray(rmsip)), "pca_pc12_total_variation": finite(np.asarray(tv)),
                     **({"pca_space": "internal"} if internal is not None else {"pca_truth_rmsf_mean": float(t_cov.rmsf().mean())})})
        if a.tica is not None and 0 < a.tica < S - 1:
            t_tica = fc.tica(t_cov, fc.covariance(t_al, t_cov.mean, a.tica), K)
            f_cov = fc.covariance(f_al) if internal is not None else eng.covariance(reference)
            dist.update({"tica_lag": a.tica, "tica_truth_timescales": finite(t_tica.timescales().cpu())})
            if bool(torch.isfinite(f_cov.sums).all()):
                f_lag = fc.covariance(f_al, f_cov.mean, a.tica) if internal is not None else eng.covariance(reference, f_cov.mean, a.tica)
                f_tica = fc.tica(f_cov, f_lag, K)
                dist["tica_forecast_timescales"] = finite(f_tica.timescales().cpu())
        if a.msm is not None:
            n_states, lag = a.msm
            comps = t_tica if a.tica is not None and 0 < a.tica < S - 1 else t_pc    # the truth's own slow (or principal) coordinates
            if internal is not None:
                disc = fc.discretize(truth, n_states, components=comps, featurizer=internal[0], box=eng.box)
            else:
                disc = fc.discretize(truth, n_states, components=comps, reference=reference)
            t_as, f_as = disc.assign(truth), eng.assign(disc)                        # labels [S], [S, M]
            t_pop, f_pop = t_as.populations(n_states), f_as.populations(n_states)    # [n], [M, n]
            t_counts = fc.transition_counts(t_as.labels, n_states, [lag])
            f_counts = fc.transition_counts(f_as.labels, n_states, [lag]).cpu()
            lead = 3

            def timescales(counts, member=None):
                try:
                    ts = fc.markov_model(counts, member=member).timescales()[:lead]
                except fc.MdnoError:                                                 # (no transition was counted)
                    return []
                return finite(ts)
            dist.update({"msm_states": n_states, "msm_lag": lag, "msm_space": ("internal " if internal is not None else "") + ("tica" if comps is not t_pc else "pca"),
                         "msm_covering_radius": float(disc.radius),
                         "msm_population_total_variation": finite((0.5 * (f_pop - t_pop[None]).abs().sum(1)).cpu()),
                         "msm_fraction_outside_truth_radius": finite(f_as.outside(disc.radius).cpu()),
                         "msm_truth_timescales": timescales(t_counts.cpu()),
                         "msm_forecast_timescales": [timescales(f_counts, m) for m in range(M)],
                         "msm_pairs_skipped": int(f_counts.n_skipped.sum())})

    if a.constrain is not None and S > 0:
        from molecular_dynamics_neural_operator_amd import forecast as fc
        bonds = fc.Featurizer.of(pairs=fc.DistanceConstraints.chain(N, 0.0, 1.0).pairs, n_atoms=N).to(dev)     # the pseudo-bonds
        cons = fc.DistanceConstraints.from_frames(truth, bonds, margin=a.constrain, box=eng.box)
        eng_c = RolloutEngine(model, M, N, W, a.threshold, max_steps=S, device=dev, noise_sigma=a.noise_sigma,
                              noise_seed=a.noise_seed, constraints=cons, constraint_iterations=a.constrain_iterations)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng_c.run(torch.from_numpy(np.ascontiguousarray(wins.transpose(1, 0, 2, 3))), torch.from_numpy(syn.amino_acids(N, seed=1)), S)
        torch.cuda.synchronize()
        produce_c = time.perf_counter() - t0
        cc, rep = eng_c.score(truth).cpu(), eng_c.constraint_report()
        t_b = fc.internal_coordinates(truth, bonds, box=eng.box)
        b_lo, b_hi = float(t_b.min()), float(t_b.max())

        def outside(e):                                                              # share of bond lengths outside the truth's range
            return finite(fc.feature_histograms(e.internal_coordinates(bonds), b_lo, b_hi, 1).outside().mean(1).cpu())
        dist["constrained"] = {
            "margin": a.constrain, "iterations": a.constrain_iterations, "constraints": len(cons), "colours": cons.coloured(dev).n_colours,
            "members_diverged": [int((c.first_nonfinite >= 0).sum()), int((cc.first_nonfinite >= 0).sum())],
            "mean_rmsd": [series(c.rmsd.nanmean(1)), series(cc.rmsd.nanmean(1))],
            "mean_native_fraction": [series(c.native_fraction().nanmean(1)), series(cc.native_fraction().nanmean(1))],
            "mean_jaccard": [series(c.jaccard().nanmean(1)), series(cc.jaccard().nanmean(1))],
            "bond_fraction_outside_truth_range": [outside(eng), outside(eng_c)],
            "mean_viol_in": series(rep.viol_in.mean(1).cpu()), "mean_viol_out": series(rep.viol_out.mean(1).cpu()),
            "mean_sweeps": series(rep.sweeps.double().mean(1).cpu()),
            "produce_s": [produce_s, produce_c], "note": "every pair is [free run, constrained run]"}
        eng_c.close()

    print(json.dumps({
        "members": M, "atoms": N, "steps": S, "window": W, "threshold": a.threshold, "conv_mode": eng.conv_mode,
        "first_nonfinite_step": c.first_nonfinite.tolist(),
        "members_diverged": int((c.first_nonfinite >= 0).sum()),
        "step_index": list(range(0, S, a.every)),
        "mean_mse": series(c.mse.nanmean(1)), "mean_rmsd": series(c.rmsd.nanmean(1)),
        "mean_native_fraction": series(c.native_fraction().nanmean(1)), "mean_jaccard": series(c.jaccard().nanmean(1)),
        "score_ms": best, "score_ms_all": ms, "score_us_per_member_step": best * 1e3 / max(S * M, 1),
        "produce_s": produce_s, "produce_ms_per_member_step": produce_s * 1e3 / max(S * M, 1),
        "score_over_produce": best * 1e-3 / produce_s,
        "pair_tests": pair_tests, "pair_tests_per_s": pair_tests / (best * 1e-3), **dist,
    }))
    eng.close()


if __name__ == "__main__":
    main()
