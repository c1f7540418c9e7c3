"""How good is a rollout?  Forecast frames scored against the true trajectory on the device.

The reference looks at its forecasts on the host after every epoch: `make_propagation_movie` / `get_contact_map`
(graph_kernel.py:416-443) put the forecast's contact map beside the real one, the notebook's `propogate`
(bba_analysis.ipynb:351) records the per-step MSE, and the data set's `rmsd` values (dataset.py:118) colour every plot.
Here the frames of a `RolloutEngine` and the true frames of a `training.DeviceTrajectory` are both resident in HBM, and
one call scores every (step, member) there (csrc/forecast.hip) — 64 members x 1,000 steps without copying a frame back:

    eng.run(windows, x_aminoacid, steps)
    score = eng.score(traj.truth_frames(start, steps))      # = score_forecast(eng.frames(), truth, eng.threshold)
    score.first_nonfinite                                    # i32 [M]: the step at which a member diverged, -1 = never
    score.mse.mean(1), score.jaccard().mean(1)               # per-step ensemble means, still on the device

Definitions, per (step s, member m):
    mse       mean over the 3N coordinates of (frame - truth)^2 — `propogate`'s number, in fp64
    rmsd      after optimal rigid superposition (centroids removed, proper rotations only: a mirror image is not 0)
    contacts  i64 (in the forecast, in the truth, in both): ordered pairs (i, j), diagonal included, closer than
              `threshold` by the radius graph's own test — the non-zeros of `get_contact_map`'s dense matrices
    first_nonfinite[m]  the first step whose forecast frame holds a NaN or Inf (that entry's mse and rmsd are NaN)

One reference quirk is documented, not copied: the movie compares forecast step i with the STORED contact map of
`dataset[i + 1]`, which is that window's FIRST frame (dataset.py:189); here the truth is the frame the forecast
predicts (`DeviceTrajectory.truth_frames`).  The two coincide at window 1.

Distributional scoring.  Past the decorrelation time a forecast and the truth are two different trajectories, and the
numbers above only say so; what can still be asked is whether the forecast samples the right STRUCTURES.  For that the
pair distances of every frame are binned on the device (csrc/observe.hip, include/mdno_observe.h has the rule) and the
per-frame radius of gyration is taken beside them:

    h = eng.pair_histogram(r_max=8.5, n_bins=200).sum((0,))    # PairHistogram: counts i64 [M, 200], summed over the steps
    t = pair_histogram(truth, 8.5, 200, box=eng.box).sum((0,)) # the truth's, from frames [S, N, 3]
    h.total_variation(t)                                        # f64 [M]: 0 = the same distribution of distances, 1 = disjoint
    h.rdf()                                                     # g(r) per member (a box with three periodic axes)
    eng.radius_of_gyration()                                    # f64 [S, M]

Dynamical scoring.  A forecast can sample the right structures and still freeze, or heat up: whether it has the right
DYNAMICS is asked of the displacements over a time lag, averaged over all time origins (csrc/dynamics.hip,
include/mdno_dynamics.h has the rule):

    d = eng.displacement_stats(r_max=4.0, n_bins=64)            # DisplacementStats over ~33 log-spaced lags
    t = displacement_stats(truth, d.lags.tolist(), r_max=4.0, n_bins=64)
    d.msd(), d.non_gaussian()                                   # f64 [M, L]: MSD(tau) and alpha_2(tau)
    d.total_variation(t)                                        # f64 [M, L]: the self van Hove functions compared per lag
    d.diffusion_coefficient(dt)                                 # f64 [M]: slope of MSD / 6
    c, lags = eng.velocity_autocorrelation()                    # f64 [M, L]: <v(t) . v(t + tau)>, finite differences
    unwrap(frames, box)                                         # for truth data that arrives wrapped into its cell

Ensemble verification.  Everything above scores each member on its own.  Whether a stochastic ensemble (`noise_sigma`) is
CALIBRATED — its spread as large as the error of its mean, the truth indistinguishable from one more member — is asked of
the members together, per step over every atom and component (csrc/ensemble.hip, include/mdno_ensemble.h has the rule):

    e = eng.ensemble_score(truth)                               # EnsembleScore, one row per step
    e.rmse(), e.spread(), e.spread_skill()                      # f64 [S]: spread-skill 1 = calibrated, < 1 under-dispersed
    e.crps(), e.crps(fair=True)                                 # f64 [S]
    e.sum().rank_flatness()                                     # the pooled rank histogram's distance from uniform

Structural coverage.  Past the decorrelation time a free run and the truth are different trajectories and a same-step RMSD
only says so.  Whether the run visits the RIGHT STRUCTURES is asked of every produced frame against every true frame
(csrc/conformations.hip on the fp64 matrix pipe, include/mdno_conformations.h has the rule):

    c = eng.cross_rmsd(truth, matrix=False)                     # CrossRmsd: nearest [S, M], cover [M, Fb] and their indices
    c.precision(2.0), c.coverage(2.0)                           # f64 [M]: frames near some true frame / true frames visited
    cross_rmsd(frames, folded[None]).to_reference(0)            # f64 [S, M]: the RMSD time series to one structure

Essential dynamics.  Whether the run moves along the right collective coordinates, with the right amplitudes and the right
slow timescales, is asked of the principal components of the superposed trajectory and of their time-lagged version
(csrc/essential.hip: the covariance is one fp64 GEMM over the rows on the matrix pipe; include/mdno_essential.h has the rule):

    aligned, rmsd = eng.superpose(reference)                    # every frame in the reference's frame of reference
    pc = pca(covariance(superpose(truth, reference)[0]), 10)    # Components of the truth: values, vectors [3 N, 10]
    pca(covariance(aligned[:, m].contiguous()), 10).rmsip(pc)   # member m's subspace against the truth's
    free_energy(project(aligned, pc), 0, 1)                     # F [bins, bins] in kT over PC1/PC2, counts, edges
    tica(c0, covariance(x, c0.mean, lag=10), 5).timescales()    # implied timescales in steps

Markov state models.  Whether the run populates the truth's STATES with the right weights and hops between them at the right
rates is asked of a partition of the projected (or superposed) space: cluster the truth, assign every frame of truth and run
to the nearest centre (csrc/markov.hip: the inner products on the fp64 matrix pipe; include/mdno_markov.h has the rule), count
the transitions at a lag on the device and estimate the model on the host:

    disc = discretize(truth, 100, components=tc)                # Discretization: k-centres (or k-means) in the truth's TICA space
    a = eng.assign(disc)                                        # Assignment: labels i32, dist2 f64 [S, M]
    a.outside(disc.radius)                                      # f64 [M]: the share of the run off the truth's manifold
    counts = transition_counts(a.labels, 100, [10, 20, 40])     # TransitionCounts: i64 [L, M, n, n], exact
    msm = markov_model(counts)                                  # MarkovModel: active set, T, spectrum, stationary distribution
    msm.timescales(5), msm.chapman_kolmogorov(counts, 1)        # implied timescales in steps; T^2 against the lag-20 estimate
    msm.population_total_variation(markov_model(truth_counts))  # 0 = the truth's state weights, 1 = disjoint

Internal coordinates.  Superposing onto one frame mixes the overall rotation into every coordinate once a structure leaves
that frame's basin; pair distances and the cos / sin of (pseudo-)dihedrals do not depend on a reference frame at all
(csrc/internal.hip: fp64 on the fp32 coordinates in a fixed order; include/mdno_internal.h has the rule), and they say
whether the produced frames are physical chains:

    ft = Featurizer.backbone(N, min_separation=3, stride=4)     # pseudo-bonds, strided pairs, pseudo-angles, pseudo-dihedrals
    x = eng.internal_coordinates(ft)                            # f32 [S, M, D] = internal_coordinates(eng.frames(), ft, box=eng.box)
    h = feature_histograms(x, *feature_ranges(truth_x), 32)     # FeatureHistograms: counts i64 [M, D, 34]
    h.total_variation(truth_h), h.outside()                     # f64 [M, D]: per column against the truth; share outside its range
    disc = discretize(truth, 100, components=tc, featurizer=ft) # states in internal coordinates: no reference frame

Distance constraints.  The scores above say, after the fact, that a run has left the chain manifold; a SHAKE-style projection
keeps a produced frame on it before it is fed back (csrc/constrain.hip: whole frames staged in LDS as fp64, the constraints
walked colour by colour; include/mdno_constrain.h has the rule):

    cons = DistanceConstraints.from_frames(truth, ft, margin=0.1)  # every listed pair inside the truth's own range
    frames, rep = project_constraints(frames, cons, iterations=8)  # ConstraintReport: sweeps i32, viol_in, viol_out f64 [S, M]
    RolloutEngine(model, M, N, W, constraints=cons)                # the same projection at the end of every step

Contact statistics.  The three pictures a fast folder is judged by — the contact-probability map of the run beside the
truth's, the fraction of native contacts Q(t) against a native set fixed ONCE, and how long a contact lives — need the
reduction over time, not one dense map per frame (csrc/contacts.hip: per-pair accumulators in registers over blocks of
steps, one bit per (member, pair, step); include/mdno_contacts.h has the rule):

    st = eng.pair_statistics(block_len=64)                      # PairStatistics: count i32, sum_r, sum_r2 f64 [Bk, M, N, N]
    tr = pair_statistics(truth[:, None], eng.threshold)         # the truth as one member
    st.total().map_error(tr.total(), min_separation=3)          # f64 [M]: mean |P_run - P_truth| over the pairs
    native = ContactPairs.native(folded, 8.0, factor=1.2)       # or ContactPairs.from_statistics(tr): P >= 0.5 in the truth
    cs = eng.contact_series(native)                             # ContactSeries: bits [M, P, S / 64], per_frame i32 [S, M]
    cs.fraction()                                               # Q(t), f64 [S, M]
    cc = cs.correlation()                                       # ContactCorrelation over ~33 log-spaced lags
    cc.survival(), cc.lifetime(dt)                              # f64 [M, L]: P(contact at t + lag | contact at t); f64 [M]

Solvent-accessible surface.  A chain can stay connected, keep its contact map and its radius of gyration and still turn its
core inside out: which SIDE of an atom is covered is asked of Shrake and Rupley's count of exposed sphere points per atom
(csrc/surface.hip: one wave per atom, neighbours compacted by ballot, one buried bit per point; include/mdno_surface.h has the
rule):

    sp = Spheres(radii, probe=1.4, n_points=96)                 # expanded radii, the golden-section spiral, reach — on the host
    area = eng.surface_area(sp)                                 # SurfaceArea: counts i32 [S, M, N], -1 for a non-finite atom
    area.total(), area.per_group(residue, n_residues)           # f64 [S, M], [S, M, n_residues]: 4 pi R^2 count / P summed
    area.difference(surface_area(truth[:, None], sp))           # f64 [M]: RMS over the atoms of the mean burial against the truth's
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple

import torch

from . import ops
from ._args import INT_MAX, device_tensor, integer, on_device, tensor
from ._lib import MdnoError


def _ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """num / den in f64 (broadcast), NaN where den == 0 (no host read, no exception); a NaN or Inf in num passes through."""
    num, den = torch.broadcast_tensors(num.to(torch.float64), den.to(torch.float64))
    return torch.where(den == 0, torch.full_like(den, float("nan")), num / torch.where(den == 0, torch.ones_like(den), den))


@dataclass
class ForecastScore:
    mse: torch.Tensor                 # f64 [S, M]
    rmsd: torch.Tensor                # f64 [S, M]
    contacts: torch.Tensor            # i64 [S, M, 3]: forecast, truth, both
    first_nonfinite: torch.Tensor     # i32 [M]

    _ratio = staticmethod(_ratio)

    def precision(self) -> torch.Tensor:
        """Contacts in both / contacts in the forecast: f64 [S, M]."""
        return _ratio(self.contacts[..., 2], self.contacts[..., 0])

    def recall(self) -> torch.Tensor:
        """Contacts in both / contacts in the truth: f64 [S, M]."""
        return _ratio(self.contacts[..., 2], self.contacts[..., 1])

    def native_fraction(self) -> torch.Tensor:
        """The fraction of the true ("native") contacts the forecast keeps: both / truth, f64 [S, M]."""
        return self.recall()

    def jaccard(self) -> torch.Tensor:
        """Contacts in both / contacts in either: f64 [S, M]."""
        c = self.contacts
        return _ratio(c[..., 2], c[..., 0] + c[..., 1] - c[..., 2])

    def cpu(self) -> "ForecastScore":
        return ForecastScore(self.mse.cpu(), self.rmsd.cpu(), self.contacts.cpu(), self.first_nonfinite.cpu())

    @staticmethod
    def cat(parts: Sequence["ForecastScore"]) -> "ForecastScore":
        """Scores of disjoint member ranges of the same steps, members in order."""
        return ForecastScore(torch.cat([p.mse for p in parts], 1), torch.cat([p.rmsd for p in parts], 1),
                             torch.cat([p.contacts for p in parts], 1), torch.cat([p.first_nonfinite for p in parts], 0))


def score_forecast(frames: torch.Tensor, truth: torch.Tensor, threshold: float = 8.0, form: str = "auto",
                   box=None) -> ForecastScore:
    """frames f32 [S, M, N, 3] (device) against truth [S, N, 3] (the same for every member) or [S, M, N, 3].
    Asynchronous on the current stream: nothing is read back, nothing waits for the device.  CPU tensors, wrong ranks
    and mismatched S, M or N raise `MdnoError` before any device work.  `form` forces one of the two kernel forms
    (ops.forecast_score); the default chooses by N.  `box` = (Lx, Ly, Lz), 0 for an open axis: contacts are counted
    under the minimum-image rule of a periodic cell (include/mdno_pbc.h); mse, rmsd and first_nonfinite are unchanged."""
    return ForecastScore(*ops.forecast_score(frames, truth, threshold, form, box))


def contact_maps(frames: torch.Tensor, threshold: float = 8.0, box=None) -> torch.Tensor:
    """u8 [..., N, N] for frames [..., N, 3]: the reference's `get_contact_map`, for the movie.  `box`: a periodic cell
    (Lx, Ly, Lz), contacts by the minimum image."""
    return ops.contact_maps(frames, threshold, box)


@dataclass
class PairHistogram:
    """Histograms of pair distances (ops.pair_histogram): `counts` i64 [..., n_bins] of UNORDERED pairs i < j per bin of
    width r_max / n_bins over [0, r_max), under `box` (None: open).  `n_frames`: how many frames were summed into every
    row (1 as computed; `sum` multiplies it).  Every method runs in fp64 on the device of `counts` and reads nothing
    back."""
    counts: torch.Tensor
    r_max: float
    n_bins: int
    n_atoms: int
    box: Optional[Tuple[float, float, float]] = None
    n_frames: int = 1

    def edges(self) -> torch.Tensor:
        """Bin edges r_0 = 0 .. r_n = r_max: f64 [n_bins + 1], edge b = b * r_max / n_bins."""
        k = torch.arange(self.n_bins + 1, dtype=torch.float64, device=self.counts.device)
        return k * self.r_max / self.n_bins

    def centers(self) -> torch.Tensor:
        """Bin midpoints: f64 [n_bins]."""
        e = self.edges()
        return 0.5 * (e[:-1] + e[1:])

    def sum(self, dims) -> "PairHistogram":
        """Counts summed over the given LEADING dimensions (steps, members, windows): the histogram of all those frames."""
        dims = (dims,) if isinstance(dims, int) else tuple(int(d) for d in dims)
        lead = self.counts.dim() - 1
        norm = sorted({d + lead if d < 0 else d for d in dims})
        if len(norm) != len(dims) or any(not 0 <= d < lead for d in norm):
            raise MdnoError(f"PairHistogram.sum: dims {dims} are not distinct leading dimensions of counts "
                            f"{tuple(self.counts.shape)}")
        frames = self.n_frames
        for d in norm:
            frames *= self.counts.shape[d]
        counts = self.counts.sum(norm) if norm else self.counts
        return PairHistogram(counts, self.r_max, self.n_bins, self.n_atoms, self.box, frames)

    def distribution(self) -> torch.Tensor:
        """counts / their total per row: f64 [..., n_bins], the distribution p(r) of the pair distances below r_max;
        NaN where the total is 0."""
        c = self.counts.to(torch.float64)
        return _ratio(c, c.sum(-1, keepdim=True).expand_as(c))

    def rdf(self) -> torch.Tensor:
        """The radial distribution function g(r) per bin: f64 [..., n_bins], counts over what an ideal gas of the same
        density would put into the bin's shell, n_frames * N (N - 1) / 2 * (4 pi / 3) (r_{b+1}^3 - r_b^3) / (Lx Ly Lz).
        Defined for a box with three periodic axes only (r_max <= L / 2 holds by construction, so a shell never meets
        its own image); an open or slab box has no density to normalise by: use `distribution()`."""
        if self.box is None or not all(L > 0.0 for L in self.box):
            raise MdnoError(f"rdf: box={self.box} is not periodic in all three axes, so there is no bulk density to "
                            f"normalise by; use distribution() for an open or slab system")
        e = self.edges()
        shell = (4.0 * math.pi / 3.0) * (e[1:] ** 3 - e[:-1] ** 3)
        pairs = self.n_frames * (self.n_atoms * (self.n_atoms - 1) / 2.0)
        ideal = shell * (pairs / (self.box[0] * self.box[1] * self.box[2]))
        return self.counts.to(torch.float64) / ideal

    def total_variation(self, other: "PairHistogram") -> torch.Tensor:
        """0.5 * sum_b |p_b - q_b| of the two `distribution()`s (leading shapes broadcast): 0 for equal distributions,
        1 for disjoint ones.  Both histograms must have the same r_max and n_bins."""
        if not isinstance(other, PairHistogram) or other.r_max != self.r_max or other.n_bins != self.n_bins:
            raise MdnoError("total_variation: the two histograms must have the same r_max and n_bins")
        return 0.5 * (self.distribution() - other.distribution()).abs().sum(-1)

    def cpu(self) -> "PairHistogram":
        return PairHistogram(self.counts.cpu(), self.r_max, self.n_bins, self.n_atoms, self.box, self.n_frames)

    @staticmethod
    def cat(parts: Sequence["PairHistogram"], dim: int = 1) -> "PairHistogram":
        """Histograms of disjoint member ranges of the same steps, members in order."""
        p = parts[0]
        return PairHistogram(torch.cat([q.counts for q in parts], dim), p.r_max, p.n_bins, p.n_atoms, p.box, p.n_frames)


def pair_histogram(frames: torch.Tensor, r_max: float, n_bins: int = 200, box=None, form: str = "auto") -> PairHistogram:
    """frames f32 [..., N, 3] (device) -> `PairHistogram` with counts i64 [..., n_bins], one row per frame (sum over steps
    or members with `.sum`).  `box` = (Lx, Ly, Lz), 0 for an open axis: distances by the minimum image
    (include/mdno_observe.h); every periodic axis must be >= 2 * r_max.  Asynchronous on the current stream; CPU tensors
    and bad arguments raise `MdnoError` before any device work."""
    r_max, n_bins, box = ops.check_histogram_args(r_max, n_bins, box)
    counts = ops.pair_histogram(frames, r_max, n_bins, box, form)
    return PairHistogram(counts, r_max, n_bins, int(frames.shape[-2]), box)


def radius_of_gyration(frames: torch.Tensor) -> torch.Tensor:
    """f64 [...] for frames f32 [..., N, 3] (device): sqrt(mean_i |x_i - centroid|^2), NaN for a non-finite frame."""
    return ops.radius_of_gyration(frames)


@dataclass
class DisplacementStats:
    """Displacement statistics per member and lag (ops.displacement_stats): `sum2`, `sum4` f64 [M, L], the sums of
    |x_i(t + lag) - x_i(t)|^2 and of its square over origins and atoms; `counts` i64 [M, L, n_bins] (None without a
    histogram) of the displacements per bin of width r_max / n_bins over [0, r_max); `lags` i64 [L]; `n_samples` i64 [L],
    origins times atoms of every lag.  Every method runs in fp64 on the device of the sums and reads nothing back."""
    sum2: torch.Tensor
    sum4: torch.Tensor
    counts: Optional[torch.Tensor]
    lags: torch.Tensor
    n_samples: torch.Tensor
    r_max: Optional[float] = None
    n_bins: int = 0

    def _n(self) -> torch.Tensor:
        return self.n_samples.to(torch.float64).expand_as(self.sum2)

    def msd(self) -> torch.Tensor:
        """Mean squared displacement <r^2>(lag): f64 [M, L]; NaN for a lag without samples."""
        return _ratio(self.sum2, self._n())

    def non_gaussian(self) -> torch.Tensor:
        """alpha_2(lag) = 3 <r^4> / (5 <r^2>^2) - 1: f64 [M, L], 0 for Gaussian displacements in three dimensions; NaN
        where <r^2> is 0 (lag 0) or there is no sample."""
        r2 = self.msd()
        r4 = _ratio(self.sum4, self._n())
        return 3.0 * r4 / (5.0 * r2 * r2) - 1.0

    def _need_counts(self, what: str) -> torch.Tensor:
        if self.counts is None or self.n_bins <= 0 or self.r_max is None:
            raise MdnoError(f"{what}: no histogram was taken (n_bins=0); pass r_max and n_bins to displacement_stats")
        return self.counts.to(torch.float64)

    def edges(self) -> torch.Tensor:
        """Bin edges 0 .. r_max: f64 [n_bins + 1]."""
        self._need_counts("edges")
        k = torch.arange(self.n_bins + 1, dtype=torch.float64, device=self.sum2.device)
        return k * self.r_max / self.n_bins

    def van_hove(self) -> torch.Tensor:
        """The self part of the van Hove function as a density in r: counts / (n_samples * dr), f64 [M, L, n_bins]; its
        integral over [0, r_max) is the fraction of the displacements below r_max."""
        c = self._need_counts("van_hove")
        den = (self.n_samples.to(torch.float64)[None, :, None] * (self.r_max / self.n_bins)).expand_as(c)
        return torch.where(den == 0, torch.full_like(c, float("nan")), c / den)

    def distribution(self) -> torch.Tensor:
        """counts / their total per (member, lag): f64 [M, L, n_bins]; NaN where the total is 0."""
        c = self._need_counts("distribution")
        return _ratio(c, c.sum(-1, keepdim=True).expand_as(c))

    def total_variation(self, other: "DisplacementStats") -> torch.Tensor:
        """0.5 * sum_b |p_b - q_b| of the two `distribution()`s per lag: f64 [M, L] (members broadcast, so a truth with
        M = 1 serves every member); 0 for equal distributions, 1 for disjoint ones.  Both must have the same lags, r_max
        and n_bins."""
        if not isinstance(other, DisplacementStats) or other.r_max != self.r_max or other.n_bins != self.n_bins or \
                tuple(other.lags.shape) != tuple(self.lags.shape):
            raise MdnoError("total_variation: the two statistics must have the same lags, r_max and n_bins")
        return 0.5 * (self.distribution() - other.distribution()).abs().sum(-1)

    def diffusion_coefficient(self, dt: float = 1.0, first: int = 0, last: Optional[int] = None) -> torch.Tensor:
        """The least-squares slope (with intercept) of MSD over lags * dt, divided by 6: f64 [M].  `first`, `last`: the
        slice lags[first:last] that is fitted (leave the ballistic short lags out); needs two distinct lags."""
        x = self.lags[first:last].to(torch.float64) * float(dt)
        y = self.msd()[:, first:last]
        if x.numel() < 2:
            raise MdnoError(f"diffusion_coefficient: lags[{first}:{last}] holds {x.numel()} lag(s), a slope needs two")
        xc = x - x.mean()
        return (xc * (y - y.mean(1, keepdim=True))).sum(1) / (xc * xc).sum() / 6.0

    def cpu(self) -> "DisplacementStats":
        return DisplacementStats(self.sum2.cpu(), self.sum4.cpu(), None if self.counts is None else self.counts.cpu(),
                                 self.lags.cpu(), self.n_samples.cpu(), self.r_max, self.n_bins)

    @staticmethod
    def cat(parts: Sequence["DisplacementStats"]) -> "DisplacementStats":
        """Statistics of disjoint member ranges of the same steps and lags, members in order."""
        p = parts[0]
        counts = None if p.counts is None else torch.cat([q.counts for q in parts], 0)
        return DisplacementStats(torch.cat([q.sum2 for q in parts], 0), torch.cat([q.sum4 for q in parts], 0), counts,
                                 p.lags, p.n_samples, p.r_max, p.n_bins)


def default_lags(S: int, span: int = 0):
    """0 and about 32 log-spaced distinct integers from 1 up to (S - 1 - span) // 2 (half the trajectory: every lag keeps
    at least as many origins as it is long), ascending; [0] for a trajectory too short for a lag."""
    top = (int(S) - 1 - span) // 2
    if top < 1:
        return [0]
    lags = {0, top}
    for k in range(32):
        lags.add(int(round(top ** (k / 31.0))))
    return sorted(lags)


def _lag_tensors(lags, S: int, N: int, stride: int, span: int, device):
    n = [ops.n_origins(S, tau, stride, span) * N for tau in lags]
    return (torch.tensor(lags, dtype=torch.int64, device=device), torch.tensor(n, dtype=torch.int64, device=device))


def displacement_stats(frames: torch.Tensor, lags=None, origin_stride: int = 1, remove_com: bool = False, r_max=None,
                       n_bins: int = 0) -> DisplacementStats:
    """frames f32 [S, M, N, 3] (device; [S, N, 3] is M = 1) -> `DisplacementStats` over `lags` (default: `default_lags`),
    every lag averaged over the origins t = 0, origin_stride, ... (include/mdno_dynamics.h).  `remove_com`: the centroid's
    motion is subtracted.  `r_max`, `n_bins` > 0: also the histogram of the displacements (the self van Hove function).
    Asynchronous on the current stream; CPU tensors and bad arguments raise `MdnoError` before any device work."""
    if not torch.is_tensor(frames) or frames.dim() not in (3, 4):
        device_tensor(frames, "frames", (3, 4), last=3)           # raises: no tensor, a CPU tensor or this shape
    S, N = int(frames.shape[0]), int(frames.shape[-2])
    lags = default_lags(S) if lags is None else ops.check_lags(lags, max(S, 1))
    stride = ops.check_origin_stride(origin_stride)
    sum2, sum4, counts = ops.displacement_stats(frames, lags, stride, remove_com, r_max, n_bins)
    lt, nt = _lag_tensors(lags, S, N, stride, 0, sum2.device)
    return DisplacementStats(sum2, sum4, counts, lt, nt, float(r_max) if counts is not None else None, int(n_bins))


def velocity_autocorrelation(frames: torch.Tensor, lags=None, origin_stride: int = 1, remove_com: bool = False,
                             normalized: bool = False):
    """frames f32 [S, M, N, 3] (device) -> (C f64 [M, L], lags i64 [L]): C(lag) = the mean over origins and atoms of
    v_i(t) . v_i(t + lag), v(t) = x(t + 1) - x(t) (divide by dt^2 for physical units).  `normalized`: C(lag) / C(0), which
    needs lag 0 among the lags (the default set has it).  Lags in 0 .. S - 2."""
    if not torch.is_tensor(frames) or frames.dim() not in (3, 4):
        device_tensor(frames, "frames", (3, 4), last=3)
    S, N = int(frames.shape[0]), int(frames.shape[-2])
    lags = default_lags(S, 1) if lags is None else ops.check_lags(lags, max(S, 2), 1, "velocity_autocorrelation")
    stride = ops.check_origin_stride(origin_stride, "velocity_autocorrelation")
    corr = ops.velocity_autocorrelation(frames, lags, stride, remove_com)
    lt, nt = _lag_tensors(lags, S, N, stride, 1, corr.device)
    c = _ratio(corr, nt.to(torch.float64).expand_as(corr))
    if normalized:
        if 0 not in lags:
            raise MdnoError("velocity_autocorrelation: normalized=True needs lag 0 among the lags")
        c = c / c[:, lags.index(0)][:, None]
    return c, lt


def unwrap(frames: torch.Tensor, box) -> torch.Tensor:
    """Frames wrapped into the periodic cell `box` = (Lx, Ly, Lz), 0 for an open axis -> the unwrapped trajectory
    (ops.unwrap_frames), so that displacements mean something for data that arrives wrapped."""
    return ops.unwrap_frames(frames, box)


@dataclass
class EnsembleScore:
    """The verification sums of an ensemble per step (ops.ensemble_score; include/mdno_ensemble.h has the rule): `sums`
    f64 [S, 4] over the step's samples (atom, component) of the squared error of the ensemble mean, the unbiased ensemble
    variance, sum_m |x_m - y| and sum_{m<k} |x_m - x_k|; `rank_hist` i64 [S, M + 1], the truth's rank among the sorted
    members; `n_invalid` i64 [S], samples left out because a value is not finite (their row of `sums` is NaN); `n_ties`
    i64 [S], samples where a member equals the truth; `members` = M; `samples_per_step` = 3 N; `n_steps`: how many steps
    were pooled into every row (1 as computed; `sum` raises it).  Every method runs in fp64 on the device of the sums and
    reads nothing back; a row without samples gives NaN."""
    sums: torch.Tensor
    rank_hist: torch.Tensor
    n_invalid: torch.Tensor
    n_ties: torch.Tensor
    members: int
    samples_per_step: int
    n_steps: int = 1

    def _mean(self, c: int) -> torch.Tensor:
        n = torch.full_like(self.sums[:, c], float(self.samples_per_step * self.n_steps))
        return _ratio(self.sums[:, c], n)

    def rmse(self) -> torch.Tensor:
        """Root mean squared error of the ensemble mean: f64 [S]."""
        return self._mean(0).sqrt()

    def spread(self) -> torch.Tensor:
        """Root of the mean unbiased ensemble variance: f64 [S]; 0 for one member."""
        return self._mean(1).sqrt()

    def spread_skill(self) -> torch.Tensor:
        """sqrt((M + 1) / M) * spread / rmse: f64 [S]; 1 for a calibrated ensemble (the truth one more draw from the
        members' distribution), below 1 under-dispersed, above 1 over-dispersed."""
        M = self.members
        return math.sqrt((M + 1) / M) * self.spread() / self.rmse()

    def crps(self, fair: bool = False) -> torch.Tensor:
        """The continuous ranked probability score of the empirical distribution of the members, averaged over the
        samples: mean_m |x_m - y| - sum_{m<k} |x_m - x_k| / M^2, f64 [S].  `fair`: M (M - 1) in place of M^2, the
        estimator whose expectation does not depend on M (NaN for one member)."""
        M = self.members
        first = self._mean(2) / M
        if fair and M < 2:
            return torch.full_like(first, float("nan"))
        return first - self._mean(3) / (M * (M - 1) if fair else M * M)

    def rank_histogram(self) -> torch.Tensor:
        """rank_hist / its total per row (the valid samples): f64 [S, M + 1]; NaN where there is none."""
        c = self.rank_hist.to(torch.float64)
        return _ratio(c, c.sum(-1, keepdim=True).expand_as(c))

    def rank_flatness(self) -> torch.Tensor:
        """Total variation distance of `rank_histogram()` from the uniform 1 / (M + 1): f64 [S], 0 = flat."""
        return 0.5 * (self.rank_histogram() - 1.0 / (self.members + 1)).abs().sum(-1)

    def sum(self, steps=None) -> "EnsembleScore":
        """The given steps (an index, slice, list or index tensor; default: all) pooled into ONE row, before any ratio is
        taken."""
        pick = (lambda t: t) if steps is None else (lambda t: t[steps].reshape((-1,) + tuple(t.shape[1:])))
        parts = [pick(t) for t in (self.sums, self.rank_hist, self.n_invalid, self.n_ties)]
        rows = parts[0].shape[0]
        return EnsembleScore(*(t.sum(0, keepdim=True) for t in parts), self.members, self.samples_per_step, self.n_steps * rows)

    def cpu(self) -> "EnsembleScore":
        return EnsembleScore(self.sums.cpu(), self.rank_hist.cpu(), self.n_invalid.cpu(), self.n_ties.cpu(), self.members,
                             self.samples_per_step, self.n_steps)

    @staticmethod
    def cat(parts: Sequence["EnsembleScore"]) -> "EnsembleScore":
        """Scores of consecutive step ranges of the same ensemble, steps in order."""
        p = parts[0]
        if any((q.members, q.samples_per_step, q.n_steps) != (p.members, p.samples_per_step, p.n_steps) for q in parts):
            raise MdnoError("EnsembleScore.cat: the parts must have the same members, samples per step and pooling")
        return EnsembleScore(torch.cat([q.sums for q in parts], 0), torch.cat([q.rank_hist for q in parts], 0),
                             torch.cat([q.n_invalid for q in parts], 0), torch.cat([q.n_ties for q in parts], 0), p.members,
                             p.samples_per_step, p.n_steps)


def ensemble_score(frames: torch.Tensor, truth: torch.Tensor, form: str = "auto") -> EnsembleScore:
    """frames f32 [S, M, N, 3] (device), the M members of ONE ensemble, against truth [S, N, 3] -> `EnsembleScore`, one row
    per step.  The result does not depend on the order of the members (so not on how they were sharded, grouped or
    gathered), and is the same bits on every run.  Asynchronous on the current stream; CPU tensors and bad arguments raise
    `MdnoError` before any device work.  `form` forces one of the two kernel forms (ops.ensemble_score)."""
    sums, rank_hist, n_invalid, n_ties = ops.ensemble_score(frames, truth, form)
    return EnsembleScore(sums, rank_hist, n_invalid, n_ties, int(frames.shape[1]), 3 * int(frames.shape[2]))


@dataclass
class CrossRmsd:
    """Every produced frame against every reference frame (ops.cross_rmsd; include/mdno_conformations.h has the rule):
    `matrix` f64 [S, M, Fb], the RMSD after the optimal rigid superposition (None when it was not asked for); `nearest` f64
    [S, M] and `nearest_index` i64 [S, M], the smallest of a frame's row and the lowest reference index that attains it;
    `cover` f64 [M, Fb] and `cover_step` i64 [M, Fb], per member the smallest of a reference frame's column and the lowest
    step that attains it.  A frame with a NaN or Inf coordinate is NaN in its row (column) and never chosen; NaN and -1 where
    nothing valid is left.  Every method runs in fp64 on the device of the fields and reads nothing back."""
    matrix: Optional[torch.Tensor]
    nearest: torch.Tensor
    nearest_index: torch.Tensor
    cover: torch.Tensor
    cover_step: torch.Tensor

    def precision(self, radius: float) -> torch.Tensor:
        """Is every produced frame close to SOME reference frame: per member the share of its valid frames with
        nearest <= radius, f64 [M]; NaN for a member without a valid frame (or without a valid reference)."""
        valid = self.nearest_index >= 0
        return _ratio(((self.nearest <= radius) & valid).sum(0), valid.sum(0))

    def coverage(self, radius: float) -> torch.Tensor:
        """Is every reference frame visited by the run: per member the share of the valid reference frames with
        cover <= radius, f64 [M]; NaN for a member without a valid step (or without a valid reference)."""
        valid = self.cover_step >= 0
        return _ratio(((self.cover <= radius) & valid).sum(1), valid.sum(1))

    def to_reference(self, j: int) -> torch.Tensor:
        """Column j of the matrix, f64 [S, M]: the RMSD time series of every member to ONE structure (a folded state)."""
        if self.matrix is None:
            raise MdnoError("CrossRmsd.to_reference needs the matrix: ask for it (matrix=True)")
        return self.matrix[:, :, j]

    def cpu(self) -> "CrossRmsd":
        return CrossRmsd(None if self.matrix is None else self.matrix.cpu(), self.nearest.cpu(), self.nearest_index.cpu(),
                         self.cover.cpu(), self.cover_step.cpu())

    @staticmethod
    def cat(parts: Sequence["CrossRmsd"]) -> "CrossRmsd":
        """Results of disjoint member ranges of the same steps against the same reference, members in order.  Rows and
        per-member columns never cross members, so this is the result of scoring all members at once, bit for bit."""
        if any((q.matrix is None) != (parts[0].matrix is None) for q in parts):
            raise MdnoError("CrossRmsd.cat: either every part holds the matrix or none does")
        return CrossRmsd(None if parts[0].matrix is None else torch.cat([q.matrix for q in parts], 1),
                         torch.cat([q.nearest for q in parts], 1), torch.cat([q.nearest_index for q in parts], 1),
                         torch.cat([q.cover for q in parts], 0), torch.cat([q.cover_step for q in parts], 0))


def cross_rmsd(frames: torch.Tensor, reference: torch.Tensor, matrix: bool = True) -> CrossRmsd:
    """frames f32 [S, M, N, 3] (device; [F, N, 3] is one member) against reference f32 [Fb, N, 3] -> `CrossRmsd`: the nearest
    reference frame of every produced frame, the nearest produced frame of every reference frame per member, and with
    `matrix` the full [S, M, Fb] RMSD map (8 S M Fb bytes: 512 MB for 64 members x 1,000 steps x 1,000 reference frames —
    pass matrix=False where only precision and coverage are wanted).  `reference` may be `frames` itself (one member): the
    run's own 2-D RMSD map.  The bits of an element depend on its two frames alone, never on the batch.  No periodic box:
    a superposition needs whole molecules (ops.cross_rmsd).  Asynchronous on the current stream; CPU tensors and bad
    arguments raise `MdnoError` before any device work."""
    return CrossRmsd(*ops.cross_rmsd(frames, reference, matrix=matrix, nearest=True, cover=True))


# ------------------------------------------------------------------------------------------------
# Essential dynamics (csrc/essential.hip, include/mdno_essential.h has the rules)
def superpose(frames: torch.Tensor, reference: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """frames f32 [S, M, N, 3] (device; [F, N, 3] is one member) onto reference f32 [N, 3] -> (aligned f32 [S, M, N, 3],
    rmsd f64 [S, M]): every frame in the reference's frame of reference (optimal proper rotation, centroid on the
    reference's) and its RMSD to it.  A frame with a non-finite coordinate comes back as NaN.  Asynchronous on the current
    stream; CPU tensors and bad arguments raise `MdnoError` before any device work."""
    return ops.superpose_frames(frames, reference, aligned=True, rmsd=True)


def _feature_rows(X: torch.Tensor, what: str = "X") -> Tuple[torch.Tensor, Tuple[int, ...]]:
    """(X as [S, M, D], its leading shape): [S, M, N, 3] -> D = 3 N; [F, N, 3] -> one member, D = 3 N; [S, M, D]; [F, D] -> one
    member.  A rank-3 tensor whose last dimension is 3 is taken as FRAMES [F, N, 3]: pass three features of M members as
    [S, M, 1, 3]."""
    if tensor(X, what).dim() == 4 and X.shape[-1] == 3:
        return X.reshape(X.shape[0], X.shape[1], -1), tuple(X.shape[:2])
    if X.dim() == 3 and X.shape[-1] == 3:
        return X.reshape(X.shape[0], 1, -1), tuple(X.shape[:1])
    if X.dim() == 3:
        return X, tuple(X.shape[:2])
    if X.dim() == 2:
        return X[:, None], tuple(X.shape[:1])
    raise MdnoError(f"{what} has shape {tuple(X.shape)}: expected [S, M, N, 3], [F, N, 3], [S, M, D] or [F, D]")


@dataclass
class Covariance:
    """The pooled second-moment SUMS of `covariance`: sums[a, b] = sum over the n pairs of rows (t, t + lag) of the same member
    of (x[t, a] - mean[a]) (x[t + lag, b] - mean[b])."""
    mean: torch.Tensor               # f64 [D]
    sums: torch.Tensor               # f64 [D, D]
    n: int                           # M (S - lag) pairs
    lag: int

    def matrix(self) -> torch.Tensor:
        """sums / (n - 1) at lag 0 (the unbiased covariance), sums / n at a lag; NaN where that divides by zero."""
        return self.sums / float(self.n - 1 if self.lag == 0 else self.n)

    def symmetrized(self) -> torch.Tensor:
        """(matrix + matrix^T) / 2: the estimate TICA uses for a reversible process."""
        m = self.matrix()
        return 0.5 * (m + m.transpose(0, 1))

    def rmsf(self) -> torch.Tensor:
        """f64 [N] for D = 3 N coordinates: sqrt of the summed diagonal variances of each atom's x, y, z."""
        D = self.sums.shape[0]
        if D % 3:
            raise MdnoError(f"Covariance.rmsf needs D = 3 N coordinates, D = {D}")
        return torch.sqrt(torch.diagonal(self.matrix()).reshape(-1, 3).sum(1))

    def cpu(self) -> "Covariance":
        return Covariance(self.mean.cpu(), self.sums.cpu(), self.n, self.lag)


def covariance(X: torch.Tensor, mean: Optional[torch.Tensor] = None, lag: int = 0) -> Covariance:
    """X f32 [S, M, N, 3], [F, N, 3] (superposed frames: `superpose` first) or any feature matrix [S, M, D] / [F, D] (a latent
    matrix from forward(..., return_latent=True)) -> `Covariance`, pooled over the members, time lag `lag` along the first
    axis.  `mean` f64 [D]: the centre, by default the mean over all S M rows (ops.feature_sums; computed on the device, not
    read back).  One fp64 GEMM on the matrix pipe without an fp64 copy of X (ops.feature_covariance).  Asynchronous on the
    current stream."""
    x, _ = _feature_rows(X)
    x, S, M, D = ops._features(x, "X")
    if mean is None:
        total, _ = ops.feature_sums(x.reshape(S * M, D))
        mean = total / float(S * M)
    sums = ops.feature_covariance(x, mean, lag)
    return Covariance(mean if mean.dtype == torch.float64 else mean.to(torch.float64), sums, M * max(S - int(lag), 0), int(lag))


def _fix_signs(v: torch.Tensor) -> torch.Tensor:
    """Every column's largest-magnitude entry positive (the lowest index on a tie)."""
    if v.numel() == 0:
        return v
    big = v.abs()
    idx = (big == big.max(0, keepdim=True).values).to(torch.int8).argmax(0)          # the first maximal entry
    sign = torch.where(v.gather(0, idx[None]) < 0, -1.0, 1.0).to(v.dtype)
    return v * sign


@dataclass
class Components:
    """k directions of feature space (`pca`, `tica`): values descending, vectors[:, c] the c-th direction."""
    values: torch.Tensor             # f64 [k]
    vectors: torch.Tensor            # f64 [D, k]
    mean: torch.Tensor               # f64 [D]
    total: float                     # pca: the trace of the covariance; tica: the number of whitened dimensions kept
    lag: int = 0                     # tica: the lag of the time-lagged matrix

    def explained_ratio(self) -> torch.Tensor:
        """pca: values / trace of the covariance, f64 [k]."""
        return self.values / self.total

    def rmsip(self, other: "Components") -> float:
        """The root-mean-square inner product of the two k-subspaces, sqrt(sum_ij (v_i . w_j)^2 / k): 1 = the same
        subspace, 0 = orthogonal ones (orthonormal vectors: pca's)."""
        k = self.vectors.shape[1]
        if other.vectors.shape != self.vectors.shape:
            raise MdnoError(f"rmsip: {tuple(self.vectors.shape)} against {tuple(other.vectors.shape)}")
        g = self.vectors.cpu().transpose(0, 1) @ other.vectors.cpu()
        return math.sqrt(float((g * g).sum()) / k)

    def timescales(self) -> torch.Tensor:
        """tica: the implied timescales -lag / ln |value| in steps, f64 [k] (inf at |value| = 1, 0 at value 0)."""
        if self.lag <= 0:
            raise MdnoError("timescales: these components have no lag (tica's have)")
        return -float(self.lag) / torch.log(self.values.abs())

    def cpu(self) -> "Components":
        return Components(self.values.cpu(), self.vectors.cpu(), self.mean.cpu(), self.total, self.lag)


def pca(cov: Covariance, k: int) -> Components:
    """The k leading principal components of a lag-0 `Covariance`: fp64 torch.linalg.eigh of cov.matrix() on the HOST copy
    (one read-back of D^2 doubles), eigenvalues descending, every vector's largest-magnitude entry positive (the lowest
    index on a tie).  The result lives on cov's device."""
    if cov.lag != 0:
        raise MdnoError(f"pca needs a lag-0 covariance, got lag {cov.lag}")
    D = cov.sums.shape[0]
    k = integer(k, "pca: k", 1, D)
    m = cov.matrix().cpu()
    w, v = torch.linalg.eigh(0.5 * (m + m.transpose(0, 1)))
    w, v = w.flip(0)[:k], _fix_signs(v.flip(1)[:, :k].contiguous())
    dev = cov.sums.device
    return Components(w.to(dev), v.to(dev), cov.mean, float(torch.diagonal(m).sum()))


def tica(cov0: Covariance, cov_lag: Covariance, k: int, eps: float = 1e-10) -> Components:
    """Time-lagged independent components: whiten with the eigenpairs of C(0) above eps * lambda_max (superposition makes
    C(0) rank-deficient by six, so the truncation is required), eigh of the whitened symmetrised C(lag) -> the k slowest
    directions, values = their autocorrelations at the lag (descending), vectors [D, k] in the original features
    (C(0)-orthonormal), signs as in `pca`.  `.timescales()` gives -lag / ln |value|.  On the host copy, fp64."""
    if cov0.lag != 0 or cov_lag.lag <= 0:
        raise MdnoError(f"tica needs C(0) and C(lag > 0), got lags {cov0.lag} and {cov_lag.lag}")
    if cov0.sums.shape != cov_lag.sums.shape:
        raise MdnoError(f"tica: C(0) is {tuple(cov0.sums.shape)}, C(lag) {tuple(cov_lag.sums.shape)}")
    c0, ct = cov0.symmetrized().cpu(), cov_lag.symmetrized().cpu()
    w, u = torch.linalg.eigh(c0)
    keep = w > eps * w[-1] if w.numel() and w[-1] > 0 else torch.zeros_like(w, dtype=torch.bool)
    r = int(keep.sum())
    k = integer(k, f"tica ({r} of {w.numel()} dimensions above eps): k" if r else "tica (C(0) has no positive eigenvalue): k", 1, r)
    white = u[:, keep] / torch.sqrt(w[keep])
    lam, q = torch.linalg.eigh(white.transpose(0, 1) @ ct @ white)
    lam, q = lam.flip(0)[:k], q.flip(1)[:, :k]
    dev = cov0.sums.device
    return Components(lam.to(dev), _fix_signs((white @ q).contiguous()).to(dev), cov0.mean, float(r), cov_lag.lag)


def project(X: torch.Tensor, components: Components) -> torch.Tensor:
    """X (any form `covariance` takes) onto `components` -> P f64 [S, M, k] ([F, k] for a plain stack):
    P[..., c] = (x - components.mean) . components.vectors[:, c], in fp64 on the device (ops.project_features)."""
    x, lead = _feature_rows(X)
    x, S, M, D = ops._features(x, "X")
    return ops.project_features(x.reshape(S * M, D), components.mean, components.vectors).reshape(lead + (components.vectors.shape[1],))


def free_energy(P: torch.Tensor, i: int = 0, j: int = 1, bins: int = 50, range=None):
    """The free-energy surface over components i and j of the projections P f64 [..., k] -> (F f64 [bins, bins] in kT,
    minimum at 0, +inf where a bin is empty; counts i64 [bins, bins]; edges f64 [2, bins + 1]).  `range` = ((lo_i, hi_i),
    (lo_j, hi_j)), by default the data's own extent (one read-back); a point is counted in bin b when
    edges[b] <= p < edges[b + 1], the last bin closed, and dropped outside the range or where it is NaN — comparisons
    against the edges and integer counts on P's device, nothing rounded."""
    if not torch.is_tensor(P) or P.dim() < 1:
        raise MdnoError("free_energy: P must be a tensor [..., k]")
    k = P.shape[-1]
    bins = integer(bins, "free_energy: bins", 1, None)
    if not (0 <= i < k and 0 <= j < k):
        raise MdnoError(f"free_energy: components {i} and {j} of {k}")
    pts = [P[..., c].reshape(-1).to(torch.float64).contiguous() for c in (i, j)]
    if range is None:
        if pts[0].numel() == 0:
            raise MdnoError("free_energy: no points and no range")
        range = tuple((float(torch.nan_to_num(p, nan=float("inf")).min()), float(torch.nan_to_num(p, nan=float("-inf")).max())) for p in pts)
    edges, idx, ok = [], [], None
    for p, (lo, hi) in zip(pts, range):
        lo, hi = float(lo), float(hi)
        if not (math.isfinite(lo) and math.isfinite(hi)) or hi < lo:
            raise MdnoError(f"free_energy: range ({lo}, {hi})")
        if hi == lo:
            lo, hi = lo - 0.5, hi + 0.5
        e = torch.linspace(lo, hi, bins + 1, dtype=torch.float64)                      # (on the host: the same edges for any device)
        e[0], e[-1] = lo, hi
        e = e.to(P.device)
        b = torch.bucketize(p, e, right=True) - 1
        b = torch.where(p == hi, torch.full_like(b, bins - 1), b)
        inside = (p >= lo) & (p <= hi)
        ok = inside if ok is None else ok & inside
        edges.append(e)
        idx.append(b)
    flat = (idx[0] * bins + idx[1])[ok]
    counts = torch.bincount(flat, minlength=bins * bins).reshape(bins, bins)
    total = counts.sum()
    F = -torch.log(counts.to(torch.float64) / total.to(torch.float64))
    F = F - F.min() if int(total) else torch.full_like(F, float("inf"))
    return F, counts, torch.stack(edges)


def histogram_total_variation(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Total variation distance of two count arrays of the same binning, [..., bins, bins] -> f64 [...]:
    0.5 sum |a / sum a - b / sum b| (0 = the same distribution, 1 = disjoint; NaN where one is empty)."""
    if a.shape[-2:] != b.shape[-2:]:
        raise MdnoError(f"histogram_total_variation: {tuple(a.shape)} against {tuple(b.shape)}")
    a, b = a.to(torch.float64), b.to(torch.float64)
    pa, pb = a / a.sum((-2, -1), keepdim=True), b / b.sum((-2, -1), keepdim=True)
    return 0.5 * (pa - pb).abs().sum((-2, -1))


# ------------------------------------------------------------------------------------------------
# Internal coordinates (csrc/internal.hip, include/mdno_internal.h has the rule)
def _index_array(a, width: int, n_atoms: Optional[int], what: str) -> torch.Tensor:
    """A host index array as int32 [n, width], validated: integer dtype, shape, 0 <= index (< n_atoms)."""
    if a is None:
        return torch.zeros((0, width), dtype=torch.int32)
    t = a.detach().cpu() if torch.is_tensor(a) else torch.as_tensor(a)
    if t.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise MdnoError(f"{what}: indices are {t.dtype}, expected an integer array")
    if t.numel() == 0:
        return torch.zeros((0, width), dtype=torch.int32)
    if t.dim() != 2 or t.shape[1] != width:
        raise MdnoError(f"{what} has shape {tuple(t.shape)}: expected [n, {width}]")
    lo, hi = int(t.min()), int(t.max())
    if lo < 0:
        raise MdnoError(f"{what}: index {lo} is negative")
    if hi >= (INT_MAX if n_atoms is None else n_atoms):
        raise MdnoError(f"{what}: index {hi} is outside 0 .. {(INT_MAX if n_atoms is None else n_atoms) - 1}")
    return t.to(torch.int32).contiguous()


@dataclass
class Featurizer:
    """Which internal coordinates make up a feature row: `pairs` i32 [P, 2] (distances), `triples` i32 [A, 3] (the angle at
    the middle atom) and `quads` i32 [T, 4] (dihedrals, IUPAC sign), columns in that order, for frames of `n_atoms` atoms
    (None: any frame that holds the largest index, `top`).  Built from host arrays by `Featurizer.of` and the constructors
    below, which validate once on the host; `.to(device)` moves the index tensors.  `a + b` concatenates kind by kind."""
    pairs: torch.Tensor
    triples: torch.Tensor
    quads: torch.Tensor
    n_atoms: Optional[int] = None
    top: int = -1
    _incidence: dict = field(default_factory=dict, init=False, repr=False, compare=False)    # (n_atoms, device) -> table

    @staticmethod
    def of(pairs=None, triples=None, quads=None, n_atoms: Optional[int] = None, device=None) -> "Featurizer":
        if n_atoms is not None:
            integer(n_atoms, "Featurizer: n_atoms", 0, None)
        arrays = [_index_array(a, w, n_atoms, what) for a, w, what in ((pairs, 2, "pairs"), (triples, 3, "triples"), (quads, 4, "quads"))]
        top = max([int(t.max()) for t in arrays if t.numel()], default=-1)
        f = Featurizer(arrays[0], arrays[1], arrays[2], n_atoms, top)
        return f if device is None else f.to(device)

    @staticmethod
    def distances(pairs, n_atoms: Optional[int] = None) -> "Featurizer":
        return Featurizer.of(pairs=pairs, n_atoms=n_atoms)

    @staticmethod
    def angles(triples, n_atoms: Optional[int] = None) -> "Featurizer":
        return Featurizer.of(triples=triples, n_atoms=n_atoms)

    @staticmethod
    def dihedrals(quads, n_atoms: Optional[int] = None) -> "Featurizer":
        return Featurizer.of(quads=quads, n_atoms=n_atoms)

    @staticmethod
    def backbone(n_atoms: int, min_separation: int = 3, stride: int = 1) -> "Featurizer":
        """The usual feature set of a chain with one site per residue: the n - 1 consecutive pseudo-bonds, every pair
        (i, j) of the atoms 0, stride, 2 stride, ... with j - i >= min_separation, the n - 2 pseudo-angles and the n - 3
        pseudo-dihedrals."""
        for name, v, low in (("n_atoms", n_atoms, 0), ("min_separation", min_separation, 1), ("stride", stride, 1)):
            integer(v, f"Featurizer.backbone: {name}", low, None)
        n = n_atoms
        idx = torch.arange(n, dtype=torch.int64)
        bonds = torch.stack([idx[:-1], idx[1:]], 1) if n > 1 else torch.zeros((0, 2), dtype=torch.int64)
        sub = idx[::stride]
        i, j = torch.triu_indices(sub.numel(), sub.numel(), 1)
        far = torch.stack([sub[i], sub[j]], 1)
        far = far[far[:, 1] - far[:, 0] >= min_separation]
        triples = torch.stack([idx[:-2], idx[1:-1], idx[2:]], 1) if n > 2 else None
        quads = torch.stack([idx[:-3], idx[1:-2], idx[2:-1], idx[3:]], 1) if n > 3 else None
        return Featurizer.of(torch.cat([bonds, far]), triples, quads, n_atoms=n)

    def __add__(self, other: "Featurizer") -> "Featurizer":
        if not isinstance(other, Featurizer):
            return NotImplemented
        if self.n_atoms is not None and other.n_atoms is not None and self.n_atoms != other.n_atoms:
            raise MdnoError(f"Featurizer: n_atoms {self.n_atoms} + n_atoms {other.n_atoms}")
        if self.pairs.device != other.pairs.device:
            raise MdnoError(f"Featurizer: indices on {self.pairs.device} + indices on {other.pairs.device}")
        return Featurizer(torch.cat([self.pairs, other.pairs]), torch.cat([self.triples, other.triples]),
                          torch.cat([self.quads, other.quads]), self.n_atoms if self.n_atoms is not None else other.n_atoms,
                          max(self.top, other.top))

    @property
    def n_bonds(self) -> int:
        """How many of the leading distance columns are consecutive (i, i + 1) pairs — the pseudo-bonds of `backbone`."""
        p = self.pairs.cpu()
        run = (p[:, 1] - p[:, 0] == 1).to(torch.int64).cumprod(0) if p.shape[0] else p.new_zeros(0)
        return int(run.sum())

    def dim(self, radians: bool = False) -> int:
        return int(self.pairs.shape[0] + self.triples.shape[0] + (1 if radians else 2) * self.quads.shape[0])

    def names(self, radians: bool = False):
        """One name per column: "d 3-17", "cos a 4-5-6", "cos t 1-2-3-4", "sin t 1-2-3-4" ("a ..." and "t ..." in radians)."""
        join = lambda row: "-".join(str(int(v)) for v in row)
        out = ["d " + join(r) for r in self.pairs.tolist()]
        out += [("a " if radians else "cos a ") + join(r) for r in self.triples.tolist()]
        for r in self.quads.tolist():
            out += ["t " + join(r)] if radians else ["cos t " + join(r), "sin t " + join(r)]
        return out

    def to(self, device) -> "Featurizer":
        return Featurizer(self.pairs.to(device), self.triples.to(device), self.quads.to(device), self.n_atoms, self.top)

    def incidence(self, n_atoms: int, device=None):
        """The incidence table the backward kernel walks (include/mdno_internal_grad.h): (atom_ptr i32 [n_atoms + 1],
        inc i32 [n_inc]) on `device` (None: where the indices are), a CSR by atom with inc[e] = item * 4 + slot, items
        counting the pairs, then the triples, then the quads, slot = the position in the tuple.  Built on the host: the
        tuples flattened in (item, slot) order, stably sorted by atom (so an atom's entries ascend; a tuple that names an
        atom twice gives it two), entries whose atom is >= n_atoms dropped.  Cached per (n_atoms, device) on this instance;
        `.to` and `+` make instances without a cache."""
        integer(n_atoms, "Featurizer.incidence: n_atoms", 0, None)
        device = self.pairs.device if device is None else torch.device(device)
        key = (n_atoms, str(device))
        hit = self._incidence.get(key)
        if hit is not None:
            return hit
        items = self.pairs.shape[0] + self.triples.shape[0] + self.quads.shape[0]
        if items >= ops.ICG_MAX_ITEMS:
            raise MdnoError(f"Featurizer.incidence: {items} index tuples, the table holds fewer than 2^29")
        atoms, codes, first = [], [], 0
        for t in (self.pairs, self.triples, self.quads):
            n, w = t.shape
            atoms.append(t.detach().cpu().to(torch.int64).reshape(-1))
            codes.append(((first + torch.arange(n, dtype=torch.int64))[:, None] * 4 + torch.arange(w, dtype=torch.int64)[None, :]).reshape(-1))
            first += n
        atoms, codes = torch.cat(atoms), torch.cat(codes)
        keep = (atoms >= 0) & (atoms < n_atoms)
        atoms, codes = atoms[keep], codes[keep]
        order = torch.sort(atoms, stable=True).indices
        atom_ptr = torch.zeros(n_atoms + 1, dtype=torch.int64)
        atom_ptr[1:] = torch.cumsum(torch.bincount(atoms, minlength=n_atoms), 0)
        table = (atom_ptr.to(torch.int32).to(device), codes[order].to(torch.int32).to(device))
        self._incidence[key] = table
        return table

    def check_frames(self, n_atoms: int) -> None:
        if (self.n_atoms is not None and n_atoms != self.n_atoms) or self.top >= n_atoms:
            want = f"{self.n_atoms}" if self.n_atoms is not None else f"more than {self.top}"
            raise MdnoError(f"the featurizer was built for frames of {want} atoms, these have {n_atoms}")


class _InternalCoordinatesFn(torch.autograd.Function):
    """internal_coordinates under autograd: the forward is the ops.internal_features call it always was (the same bits), the
    backward one mdnoicg_features_bwd launch (include/mdno_internal_grad.h) over the featurizer's incidence table."""

    @staticmethod
    def forward(ctx, frames, featurizer, owner, box, dtype):
        ctx.save_for_backward(frames)
        ctx.featurizer, ctx.owner, ctx.box = featurizer, owner, box          # owner: the caller's instance, which keeps the table
        return ops.internal_features(frames, featurizer.pairs, featurizer.triples, featurizer.quads, box=box, dtype=dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        frames, = ctx.saved_tensors
        ft = ctx.featurizer
        atom_ptr, inc = ctx.owner.incidence(int(frames.shape[-2]), frames.device)
        wide = frames.dtype == torch.float64
        grad = ops.internal_features_bwd(frames, g.contiguous(), ft.pairs, ft.triples, ft.quads, atom_ptr, inc, box=ctx.box,
                                         dtype=torch.float64 if wide else torch.float32)      # (a stride-0 g: sum().backward())
        return grad if grad.dtype == frames.dtype else grad.to(frames.dtype), None, None, None, None


def internal_coordinates(frames: torch.Tensor, featurizer: Featurizer, box=None, radians: bool = False,
                         dtype=torch.float32) -> torch.Tensor:
    """frames f32 [S, M, N, 3] (device; [F, N, 3] is a plain stack) -> features [S, M, D] ([F, D]) of `dtype`: the distances,
    angle cosines and dihedral (cos, sin) the featurizer lists, in fp64 on the fp32 coordinates (include/mdno_internal.h has
    the rule; ops.internal_features).  They do not depend on a reference frame, so they are what `covariance`, `tica`,
    `kcenters` and `assign` should be fed for anything that unfolds, hinges or diffuses.  `radians`: angles and dihedrals as
    one column each (what `free_energy` takes for a map of two torsions).  `box`: bond vectors by the minimum image.
    Asynchronous on the current stream, nothing is read back; CPU tensors and bad arguments raise `MdnoError` before any
    device work.
    DIFFERENTIABLE in the default mode: where `frames.requires_grad` and grad mode is on, the result carries a grad_fn whose
    backward is one hand-written kernel (include/mdno_internal_grad.h has the rule: every clamp as the identity, an item
    whose incoming gradient is exactly zero skipped — mask a degenerate feature by zeroing its gradient —, no double
    backward).  The forward is the same launch and the same bits either way.  `radians=True` has no gradient: with frames
    that require grad it raises `MdnoError` (detach them)."""
    if not isinstance(featurizer, Featurizer):
        raise MdnoError(f"internal_coordinates: featurizer is a {type(featurizer).__name__}")
    if not torch.is_tensor(frames) or frames.dim() not in (3, 4) or frames.shape[-1] != 3:
        raise MdnoError("internal_coordinates: frames must be [S, M, N, 3] or [F, N, 3]")
    featurizer.check_frames(int(frames.shape[-2]))
    wants_grad = frames.requires_grad and torch.is_grad_enabled()
    if wants_grad and radians:
        raise MdnoError("internal_coordinates: radians=True is not differentiable and frames requires grad (detach the frames, "
                        "or take the cosine and sine columns of the default mode)")
    on_device(frames, "frames")
    owner = featurizer
    if featurizer.pairs.device != frames.device:
        featurizer = featurizer.to(frames.device)
    if wants_grad:
        return _InternalCoordinatesFn.apply(frames, featurizer, owner, box, dtype)
    return ops.internal_features(frames, featurizer.pairs, featurizer.triples, featurizer.quads, box=box, radians=radians,
                                 dtype=dtype)


@dataclass
class FeatureHistograms:
    """Per-column histograms of a feature matrix (`feature_histograms`): `counts` i64 [M, D, bins + 2] for features
    [S, M, D] ([D, bins + 2] for [F, D]) — bin 0 holds the values below lo, the last bin those at or above hi —, `n_nan`
    i64 [M, D] the NaNs (counted in no bin), `lo` and `hi` the ranges as lists of floats (one entry: shared)."""
    counts: torch.Tensor
    n_nan: torch.Tensor
    lo: Sequence[float]
    hi: Sequence[float]

    def distribution(self) -> torch.Tensor:
        """counts / their sum per column, f64 (NaN for a column without a counted value)."""
        return _ratio(self.counts, self.counts.sum(-1, keepdim=True).expand_as(self.counts))

    def total_variation(self, other: "FeatureHistograms") -> torch.Tensor:
        """Per column, 0.5 sum |p - q| over all bins + 2 bins: f64 [M, D] or [D]; the other's leading dimensions broadcast
        (a run [M, D, .] against a truth [D, .])."""
        if self.counts.shape[-2:] != other.counts.shape[-2:]:
            raise MdnoError(f"total_variation: {tuple(self.counts.shape)} against {tuple(other.counts.shape)}")
        return 0.5 * (self.distribution() - other.distribution()).abs().sum(-1)

    def outside(self) -> torch.Tensor:
        """The share of the counted values below lo or at or above hi, per column: f64 [M, D] or [D]."""
        return _ratio(self.counts[..., 0] + self.counts[..., -1], self.counts.sum(-1))

    def cpu(self) -> "FeatureHistograms":
        return FeatureHistograms(self.counts.cpu(), self.n_nan.cpu(), self.lo, self.hi)


def feature_ranges(features: torch.Tensor):
    """(lo, hi) as lists of D floats: per column the smallest value and the next double above the largest (so that the
    largest falls into the last regular bin), NaNs left out; a constant column gets [v - 0.5, v + 0.5).  One read-back."""
    if not torch.is_tensor(features) or features.dim() not in (2, 3) or features.numel() == 0:
        raise MdnoError("feature_ranges: features must be a non-empty [S, M, D] or [F, D]")
    x = features.reshape(-1, features.shape[-1]).to(torch.float64)
    lo = torch.nan_to_num(x, nan=float("inf")).min(0).values.cpu().tolist()
    hi = torch.nan_to_num(x, nan=float("-inf")).max(0).values.cpu().tolist()
    out_lo, out_hi = [], []
    for l, h in zip(lo, hi):
        if not (math.isfinite(l) and math.isfinite(h)):
            raise MdnoError("feature_ranges: a column holds no finite value (or an infinite one)")
        out_lo.append(l if h > l else l - 0.5)
        out_hi.append(math.nextafter(h, math.inf) if h > l else l + 0.5)
    return out_lo, out_hi


def feature_histograms(features: torch.Tensor, lo, hi, bins: int = 50) -> FeatureHistograms:
    """features [S, M, D] or [F, D] (device, f32 or f64) -> `FeatureHistograms` over `bins` equal bins of [lo, hi) per column
    (lo, hi: a number each, or D numbers — `feature_ranges` of the truth), per member for [S, M, D]; counted on the device
    with integer atomics (ops.column_histogram), nothing read back."""
    if not torch.is_tensor(features) or features.dim() not in (2, 3):
        raise MdnoError("feature_histograms: features must be [S, M, D] or [F, D]")
    D = features.shape[-1]
    lo, hi, bins = ops.check_column_ranges(lo, hi, bins, D)
    members = features.shape[1] if features.dim() == 3 else 1
    if members == 0:
        raise MdnoError("feature_histograms: features has no member")
    counts, n_nan = ops.column_histogram(features.reshape(features.shape[0], members * D), lo, hi, bins, groups=members)
    lead = (members, D) if features.dim() == 3 else (D,)
    return FeatureHistograms(counts.reshape(lead + (bins + 2,)), n_nan.reshape(lead), lo, hi)


# ------------------------------------------------------------------------------------------------
# Markov state models (csrc/markov.hip, include/mdno_markov.h has the rules)
@dataclass
class Assignment:
    """Every frame's state (`assign`): `labels` i32 and `dist2` f64, shaped like the input's leading dimensions ([S, M], or
    [F] for a plain stack): the index of the nearest centre and the squared distance to it; -1 and NaN for a frame that
    holds a non-finite value (or where no centre could be chosen).  Methods run on the device of the fields."""
    labels: torch.Tensor
    dist2: torch.Tensor

    def outside(self, radius) -> torch.Tensor:
        """The share of the frames, per member (f64 [M]; a scalar for [F]), that lie farther than `radius` from EVERY centre
        — with the truth's covering radius, how much of a run is off the truth's manifold.  A frame without a label counts
        as outside; NaN without frames."""
        r = radius.to(self.dist2.device, torch.float64) if torch.is_tensor(radius) else float(radius)
        inside = torch.sqrt(self.dist2) <= r                                        # (NaN: not inside; sqrt is monotone, so a
        #                                                                             frame AT the covering radius is inside)
        return _ratio((~inside).sum(0), torch.full_like(inside.sum(0), self.dist2.shape[0] if self.dist2.dim() else 1))

    def populations(self, n_states: int) -> torch.Tensor:
        """The share of the labelled frames in each state, per member: f64 [M, n_states] ([n_states] for [F]); NaN for a
        member without a labelled frame.  Labels outside 0 .. n_states - 1 are left out."""
        lab = self.labels.reshape(self.labels.shape[0], -1).to(torch.int64)
        M = lab.shape[1]
        ok = (lab >= 0) & (lab < n_states)
        flat = (torch.arange(M, device=lab.device)[None] * n_states + lab)[ok]
        counts = torch.bincount(flat, minlength=M * n_states).reshape(M, n_states)
        pops = _ratio(counts, counts.sum(1, keepdim=True).expand_as(counts))
        return pops.reshape(self.labels.shape[1:] + (n_states,))

    def cpu(self) -> "Assignment":
        return Assignment(self.labels.cpu(), self.dist2.cpu())

    @staticmethod
    def cat(parts: Sequence["Assignment"]) -> "Assignment":
        """Results of disjoint member ranges of the same steps against the same centres, members in order."""
        return Assignment(torch.cat([q.labels for q in parts], 1), torch.cat([q.dist2 for q in parts], 1))


def _state_rows(X: torch.Tensor, what: str = "X"):
    """(X as a matrix of rows [R, D] — f64 stays f64, anything else becomes f32 —, its leading shape), forms as in
    `_feature_rows`."""
    x, lead = _feature_rows(X, what)
    return x.reshape(-1, x.shape[-1]), lead


def _centre_rows(centres: torch.Tensor) -> torch.Tensor:
    if not torch.is_tensor(centres) or centres.dim() not in (2, 3):
        raise MdnoError("centres: expected a tensor [k, D] or frames [k, N, 3]")
    return centres.reshape(centres.shape[0], -1)


def _assign_rows(rows: torch.Tensor, lead, centres: torch.Tensor, origin) -> Assignment:
    centres = _centre_rows(centres)
    if torch.is_tensor(rows) and torch.is_tensor(centres) and rows.dtype != centres.dtype and rows.is_cuda and centres.is_cuda:
        centres = centres.to(torch.float64 if rows.dtype == torch.float64 else torch.float32)
    if origin is None and centres.is_cuda and centres.shape[0] > 0:
        origin = centres.to(torch.float64).mean(0)
    labels, dist2 = ops.assign_features(rows, centres, origin)
    return Assignment(labels.reshape(lead), dist2.reshape(lead))


def assign(X: torch.Tensor, centres: torch.Tensor, origin: Optional[torch.Tensor] = None) -> Assignment:
    """X — any form `covariance` takes, or the f64 projections of `project` ([S, M, k] / [F, k]; like there, a rank-3 tensor
    whose last dimension is 3 is taken as frames) — against centres [k, D] (or frames [k, N, 3]) -> `Assignment`: the nearest
    centre of every frame in fp64, the inner products on the matrix pipe (ops.assign_features).  `origin` f64 [D]: the point
    the expansion |x|^2 + |c|^2 - 2 x.c is taken about, by default the centres' mean in fp64 — it keeps the cancellation
    small where the coordinates carry a large common offset; the labels do not depend on it beyond rounding.  Asynchronous
    on the current stream; CPU tensors and bad arguments raise `MdnoError` before any device work."""
    rows, lead = _state_rows(X)
    return _assign_rows(rows, lead, centres, origin)


def kcenters(X: torch.Tensor, k: int, first: int = 0):
    """Deterministic farthest-point seeding of k centres among the frames of X (forms as in `assign`), starting from row
    `first` of the flat [S M, D] matrix -> (centres [k, D] in X's element type, index i64 [k], radius f64 [k]); radius[i]
    is the covering radius before centre i was added (radius[0] = +inf).  All on the device, nothing read back
    (ops.kcenters)."""
    rows, _ = _state_rows(X)
    index, radius = ops.kcenters(rows, k, first)
    rows = rows if rows.dtype == torch.float64 else rows.to(torch.float32)
    return rows.index_select(0, index.clamp(min=0)), index, radius


def kmeans(X: torch.Tensor, k: int, iters: int = 10, init: Optional[torch.Tensor] = None):
    """k-means on the device: k-centres seeding (or `init` [k, D]), then `iters` Lloyd rounds of `assign` + ops.centroid_sums
    -> (centres [k, D] in X's element type, `Assignment` of X against them, moved i64 [iters]).  A state without frames keeps
    its centre; new centres are sums / counts in fp64, rounded once to X's element type.  moved[i] is the number of frames
    whose label round i changed (0: converged); it stays on the device, like everything inside the loop — nothing is read
    back."""
    rows, lead = _state_rows(X)
    iters = integer(iters, "kmeans: iters", 0, None)
    if init is None:
        centres = kcenters(rows, k)[0]
    else:
        centres = _centre_rows(init)
        if centres.shape[0] != k:
            raise MdnoError(f"kmeans: init has {centres.shape[0]} rows, k = {k}")
    dtype = torch.float64 if rows.dtype == torch.float64 else torch.float32
    centres = centres.to(dtype)
    flat = (rows.shape[0],)
    current = _assign_rows(rows, flat, centres, None)
    moved = []
    for _ in range(iters):
        sums, counts = ops.centroid_sums(rows, current.labels, k)
        mean = sums / counts.to(torch.float64)[:, None]
        centres = torch.where((counts > 0)[:, None], mean, centres.to(torch.float64)).to(dtype)
        nxt = _assign_rows(rows, flat, centres, None)
        moved.append((nxt.labels != current.labels).sum())
        current = nxt
    moved = torch.stack(moved) if moved else torch.zeros(0, dtype=torch.int64, device=rows.device)
    return centres, Assignment(current.labels.reshape(lead), current.dist2.reshape(lead)), moved


@dataclass
class Discretization:
    """A partition of conformation space into states (`discretize`): frames are superposed onto `reference` f32 [N, 3],
    projected onto `components` (if any) and assigned to the nearest of `centres` [k, D]; `radius` (an f64 scalar on the
    device) is the covering radius of the frames it was built from: the largest distance of one of them to its centre.
    With a `featurizer` the frames are not superposed at all: their internal coordinates (`internal_coordinates`, under
    `box`) take the place of the superposed Cartesians, and `reference` is None."""
    reference: Optional[torch.Tensor]
    components: Optional[Components]
    centres: torch.Tensor
    radius: torch.Tensor
    featurizer: Optional[Featurizer] = None
    box: Optional[Tuple[float, float, float]] = None

    @property
    def n_states(self) -> int:
        return int(self.centres.shape[0])

    def features(self, frames: torch.Tensor):
        """(rows [S M, D], leading shape) of frames f32 [S, M, N, 3] or [F, N, 3]: superposed (or, with a featurizer, turned
        into internal coordinates), then projected."""
        if self.featurizer is not None:
            X = internal_coordinates(frames, self.featurizer, box=self.box)
            lead = tuple(X.shape[:-1])
            X = X.reshape(-1, X.shape[-1])
            if self.components is not None:                       # (not `project`: it would take three columns for frames)
                X = ops.project_features(X, self.components.mean, self.components.vectors)
            return X, lead
        aligned, _ = superpose(frames, self.reference)
        lead = tuple(frames.shape[:-2])
        if self.components is None:
            return aligned.reshape(-1, aligned.shape[-2] * 3), lead
        P = project(aligned, self.components)
        return P.reshape(-1, P.shape[-1]), lead

    def assign(self, frames: torch.Tensor) -> Assignment:
        """superpose -> project (if components) -> assign; labels and dist2 shaped like the frames' leading dimensions.  A
        frame's result depends on that frame alone."""
        rows, lead = self.features(frames)
        return _assign_rows(rows, lead, self.centres, None)


def discretize(truth: torch.Tensor, n_states: int, components: Optional[Components] = None, method: str = "kcenters",
               iters: int = 10, reference: Optional[torch.Tensor] = None, featurizer: Optional[Featurizer] = None,
               box=None) -> Discretization:
    """Cut the space the frames of `truth` (f32 [S, M, N, 3] or [F, N, 3]) visit into `n_states` states: superposed onto
    `reference` (by default the first frame), projected onto `components` if given (pca / tica of the same superposed
    frames), then clustered by "kcenters" (farthest-point: even coverage, the covering radius is minimised greedily) or
    "kmeans" (`iters` Lloyd rounds from that seeding).  With a `featurizer` the frames' internal coordinates (under `box`)
    take the place of the superposed Cartesians — no reference frame is involved, and `components` are then those of the
    internal coordinates; without one nothing changes."""
    if method not in ("kcenters", "kmeans"):
        raise MdnoError(f"discretize: method = {method!r}, expected 'kcenters' or 'kmeans'")
    if not torch.is_tensor(truth) or truth.dim() not in (3, 4) or truth.shape[-1] != 3:
        raise MdnoError("discretize: truth must be frames [S, M, N, 3] or [F, N, 3]")
    if featurizer is not None:
        if reference is not None:
            raise MdnoError("discretize: a featurizer and a reference frame were both given (internal coordinates need none)")
        box = ops.check_box(box, 0.0)
    elif box is not None:
        raise MdnoError("discretize: box is only used with a featurizer")
    elif reference is None:
        reference = truth.reshape(-1, truth.shape[-2], 3)[0].contiguous() if truth.numel() else truth.new_zeros(truth.shape[-2], 3)
    d = Discretization(reference, components, truth.new_zeros(0, 0), torch.zeros((), dtype=torch.float64), featurizer, box)
    rows, _ = d.features(truth)
    if method == "kcenters":
        centres = kcenters(rows, n_states)[0]
        fit = _assign_rows(rows, (rows.shape[0],), centres, None)
    else:
        centres, fit, _ = kmeans(rows, n_states, iters)
    worst = torch.nan_to_num(fit.dist2.reshape(-1), nan=0.0).max() if rows.shape[0] else torch.zeros((), dtype=torch.float64, device=rows.device)
    return Discretization(reference, components, centres, torch.sqrt(worst), featurizer, box)


@dataclass
class TransitionCounts:
    """`transition_counts`: counts i64 [L, M (or 1 when pooled), n, n], counts[l, m, i, j] = the number of origins t with
    label[t, m] = i and label[t + lags[l], m] = j; n_skipped i64 [L], the pairs with a label outside 0 .. n - 1."""
    counts: torch.Tensor
    n_skipped: torch.Tensor
    lags: Tuple[int, ...]

    def sum_members(self) -> "TransitionCounts":
        return TransitionCounts(self.counts.sum(1, keepdim=True), self.n_skipped, self.lags)

    def cpu(self) -> "TransitionCounts":
        return TransitionCounts(self.counts.cpu(), self.n_skipped.cpu(), self.lags)

    @staticmethod
    def cat(parts: Sequence["TransitionCounts"]) -> "TransitionCounts":
        """Per-member counts of disjoint member ranges at the same lags, members in order."""
        if any(q.lags != parts[0].lags for q in parts):
            raise MdnoError("TransitionCounts.cat: the parts were counted at different lags")
        return TransitionCounts(torch.cat([q.counts for q in parts], 1), torch.stack([q.n_skipped for q in parts]).sum(0), parts[0].lags)


def transition_counts(labels: torch.Tensor, n_states: int, lags, pooled: bool = False) -> TransitionCounts:
    """labels i32 [S, M] (`Assignment.labels`; [S] is one member) -> `TransitionCounts` at the given lags, sliding window,
    per member or pooled; exact integer counts on the device (ops.transition_counts)."""
    counts, skipped = ops.transition_counts(labels, n_states, lags, pooled)
    return TransitionCounts(counts, skipped, tuple(ops.check_msm_lags(lags)))


def _largest_connected_set(c: torch.Tensor):
    """The largest strongly connected set of the graph with an edge i -> j where c[i, j] > 0, among the visited states (a
    state with a count in its row or column); of equally large sets the one that holds the lowest state.  A sorted list."""
    n = c.shape[0]
    pos = c > 0
    visited = (pos.any(0) | pos.any(1)).tolist()
    fwd = [torch.nonzero(pos[i]).reshape(-1).tolist() for i in range(n)]
    bwd = [torch.nonzero(pos[:, i]).reshape(-1).tolist() for i in range(n)]

    def reach(start, adj):
        seen, stack = {start}, [start]
        while stack:
            for j in adj[stack.pop()]:
                if j not in seen:
                    seen.add(j)
                    stack.append(j)
        return seen
    best, done = [], set()
    for s in range(n):
        if not visited[s] or s in done:
            continue
        comp = reach(s, fwd) & reach(s, bwd)
        done |= comp
        if len(comp) > len(best):                                                  # (ascending s: the first of equals stays)
            best = sorted(comp)
    return best


def _transition_matrix(c: torch.Tensor, reversible: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(T, the matrix whose rows were normalised): c + c^T for the reversible estimate, c otherwise; a row without counts
    becomes NaN."""
    m = c + c.transpose(0, 1) if reversible else c
    return m / m.sum(1, keepdim=True), m


@dataclass
class MarkovModel:
    """`markov_model`: the transition matrix `T` f64 [a, a] among the `active` states (i64 [a], ascending), its
    `eigenvalues` (descending in magnitude; real f64 for the reversible estimate, complex otherwise) and the stationary
    distribution `pi` f64 [a], all on the host."""
    lag: int
    n_states: int
    active: torch.Tensor
    T: torch.Tensor
    eigenvalues: torch.Tensor
    pi: torch.Tensor
    reversible: bool

    def stationary(self) -> torch.Tensor:
        """f64 [n_states]: pi on the active states, 0 elsewhere."""
        out = torch.zeros(self.n_states, dtype=torch.float64)
        out[self.active] = self.pi
        return out

    def timescales(self, k: Optional[int] = None) -> torch.Tensor:
        """The implied timescales -lag / ln |lambda_i| in steps for i = 2 .. k + 1 (default: all), f64 [k]: inf at
        |lambda| = 1, 0 at lambda = 0."""
        a = self.eigenvalues.shape[0]
        k = a - 1 if k is None else integer(k, "timescales: k" if a > 1 else "timescales (one active state): k", 1, max(a - 1, 0))
        mag = self.eigenvalues.abs()[1:k + 1].to(torch.float64)
        ts = -float(self.lag) / torch.log(mag)
        return torch.where(mag >= 1.0, torch.full_like(ts, float("inf")), torch.where(mag == 0.0, torch.zeros_like(ts), ts))

    def free_energies(self) -> torch.Tensor:
        """-ln pi in kT over the active states, minimum 0, f64 [a]."""
        f = -torch.log(self.pi)
        return f - f.min()

    def chapman_kolmogorov(self, counts: TransitionCounts, lag_index: int) -> torch.Tensor:
        """Does the model predict the kinetics at a longer lag: with n = counts.lags[lag_index] / lag (a positive integer,
        else MdnoError), per active state i the total variation 0.5 sum_j |T^n[i, j] - T_n[i, j]| between the model's n-th
        power and the matrix estimated the same way, on the same active set, from the counts at n x lag; f64 [a].  NaN for
        a state without counts at that lag."""
        if not 0 <= lag_index < len(counts.lags):
            raise MdnoError(f"chapman_kolmogorov: lag_index = {lag_index} of {len(counts.lags)} lags")
        big = counts.lags[lag_index]
        if big % self.lag:
            raise MdnoError(f"chapman_kolmogorov: lag {big} is no multiple of the model's lag {self.lag}")
        c = counts.counts[lag_index].sum(0).cpu().to(torch.float64)[self.active][:, self.active]
        t_n, _ = _transition_matrix(c, self.reversible)
        return 0.5 * (torch.linalg.matrix_power(self.T, big // self.lag) - t_n).abs().sum(1)

    def population_total_variation(self, other: "MarkovModel") -> torch.Tensor:
        """The total variation distance of the two stationary distributions over the union of the active sets (a state
        outside a model's active set has weight 0 there): 0 = the same populations, 1 = disjoint."""
        if other.n_states != self.n_states:
            raise MdnoError(f"population_total_variation: {self.n_states} states against {other.n_states}")
        return 0.5 * (self.stationary() - other.stationary()).abs().sum()


def markov_model(counts: TransitionCounts, lag_index: int = 0, reversible: bool = True, member: Optional[int] = None) -> MarkovModel:
    """A Markov state model from the counts at lags[lag_index], summed over the members (or of one `member`), on the host
    copy in fp64.  The active set is the largest strongly connected set of the count graph among the visited states (ties:
    the set with the lowest state).  reversible=True: T = (C + C^T) row-normalised — the symmetrised estimate `tica` uses —,
    pi = its row sums normalised, spectrum by eigh of D^-1/2 (C + C^T) D^-1/2 (real).  reversible=False: T = C
    row-normalised, spectrum and pi by eig."""
    if not 0 <= lag_index < len(counts.lags):
        raise MdnoError(f"markov_model: lag_index = {lag_index} of {len(counts.lags)} lags")
    c = counts.counts[lag_index].cpu()
    c = (c.sum(0) if member is None else c[member]).to(torch.float64)
    n = c.shape[0]
    active = _largest_connected_set(c)
    if not active:
        raise MdnoError("markov_model: no transition was counted")
    idx = torch.tensor(active, dtype=torch.int64)
    T, m = _transition_matrix(c[idx][:, idx], reversible)
    d = m.sum(1)
    empty = d == 0                                                                 # (a single state that was only left)
    T = torch.where(empty[:, None], torch.eye(len(active), dtype=torch.float64), T)
    if reversible:
        pi = torch.where(empty, torch.ones_like(d), d)
        pi = pi / pi.sum()
        s = 1.0 / torch.sqrt(torch.where(empty, torch.ones_like(d), d))
        sym = s[:, None] * m * s[None] + torch.diag(empty.to(torch.float64))
        lam = torch.linalg.eigvalsh(0.5 * (sym + sym.transpose(0, 1))).flip(0)
        lam = lam[torch.argsort(lam.abs(), descending=True, stable=True)]
    else:
        lam = torch.linalg.eigvals(T)
        lam = lam[torch.argsort(lam.abs(), descending=True, stable=True)]
        w, v = torch.linalg.eig(T.transpose(0, 1))
        pi = v[:, torch.argmin((w - 1.0).abs())].real
        pi = pi.abs() / pi.abs().sum()
    return MarkovModel(int(counts.lags[lag_index]), n, idx, T, lam, pi, bool(reversible))


# ------------------------------------------------------------------------------------------------
# Distance constraints (csrc/constrain.hip, include/mdno_constrain.h has the rule)
def greedy_colours(pairs) -> list:
    """The colour of every constraint of a host list of (i, j): in list order, each takes the lowest colour that neither of
    its atoms has yet (include/mdno_constrain.h, ORDER).  Within a colour no two constraints share an atom."""
    used, colours = {}, []
    for i, j in pairs:
        m = used.get(i, 0) | used.get(j, 0)
        bit = (m + 1) & ~m                       # the lowest zero bit of m
        used[i] = used.get(i, 0) | bit
        used[j] = used.get(j, 0) | bit
        colours.append(bit.bit_length() - 1)
    return colours


@dataclass
class ColouredConstraints:
    """A constraint table as the kernel takes it (`DistanceConstraints.coloured`): sorted by colour, on one device."""
    pairs: torch.Tensor              # i32 [C, 2]
    lo: torch.Tensor                 # f64 [C]
    hi: torch.Tensor                 # f64 [C]
    colour_ptr: torch.Tensor         # i32 [n_colours + 1]
    weights: Optional[torch.Tensor]  # f32 [N] or None
    order: torch.Tensor              # i64 [C] (host): row k of the table is constraint order[k] of the list

    @property
    def n_colours(self) -> int:
        return int(self.colour_ptr.shape[0]) - 1


@dataclass
class ConstraintReport:
    """What a projection did per frame: `sweeps` i32, `viol_in` and `viol_out` f64, the largest |length - band| before the
    first and after the last sweep, shaped as the frames' leading dimensions ([S, M] or [F])."""
    sweeps: torch.Tensor
    viol_in: torch.Tensor
    viol_out: torch.Tensor

    @staticmethod
    def cat(parts: Sequence["ConstraintReport"], dim: int = 1) -> "ConstraintReport":
        return ConstraintReport(torch.cat([p.sweeps for p in parts], dim), torch.cat([p.viol_in for p in parts], dim),
                                torch.cat([p.viol_out for p in parts], dim))


@dataclass
class DistanceConstraints:
    """Distance bands lo <= |x_i - x_j| <= hi for the pairs of `pairs` i32 [C, 2] (lo, hi f64 [C]; hi = inf: a lower bound
    only; lo == hi: an equality) with optional per-atom `weights` f32 [n_atoms] in the role of inverse masses (0 pins an
    atom; None: 1 everywhere).  Built and validated on the host by `of`, `chain` and `from_frames`; `a + b` concatenates two
    lists (the weights must agree), `.to(device)` moves the tensors, `.coloured(device)` is the table the kernel walks."""
    pairs: torch.Tensor
    lo: torch.Tensor
    hi: torch.Tensor
    weights: Optional[torch.Tensor] = None
    n_atoms: Optional[int] = None
    top: int = -1
    _coloured: dict = field(default_factory=dict, init=False, repr=False, compare=False)     # device -> ColouredConstraints

    @staticmethod
    def of(pairs, lo, hi, weights=None, n_atoms: Optional[int] = None) -> "DistanceConstraints":
        if n_atoms is not None:
            integer(n_atoms, "DistanceConstraints: n_atoms", 0, None)
        p = _index_array(pairs, 2, n_atoms, "pairs")
        n_c = int(p.shape[0])
        if n_c > ops.CST_MAX_CONSTRAINTS:
            raise MdnoError(f"DistanceConstraints: {n_c} constraints, more than {ops.CST_MAX_CONSTRAINTS}")
        if n_c and bool((p[:, 0] == p[:, 1]).any()):
            k = int((p[:, 0] == p[:, 1]).nonzero()[0])
            raise MdnoError(f"DistanceConstraints: constraint {k} joins atom {int(p[k, 0])} to itself (i == j)")
        bounds = []
        for v, what in ((lo, "lo"), (hi, "hi")):
            try:      # (Python numbers straight to f64: as_tensor alone would round them to f32 first)
                t = v.detach().cpu().to(torch.float64) if torch.is_tensor(v) else torch.as_tensor(v, dtype=torch.float64)
                t = t.reshape(-1)
            except (TypeError, ValueError, RuntimeError):
                raise MdnoError(f"DistanceConstraints: {what} is not an array of numbers") from None
            if t.numel() == 1 and n_c != 1:
                t = t.expand(n_c)
            if t.numel() != n_c:
                raise MdnoError(f"DistanceConstraints: {t.numel()} entries of {what} for {n_c} constraints")
            if bool(torch.isnan(t).any()):
                raise MdnoError(f"DistanceConstraints: {what} holds a NaN")
            if bool((t < 0).any()):
                raise MdnoError(f"DistanceConstraints: {what} holds a negative bound")
            bounds.append(t.contiguous().clone())
        lo_t, hi_t = bounds
        if bool(torch.isinf(lo_t).any()):
            raise MdnoError("DistanceConstraints: lo holds an infinite bound")
        if bool((lo_t > hi_t).any()):
            k = int((lo_t > hi_t).nonzero()[0])
            raise MdnoError(f"DistanceConstraints: constraint {k} has lo = {float(lo_t[k])} > hi = {float(hi_t[k])}")
        top = int(p.max()) if n_c else -1
        w = None
        if weights is not None:
            w = weights.detach().cpu() if torch.is_tensor(weights) else torch.as_tensor(weights)
            w = w.to(torch.float32).reshape(-1).contiguous().clone()
            if n_atoms is None:
                n_atoms = int(w.numel())
            if w.numel() != n_atoms or top >= n_atoms:
                raise MdnoError(f"DistanceConstraints: {w.numel()} weights for frames of {max(n_atoms, top + 1)} atoms")
            if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
                raise MdnoError("DistanceConstraints: weights must be finite and >= 0")
        return DistanceConstraints(p, lo_t, hi_t, w, n_atoms, top)

    @staticmethod
    def chain(n_atoms: int, lo, hi, weights=None) -> "DistanceConstraints":
        """The n - 1 consecutive pseudo-bonds (i, i + 1) of a chain, each inside [lo, hi] (numbers, or one per bond)."""
        integer(n_atoms, "DistanceConstraints.chain: n_atoms", 0, None)
        idx = torch.arange(n_atoms, dtype=torch.int64)
        bonds = torch.stack([idx[:-1], idx[1:]], 1) if n_atoms > 1 else torch.zeros((0, 2), dtype=torch.int64)
        return DistanceConstraints.of(bonds, lo, hi, weights, n_atoms)

    @staticmethod
    def from_frames(truth: torch.Tensor, pairs_or_featurizer, margin: float = 0.0, box=None, weights=None) -> "DistanceConstraints":
        """Bands taken from a true trajectory: for every pair (an index array [C, 2], or the distance columns of a
        `Featurizer`) the smallest and the largest distance over all frames of truth f32 [..., N, 3] (device), through
        `internal_coordinates` in f64 and amin / amax, widened by `margin` on both sides (lo - margin clamped at 0)."""
        margin = float(margin)
        if not (math.isfinite(margin) and margin >= 0.0):
            raise MdnoError(f"DistanceConstraints.from_frames: margin = {margin}, expected a finite number >= 0")
        if not torch.is_tensor(truth) or truth.dim() < 3 or truth.shape[-1] != 3:
            raise MdnoError("DistanceConstraints.from_frames: truth must be [..., N, 3]")
        n = int(truth.shape[-2])
        pairs = pairs_or_featurizer.pairs if isinstance(pairs_or_featurizer, Featurizer) else pairs_or_featurizer
        ft = Featurizer.of(pairs=pairs, n_atoms=n)
        if ft.pairs.shape[0] == 0 or truth.numel() == 0:
            raise MdnoError("DistanceConstraints.from_frames: no pairs or no frames")
        d = internal_coordinates(truth.detach().reshape(-1, n, 3), ft, box=box, dtype=torch.float64)
        lo = (torch.amin(d, 0) - margin).clamp_min(0.0)
        hi = torch.amax(d, 0) + margin
        return DistanceConstraints.of(ft.pairs, lo.cpu(), hi.cpu(), weights, n)

    def __len__(self) -> int:
        return int(self.pairs.shape[0])

    def __add__(self, other: "DistanceConstraints") -> "DistanceConstraints":
        if not isinstance(other, DistanceConstraints):
            return NotImplemented
        if self.n_atoms is not None and other.n_atoms is not None and self.n_atoms != other.n_atoms:
            raise MdnoError(f"DistanceConstraints: n_atoms {self.n_atoms} + n_atoms {other.n_atoms}")
        if self.pairs.device != other.pairs.device:
            raise MdnoError(f"DistanceConstraints: a list on {self.pairs.device} + a list on {other.pairs.device}")
        a, b = self.weights, other.weights
        if (a is None) != (b is None) or (a is not None and not torch.equal(a, b)):
            raise MdnoError("DistanceConstraints: the two lists carry different weights")
        return DistanceConstraints(torch.cat([self.pairs, other.pairs]), torch.cat([self.lo, other.lo]), torch.cat([self.hi, other.hi]),
                                   a, self.n_atoms if self.n_atoms is not None else other.n_atoms, max(self.top, other.top))

    def to(self, device) -> "DistanceConstraints":
        return DistanceConstraints(self.pairs.to(device), self.lo.to(device), self.hi.to(device),
                                   None if self.weights is None else self.weights.to(device), self.n_atoms, self.top)

    def colours(self) -> list:
        """The colour of every constraint, in list order (`greedy_colours`)."""
        return greedy_colours(self.pairs.cpu().tolist())

    def coloured(self, device=None) -> ColouredConstraints:
        """The table sorted stably by colour on `device` (None: where the list is), with its colour_ptr; coloured on the host,
        once per device (`.to` and `+` make instances without a cache)."""
        device = self.pairs.device if device is None else torch.device(device)
        hit = self._coloured.get(str(device))
        if hit is not None:
            return hit
        col = torch.tensor(self.colours(), dtype=torch.int64)
        order = torch.sort(col, stable=True).indices if col.numel() else col
        n_colours = int(col.max()) + 1 if col.numel() else 0
        ptr_ = torch.zeros(n_colours + 1, dtype=torch.int64)
        if n_colours:
            ptr_[1:] = torch.cumsum(torch.bincount(col, minlength=n_colours), 0)
        table = ColouredConstraints(self.pairs.cpu()[order].contiguous().to(device), self.lo.cpu()[order].contiguous().to(device),
                                    self.hi.cpu()[order].contiguous().to(device), ptr_.to(torch.int32).to(device),
                                    None if self.weights is None else self.weights.to(device), order)
        self._coloured[str(device)] = table
        return table

    def check_frames(self, n_atoms: int) -> None:
        if (self.n_atoms is not None and n_atoms != self.n_atoms) or self.top >= n_atoms:
            want = f"{self.n_atoms}" if self.n_atoms is not None else f"more than {self.top}"
            raise MdnoError(f"the constraints were built for frames of {want} atoms, these have {n_atoms}")
        if self.weights is not None and int(self.weights.numel()) != n_atoms:
            raise MdnoError(f"the constraints carry {int(self.weights.numel())} weights, the frames have {n_atoms} atoms")


def project_constraints(frames: torch.Tensor, constraints: DistanceConstraints, box=None, iterations: int = 8, tol: float = 0.0,
                        out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, ConstraintReport]:
    """frames f32 [S, M, N, 3] (device; [F, N, 3] is a plain stack) -> (the frames with every listed pair distance moved
    towards its band, ConstraintReport): per frame up to `iterations` sweeps over the coloured constraints, SHAKE-style, in
    fp64 on the fp32 coordinates, until the largest |length - band| is at most `tol` (include/mdno_constrain.h has the rule;
    ops.project_constraints).  A frame inside every band comes back with the same bits and 0 sweeps; `iterations=0` only
    measures.  `out=frames` projects in place.  `box`: bond vectors by the minimum image.  Frames of at most
    `ops.CST_MAX_ATOMS` atoms.  Not differentiable.  Asynchronous on the current stream, nothing is read back; CPU tensors
    and bad arguments raise `MdnoError` before any device work."""
    if not isinstance(constraints, DistanceConstraints):
        raise MdnoError(f"project_constraints: constraints is a {type(constraints).__name__}")
    if not torch.is_tensor(frames) or frames.dim() not in (3, 4) or frames.shape[-1] != 3:
        raise MdnoError("project_constraints: frames must be [S, M, N, 3] or [F, N, 3]")
    constraints.check_frames(int(frames.shape[-2]))
    on_device(frames, "frames")
    t = constraints.coloured(frames.device)
    res, sweeps, vin, vout = ops.project_constraints(frames.detach(), t.pairs, t.lo, t.hi, t.colour_ptr, t.weights, box=box,
                                                     iterations=iterations, tol=tol, out=out)
    return res, ConstraintReport(sweeps, vin, vout)


# ------------------------------------------------------------------------------------------------
# Contact statistics over time (csrc/contacts.hip, include/mdno_contacts.h has the rule)
@dataclass
class PairStatistics:
    """Per-pair statistics over blocks of consecutive steps (ops.pair_statistics): `count` i32 [Bk, M, N, N], the frames of
    the block in which the pair is closer than `threshold`; `sum_r`, `sum_r2` f64 of the same shape (None without the
    moments), the sums of the distance and of its square; `n_frames` i64 [Bk], the frames of every block.  Full symmetric
    maps, diagonal included.  After `total()` the block axis is gone: [M, N, N] and a 0-dim `n_frames`.  Every method runs in
    fp64 on the device of `count` and reads nothing back."""
    count: torch.Tensor
    sum_r: Optional[torch.Tensor]
    sum_r2: Optional[torch.Tensor]
    n_frames: torch.Tensor
    threshold: float
    box: Optional[Tuple[float, float, float]] = None

    def _n(self) -> torch.Tensor:
        return self.n_frames.to(torch.float64).reshape(self.n_frames.shape + (1, 1, 1))

    def _moments(self, what: str):
        if self.sum_r is None or self.sum_r2 is None:
            raise MdnoError(f"{what}: these statistics were taken without the moments (moments=False)")
        return self.sum_r, self.sum_r2

    def total(self) -> "PairStatistics":
        """The statistics of all blocks together: the blocks added in ASCENDING order, one elementwise add per block, so the
        bits of the two sums are defined (those of the restatement with the same block_len).  No block: zero maps, 0 frames."""
        if self.count.dim() == 3:
            return self
        Bk = self.count.shape[0]

        def fold(t, dtype):
            if t is None:
                return None
            if Bk == 0:
                return torch.zeros(t.shape[1:], dtype=dtype, device=t.device)
            acc = t[0].clone()
            for b in range(1, Bk):
                acc = acc + t[b]
            return acc
        return PairStatistics(fold(self.count, torch.int32), fold(self.sum_r, torch.float64), fold(self.sum_r2, torch.float64),
                              self.n_frames.sum(), self.threshold, self.box)

    def probability(self) -> torch.Tensor:
        """count / n_frames: f64 [..., M, N, N], the contact-probability map; NaN for a block without frames."""
        return _ratio(self.count, self._n())

    def mean_distance(self) -> torch.Tensor:
        """sum_r / n_frames: f64 [..., M, N, N]; NaN for a block without frames or a pair with a non-finite distance."""
        return _ratio(self._moments("mean_distance")[0], self._n())

    def distance_std(self) -> torch.Tensor:
        """sqrt(max(sum_r2 / n - (sum_r / n)^2, 0)): f64 [..., M, N, N], the population standard deviation of the distance."""
        sr, sr2 = self._moments("distance_std")
        mean = _ratio(sr, self._n())
        var = _ratio(sr2, self._n()) - mean * mean
        return torch.sqrt(torch.where(var < 0, torch.zeros_like(var), var))          # (a NaN fails the test and stays)

    def difference(self, other: "PairStatistics") -> torch.Tensor:
        """probability() - other.probability(): the delta-probability map.  `other` may hold one member (the truth), which
        is broadcast against this one's M."""
        if not isinstance(other, PairStatistics):
            raise MdnoError(f"difference: other is a {type(other).__name__}")
        a, b = self.probability(), other.probability()
        members = {a.shape[-3], b.shape[-3]}
        if a.dim() != b.dim() or a.shape[-1] != b.shape[-1] or a.shape[:-3] != b.shape[:-3] or (len(members) == 2 and 1 not in members):
            raise MdnoError(f"difference: maps of shape {tuple(a.shape)} and {tuple(b.shape)}")
        return a - b

    def map_error(self, other: "PairStatistics", min_separation: int = 0) -> torch.Tensor:
        """The mean of |difference(other)| over the ordered pairs with |i - j| >= min_separation: f64 [..., M]; NaN where
        no pair is that far apart."""
        integer(min_separation, "map_error: min_separation", 0, None)
        d = self.difference(other).abs()
        idx = torch.arange(d.shape[-1], device=d.device)
        keep = ((idx[:, None] - idx[None, :]).abs() >= min_separation).to(torch.float64)
        return _ratio((d * keep).sum((-2, -1)), keep.sum().expand(d.shape[:-2]))

    def cpu(self) -> "PairStatistics":
        return PairStatistics(self.count.cpu(), None if self.sum_r is None else self.sum_r.cpu(),
                              None if self.sum_r2 is None else self.sum_r2.cpu(), self.n_frames.cpu(), self.threshold, self.box)

    @staticmethod
    def cat(parts: Sequence["PairStatistics"]) -> "PairStatistics":
        """Statistics of disjoint member ranges of the same steps and blocks, members in order."""
        p = parts[0]
        join = lambda ts: None if ts[0] is None else torch.cat(ts, -3)      # noqa: E731
        return PairStatistics(join([q.count for q in parts]), join([q.sum_r for q in parts]), join([q.sum_r2 for q in parts]),
                              p.n_frames, p.threshold, p.box)


def pair_statistics(frames: torch.Tensor, threshold: float = 8.0, box=None, block_len: int = 64, moments: bool = True) -> PairStatistics:
    """frames f32 [S, M, N, 3] (device) -> `PairStatistics` over blocks of `block_len` steps: per pair the frames in contact
    (closer than `threshold`, strictly) and, with `moments`, the sums of the distance and of its square, reduced over time on
    the device (include/mdno_contacts.h has the rule) — the contact-probability map of a run without a dense map per frame.
    `box` = (Lx, Ly, Lz), 0 for an open axis: distances by the minimum image; every periodic axis must be >= 2 * threshold.
    Asynchronous on the current stream; CPU tensors and bad arguments raise `MdnoError` before any device work."""
    threshold, box, block_len = ops.check_contact_args(threshold, box, block_len)
    count, sum_r, sum_r2 = ops.pair_statistics(frames, threshold, box, block_len, bool(moments))
    S = int(frames.shape[0])
    n = [min(block_len, S - b * block_len) for b in range(count.shape[0])]
    return PairStatistics(count, sum_r, sum_r2, torch.tensor(n, dtype=torch.int64, device=count.device), threshold, box)


def _rule_distances(x: torch.Tensor, box) -> torch.Tensor:
    """r f64 [N, N] of ONE host frame by the rule of include/mdno_contacts.h, in torch on the CPU (every operation rounded
    once: elementwise kernels are not contracted): r[i, j] from d = x_j - x_i."""
    x = x.detach().cpu().to(torch.float32).to(torch.float64)
    d = x[None, :, :] - x[:, None, :]
    sq = []
    for a in range(3):
        da = d[..., a]
        L = 0.0 if box is None else float(box[a])
        if L > 0.0:
            da = da - torch.round(da * (1.0 / L)) * L          # (torch.round: half to even, as rint)
        sq.append(da * da)
    return torch.sqrt((sq[0] + sq[1]) + sq[2])


@dataclass
class ContactPairs:
    """A list of pairs with one contact cutoff each — a native-contact definition: `pairs` i32 [P, 2], `cut` f64 [P],
    `cut_max` (a Python float: the largest cutoff, what a periodic box is checked against), for frames of `n_atoms` atoms
    (None: any frame that holds the largest index, `top`).  Built and validated on the host by `of`, `native` and
    `from_statistics`; `.to(device)` moves the tensors."""
    pairs: torch.Tensor
    cut: torch.Tensor
    cut_max: float
    n_atoms: Optional[int] = None
    top: int = -1

    @staticmethod
    def of(pairs, cut, n_atoms: Optional[int] = None) -> "ContactPairs":
        if n_atoms is not None:
            integer(n_atoms, "ContactPairs: n_atoms", 0, None)
        p = _index_array(pairs, 2, n_atoms, "pairs")
        n_p = int(p.shape[0])
        try:      # (Python numbers straight to f64)
            c = cut.detach().cpu().to(torch.float64) if torch.is_tensor(cut) else torch.as_tensor(cut, dtype=torch.float64)
            c = c.reshape(-1)
        except (TypeError, ValueError, RuntimeError):
            raise MdnoError("ContactPairs: cut is not an array of numbers") from None
        if c.numel() == 1 and n_p != 1:
            c = c.expand(n_p)
        if c.numel() != n_p:
            raise MdnoError(f"ContactPairs: {c.numel()} cutoffs for {n_p} pairs")
        c = c.contiguous().clone()
        if n_p and not (bool(torch.isfinite(c).all()) and bool((c >= 0).all())):
            raise MdnoError("ContactPairs: cut must be finite and >= 0")
        cut_max = float(c.max()) if n_p else 0.0
        if n_p and not cut_max > 0.0:
            raise MdnoError("ContactPairs: every cutoff is 0, no pair can be in contact")
        return ContactPairs(p, c, cut_max, n_atoms, int(p.max()) if n_p else -1)

    @staticmethod
    def _separated(n: int, min_separation) -> Tuple[torch.Tensor, torch.Tensor]:
        integer(min_separation, "ContactPairs: min_separation", 0, None)
        i, j = torch.triu_indices(n, n, 1)
        far = (j - i) >= min_separation
        return i[far], j[far]

    @staticmethod
    def native(reference_frame, threshold: float = 8.0, min_separation: int = 3, factor: float = 1.0, box=None) -> "ContactPairs":
        """The native contacts of ONE frame f32 [N, 3] (host or device; evaluated on the host by the rule): the pairs i < j with
        j - i >= min_separation and d0 < threshold.  Each pair's cutoff is factor * d0 where factor != 1 (the usual
        definition of Q: a native pair counts while it is closer than e.g. 1.2 x its native distance), else `threshold`."""
        threshold, box, _ = ops.check_contact_args(threshold, box, 1, "ContactPairs.native")
        factor = float(factor)
        if not (math.isfinite(factor) and factor > 0.0):
            raise MdnoError(f"ContactPairs.native: factor={factor}: expected a finite number > 0")
        x = reference_frame if torch.is_tensor(reference_frame) else torch.as_tensor(reference_frame)
        if x.dim() != 2 or x.shape[1] != 3:
            raise MdnoError(f"ContactPairs.native: reference_frame has shape {tuple(x.shape)}, expected ONE frame [N, 3]")
        n = int(x.shape[0])
        i, j = ContactPairs._separated(n, min_separation)
        d0 = _rule_distances(x, box)[i, j]
        keep = d0 < threshold
        i, j, d0 = i[keep], j[keep], d0[keep]
        cut = factor * d0 if factor != 1.0 else torch.full_like(d0, threshold)
        return ContactPairs.of(torch.stack([i, j], 1), cut, n)

    @staticmethod
    def from_statistics(stats: PairStatistics, min_probability: float = 0.5, min_separation: int = 3) -> "ContactPairs":
        """The pairs i < j with j - i >= min_separation whose contact probability over ALL of `stats` (one member: the truth)
        is >= min_probability, each with the statistics' threshold as its cutoff.  One read-back of the probability map."""
        if not isinstance(stats, PairStatistics):
            raise MdnoError(f"ContactPairs.from_statistics: stats is a {type(stats).__name__}")
        prob = stats.total().probability()
        if prob.shape[0] != 1:
            raise MdnoError(f"ContactPairs.from_statistics: the statistics hold {prob.shape[0]} members, expected one (the truth)")
        prob = prob[0].cpu()
        n = int(prob.shape[-1])
        i, j = ContactPairs._separated(n, min_separation)
        keep = prob[i, j] >= float(min_probability)
        i, j = i[keep], j[keep]
        return ContactPairs.of(torch.stack([i, j], 1), torch.full((int(i.numel()),), float(stats.threshold), dtype=torch.float64), n)

    def __len__(self) -> int:
        return int(self.pairs.shape[0])

    def to(self, device) -> "ContactPairs":
        return ContactPairs(self.pairs.to(device), self.cut.to(device), self.cut_max, self.n_atoms, self.top)

    def check_frames(self, n_atoms: int) -> None:
        if (self.n_atoms is not None and n_atoms != self.n_atoms) or self.top >= n_atoms:
            want = f"{self.n_atoms}" if self.n_atoms is not None else f"more than {self.top}"
            raise MdnoError(f"the contact pairs were built for frames of {want} atoms, these have {n_atoms}")


@dataclass
class ContactCorrelation:
    """Contact autocorrelation counts (ops.contact_correlation): `origins`, `both` i32 [M, P, L] per member, pair and lag —
    the steps t < S - lag in contact, and those in contact at t and at t + lag; `lags` i64 [L].  Every method runs in fp64
    on the device of the counts and reads nothing back."""
    origins: torch.Tensor
    both: torch.Tensor
    lags: torch.Tensor

    def survival(self) -> torch.Tensor:
        """sum_p both / sum_p origins: f64 [M, L], P(contact at t + lag | contact at t) pooled over the pairs; NaN where no
        pair was ever in contact."""
        return _ratio(self.both.sum(1, dtype=torch.int64), self.origins.sum(1, dtype=torch.int64))

    def per_pair(self) -> torch.Tensor:
        """both / origins: f64 [M, P, L]; NaN for a pair that was never in contact at an origin."""
        return _ratio(self.both, self.origins)

    def lifetime(self, dt: float = 1.0) -> torch.Tensor:
        """The trapezoid sum of survival() over the given lags times `dt`: f64 [M], a contact lifetime (in steps for dt = 1)
        up to the largest lag.  Fewer than two lags: 0."""
        s = self.survival()
        w = (self.lags[1:] - self.lags[:-1]).to(torch.float64) * float(dt)
        return (0.5 * (s[:, 1:] + s[:, :-1]) * w).sum(1)

    def total_variation(self, other: "ContactCorrelation") -> torch.Tensor:
        """|survival() - other.survival()| per lag: f64 [M, L] (`other` with one member is broadcast).  Same lags."""
        if not isinstance(other, ContactCorrelation) or not torch.equal(other.lags.cpu(), self.lags.cpu()):
            raise MdnoError("total_variation: the two correlations must have the same lags")
        return (self.survival() - other.survival()).abs()

    def cpu(self) -> "ContactCorrelation":
        return ContactCorrelation(self.origins.cpu(), self.both.cpu(), self.lags.cpu())

    @staticmethod
    def cat(parts: Sequence["ContactCorrelation"]) -> "ContactCorrelation":
        """Correlations of disjoint member ranges of the same pairs and lags, members in order."""
        return ContactCorrelation(torch.cat([q.origins for q in parts], 0), torch.cat([q.both for q in parts], 0), parts[0].lags)


@dataclass
class ContactSeries:
    """The contact indicator of a pair list at every step (ops.contact_bits): `bits` int64 [M, P, ceil(S / 64)] holding the
    words of the header's u64 (bit s % 64 of word s / 64 = pair p of member m in contact at step s), `per_frame` i32 [S, M]
    the listed pairs in contact per frame, `n_steps` = S and the `pairs` they belong to."""
    bits: torch.Tensor
    per_frame: torch.Tensor
    n_steps: int
    pairs: ContactPairs

    def fraction(self) -> torch.Tensor:
        """per_frame / P: f64 [S, M], the fraction of the listed (native) contacts present — Q(t); NaN for an empty list."""
        return _ratio(self.per_frame, torch.full((), len(self.pairs), dtype=torch.float64, device=self.per_frame.device))

    def series(self) -> torch.Tensor:
        """The bits unpacked: bool [M, P, S]."""
        k = torch.arange(64, dtype=torch.int64, device=self.bits.device)
        M, P, Wd = self.bits.shape
        return (((self.bits[..., None] >> k) & 1) != 0).reshape(M, P, Wd * 64)[..., :self.n_steps]

    def correlation(self, lags=None) -> ContactCorrelation:
        """origins and both per member, pair and lag (`lags`: integers in 0 .. S - 1, default `default_lags(S)`) from shifted
        words, AND and population count on the device -> `ContactCorrelation`."""
        if lags is None:
            lags = default_lags(self.n_steps) if self.n_steps > 0 else []
        vals = ops.check_contact_lags(lags, self.n_steps)
        origins, both = ops.contact_correlation(self.bits, self.n_steps, vals)
        return ContactCorrelation(origins, both, torch.tensor(vals, dtype=torch.int64, device=self.bits.device))

    def cpu(self) -> "ContactSeries":
        return ContactSeries(self.bits.cpu(), self.per_frame.cpu(), self.n_steps, self.pairs.to("cpu"))

    @staticmethod
    def cat(parts: Sequence["ContactSeries"]) -> "ContactSeries":
        """Series of disjoint member ranges of the same steps and pairs, members in order."""
        p = parts[0]
        return ContactSeries(torch.cat([q.bits for q in parts], 0), torch.cat([q.per_frame for q in parts], 1), p.n_steps, p.pairs)


def contact_series(frames: torch.Tensor, contact_pairs: ContactPairs, box=None) -> ContactSeries:
    """frames f32 [S, M, N, 3] (device) and a `ContactPairs` -> `ContactSeries`: one bit per (member, pair, step) and the
    number of listed pairs in contact per frame (include/mdno_contacts.h (b)).  `box`: distances by the minimum image, every
    periodic axis >= 2 * contact_pairs.cut_max.  Asynchronous on the current stream, nothing is read back; CPU tensors and
    bad arguments raise `MdnoError` before any device work."""
    if not isinstance(contact_pairs, ContactPairs):
        raise MdnoError(f"contact_series: contact_pairs is a {type(contact_pairs).__name__}")
    if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[-1] != 3:
        raise MdnoError("contact_series: frames must be [S, M, N, 3]")
    contact_pairs.check_frames(int(frames.shape[-2]))
    on_device(frames, "frames")
    if contact_pairs.pairs.device != frames.device:
        contact_pairs = contact_pairs.to(frames.device)
    S, M = int(frames.shape[0]), int(frames.shape[1])
    if len(contact_pairs) == 0:        # (no pair, no cutoff to check a box against: nothing to launch)
        ops.check_box(box, 0.0)
        return ContactSeries(torch.zeros((M, 0, -(-S // 64)), dtype=torch.int64, device=frames.device),
                             torch.zeros((S, M), dtype=torch.int32, device=frames.device), S, contact_pairs)
    bits, per_frame = ops.contact_bits(frames, contact_pairs.pairs, contact_pairs.cut, contact_pairs.cut_max, box)
    return ContactSeries(bits, per_frame, S, contact_pairs)


# ------------------------------------------------------------------------------------------------
# Solvent-accessible surface (csrc/surface.hip, include/mdno_surface.h has the rule)
def golden_spiral(n_points: int) -> torch.Tensor:
    """The default point table, f64 [n_points, 3], formed in numpy fp64 on the host: for k = 0 .. P - 1
        z = 1 - (2 k + 1) / P,   rho = sqrt(1 - z z),   phi = k * pi * (3 - sqrt(5))
        U[k] = (rho cos(phi), rho sin(phi), z)
    — equal steps in z (equal areas) and the golden angle between neighbours."""
    import numpy as np
    n_points = integer(n_points, "Spheres: n_points", 1, ops.SA_MAX_POINTS, exact=True)
    k = np.arange(n_points, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / float(n_points)
    rho = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return torch.from_numpy(np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1))


class Spheres:
    """The spheres a surface is taken of: `R` f64 [N], the EXPANDED radii r_i + probe; `points` f64 [P, 3], the sphere table;
    `reach` = 2 * max(R), a Python float (what a periodic box is checked against); `radii` and `probe` as given.  Built and
    validated on the host; `.to(device)` uploads once per device and hands the same object back after that.

    `radii`: a number (with `n_atoms`), a sequence or a CPU tensor of N van der Waals radii, each finite and > 0.  `probe`:
    finite and >= 0 (1.4 A: water).  `points`: any table f64 [P, 3] (P in 1 .. 1,024), by default `golden_spiral(n_points)`."""

    def __init__(self, radii, probe: float = 1.4, n_points: int = 96, points=None, n_atoms: Optional[int] = None):
        try:
            probe = float(probe)
        except (TypeError, ValueError):
            raise MdnoError(f"Spheres: probe = {probe!r}: expected a number") from None
        if not (math.isfinite(probe) and probe >= 0.0):
            raise MdnoError(f"Spheres: probe = {probe}: expected a finite number >= 0")
        try:      # (Python numbers straight to f64)
            r = radii.detach().cpu().to(torch.float64) if torch.is_tensor(radii) else torch.as_tensor(radii, dtype=torch.float64)
        except (TypeError, ValueError, RuntimeError):
            raise MdnoError("Spheres: radii is not a number or an array of numbers") from None
        if r.dim() == 0:
            if n_atoms is None:
                raise MdnoError("Spheres: one radius for every atom needs n_atoms")
            r = r.expand(integer(n_atoms, "Spheres: n_atoms", 0, exact=True))
        elif r.dim() != 1 or (n_atoms is not None and r.numel() != n_atoms):
            raise MdnoError(f"Spheres: radii has shape {tuple(r.shape)}, expected [N]" + ("" if n_atoms is None else f" with N = {n_atoms}"))
        r = r.contiguous().clone()
        if r.numel() and not (bool(torch.isfinite(r).all()) and bool((r > 0).all())):
            raise MdnoError("Spheres: every radius must be finite and > 0")
        if points is None:
            table = golden_spiral(n_points)
        else:
            try:
                table = points.detach().cpu().to(torch.float64) if torch.is_tensor(points) else torch.as_tensor(points, dtype=torch.float64)
            except (TypeError, ValueError, RuntimeError):
                raise MdnoError("Spheres: points is not an array of numbers") from None
            if table.dim() != 2 or table.shape[1] != 3 or not 1 <= table.shape[0] <= ops.SA_MAX_POINTS:
                raise MdnoError(f"Spheres: points has shape {tuple(table.shape)}, expected [P, 3] with P in 1 .. {ops.SA_MAX_POINTS}")
            if not bool(torch.isfinite(table).all()):
                raise MdnoError("Spheres: points must be finite")
            table = table.contiguous().clone()
        self.radii, self.probe = r, probe
        self.R = r + probe                       # fp64, one add per atom: the R of the rule
        self.points = table
        self.reach = 2.0 * float(self.R.max()) if r.numel() else 0.0
        if r.numel() and not math.isfinite(self.reach):
            raise MdnoError("Spheres: radius + probe overflows")
        self._on = {}

    @property
    def n_atoms(self) -> int:
        return int(self.R.shape[0])

    @property
    def n_points(self) -> int:
        return int(self.points.shape[0])

    def to(self, device) -> "Spheres":
        device = torch.device(device)
        if device == self.R.device:
            return self
        if device not in self._on:
            s = object.__new__(Spheres)
            s.radii, s.probe, s.reach = self.radii, self.probe, self.reach
            s.R, s.points = self.R.to(device), self.points.to(device)
            s._on = self._on
            self._on[device] = s
        return self._on[device]

    def check_frames(self, n_atoms: int) -> None:
        if n_atoms != self.n_atoms:
            raise MdnoError(f"the spheres were built for frames of {self.n_atoms} atoms, these have {n_atoms}")


@dataclass
class SurfaceArea:
    """Exposed-point counts of a run (ops.exposed_points): `counts` i32 [S, M, N] (or the frames' leading shape + [N]), -1 for
    an atom with a non-finite coordinate; `R` f64 [N], the expanded radii, on the device of the counts; `n_points` = P.  The
    area of a sphere's exposed part is 4 pi R_i^2 * count / P.  Every method is a few torch operations in fp64 on the device
    of `counts` and reads nothing back."""
    counts: torch.Tensor
    R: torch.Tensor
    n_points: int

    def _fraction(self) -> torch.Tensor:
        c = self.counts.to(torch.float64)
        return torch.where(self.counts < 0, torch.full_like(c, float("nan")), c) / float(self.n_points)

    def per_atom(self) -> torch.Tensor:
        """4 pi R_i^2 * counts / P: f64 like `counts`; NaN where the count is -1."""
        return (4.0 * math.pi) * (self.R * self.R) * self._fraction()

    def total(self) -> torch.Tensor:
        """The sum of per_atom() over the atoms: f64 [S, M]; NaN for a frame that holds a -1."""
        return self.per_atom().sum(-1)

    def per_group(self, index, n_groups: int) -> torch.Tensor:
        """The sum of per_atom() over the atoms of every group (residue): `index` [N], integers in 0 .. n_groups - 1 ->
        f64 [..., n_groups]; NaN for a group that holds a -1."""
        n_groups = integer(n_groups, "per_group: n_groups", 0, None)
        idx = (index.detach() if torch.is_tensor(index) else torch.as_tensor(index)).reshape(-1).cpu()
        if idx.numel() != self.counts.shape[-1] or idx.dtype.is_floating_point or idx.dtype == torch.bool or \
                (idx.numel() and not (0 <= int(idx.min()) and int(idx.max()) < n_groups)):
            raise MdnoError(f"per_group: index must hold {self.counts.shape[-1]} integers in 0 .. {n_groups - 1}")
        a = self.per_atom()
        out = torch.zeros(a.shape[:-1] + (n_groups,), dtype=torch.float64, device=a.device)
        return out.index_add_(-1, idx.to(torch.int64).to(a.device), a)

    def burial(self) -> torch.Tensor:
        """1 - counts / P: f64 like `counts`, the covered share of every sphere; NaN where the count is -1."""
        return 1.0 - self._fraction()

    def mean(self) -> torch.Tensor:
        """per_atom() averaged over the steps (the first axis): f64 [M, N]; NaN without steps."""
        a = self.per_atom()
        return _ratio(a.sum(0), torch.full((), a.shape[0], dtype=torch.float64, device=a.device))

    def mean_burial(self) -> torch.Tensor:
        """burial() averaged over the steps: f64 [M, N]."""
        b = self.burial()
        return _ratio(b.sum(0), torch.full((), b.shape[0], dtype=torch.float64, device=b.device))

    def difference(self, other: "SurfaceArea") -> torch.Tensor:
        """The RMS over the atoms of mean_burial() - other.mean_burial(): f64 [M] — 0 = every atom as buried, on average, as
        in the other run.  `other` may hold one member (the truth), which is broadcast against this one's M."""
        if not isinstance(other, SurfaceArea):
            raise MdnoError(f"difference: other is a {type(other).__name__}")
        a, b = self.mean_burial(), other.mean_burial()
        if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or (a.shape[0] != b.shape[0] and 1 not in (a.shape[0], b.shape[0])):
            raise MdnoError(f"difference: mean burials of shape {tuple(a.shape)} and {tuple(b.shape)}, expected [M, N] each")
        d = a - b
        return torch.sqrt(_ratio((d * d).sum(1), torch.full((), d.shape[1], dtype=torch.float64, device=d.device)))

    def cpu(self) -> "SurfaceArea":
        return SurfaceArea(self.counts.cpu(), self.R.cpu(), self.n_points)

    @staticmethod
    def cat(parts: Sequence["SurfaceArea"]) -> "SurfaceArea":
        """Counts of disjoint member ranges of the same steps and spheres, members in order."""
        return SurfaceArea(torch.cat([q.counts for q in parts], -2), parts[0].R, parts[0].n_points)


def surface_area(frames: torch.Tensor, spheres: Spheres, box=None, form: str = "auto") -> SurfaceArea:
    """frames f32 [S, M, N, 3] (or any [..., N, 3], device) and `Spheres` -> `SurfaceArea`: the Shrake-Rupley count of every
    atom of every frame (include/mdno_surface.h has the rule).  `box` = (Lx, Ly, Lz), 0 for an open axis: neighbours by the
    minimum image; every periodic axis must be >= 2 * spheres.reach.  Asynchronous on the current stream, nothing is read
    back; CPU tensors and bad arguments raise `MdnoError` before any device work."""
    if not torch.is_tensor(frames) or frames.dim() < 2 or frames.shape[-1] != 3:
        raise MdnoError("surface_area: frames must be [..., N, 3]")
    if not isinstance(spheres, Spheres):
        raise MdnoError(f"surface_area: spheres is a {type(spheres).__name__}")
    spheres.check_frames(int(frames.shape[-2]))
    if spheres.n_atoms == 0:            # (no sphere, no reach to check a box against: nothing to launch)
        ops.check_box(box, 0.0)
        ops.form_code(form, ops.FORECAST_FORMS)
        on_device(frames, "frames")
        return SurfaceArea(torch.zeros(tuple(frames.shape[:-1]), dtype=torch.int32, device=frames.device),
                           spheres.to(frames.device).R, spheres.n_points)
    ops.check_surface_args(spheres.reach, box, form)
    on_device(frames, "frames")
    sp = spheres.to(frames.device)
    return SurfaceArea(ops.exposed_points(frames, sp.R, sp.points, box, sp.reach, form), sp.R, sp.n_points)


def gather_scores(local_score: ForecastScore, total_members: int, group=None) -> ForecastScore:
    """The multi-rank counterpart of `rollout.gather_trajectories` for scores: every rank passes the score of ITS members
    (`rollout.shard_members`: member m runs on rank m % world) and receives the score of all `total_members`, members in
    global order — so a member that diverged on one rank is visible on all.  One collective over the small per-member
    arrays (8 * 5 * (S + 1) bytes per member).  Without torch.distributed, or at world size 1, returns its input."""
    import torch.distributed as dist

    from .rollout import gather_trajectories
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return local_score
    sc = local_score
    S, Ml = sc.mse.shape
    # one i64 payload [S + 1, M_local, 1, 5]: rows < S = (mse bits, rmsd bits, contacts); row S = first_nonfinite
    pay = torch.zeros((S + 1, Ml, 1, 5), dtype=torch.int64, device=sc.mse.device)
    pay[:S, :, 0, 0] = sc.mse.contiguous().view(torch.int64)
    pay[:S, :, 0, 1] = sc.rmsd.contiguous().view(torch.int64)
    pay[:S, :, 0, 2:] = sc.contacts
    pay[S, :, 0, 0] = sc.first_nonfinite.to(torch.int64)
    full = gather_trajectories(pay, total_members, group)
    return ForecastScore(full[:S, :, 0, 0].contiguous().view(torch.float64), full[:S, :, 0, 1].contiguous().view(torch.float64),
                         full[:S, :, 0, 2:].contiguous(), full[S, :, 0, 0].to(torch.int32))
