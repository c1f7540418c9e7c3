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
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import torch

from . import ops


@dataclass
class ForecastScore:
    mse: torch.Tensor                 # f64 [S, M]
    rmsd: torch.Tensor                # f64 [S, M]
    contacts: torch.Tensor            # i64 [S, M, 3]: forecast, truth, both
    first_nonfinite: torch.Tensor     # i32 [M]

    @staticmethod
    def _ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
        """num / den as f64, NaN where den == 0 (no host read, no exception)."""
        num, den = num.to(torch.float64), den.to(torch.float64)
        return torch.where(den == 0, torch.full_like(den, float("nan")), num / den.clamp_min(1.0))

    def precision(self) -> torch.Tensor:
        """Contacts in both / contacts in the forecast: f64 [S, M]."""
        return self._ratio(self.contacts[..., 2], self.contacts[..., 0])

    def recall(self) -> torch.Tensor:
        """Contacts in both / contacts in the truth: f64 [S, M]."""
        return self._ratio(self.contacts[..., 2], self.contacts[..., 1])

    def native_fraction(self) -> torch.Tensor:
        """The fraction of the true ("native") contacts the forecast keeps: both / truth, f64 [S, M]."""
        return self.recall()

    def jaccard(self) -> torch.Tensor:
        """Contacts in both / contacts in either: f64 [S, M]."""
        c = self.contacts
        return self._ratio(c[..., 2], c[..., 0] + c[..., 1] - c[..., 2])

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
