"""On-device autoregressive rollout and ensemble sharding.

`RolloutEngine` drives `mdno_rollout_plan_*` (include/mdno.h): the whole loop of
recursive_propagation (graph_kernel.py:396-413) — graph rebuild on the newest frame, forward,
window slide — stays in HBM; one step is captured into a hipGraph and replayed.

Ensemble members are independent trajectories (block-diagonal graph, no cross-member edges; the
reference's own batching never creates them either, dataset.py:41-45).  Across GPUs they are
sharded by member with NO collective during stepping; `gather_trajectories` is the single
RCCL all-gather (over xGMI on an MI355X node) that collects the finished trajectories.  It
replaces torch_geometric.nn.DataParallel (graph_kernel.py:528), which broadcasts parameters and
gathers outputs every step inside one process.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import torch

from . import _lib, forecast, ops
from ._args import INT_MAX
from ._lib import MdnoError, STATUS_EDGE_OVERFLOW, check, f32, ptr, raise_on_status, require_gpu


def default_edge_cap(members: int, n_atoms: int, threshold: float, density: float = 0.1, slack: float = 1.6) -> int:
    """Edge capacity for W_e: expected in-degree of a uniform cloud at `density` atoms/A^3 within
    `threshold`, times `slack`, bounded by the complete graph."""
    import math
    deg = 4.0 / 3.0 * math.pi * threshold ** 3 * density + 1.0
    per_member = min(n_atoms * n_atoms, int(n_atoms * deg * slack) + n_atoms)
    return max(members * per_member, members * n_atoms)


# conv_mode "auto", decided on the window an engine is reset with (include/mdno.h mdno_conv_mode_for_graph: factored
# from a mean degree of 40 and 16,384 edges per member on — measured on one box: chains of 600-1,300 atoms at 25-30
# edges per atom are 3-25 % faster materialised, the 504-atom box at 120 per atom 2.2x faster factored).  Protein-like
# chains (10-30 neighbours within 8 A) stay materialised whatever their length; dense boxes go factored.
AUTO_FACTORED_MIN_DEGREE = 40          # (probe bounds only: the rule itself lives in the library)
AUTO_FACTORED_MIN_EDGES = 16384        # per member
AUTO_MATERIALIZED_MAX_WORKSPACE = 64 << 30


def _model_ker_in(model) -> Optional[int]:
    """Edge attributes per edge of a KernelNN or an ops.ParamPack, read on the host (None: not recognisable here)."""
    if isinstance(model, ops.ParamPack):
        return int(model.tensors["k_w0"].shape[1])
    try:
        return int(model.state_dict()["conv1.net.layers.0.weight"].shape[1])
    except (AttributeError, KeyError):
        return None


def check_rollout_box(model, box, threshold: float):
    """`box` of an engine as ops.check_box returns it, plus what a periodic step needs of the model (ker_in == 6);
    MdnoError otherwise, before any device work."""
    box = ops.check_box(box, threshold)
    if box is not None and _model_ker_in(model) not in (None, 6):
        raise MdnoError(f"box: the model reads ker_in={_model_ker_in(model)} edge attributes, a periodic step forms "
                        f"[image of the source, destination] (6)")
    return box


def probe_edges(last: torch.Tensor, M: int, N: int, threshold: float, box) -> Tuple[int, bool]:
    """Edges of the radius graph (the periodic one under `box`) of a window's last frame [M,N,3], counted up to the
    bounds the "auto" and capacity decisions look at; (count, True) when there are more."""
    R = M * N
    probe_cap = max(AUTO_FACTORED_MIN_DEGREE * R, M * AUTO_FACTORED_MIN_EDGES) + R
    last = last.reshape(R, 3)
    if box is not None:
        g, _ = ops.radius_graph_pbc(last, N, threshold, box, edge_cap=probe_cap, with_attr=False)
    else:
        g = ops.radius_graph(last, N, threshold, edge_cap=probe_cap)
    return int(g.num_edges.item()), bool(int(g.status.item()) & STATUS_EDGE_OVERFLOW)


def _join_members(parts, join):
    """Results of disjoint member ranges of the same steps, members in order, as one.  `join` is the result's own rule: a
    record's `cat`; for a plain tensor the member axis to `torch.cat` along; for a tuple of tensors one axis per element
    (None: the element is the same for every range, taken from the first).  One range is its own result: nothing is copied
    and nothing launched."""
    if len(parts) == 1:
        return parts[0]
    if callable(join):
        return join(parts)
    if isinstance(join, int):
        return torch.cat(parts, join)
    return tuple(parts[0][i] if dim is None else torch.cat([p[i] for p in parts], dim) for i, dim in enumerate(join))


class _ProducedFrames:
    """What both engines offer on the frames they have produced: `run`, and the analyses of `forecast` / `ops` on the frames
    of steps first_step .. first_step + steps - 1 (default: all produced).  Each is defined here once, against `self.box`,
    `self.threshold`, `self.M` and one primitive an engine implements, `_member_views`, by a method that names its function
    and one of two rules:

    * per member (`_per_member`): the function runs on each part's frames and the results are joined along the member
      axis.  A member's result depends on its own frames alone, so a grouped engine gives the bits of one engine holding
      every member, and an engine of one part returns that part's result as it is.
    * pooled over the members (`_pooled`): the parts' frames are concatenated along the member axis (one copy; one part is
      taken as it is) and the function is called once.

    The frames are read where they lie — views of the trajectory buffers, never written — on the current stream after the
    engine's enqueued steps, without waiting on the host.  Arguments are refused on the host (`MdnoError`), in the engine's
    own box, before anything is enqueued."""

    _OWN_BOX = object()

    def run(self, window: torch.Tensor, x_aminoacid: torch.Tensor, steps: int) -> torch.Tensor:
        """reset + step + synchronize; returns the produced frames f32 [steps, M, N, 3] (`frames()`)."""
        self.reset(window, x_aminoacid)
        self.step(steps)
        self.synchronize()
        return self.frames()

    def _member_views(self, first_step: int, steps: Optional[int]) -> List[Tuple[int, int, torch.Tensor]]:
        """[(lo, hi, frames of members lo .. hi - 1: f32 [steps, hi - lo, N, 3]), ..] covering 0 .. M in member order, each a
        view handed out after the range was validated and the current stream made to wait for the stream that produces it."""
        raise NotImplementedError

    def _per_member(self, fn, join, first_step: int, steps: Optional[int]):
        return _join_members([fn(x) for _, _, x in self._member_views(first_step, steps)], join)

    def _pooled(self, first_step: int, steps: Optional[int]) -> torch.Tensor:
        return _join_members([x for _, _, x in self._member_views(first_step, steps)], 1)

    def score(self, truth: torch.Tensor, first_step: int = 0, steps: Optional[int] = None,
              threshold: Optional[float] = None, box=_OWN_BOX):
        """Per member: `forecast.score_forecast` against truth f32 [steps, N, 3] (every member against the same frames) or
        [steps, M, N, 3] (each part against its own members' slice) -> `forecast.ForecastScore`.  `threshold`: the contact
        cutoff, the engine's own by default.  `box`: the periodic cell the contacts are counted in, the engine's own by
        default (None: open)."""
        per_member = torch.is_tensor(truth) and truth.dim() == 4
        if per_member and truth.shape[1] != self.M:
            raise MdnoError(f"truth shape {tuple(truth.shape)}: expected {self.M} members")
        threshold = self.threshold if threshold is None else threshold
        box = self.box if box is _ProducedFrames._OWN_BOX else ops.check_box(box, threshold)
        views = self._member_views(first_step, steps)
        whole = len(views) == 1 or not per_member
        return _join_members([forecast.score_forecast(x, truth if whole else truth[:, lo:hi].contiguous(), threshold, box=box)
                              for lo, hi, x in views], forecast.ForecastScore.cat)

    def pair_histogram(self, r_max: float, n_bins: int = 200, first_step: int = 0, steps: Optional[int] = None):
        """Per member: `forecast.pair_histogram` in the engine's own box -> `forecast.PairHistogram`, counts i64
        [steps, M, n_bins]."""
        ops.check_histogram_args(r_max, n_bins, self.box)
        return self._per_member(lambda x: forecast.pair_histogram(x, r_max, n_bins, box=self.box),
                                forecast.PairHistogram.cat, first_step, steps)

    def radius_of_gyration(self, first_step: int = 0, steps: Optional[int] = None) -> torch.Tensor:
        """Per member: `ops.radius_of_gyration` -> f64 [steps, M]."""
        return self._per_member(ops.radius_of_gyration, 1, first_step, steps)

    def displacement_stats(self, lags=None, origin_stride: int = 1, remove_com: bool = False, r_max=None, n_bins: int = 0,
                           first_step: int = 0, steps: Optional[int] = None):
        """Per member: `forecast.displacement_stats` (MSD, non-Gaussian parameter, self van Hove histogram per member and
        lag) -> `forecast.DisplacementStats`."""
        return self._per_member(lambda x: forecast.displacement_stats(x, lags, origin_stride, remove_com, r_max, n_bins),
                                forecast.DisplacementStats.cat, first_step, steps)

    def velocity_autocorrelation(self, lags=None, origin_stride: int = 1, remove_com: bool = False,
                                 normalized: bool = False, first_step: int = 0, steps: Optional[int] = None):
        """Per member: `forecast.velocity_autocorrelation` -> (C f64 [M, L], lags i64 [L]; the lags are every part's)."""
        return self._per_member(lambda x: forecast.velocity_autocorrelation(x, lags, origin_stride, remove_com, normalized),
                                (0, None), first_step, steps)

    def ensemble_score(self, truth: torch.Tensor, first_step: int = 0, steps: Optional[int] = None):
        """Pooled: `forecast.ensemble_score` (error of the ensemble mean, spread, CRPS sums and rank histogram per step) of
        ALL the engine's M members taken as ONE ensemble, against truth f32 [steps, N, 3] -> `forecast.EnsembleScore`.
        Unlike the per-member statistics this cannot be merged from per-group results — the pair term
        sum_{m<k} |x_m - x_k| and the ranks run across the groups — so it is the bits of
        `forecast.ensemble_score(self.produced(first_step, steps), truth)`."""
        return forecast.ensemble_score(self._pooled(first_step, steps), truth)

    def cross_rmsd(self, reference: torch.Tensor, first_step: int = 0, steps: Optional[int] = None, matrix: bool = True):
        """Per member: `forecast.cross_rmsd` against reference f32 [Fb, N, 3] (superposed RMSD of every produced frame
        against every reference frame, the nearest reference frame per frame and the nearest produced frame per member and
        reference frame) -> `forecast.CrossRmsd`.  Rows and per-member columns never cross members and an element's bits
        depend on its two frames alone."""
        return self._per_member(lambda x: forecast.cross_rmsd(x, reference, matrix), forecast.CrossRmsd.cat, first_step, steps)

    def superpose(self, reference: torch.Tensor, first_step: int = 0, steps: Optional[int] = None):
        """Per member: `forecast.superpose` onto reference f32 [N, 3] -> (aligned f32 [steps, M, N, 3], rmsd f64 [steps, M]);
        a frame's outputs depend on that frame and the reference alone."""
        return self._per_member(lambda x: forecast.superpose(x, reference), (1, 1), first_step, steps)

    def assign(self, discretization, first_step: int = 0, steps: Optional[int] = None):
        """Per member: `forecast.Discretization.assign` -> `forecast.Assignment`, labels i32 and dist2 f64 [steps, M]: the
        state of every frame in a partition built from the truth (`forecast.discretize`)."""
        return self._per_member(discretization.assign, forecast.Assignment.cat, first_step, steps)

    def internal_coordinates(self, featurizer, radians: bool = False, dtype=torch.float32, first_step: int = 0,
                             steps: Optional[int] = None) -> torch.Tensor:
        """Per member: `forecast.internal_coordinates` in the engine's own box -> features [steps, M, D]: distances, angle
        cosines and dihedral (cos, sin) that do not depend on a reference frame."""
        return self._per_member(lambda x: forecast.internal_coordinates(x, featurizer, box=self.box, radians=radians, dtype=dtype),
                                1, first_step, steps)

    def pair_statistics(self, threshold: Optional[float] = None, block_len: int = 64, moments: bool = True, first_step: int = 0,
                        steps: Optional[int] = None):
        """Per member: `forecast.pair_statistics` (per pair and block of `block_len` steps: frames in contact, sums of the
        distance and of its square) in the engine's own box, at the engine's own threshold by default ->
        `forecast.PairStatistics`."""
        threshold = self.threshold if threshold is None else threshold
        ops.check_contact_args(threshold, self.box, block_len)
        return self._per_member(lambda x: forecast.pair_statistics(x, threshold, box=self.box, block_len=block_len, moments=moments),
                                forecast.PairStatistics.cat, first_step, steps)

    def contact_series(self, contact_pairs, first_step: int = 0, steps: Optional[int] = None):
        """Per member: `forecast.contact_series` (one bit per member, listed pair and step, and the listed pairs in contact
        per frame: Q(t)) in the engine's own box -> `forecast.ContactSeries`."""
        return self._per_member(lambda x: forecast.contact_series(x, contact_pairs, box=self.box),
                                forecast.ContactSeries.cat, first_step, steps)

    def surface_area(self, spheres, first_step: int = 0, steps: Optional[int] = None):
        """Per member: `forecast.surface_area` (the Shrake-Rupley count of exposed sphere points of every atom of every
        frame) in the engine's own box -> `forecast.SurfaceArea`, counts i32 [steps, M, N]."""
        if not isinstance(spheres, forecast.Spheres):
            raise MdnoError(f"surface_area: spheres is a {type(spheres).__name__}")
        ops.check_box(self.box, spheres.reach)
        return self._per_member(lambda x: forecast.surface_area(x, spheres, box=self.box), forecast.SurfaceArea.cat,
                                first_step, steps)

    def covariance(self, reference: torch.Tensor, mean: Optional[torch.Tensor] = None, lag: int = 0, first_step: int = 0,
                   steps: Optional[int] = None):
        """Pooled: `forecast.covariance` over the 3 N coordinates after the superposition onto reference f32 [N, 3] ->
        `forecast.Covariance`.  The sums run across the members, so `superpose` runs per member, its aligned frames are
        joined and ONE covariance call follows: the bits of
        `forecast.covariance(forecast.superpose(self.produced(first_step, steps), reference)[0], mean, lag)`."""
        return forecast.covariance(self.superpose(reference, first_step, steps)[0], mean, lag)


class RolloutEngine(_ProducedFrames):
    """Owns the trajectory buffer [W+max_steps, M, N, 3], the workspace and the captured step.

    noise_sigma > 0: a stochastic rollout (include/mdno_noise.h mdno_rollout_plan_set_noise) —
    every step adds noise_sigma * z(noise_seed, member_ids[m], absolute step, atom, component) to the frame it produces,
    before the frame is stored and read again.  `member_ids` (default 0 .. M-1) are the members' GLOBAL ids: member g
    draws the same noise alone, in any batch, group or rank (pass `shard_members(...)` on a rank).  With noise_sigma = 0
    (the default) nothing of this is launched or captured.

    box = (Lx, Ly, Lz): a periodic rollout (include/mdno_pbc.h mdno_rollout_plan_set_box) —
    every step builds the minimum-image radius graph of its newest frame and the forward reads the imaged edge
    attributes the graph kernel wrote (a buffer [edge_cap, 6] the engine owns).  0 = an open axis; every periodic axis
    needs L >= 2 * threshold; one box for all members, constant in time.  Frames are never wrapped.  With box = None
    (the default) nothing of this is launched or captured.  `first_step_from_sample` is unchanged: the sample brings
    its own edges (graph_kernel.construct_pairdata(..., box=)).

    constraints = a `forecast.DistanceConstraints`: a constrained rollout (include/mdno_constrain.h
    mdnocst_rollout_plan_set_constraints) — every step projects the frame it produces onto the
    distance bands where it lies, after the noise and before anything reads it: up to `constraint_iterations` sweeps per
    member, until its largest violation is at most `constraint_tol`, in the engine's own box.  The frames are those of
    `forecast.project_constraints` applied to every produced frame before it is fed back; `constraint_report` says what
    each step needed.  With constraints = None (the default) nothing of this is launched or captured."""

    def __init__(self, model, members: int, n_atoms: int, window: int, threshold: float = 8.0,
                 max_steps: int = 1000, edge_cap: Optional[int] = None, device=None, use_graph: bool = True,
                 noise_sigma: float = 0.0, noise_seed: int = 0, member_ids=None, box=None, constraints=None,
                 constraint_iterations: int = 8, constraint_tol: float = 0.0):
        self.box = check_rollout_box(model, box, threshold)
        self._box_attr = None            # f32 [edge_cap, 6] on the device, made with every plan of a periodic engine
        self._box_arg = None
        self.lib = _lib.load()
        self.device = require_gpu(device if device not in (None, "cuda") else None)
        fc2 = getattr(model, "fc2", None)
        out_width = fc2.out_features if fc2 is not None else getattr(getattr(model, "struct", None), "out_width", 3)
        if out_width != 3:
            raise MdnoError(f"rollout: out_width={out_width}, the model output must be a frame [N,3] (graph_kernel.py:407-410)")
        self.model = model
        self.M, self.N, self.W = int(members), int(n_atoms), int(window)
        self.threshold = float(threshold)
        self.max_steps = int(max_steps)
        self.noise_sigma, self.noise_seed = float(noise_sigma), int(noise_seed)
        if not (0.0 <= self.noise_sigma < float("inf")) or not 0 <= self.noise_seed < 2 ** 64:
            raise MdnoError(f"noise_sigma={noise_sigma} must be finite and >= 0, noise_seed={noise_seed} in [0, 2^64)")
        ids = list(range(self.M)) if member_ids is None else [int(i) for i in member_ids]
        if len(ids) != self.M or any(not 0 <= i <= INT_MAX for i in ids):
            raise MdnoError(f"member_ids: expected {self.M} ids in [0, 2^31), got {ids[:8]}{'..' if len(ids) > 8 else ''}")
        self.member_ids = ids
        self._member_ids_dev = None      # int32 [M] on the device, made when noise is on (the plan keeps its address)
        self.constraints, self.constraint_iterations, self.constraint_tol = self._check_constraints(
            constraints, constraint_iterations, constraint_tol)
        self._cst_table = None           # the coloured table on the device and the reports [max_steps, M], made when
        self._cst_report = None          # constraints are on (the plan keeps their addresses)
        self.edge_cap = int(edge_cap) if edge_cap is not None else self.M * self.N * self.N
        self.edge_cap = max(self.edge_cap, self.M * self.N)
        # no capacity given and the complete-graph bound is large (N > 256): the capacity is fitted to the graph of
        # the window the engine is reset with (4x its edges), and the workspace allocated then — W_e at N^2 edges
        # would be 16 GB at N = 1,000 for a chain that has 30,000
        self._fit_cap = edge_cap is None and self.M * self.N * self.N > 65536
        self.pack = model.param_pack(self.device) if hasattr(model, "param_pack") else model
        if not isinstance(self.pack, ops.ParamPack):
            raise MdnoError("model must be a KernelNN (or an ops.ParamPack)")
        dev = self.device
        # what conv_mode "auto" resolves to at this capacity (include/mdno.h MDNO_CONV_AUTO)
        self.conv_mode = {v: k for k, v in _lib.CONV_MODES.items()}[
            int(self.lib.mdno_resolve_conv_mode(self.pack.ref, self.M, self.edge_cap))]
        self.traj = torch.zeros((self.W + self.max_steps, self.M, self.N, 3), dtype=torch.float32, device=dev)
        self.workspace = None
        if not self._fit_cap:
            nbytes = self.lib.mdno_rollout_workspace_bytes(self.pack.ref, self.M, self.N, self.edge_cap)
            self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.edges_per_step = torch.zeros(self.max_steps, dtype=torch.int32, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.aa = None
        self.plan = C.c_void_p()
        # capture needs a real (non-default) stream
        self.stream = torch.cuda.Stream(device=dev)
        self.use_graph = bool(use_graph)
        self.steps_done = 0
        self._sample_first_step = False
        self._timer_records = 0        # capacity of the attached per-kernel timer (0 = none): re-attached to a rebuilt plan
        self.regrown = []              # (first re-run step, old edge_cap, new edge_cap) per growth of a fitted capacity
        self.mode_changes = []         # (step, from, to): "auto" changed formulation when the capacity grew mid-trajectory
        # "auto": what the edge capacity suggests until a window is known; reset() decides on its graph
        self._auto = (getattr(model, "conv_mode", None) if hasattr(model, "param_pack") else self.pack.conv_mode) == "auto"

    def _pack_for(self, conv_mode: str):
        if hasattr(self.model, "param_pack"):
            return self.model.param_pack(self.device, conv_mode=conv_mode)
        p = self.pack
        return ops.ParamPack({v: p.tensors[k] for k, v in ops.ParamPack.KEYS.items() if k in p.tensors},
                             p.struct.depth, self.device, p.gemm_mode, conv_mode)

    def _fit_capacity(self, e: int, over: bool) -> bool:
        R = self.M * self.N
        cap = self.M * self.N * self.N if over else min(self.M * self.N * self.N, max(4 * e, e + 16 * R) + R)
        if cap == self.edge_cap:
            return False
        self.edge_cap = cap
        return True

    def _wanted_mode(self, e: int, over: bool) -> str:
        """conv_mode "auto" on a counted graph of this engine's members (AUTO_FACTORED_* above)."""
        if over:
            e = max(e, self.M * max(AUTO_FACTORED_MIN_DEGREE * self.N, AUTO_FACTORED_MIN_EDGES))
        return {v: k for k, v in _lib.CONV_MODES.items()}[
            int(self.lib.mdno_conv_mode_for_graph(self.pack.ref, self.M, self.N, int(e)))]

    def _apply_mode(self, want: str, record_at: Optional[int] = None) -> bool:
        """Switch to formulation `want` where the model's dimensions (and, for materialized, the workspace bound) allow
        it.  Returns True if the engine changed formulation (its plan must then be rebuilt).  `record_at`: the step
        from which the new formulation applies when the change happens MID-trajectory (a regrown capacity) — recorded
        in `mode_changes`, step 0 included; None at reset() (the choice for the whole trajectory is no change)."""
        if want == self.conv_mode:
            return False
        pack = self._pack_for(want)
        if {v: k for k, v in _lib.CONV_MODES.items()}[
                int(self.lib.mdno_resolve_conv_mode(pack.ref, self.M, self.edge_cap))] != want:
            return False                 # (factored is not available for this model's dimensions)
        need = self.lib.mdno_rollout_workspace_bytes(pack.ref, self.M, self.N, self.edge_cap)
        if want == "materialized" and need > AUTO_MATERIALIZED_MAX_WORKSPACE:
            return False                 # W_e at this edge capacity does not fit: stay factored
        if record_at is not None:
            self.mode_changes.append((int(record_at), self.conv_mode, want))
        self.pack, self.conv_mode = pack, want
        return True

    def _resolve_auto(self, e: int, over: bool, record_at: Optional[int] = None) -> bool:
        return self._apply_mode(self._wanted_mode(e, over), record_at)

    def _create_plan(self):
        if self.plan:
            check(self.lib.mdno_rollout_plan_destroy(self.plan), "mdno_rollout_plan_destroy")
            self.plan = C.c_void_p()
        aa_pm = int(self.aa.numel() == self.M * self.N and self.M > 1)
        check(self.lib.mdno_rollout_plan_create(
            C.byref(self.plan), self.pack.ref, ptr(self.traj), self.M, self.W, self.N, self.max_steps,
            ptr(self.aa), aa_pm, self.threshold, self.edge_cap, ptr(self.workspace),
            self.workspace.numel(),
            ptr(self.edges_per_step), ptr(self.status), int(self.use_graph), self.stream.cuda_stream),
            "mdno_rollout_plan_create")
        if self.noise_sigma > 0.0:       # (a rebuilt plan — regrown capacity — draws the same noise for the same steps)
            if self._member_ids_dev is None:
                self._member_ids_dev = torch.tensor(self.member_ids, dtype=torch.int32, device=self.device)
            check(self.lib.mdno_rollout_plan_set_noise(self.plan, self.noise_sigma, self.noise_seed,
                                                       ptr(self._member_ids_dev)), "mdno_rollout_plan_set_noise")
        if self.box is not None:         # (a rebuilt plan has a new capacity: a new attribute buffer)
            self._attach_box()
        else:
            self._box_attr = None
        if self.constraints is not None:  # (a rebuilt plan gets its constraints again, as it gets its box)
            self._attach_constraints()
        if self._timer_records:          # the timer lived in the plan just destroyed: its records are gone, the attachment is not
            check(self.lib.mdno_rollout_plan_timer_attach(self.plan, self._timer_records), "timer_attach")

    def _attach_box(self) -> None:
        """A fresh attribute buffer at the current capacity, and self.box, given to the plan."""
        self._box_attr = torch.empty((self.edge_cap, 6), dtype=torch.float32, device=self.device)
        self._box_arg = ops.box_arg(self.box)
        check(self.lib.mdno_rollout_plan_set_box(self.plan, self._box_arg, ptr(self._box_attr)), "mdno_rollout_plan_set_box")

    def set_box(self, box) -> None:
        """Give the engine another periodic cell, or None for the open step (mdno_rollout_plan_set_box: with None the
        plan has the launches and the captured graph of one that never had a box).  Before the first step after
        reset() only; later resets keep it."""
        box = check_rollout_box(self.model, box, self.threshold)
        if self.steps_done != 0:
            raise MdnoError("set_box: only before the first step after reset()")
        self.box = box
        if not self.plan:
            return
        if box is None:
            self._box_attr = None
            check(self.lib.mdno_rollout_plan_set_box(self.plan, None, None), "mdno_rollout_plan_set_box")
        else:
            self._attach_box()

    def _check_constraints(self, constraints, iterations, tol):
        """(constraints or None, iterations, tol) of an engine, validated on the host; an empty list is no constraints."""
        from .forecast import DistanceConstraints
        iterations, tol = ops.check_projection_args(iterations, tol)
        if constraints is None:
            return None, iterations, tol
        if not isinstance(constraints, DistanceConstraints):
            raise MdnoError(f"constraints is a {type(constraints).__name__}: expected a forecast.DistanceConstraints or None")
        constraints.check_frames(self.N)
        if self.N > ops.CST_MAX_ATOMS:
            raise MdnoError(f"constraints: frames of {self.N} atoms, the projection holds at most {ops.CST_MAX_ATOMS}")
        return (constraints if len(constraints) else None), iterations, tol

    def _attach_constraints(self) -> None:
        """self.constraints, coloured on the device, and the report buffers, given to the plan."""
        from .forecast import ConstraintReport
        t = self.constraints.coloured(self.device)
        if self._cst_report is None:
            self._cst_report = ConstraintReport(torch.zeros((self.max_steps, self.M), dtype=torch.int32, device=self.device),
                                                torch.zeros((self.max_steps, self.M), dtype=torch.float64, device=self.device),
                                                torch.zeros((self.max_steps, self.M), dtype=torch.float64, device=self.device))
        self._cst_table, r = t, self._cst_report
        check(self.lib.mdnocst_rollout_plan_set_constraints(
            self.plan, ptr(t.pairs), ptr(t.lo), ptr(t.hi), int(t.pairs.shape[0]), ptr(t.colour_ptr), t.n_colours, ptr(t.weights),
            self.constraint_iterations, self.constraint_tol, ptr(r.sweeps), ptr(r.viol_in), ptr(r.viol_out)),
            "mdnocst_rollout_plan_set_constraints")

    def set_constraints(self, constraints, iterations: Optional[int] = None, tol: Optional[float] = None) -> None:
        """Give the engine other distance constraints, or None for the plain step (mdnocst_rollout_plan_set_constraints:
        with None the plan has the launches and the captured graph of one that never had constraints).  `iterations`, `tol`:
        None keeps the engine's.  Before the first step after reset() only; later resets keep them."""
        if self.steps_done != 0:
            raise MdnoError("set_constraints: only before the first step after reset()")
        self.constraints, self.constraint_iterations, self.constraint_tol = self._check_constraints(
            constraints, self.constraint_iterations if iterations is None else iterations,
            self.constraint_tol if tol is None else tol)
        if not self.plan:
            return
        if self.constraints is None:
            self._cst_table = None
            check(self.lib.mdnocst_rollout_plan_set_constraints(self.plan, None, None, None, 0, None, 0, None, 0, 0.0, None, None,
                                                                None), "mdnocst_rollout_plan_set_constraints")
        else:
            self._attach_constraints()

    def constraint_report(self, first_step: int = 0, steps: Optional[int] = None):
        """What the projection did to the frames of steps first_step .. first_step + steps - 1 (default: all produced) ->
        `forecast.ConstraintReport`, sweeps i32 and viol_in / viol_out f64 [steps, M] (views of the engine's buffers, read
        on the current stream after the engine's enqueued steps)."""
        from .forecast import ConstraintReport
        if self.constraints is None or self._cst_report is None:
            raise MdnoError("constraint_report: the engine has no constraints")
        first_step, steps = self._score_range(first_step, steps)
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        r = self._cst_report
        sl = slice(first_step, first_step + steps)
        return ConstraintReport(r.sweeps[sl], r.viol_in[sl], r.viol_out[sl])

    @property
    def steps_per_launch(self) -> int:
        """0 = plain launches, 1 = one captured step per graph launch, 8 = eight (short chains); include/mdno.h."""
        return int(self.lib.mdno_rollout_plan_steps_per_launch(self.plan)) if self.plan else 0

    def reset(self, window: torch.Tensor, x_aminoacid: torch.Tensor, _conv_mode: Optional[str] = None) -> None:
        """window: f32 [W,M,N,3] (time-major), [W,N,3] for M=1; x_aminoacid i64 [N] or [M*N].
        (_conv_mode: what "auto" resolved to for the whole shard this engine is a group of — GroupedRolloutEngine.)"""
        w = f32(window.to(self.device))
        if w.dim() == 3:
            w = w.unsqueeze(1)
        if tuple(w.shape) != (self.W, self.M, self.N, 3):
            raise MdnoError(f"window shape {tuple(w.shape)} != {(self.W, self.M, self.N, 3)}")
        aa = x_aminoacid.to(device=self.device, dtype=torch.long).contiguous()
        if aa.numel() not in (self.N, self.M * self.N):
            raise MdnoError(f"x_aminoacid has {aa.numel()} entries, expected {self.N} or {self.M * self.N}")
        torch.cuda.current_stream(self.device).synchronize()
        self.stream.synchronize()
        self.traj[:self.W].copy_(w)
        self.status.zero_()
        new_aa = self.aa is None or self.aa.shape != aa.shape
        if new_aa:
            self.aa = aa
        else:
            self.aa.copy_(aa)
        torch.cuda.current_stream(self.device).synchronize()
        changed = False
        e, over = 0, False
        if self._fit_cap or (self._auto and not _conv_mode):
            e, over = probe_edges(self.traj[self.W - 1], self.M, self.N, self.threshold, self.box)
        if self._fit_cap:
            changed |= self._fit_capacity(e, over)
        if self._auto:
            changed |= self._apply_mode(_conv_mode) if _conv_mode else self._resolve_auto(e, over)
        need = self.lib.mdno_rollout_workspace_bytes(self.pack.ref, self.M, self.N, self.edge_cap)
        if self.workspace is None or need > self.workspace.numel() or 2 * need < self.workspace.numel():
            self.workspace = None        # (release before allocating: the two could be tens of GB each)
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            changed = True
        if new_aa or changed or not self.plan:
            self._create_plan()
        self.steps_done = 0
        self._sample_first_step = False
        self.regrown, self.mode_changes = [], []

    def first_step_from_sample(self, edge_index: torch.Tensor, edge_attr: torch.Tensor) -> None:
        """Produce frame W from the start sample's OWN graph and edge attributes, as the reference's
        first loop iteration does (graph_kernel.py:401-404: `dataset[start]` carries the graph of the
        window's FIRST frame, dataset.py:189-201; only later steps rebuild it on the newest frame).
        Single-member engines only; call after reset().  With noise_sigma > 0 the frame gets the noise of step 0 like
        any other step's (the values `ops.noise_fill` gives for this member, added in the same fp32 arithmetic), and with
        constraints it is then projected like any other step's (`forecast.project_constraints`; row 0 of the report)."""
        if self.M != 1 or self.steps_done != 0:
            raise MdnoError("first_step_from_sample: needs M == 1 and a freshly reset engine")
        graph = ops.coo_to_csr(edge_index.to(self.device), self.N)
        # an explicit edge list runs in the engine's own formulation (the factored form takes any destination-sorted graph)
        out, _ = ops.kernelnn_forward(self.pack, self.traj[:self.W], self.aa, graph,
                                      edge_attr=edge_attr.to(self.device))
        if self.noise_sigma > 0.0:
            out = out + ops.noise_fill(self.noise_seed, self.member_ids, 0, self.N, sigma=self.noise_sigma,
                                       device=self.device).view(self.N, 3)
        if self.constraints is not None:     # and the projection of step 0, after the noise like any other step's
            from .forecast import project_constraints
            out, rep = project_constraints(out.reshape(1, self.N, 3), self.constraints, box=self.box,
                                           iterations=self.constraint_iterations, tol=self.constraint_tol)
            out, r = out.view(self.N, 3), self._cst_report
            r.sweeps[0], r.viol_in[0], r.viol_out[0] = rep.sweeps, rep.viol_in, rep.viol_out
        self.traj[self.W, 0].copy_(out)
        self.edges_per_step[0] = int(edge_index.shape[1])
        torch.cuda.current_stream(self.device).synchronize()
        self.steps_done = 1
        self._sample_first_step = True

    def step(self, steps: int) -> None:
        """Enqueue `steps` more frames on the engine's stream (asynchronous)."""
        if not self.plan:
            raise MdnoError("RolloutEngine.reset(window, x_aminoacid) must be called first")
        check(self.lib.mdno_rollout_plan_run(self.plan, self.steps_done, int(steps), self.stream.cuda_stream),
              "mdno_rollout_plan_run")
        self.steps_done += int(steps)

    KERNEL_IDS = {"nnconv": 0, "edge_mlp_gemm1": 1, "edge_mlp_gemm2": 2, "edge_mlp_l0": 3, "radius_graph": 4,
                  "node_prologue": 5, "fc_out": 6, "nnconv_combine": 7, "factored_y": 8}

    def attach_timer(self, max_records: int) -> None:
        """Per-kernel HIP-event timing (measurement aid): subsequent step() calls issue plain
        launches bracketed by events on the engine's stream."""
        check(self.lib.mdno_rollout_plan_timer_attach(self.plan, int(max_records)), "timer_attach")
        self._timer_records = int(max_records)

    def read_timer(self) -> dict:
        """{kernel: (total_ms, launches)}; synchronises the engine's stream first."""
        self.stream.synchronize()
        out = {}
        for name, kid in self.KERNEL_IDS.items():
            ms, n = C.c_double(0.0), C.c_int64(0)
            check(self.lib.mdno_rollout_plan_timer_read(self.plan, kid, C.byref(ms), C.byref(n)), "timer_read")
            out[name] = (ms.value, n.value)
        return out

    def detach_timer(self) -> None:
        self.stream.synchronize()
        check(self.lib.mdno_rollout_plan_timer_detach(self.plan), "timer_detach")
        self._timer_records = 0

    FALLBACK_KEYS = ops.FALLBACK_KEYS

    def fallback_counts(self) -> dict:
        """Which path the products of gemm_mode "split_f16" took since the last `step()` call (include/mdno.h,
        mdno_rollout_plan_fallback_counts): K1 workgroups of the factored conv rerun on bf16 planes, destinations whose
        operands were taken unscaled, edge-MLP products (GEMM x chunk) redone on bf16 planes.  All zero = every product
        ran on two fp16 planes (the fast path); non-zero = same results to fp32 rounding, more matrix work.
        Synchronises the engine's stream."""
        if not self.plan:
            return {k: 0 for k in self.FALLBACK_KEYS}
        out = (C.c_int64 * 4)()
        check(self.lib.mdno_rollout_plan_fallback_counts(self.plan, out, self.stream.cuda_stream), "fallback_counts")
        return {k: int(out[i]) for i, k in enumerate(self.FALLBACK_KEYS)}

    def _grow_and_rerun(self, st: int) -> int:
        """The radius graph of some step outgrew a capacity that was FITTED to the start window (no `edge_cap` given,
        N > 256): the reference keeps building the denser graph (graph_kernel.py:363-368), so the engine does too —
        capacity x4 (at most the complete graph), new workspace and plan, and the steps from the first truncated one
        on are run again (frames before it are untouched: their graphs fitted).  Recorded in `self.regrown`; with
        conv_mode "auto" the larger graph can take the other formulation from that step on (`self.mode_changes`; the
        two agree to fp32 reassociation, not bitwise).  An attached timer is re-attached to the new plan (its records
        up to here are lost with the old one).  Returns the new status word."""
        target = self.steps_done
        eps = self.edges_per_step[:target].cpu()
        hit = (eps >= self.edge_cap).nonzero()
        first = int(hit[0]) if hit.numel() else 0
        if self._sample_first_step:
            first = max(first, 1)                # step 0 ran on the sample's own edge list (cannot overflow)
        old = self.edge_cap
        self.edge_cap = min(self.M * self.N * self.N, 4 * old)
        self.regrown.append((first, old, self.edge_cap))
        if self._auto:
            self._resolve_auto(old, False, record_at=first)       # the graph now has at least `old` edges
        need = self.lib.mdno_rollout_workspace_bytes(self.pack.ref, self.M, self.N, self.edge_cap)
        self.workspace = None
        self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        self.status.zero_()
        torch.cuda.current_stream(self.device).synchronize()
        self._create_plan()
        self.steps_done = first
        self.step(target - first)
        self.stream.synchronize()
        return (st & ~STATUS_EDGE_OVERFLOW) | int(self.status.item())

    def synchronize(self) -> None:
        self.stream.synchronize()
        st = int(self.status.item())
        while (st & STATUS_EDGE_OVERFLOW) and self._fit_cap and self.edge_cap < self.M * self.N * self.N:
            st = self._grow_and_rerun(st)
        if st & STATUS_EDGE_OVERFLOW:
            raise MdnoError(f"radius graph exceeded edge_cap={self.edge_cap}; construct the engine with a larger cap")
        raise_on_status(st, "rollout")

    def frames(self) -> torch.Tensor:
        return self.traj[self.W:self.W + self.steps_done]

    def produced(self, first_step: int, steps: int) -> torch.Tensor:
        """Frames of steps first_step .. first_step + steps - 1: f32 [steps, M, N, 3] (a view of the trajectory buffer)."""
        return self.traj[self.W + first_step:self.W + first_step + steps]

    def _score_range(self, first_step: int, steps: Optional[int]) -> Tuple[int, int]:
        first_step = int(first_step)
        steps = self.steps_done - first_step if steps is None else int(steps)
        if first_step < 0 or steps < 0 or first_step + steps > self.steps_done:
            raise MdnoError(f"score: steps {first_step} .. {first_step + steps - 1} are not all among the "
                            f"{self.steps_done} produced")
        return first_step, steps

    def _member_views(self, first_step: int, steps: Optional[int]):
        first_step, steps = self._score_range(first_step, steps)
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return [(0, self.M, self.produced(first_step, steps))]

    def close(self) -> None:
        if self.plan:
            self.stream.synchronize()
            self.lib.mdno_rollout_plan_destroy(self.plan)
            self.plan = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GroupedRolloutEngine(_ProducedFrames):
    """The members of a shard as `groups` independent `RolloutEngine`s (contiguous member ranges), each with its own
    stream and its own captured step, stepped together.  Members never interact and conv_mode "auto" is resolved ONCE,
    on the graph of the whole shard, and given to every group (a group deciding on its own members could take the other
    formulation when densities differ), so the frames are those of one engine holding them all: bitwise for members of
    like magnitude (the ensemble case: perturbed copies of one system), and to fp32 rounding in general — the edge-MLP
    chooses between its fp16 and bf16 plane products per launch from the magnitudes it sees (split_layout.h), and a
    group can see other magnitudes than the whole shard.  A group whose FITTED capacity is outgrown mid-trajectory regrows
    on its own and re-resolves "auto" on its own members (RolloutEngine._grow_and_rerun): from that step on the groups
    may run different formulations — `conv_mode` then reads "mixed:..", every group's `mode_changes` says where — and
    the one-engine equivalence holds to fp32 reassociation only.  What changes is the schedule: one group's edge-MLP (matrix-pipe-bound) and launch tails run
    beside another group's convs (fabric-bound) — 5 % at 8 x 504 atoms, 3 % at 64 (EXPERIMENTS.md section 0.2b).  Same
    reset / step / synchronize / run / frames interface and the same analyses of the produced frames (`_ProducedFrames`: one
    part per group); `traj` and `edges_per_step` are assembled on access."""

    def __init__(self, model, members: int, n_atoms: int, window: int, threshold: float = 8.0, max_steps: int = 1000,
                 edge_cap: Optional[int] = None, device=None, use_graph: bool = True, groups: int = 2,
                 noise_sigma: float = 0.0, noise_seed: int = 0, member_ids=None, box=None, constraints=None,
                 constraint_iterations: int = 8, constraint_tol: float = 0.0):
        self.box = check_rollout_box(model, box, threshold)      # one box for every group
        self.M, self.N, self.W = int(members), int(n_atoms), int(window)
        self.threshold = float(threshold)
        ids = list(range(self.M)) if member_ids is None else [int(i) for i in member_ids]
        if len(ids) != self.M:
            raise MdnoError(f"member_ids: expected {self.M} ids, got {len(ids)}")
        self.member_ids = ids
        g = max(1, min(int(groups), self.M))
        base, extra = divmod(self.M, g)
        self.bounds, lo = [], 0
        for i in range(g):
            hi = lo + base + (1 if i < extra else 0)
            self.bounds.append((lo, hi))
            lo = hi
        self.engines = [RolloutEngine(model, hi - lo, n_atoms, window, threshold, max_steps=max_steps,
                                      edge_cap=None if edge_cap is None else max(1, -(-int(edge_cap) * (hi - lo) // self.M)),
                                      device=device, use_graph=use_graph, noise_sigma=noise_sigma, noise_seed=noise_seed,
                                      member_ids=ids[lo:hi], box=self.box, constraints=constraints,
                                      constraint_iterations=constraint_iterations, constraint_tol=constraint_tol)
                        for lo, hi in self.bounds]           # (one constraint list, one table on the device, for every group)
        self.device = self.engines[0].device
        self.max_steps = int(max_steps)

    @property
    def conv_mode(self):
        modes = {e.conv_mode for e in self.engines}
        return self.engines[0].conv_mode if len(modes) == 1 else "mixed:" + ",".join(sorted(modes))

    @property
    def steps_done(self):
        return self.engines[0].steps_done

    @property
    def regrown(self):
        return [(g,) + r for g, e in enumerate(self.engines) for r in e.regrown]

    @property
    def workspace_bytes(self) -> int:
        return sum(e.workspace.numel() for e in self.engines if e.workspace is not None)

    def reset(self, window: torch.Tensor, x_aminoacid: torch.Tensor) -> None:
        """window f32 [W,M,N,3]; x_aminoacid i64 [N] (shared) or [M*N]."""
        if window.dim() == 3:
            window = window.unsqueeze(1)
        if tuple(window.shape) != (self.W, self.M, self.N, 3):
            raise MdnoError(f"window shape {tuple(window.shape)} != {(self.W, self.M, self.N, 3)}")
        if x_aminoacid.numel() not in (self.N, self.M * self.N):
            raise MdnoError(f"x_aminoacid has {x_aminoacid.numel()} entries, expected {self.N} or {self.M * self.N}")
        per_member = x_aminoacid.numel() == self.M * self.N and self.M > 1
        want = None
        if any(e._auto for e in self.engines):      # the rule one engine holding every member would apply
            e0 = self.engines[0]
            n_e, over = probe_edges(f32(window[self.W - 1].to(self.device)), self.M, self.N, self.threshold, self.box)
            if over:
                n_e = max(n_e, self.M * max(AUTO_FACTORED_MIN_DEGREE * self.N, AUTO_FACTORED_MIN_EDGES))
            want = {v: k for k, v in _lib.CONV_MODES.items()}[
                int(e0.lib.mdno_conv_mode_for_graph(e0.pack.ref, self.M, self.N, n_e))]
        for e, (lo, hi) in zip(self.engines, self.bounds):
            e.reset(window[:, lo:hi].contiguous(), x_aminoacid[lo * self.N:hi * self.N] if per_member else x_aminoacid,
                    _conv_mode=want)

    def step(self, steps: int) -> None:
        for e in self.engines:      # asynchronous on each engine's own stream
            e.step(steps)

    @property
    def constraints(self):
        return self.engines[0].constraints

    def set_constraints(self, constraints, iterations: Optional[int] = None, tol: Optional[float] = None) -> None:
        """`RolloutEngine.set_constraints` for every group."""
        for e in self.engines:
            e.set_constraints(constraints, iterations, tol)

    def constraint_report(self, first_step: int = 0, steps: Optional[int] = None):
        """`RolloutEngine.constraint_report` of every group, members in order: a member's projection depends on its own
        frame alone, so these are the reports of one engine holding every member."""
        from .forecast import ConstraintReport
        return ConstraintReport.cat([e.constraint_report(first_step, steps) for e in self.engines])

    def fallback_counts(self) -> dict:
        """Sum of the groups' counters (RolloutEngine.fallback_counts)."""
        tot = {k: 0 for k in RolloutEngine.FALLBACK_KEYS}
        for e in self.engines:
            for k, v in e.fallback_counts().items():
                tot[k] += v
        return tot

    def wait(self) -> None:
        """Block until every group's stream has drained (no status check: `synchronize` does that)."""
        for e in self.engines:
            e.stream.synchronize()

    def synchronize(self) -> None:
        for e in self.engines:
            e.synchronize()

    @property
    def traj(self) -> torch.Tensor:
        return torch.cat([e.traj for e in self.engines], dim=1)

    def frames(self) -> torch.Tensor:
        return torch.cat([e.frames() for e in self.engines], dim=1)

    def produced(self, first_step: int, steps: int) -> torch.Tensor:
        """Frames of steps first_step .. first_step + steps - 1 of every group, members in order: [steps, M, N, 3] (only
        these frames are copied — `traj` concatenates the groups' whole buffers)."""
        return torch.cat([e.produced(first_step, steps) for e in self.engines], dim=1)

    def _member_views(self, first_step: int, steps: Optional[int]):
        return [(lo, hi, x) for e, (lo, hi) in zip(self.engines, self.bounds) for _, _, x in e._member_views(first_step, steps)]

    @property
    def edges_per_step(self) -> torch.Tensor:
        return torch.stack([e.edges_per_step for e in self.engines]).sum(0, dtype=torch.int32)

    def close(self) -> None:
        for e in self.engines:
            e.close()


# --------------------------------------------------------------------------- ensemble sharding
def shard_members(total_members: int, rank: int, world_size: int) -> List[int]:
    """Member m runs on rank m mod world_size."""
    if not (0 <= rank < world_size):
        raise ValueError(f"rank {rank} outside world of {world_size}")
    return list(range(rank, total_members, world_size))


def gather_trajectories(local: torch.Tensor, total_members: int, group=None) -> torch.Tensor:
    """All-gather member trajectories: local f32 [T, M_local, N, 3] -> [T, total_members, N, 3] on
    every rank, members in global order.  One collective (RCCL on GPUs; gloo for CPU tests).
    Ranks may hold unequal member counts (total not divisible by world): shards are padded to the
    largest count for the collective and trimmed afterwards."""
    import torch.distributed as dist
    if not dist.is_initialized():
        if local.shape[1] != total_members:
            raise ValueError("not distributed: local shard must hold every member")
        return local
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    counts = [len(shard_members(total_members, r, world)) for r in range(world)]
    if local.shape[1] != counts[rank]:
        raise ValueError(f"rank {rank} holds {local.shape[1]} members, expected {counts[rank]}")
    m_max = max(counts)
    T, _, N, D = local.shape
    send = local
    if counts[rank] < m_max:
        pad = torch.zeros((T, m_max - counts[rank], N, D), dtype=local.dtype, device=local.device)
        send = torch.cat([local, pad], dim=1)
    send = send.contiguous()
    staged = local.is_cuda and dist.get_backend(group) == "gloo"     # CPU rehearsal backend: stage through host
    if staged:
        send = send.cpu()
    recv = torch.empty((world, T, m_max, N, D), dtype=local.dtype, device=send.device)
    dist.all_gather_into_tensor(recv.view(world * T, m_max, N, D), send, group=group)   # rank r's shard = recv[r]
    if staged:
        recv = recv.to(local.device)
    out = torch.empty((T, total_members, N, D), dtype=local.dtype, device=local.device)
    if total_members == world * m_max:      # even shards: member m = j * world + r  ->  one strided copy
        out.view(T, m_max, world, N, D).copy_(recv.permute(1, 2, 0, 3, 4))
    else:                                   # rank r's members are r, r + world, ..: a strided slice each (no index tensors)
        for r in range(world):
            if counts[r]:
                out[:, r::world] = recv[r, :, :counts[r]]
    return out
