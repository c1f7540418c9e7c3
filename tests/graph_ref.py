"""The pair rule of csrc/graph.hip restated in numpy fp64 WITHOUT the dense N x N matrix (a helper module like
observe_ref.py and philox_ref.py: no fixtures, no settings, no device code), so that it reaches the sizes at which the
cell list and its second atom window run.

Open rule, for f32 coordinates: d = x_j - x_i in fp64, s = (dx * dx + dy * dy) + dz * dz (every operation a separate
array operation: nothing is contracted), edge iff sqrt(s) < cutoff, strictly.  scipy's cKDTree only proposes pairs, at
radius cutoff * (1 + 1e-6): a superset, so the tree's own arithmetic never decides an edge.  The diagonal is tested by
the same formula (it holds for a finite atom when cutoff > 0 and never for a non-finite one); atoms with a non-finite
coordinate never enter the tree and are in no pair.

`margin` = the smallest | dist - cutoff | / cutoff over the proposed pairs: an exact comparison with a kernel needs
inputs on which the last bit of a square root could not change the answer (`check_condition`: margin >= 1e-9, as
tests/test_gpu_pbc.py has it).  Frames that put pairs AT the cutoff on purpose use exactly representable coordinates
and skip that assertion.  tests/test_graph_ref_host.py checks this module against scipy's dense distance matrix.

Periodic rule: the dense restatement of tests/test_gpu_pbc.py (`pbc_graph`, `pbc_graph_members`), imported."""
import warnings

import numpy as np

MARGIN = 1e-9
SUPERSET = 1.0e-6


def _pair_dist(p, i, j):
    """sqrt((dx^2 + dy^2) + dz^2) of d = p[j] - p[i], p f64 [N, 3]; NaN where a coordinate is not finite."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = p[j] - p[i]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        s = (dx * dx + dy * dy) + dz * dz
        return np.sqrt(s)


def radius_graph(pos, cutoff):
    """One member: pos f32 [N, 3] -> dict(row_ptr i32 [N + 1], src i32 [E], dst i32 [E], margin, candidates).
    Destinations ascending, sources ascending inside a row."""
    from scipy.spatial import cKDTree
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    N, cutoff = pos.shape[0], float(cutoff)
    p = pos.astype(np.float64)
    finite = np.nonzero(np.isfinite(p).all(axis=1))[0]
    cand = np.zeros((0, 2), dtype=np.int64)
    if finite.size > 1:
        cand = finite[cKDTree(p[finite]).query_pairs(cutoff * (1.0 + SUPERSET), output_type="ndarray").astype(np.int64)]
    dist = _pair_dist(p, cand[:, 0], cand[:, 1])
    keep = dist < cutoff
    a, b = cand[keep, 0], cand[keep, 1]
    every = np.arange(N, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        diag = every[_pair_dist(p, every, every) < cutoff]
    dst = np.concatenate([a, b, diag])                  # the test is symmetric: (-d)^2 == d^2 exactly
    src = np.concatenate([b, a, diag])
    order = np.lexsort((src, dst))
    dst, src = dst[order], src[order]
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=N))])
    margin = float("inf")
    if dist.size and cutoff > 0.0:                      # (cutoff 0: sqrt(s) < 0 holds for no s, whatever its last bit)
        margin = float(np.abs(dist - cutoff).min() / cutoff)
    return dict(row_ptr=row_ptr.astype(np.int32), src=src.astype(np.int32), dst=dst.astype(np.int32), margin=margin,
                candidates=int(dist.size), cutoff=cutoff)


def radius_graph_members(pos, n_atoms, cutoff):
    """pos f32 [M * N, 3] (or [M, N, 3]): the block-diagonal graph of M members, global row numbers; margin = the
    smallest of the members'."""
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    assert n_atoms > 0 and pos.shape[0] % n_atoms == 0
    parts = [radius_graph(pos[o:o + n_atoms], cutoff) for o in range(0, pos.shape[0], n_atoms)]
    row_ptr, off = [np.zeros(1, np.int32)], 0
    for g in parts:
        row_ptr.append(g["row_ptr"][1:] + np.int32(off))
        off += g["src"].size
    return dict(row_ptr=np.concatenate(row_ptr),
                src=np.concatenate([g["src"] + np.int32(m * n_atoms) for m, g in enumerate(parts)]),
                dst=np.concatenate([g["dst"] + np.int32(m * n_atoms) for m, g in enumerate(parts)]),
                margin=min(g["margin"] for g in parts), candidates=sum(g["candidates"] for g in parts),
                cutoff=float(cutoff))


def check_condition(g):
    """The input condition of an exact comparison on random coordinates.  A condition on the inputs, not a measurement."""
    assert g["margin"] >= MARGIN, f"a pair lies within {MARGIN} (relative) of the cutoff ({g['margin']}): pick another seed"


def to_coo(g):
    """[rows; cols] i64 [2, E] in the order of oracle.graph_kernel_oracle.radius_graph_coo."""
    return np.stack([g["dst"], g["src"]]).astype(np.int64)


def rows_in_both_windows(g, split):
    """Number of rows with a source below `split` and a source at or above it (a row whose sources the cell list reads
    out of two passes over its atom mask), and the number of edges whose ends lie on different sides."""
    n = g["row_ptr"].size - 1
    lo = np.bincount(g["dst"][g["src"] < split], minlength=n) > 0
    hi = np.bincount(g["dst"][g["src"] >= split], minlength=n) > 0
    crossing = int(((g["src"] < split) != (g["dst"] < split)).sum())
    return int((lo & hi).sum()), crossing


def two_window_frame():
    """N = 65,728 atoms (one member, cutoff 4.0): more than the 65,536 atoms one pass over the cell list's mask holds.
    Uniform in a 113.5 A cube; the last 192 atoms sit 0.5 A (per axis) from atoms 65,344 .. 65,535, so that thousands of
    rows have sources on both sides of the window edge."""
    rng = np.random.default_rng(7)
    pos = (rng.random((65728, 3)) * 113.5).astype(np.float32)
    pos[65536:] = pos[65344:65536] + np.float32(0.5)
    return pos


def with_nonfinite(pos, seed=0):
    """A copy of pos f32 [N, 3] (N >= 12) in which 5 atoms have NaN in one coordinate, 3 have +Inf and 2 have -Inf
    (atom 0 is a NaN atom and atom N - 1 a -Inf one), and the indices of the ten."""
    pos = np.array(pos, dtype=np.float32).reshape(-1, 3)
    N = pos.shape[0]
    rng = np.random.default_rng(seed)
    bad = np.concatenate([[0], 1 + rng.permutation(N - 2)[:8], [N - 1]])
    pos[bad, rng.integers(0, 3, size=10)] = np.array([np.nan] * 5 + [np.inf] * 3 + [-np.inf] * 2, dtype=np.float32)
    return pos, np.sort(bad)


def with_copies(pos, seed=0):
    """A copy of pos f32 [N, 3] (N >= 20) in which 10 atoms are bitwise copies of 10 others (distance exactly 0), and
    the (copy, original) index pairs."""
    pos = np.array(pos, dtype=np.float32).reshape(-1, 3)
    pick = np.random.default_rng(seed).permutation(pos.shape[0])[:20]
    pos[pick[:10]] = pos[pick[10:]]
    return pos, np.stack([pick[:10], pick[10:]], axis=1)


TWO_WINDOW_CUTOFF = 4.0
TWO_WINDOW_EDGES = 829220
_two_window = []


def two_window_reference():
    """(frame, its graph): built once per process and shared — treat both as read-only."""
    if not _two_window:
        pos = two_window_frame()
        _two_window.append((pos, radius_graph(pos, TWO_WINDOW_CUTOFF)))
    return _two_window[0]


# ---------------------------------------------------------------------------------------------------- periodic rule
def pbc_graph_members(pos, n_atoms, cutoff, box):
    """tests/test_gpu_pbc.py's dense restatement (its input condition asserted per member)."""
    from test_gpu_pbc import pbc_graph_members as members
    return members(np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3), n_atoms, cutoff, box)


def pbc_graph_degenerate(pos, cutoff, box):
    """One member that may hold non-finite atoms, coincident atoms or cutoff 0: the same dense restatement with numpy's
    warnings silenced (a NaN distance is below no cutoff); its input condition is asserted on the finite atoms alone,
    and only where a last bit could matter (cutoff > 0)."""
    from test_gpu_pbc import check_condition as pbc_condition, pbc_graph
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g = pbc_graph(pos, cutoff, box)
    if cutoff > 0.0:
        finite = np.isfinite(pos).all(axis=1)
        pbc_condition(pbc_graph(pos[finite], cutoff, box))
    return g
