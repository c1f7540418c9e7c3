"""include/mdno_constrain.h restated in numpy fp64 (a helper module like internal_ref.py: no fixtures, no settings), written
from the header's rule, not from the kernel: the greedy colouring, the coloured table, one constraint's arithmetic with
every product, sum, quotient and root rounded once in the header's order, the sweep over ascending colours and the per-frame
loop `measure; while sweeps < iterations and v > tol: sweep; measure`.  numpy evaluates each ufunc on its own, so nothing is
contracted into a fused multiply-add; sqrt and rint (round half to even) are IEEE operations."""
import numpy as np


def greedy_colours(pairs):
    """In list order, each constraint takes the lowest colour neither of its atoms has yet."""
    taken = {}
    out = []
    for i, j in np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist():
        busy = taken.setdefault(i, set()) | taken.setdefault(j, set())
        c = 0
        while c in busy:
            c += 1
        taken[i].add(c)
        taken[j].add(c)
        out.append(c)
    return np.array(out, dtype=np.int64)


def colour_table(pairs, lo, hi):
    """(pairs i32 [C, 2], lo f64 [C], hi f64 [C], colour_ptr i32 [n_colours + 1]) stably sorted by colour, and the order."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n_c = pairs.shape[0]
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), (n_c,)).copy()
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), (n_c,)).copy()
    col = greedy_colours(pairs)
    order = np.argsort(col, kind="stable")
    n_colours = int(col.max()) + 1 if n_c else 0
    ptr = np.zeros(n_colours + 1, dtype=np.int32)
    if n_c:
        ptr[1:] = np.cumsum(np.bincount(col, minlength=n_colours))
    return pairs[order].astype(np.int32), lo[order], hi[order], ptr, order


def evaluate(x, pairs, lo, hi, weights, box):
    """Every listed constraint on the fp64 state x [N, 3] at once: (active, i, j, r [C, 3], len, t, wi, wj).  Rows that are not
    active are skipped by the rule (their other columns mean nothing)."""
    n = x.shape[0]
    i, j = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    ok = (i >= 0) & (i < n) & (j >= 0) & (j < n)
    ii, jj = np.where(ok, i, 0), np.where(ok, j, 0)
    with np.errstate(all="ignore"):
        if n == 0:
            r = np.zeros((pairs.shape[0], 3))
        else:
            r = x[ii] - x[jj]
        if box is not None:
            for a in range(3):
                L = float(box[a])
                if L > 0.0:
                    inv = 1.0 / L
                    r[:, a] = r[:, a] - np.rint(r[:, a] * inv) * L
        length = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        t = np.where(length < lo, lo, np.where(length > hi, hi, length))
        if weights is None or n == 0:
            wi = wj = np.ones(pairs.shape[0])
        else:
            w = np.asarray(weights, dtype=np.float32).astype(np.float64)
            wi, wj = w[ii], w[jj]
        active = ok & np.isfinite(length) & (length != 0.0) & (t != length) & ((wi + wj) != 0.0)
    return active, ii, jj, r, length, t, wi, wj


def measure(x, pairs, lo, hi, weights, box):
    active, _, _, _, length, t, _, _ = evaluate(x, pairs, lo, hi, weights, box)
    if not active.any():
        return 0.0
    return float(np.max(np.abs(length[active] - t[active])))


def sweep(x, pairs, lo, hi, colour_ptr, weights, box):
    """One sweep, in place: the colours in ascending order; the constraints of a colour share no atom, so applying them
    together is applying them one by one."""
    for c in range(len(colour_ptr) - 1):
        s = slice(int(colour_ptr[c]), int(colour_ptr[c + 1]))
        active, i, j, r, length, t, wi, wj = evaluate(x, pairs[s], lo[s], hi[s], weights, box)
        if not active.any():
            continue
        i, j, r, length, t, wi, wj = i[active], j[active], r[active], length[active], t[active], wi[active], wj[active]
        assert len(set(i.tolist()) | set(j.tolist())) == 2 * i.size, "the colour table lies"
        g = ((length - t) / length) / (wi + wj)
        gi, gj = (wi * g)[:, None], (wj * g)[:, None]
        x[i] = x[i] - gi * r
        x[j] = x[j] + gj * r


def project(frames, pairs, lo, hi, colour_ptr, weights=None, box=None, iterations=8, tol=0.0):
    """frames f32 [F, N, 3] and a coloured table -> (out f32 [F, N, 3] rounded once, sweeps i32 [F], viol_in f64 [F],
    viol_out f64 [F], the fp64 states [F, N, 3])."""
    frames = np.asarray(frames, dtype=np.float32)
    lead = frames.shape[:-2]
    flat = frames.reshape((-1,) + frames.shape[-2:])
    n_f = flat.shape[0]
    state = flat.astype(np.float64)
    sweeps = np.zeros(n_f, dtype=np.int32)
    vin, vout = np.zeros(n_f), np.zeros(n_f)
    for f in range(n_f):
        x = state[f]
        v = measure(x, pairs, lo, hi, weights, box)
        vin[f] = v
        while sweeps[f] < iterations and v > tol:
            sweep(x, pairs, lo, hi, colour_ptr, weights, box)
            sweeps[f] += 1
            v = measure(x, pairs, lo, hi, weights, box)
        vout[f] = v
    with np.errstate(all="ignore"):
        out = state.astype(np.float32)
    return out.reshape(frames.shape), sweeps.reshape(lead), vin.reshape(lead), vout.reshape(lead), state.reshape(frames.shape)


def chain_pairs(n, second=True):
    """(i, i + 1) for the chain, then (i, i + 2)."""
    idx = np.arange(n, dtype=np.int64)
    p = np.stack([idx[:-1], idx[1:]], 1) if n > 1 else np.zeros((0, 2), dtype=np.int64)
    if second and n > 2:
        p = np.concatenate([p, np.stack([idx[:-2], idx[2:]], 1)])
    return p


def random_walk_chain(n, bond=3.8, seed=0):
    """A random-walk chain with bonds of `bond`: f64 [n, 3] (the generator is returned for further draws)."""
    rng = np.random.default_rng(seed)
    steps = rng.normal(size=(n - 1, 3)) if n > 1 else np.zeros((0, 3))
    steps = steps / np.linalg.norm(steps, axis=1, keepdims=True) * bond
    return np.concatenate([np.zeros((1, 3)), np.cumsum(steps, 0)]), rng


def lengths(x, pairs):
    d = x[pairs[:, 0]] - x[pairs[:, 1]]
    return np.sqrt((d * d).sum(1))
