"""numpy restatement of include/mdno_internal_grad.h on top of internal_ref.py's bond / dot / cross: the same fp64
operations in the same order (elementwise + - * / sqrt rint on np.float64 arrays), so the device result can be held to it
bit for bit.  Arrays run over the frames; the atoms and their incidences are walked one by one, in the table's order."""
import numpy as np

import internal_ref as ref

WIDTH = (2, 3, 4)


def incidence(pairs=(), triples=(), quads=(), n_atoms=0):
    """(atom_ptr [n_atoms + 1], inc [n_inc]) as int64 arrays: per atom the codes item * 4 + slot of the tuples that name it,
    ascending; items count pairs, then triples, then quads; an atom outside 0 .. n_atoms - 1 has no entry."""
    rows = [[] for _ in range(n_atoms)]
    item = 0
    for tuples in (pairs, triples, quads):
        for tup in tuples:
            for slot, a in enumerate(tup):
                if 0 <= int(a) < n_atoms:
                    rows[int(a)].append(4 * item + slot)
            item += 1
    ptr = np.zeros(n_atoms + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows]) if n_atoms else 0
    return ptr, np.array([c for r in rows for c in r], np.int64)


def _bond(x, a, b, L, inv, real):
    """internal_ref.bond; in another real type (np.longdouble: the yardstick of the host test) the same expression in it."""
    if real is np.float64:
        return ref.bond(x, a, b, L, inv)
    v = []
    for c in range(3):
        d = x[:, b, c].astype(real) - x[:, a, c].astype(real)
        if L[c] > 0.0:
            d = d - np.rint(d * real(inv[c])) * real(L[c])
        v.append(d)
    return v


def _item(x, g, kind, t, tup, P, A, L, inv, real=np.float64):
    """The contributions of one item to the atoms of its tuple: ([per slot: three f64 [F] arrays], skipped bool [F])."""
    bond = lambda x, a, b, L, inv: _bond(x, a, b, L, inv, real)
    if kind == 0:
        i, j = tup
        gg = g[:, t].astype(real)
        v = bond(x, i, j, L, inv)
        r = np.sqrt(ref.dot(v, v))
        s = gg / r
        tc = [s * v[c] for c in range(3)]
        return [[-tc[c] for c in range(3)], tc], (gg == 0.0) | (r == 0.0)
    if kind == 1:
        i, j, k = tup
        gg = g[:, P + t].astype(real)
        u, w = bond(x, j, i, L, inv), bond(x, j, k, L, inv)
        uu, ww = ref.dot(u, u), ref.dot(w, w)
        den = np.sqrt(uu) * np.sqrt(ww)
        cs = ref.dot(u, w) / den
        di = [(w[c] / den) - ((cs * u[c]) / uu) for c in range(3)]
        dk = [(u[c] / den) - ((cs * w[c]) / ww) for c in range(3)]
        return [[gg * di[c] for c in range(3)], [-(gg * (di[c] + dk[c])) for c in range(3)], [gg * dk[c] for c in range(3)]], gg == 0.0
    i, j, k, l = tup
    col = P + A + 2 * t
    gc, gs = g[:, col].astype(real), g[:, col + 1].astype(real)
    b1, b2, b3 = bond(x, i, j, L, inv), bond(x, j, k, L, inv), bond(x, k, l, L, inv)
    n1, n2 = ref.cross(b1, b2), ref.cross(b2, b3)
    bb = ref.dot(b2, b2)
    lb = np.sqrt(bb)
    xx = ref.dot(n1, n2)
    yy = lb * ref.dot(b1, n2)
    h = np.sqrt(xx * xx + yy * yy)
    gphi = gs * (xx / h) - gc * (yy / h)
    ki, kl = lb / ref.dot(n1, n1), lb / ref.dot(n2, n2)
    p, q = ref.dot(b1, b2) / bb, ref.dot(b3, b2) / bb
    fi = [-(ki * n1[c]) for c in range(3)]
    fl = [kl * n2[c] for c in range(3)]
    fj = [(-fi[c] - p * fi[c]) + q * fl[c] for c in range(3)]
    fk = [(-fl[c] + p * fi[c]) - q * fl[c] for c in range(3)]
    return [[gphi * f[c] for c in range(3)] for f in (fi, fj, fk, fl)], (gc == 0.0) & (gs == 0.0)


def features_bwd(frames, g, pairs=(), triples=(), quads=(), box=None, table=None, real=np.float64):
    """frames f32 [F, N, 3], g [F, P + A + 2 T] (f32 or f64) -> (grad f64 [F, N, 3], S_abs f64 [F, N, 3]): per (frame, atom)
    the chain acc = acc + contribution from +0.0 over the atom's incidences in the table's order, and the sum of the absolute
    contributions.  `table` = (atom_ptr, inc): None builds the right one; a given one is walked as the kernel walks it (the
    range clamped into [0, n_inc], an entry skipped if its item or slot is out of range or its tuple's slot names another
    atom).  `real`: the type the arithmetic runs in (np.longdouble for a yardstick; the rule is np.float64)."""
    x = np.asarray(frames, np.float32)
    g = np.asarray(g)
    F, N = x.shape[0], x.shape[1]
    lists = [[tuple(int(v) for v in t) for t in tuples] for tuples in (pairs, triples, quads)]
    P, A, T = (len(l) for l in lists)
    assert g.shape == (F, P + A + 2 * T) and g.dtype in (np.float32, np.float64)
    L, inv = ref._box(box)
    ptr, inc = incidence(*lists, n_atoms=N) if table is None else (np.asarray(table[0], np.int64), np.asarray(table[1], np.int64))
    n_inc = len(inc)
    grad = np.zeros((F, N, 3), real)
    s_abs = np.zeros((F, N, 3), real)
    done = {}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for a in range(N):
            lo, hi = (min(max(int(v), 0), n_inc) for v in (ptr[a], ptr[a + 1]))
            for e in range(lo, hi):
                code = int(inc[e])
                it, slot = code >> 2, code & 3
                if code < 0 or it >= P + A + T:
                    continue
                kind, t = (0, it) if it < P else ((1, it - P) if it < P + A else (2, it - P - A))
                tup = lists[kind][t]
                if slot >= WIDTH[kind] or tup[slot] != a or not ref._ok(tup, N):
                    continue
                if it not in done:
                    done[it] = _item(x, g, kind, t, tup, P, A, L, inv, real)
                contrib, skipped = done[it]
                for c in range(3):
                    grad[:, a, c] = np.where(skipped, grad[:, a, c], grad[:, a, c] + contrib[slot][c])
                    s_abs[:, a, c] = np.where(skipped, s_abs[:, a, c], s_abs[:, a, c] + np.abs(contrib[slot][c]))
    return grad, s_abs
