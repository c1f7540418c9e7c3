"""numpy restatement of csrc/rigid_rule.h for tests/test_augment_host.py and tests/test_gpu_augment.py (a helper module like
philox_ref.py: no fixtures, no settings).  Written from the rule in include/mdno_augment.h: the words are
`philox_ref.noise_words(..., purpose=2)`, everything after them is fp64 with one numpy operation per rounding, in the
header's order (numpy never fuses a multiply with an add)."""
import numpy as np

import philox_ref as P

TRAIN_MOTION = 2
FIRST_ELEMENT, LAST_ELEMENT = 2, 65
LANES = 64
f64 = np.float64


def ab(seed, sample_ids, epoch, n_elems=LAST_ELEMENT + 1):
    """a_e, b_e of elements 0 .. n_elems - 1: two fp64 arrays [B, n_elems]."""
    words = P.noise_words(seed, sample_ids, epoch, n_elems, TRAIN_MOTION)
    u1, u2 = P.uniform32(words[..., 0]), P.uniform32(words[..., 1])
    return f64(2.0) * u1.astype(f64) - f64(1.0), f64(2.0) * u2.astype(f64) - f64(1.0)


def centroid(frame, n_atoms):
    """frame f32 [B * N, 3] -> fp64 [B, 3] in the header's order: 64 partial sums of rows l, l + 64, .., ascending, onto
    0.0; folded with off = 32 .. 1; divided by N."""
    x = np.asarray(frame, dtype=np.float32).reshape(-1, n_atoms, 3).astype(f64)
    B = x.shape[0]
    part = np.zeros((B, LANES, 3), dtype=f64)
    for k in range(0, n_atoms, LANES):
        chunk = x[:, k:k + LANES]
        part[:, :chunk.shape[1]] = part[:, :chunk.shape[1]] + chunk
    off = LANES // 2
    while off:
        part[:, :off] = part[:, :off] + part[:, off:2 * off]
        off //= 2
    with np.errstate(invalid="ignore"):
        return part[:, 0] / f64(n_atoms)


def motions(seed, sample_ids, epoch, rotate=True, translate=0.0, last_element=LAST_ELEMENT, first_frame=None, n_atoms=None):
    """-> dict(quaternion f64 [B,4], pivot f64 [B,3], shift f64 [B,3], attempts i32 [B,2]).  first_frame None: c = 0."""
    ids = np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    B = ids.size
    a, b = ab(seed, ids, epoch, last_element + 1 if rotate else 2)
    T = f64(translate)
    shift = np.stack([T * a[:, 0], T * b[:, 0], T * a[:, 1]], axis=1)
    q = np.zeros((B, 4), dtype=f64)
    q[:, 0] = 1.0
    attempts = np.full((B, 2), -1, dtype=np.int32)
    if rotate:
        s = a * a + b * b
        for i in range(B):
            acc = [e for e in range(FIRST_ELEMENT, last_element + 1) if s[i, e] < 1.0][:2]
            attempts[i, :len(acc)] = acc
            if len(acc) == 2:
                A, Bq = acc
                f = np.sqrt((f64(1.0) - s[i, A]) / s[i, Bq])
                q[i] = (a[i, A], b[i, A], a[i, Bq] * f, b[i, Bq] * f)
    pivot = np.zeros((B, 3), dtype=f64) if first_frame is None else centroid(first_frame, n_atoms)
    return dict(quaternion=q, pivot=pivot, shift=shift, attempts=attempts)


def matrices(q):
    """fp64 [B, 3, 3] from q [B, 4] = (w, x, y, z), the nine entries as the header writes them."""
    q = np.asarray(q, dtype=f64)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    n = ((w * w + x * x) + y * y) + z * z
    g = f64(2.0) / n
    R = np.empty((q.shape[0], 3, 3), dtype=f64)
    R[:, 0, 0] = f64(1.0) - g * (y * y + z * z)
    R[:, 0, 1] = g * (x * y - w * z)
    R[:, 0, 2] = g * (x * z + w * y)
    R[:, 1, 0] = g * (x * y + w * z)
    R[:, 1, 1] = f64(1.0) - g * (x * x + z * z)
    R[:, 1, 2] = g * (y * z - w * x)
    R[:, 2, 0] = g * (x * z - w * y)
    R[:, 2, 1] = g * (y * z + w * x)
    R[:, 2, 2] = f64(1.0) - g * (x * x + y * y)
    return R


def apply(m, x, n_atoms, inverse=False):
    """x f32 [..., B * N, 3] -> the moved rows, f32, same shape; m = motions(...)."""
    x = np.asarray(x, dtype=np.float32)
    B = m["quaternion"].shape[0]
    p = x.reshape(-1, B, n_atoms, 3).astype(f64)
    R = matrices(m["quaternion"])[None, :, None]                  # [1, B, 1, 3, 3]
    c = m["pivot"][None, :, None, :]
    ct = (m["pivot"] + m["shift"])[None, :, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        if not inverse:
            d = p - c
            r = np.stack([(R[..., a, 0] * d[..., 0] + R[..., a, 1] * d[..., 1]) + R[..., a, 2] * d[..., 2] for a in range(3)], -1)
            out = (ct + r).astype(np.float32)
        else:
            d = p - ct
            r = np.stack([(R[..., 0, a] * d[..., 0] + R[..., 1, a] * d[..., 1]) + R[..., 2, a] * d[..., 2] for a in range(3)], -1)
            out = (c + r).astype(np.float32)
    return out.reshape(x.shape)
