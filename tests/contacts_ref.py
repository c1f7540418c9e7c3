"""The rule of include/mdno_contacts.h restated in numpy fp64, operation for operation (a helper module like observe_ref.py:
no fixtures, no settings).  The pair distance is observe_ref.pair_distances (the same differences, np.rint for the minimum
image, the same parenthesisation, np.sqrt); the sums over a block are one `acc = acc + r` per step in ascending step order,
starting from 0.0; the contact series are plain bool arrays and `origins` / `both` are counted from them.  numpy evaluates
every ufunc on its own, so nothing is contracted into an FMA.  tests/test_contacts_host.py checks this file against brute-force
loops; tests/test_gpu_contacts.py holds the kernels to it exactly."""
import numpy as np

from observe_ref import pair_distances


def frame_distances(frames, box=None):
    """r f64 [S, M, N, N] for frames f32 [S, M, N, 3]."""
    frames = np.asarray(frames, dtype=np.float32)
    S, M, N = frames.shape[:3]
    r = np.empty((S, M, N, N), np.float64)
    for s in range(S):
        for m in range(M):
            r[s, m] = pair_distances(frames[s, m], box)
    return r


def frame_squares(frames, box=None):
    """s f64 [S, M, N, N]: what frame_distances takes the root of."""
    frames = np.asarray(frames, dtype=np.float32)
    S, M, N = frames.shape[:3]
    sq = np.empty((S, M, N, N), np.float64)
    for s in range(S):
        for m in range(M):
            sq[s, m] = squared(frames[s, m], box)
    return sq


def block_statistics(r, sq, threshold, block_len):
    """(count i32, sum_r f64, sum_r2 f64), each [Bk, M, N, N], and n_frames i64 [Bk] from r, sq [S, M, N, N]: per block one
    chain acc = acc + r (acc = acc + s) in ascending step order, starting from 0.0."""
    S, M, N = r.shape[:3]
    Bk = -(-S // block_len)
    count = np.zeros((Bk, M, N, N), np.int32)
    sum_r = np.zeros((Bk, M, N, N), np.float64)
    sum_r2 = np.zeros((Bk, M, N, N), np.float64)
    n_frames = np.zeros(Bk, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):                                   # ascending: the order of the chains
            b = s // block_len
            n_frames[b] += 1
            count[b] += (r[s] < threshold).astype(np.int32)
            sum_r[b] = sum_r[b] + r[s]
            sum_r2[b] = sum_r2[b] + sq[s]
    return count, sum_r, sum_r2, n_frames


def pair_statistics(frames, threshold, box=None, block_len=64):
    """block_statistics of frames f32 [S, M, N, 3]."""
    return block_statistics(frame_distances(frames, box), frame_squares(frames, box), threshold, block_len)


def squared(x, box=None):
    """s f64 [N, N] of one frame: what pair_distances takes the root of, formed the same way."""
    x = np.ascontiguousarray(x, dtype=np.float32).astype(np.float64)
    sq = []
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[None, :, :] - x[:, None, :]
        for a in range(3):
            da = d[..., a]
            L = 0.0 if box is None else float(box[a])
            if L > 0.0:
                da = da - np.rint(da * (1.0 / L)) * L
            sq.append(da * da)
        return (sq[0] + sq[1]) + sq[2]


def total(blocks):
    """The blocks [Bk, ...] added in ascending order, one elementwise add each (PairStatistics.total)."""
    blocks = np.asarray(blocks)
    if blocks.shape[0] == 0:
        return np.zeros(blocks.shape[1:], blocks.dtype)
    acc = blocks[0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(1, blocks.shape[0]):
            acc = acc + blocks[b]
    return acc


def contact_series(frames, pairs, cut, cut_max, box=None):
    """c bool [M, P, S]: pair p of member m in contact at step s (r < cut[p] and r < cut_max; an index outside the frame:
    False)."""
    frames = np.asarray(frames, dtype=np.float32)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    cut = np.asarray(cut, dtype=np.float64)
    S, M, N = frames.shape[:3]
    P = pairs.shape[0]
    c = np.zeros((M, P, S), bool)
    ok = (pairs[:, 0] >= 0) & (pairs[:, 0] < N) & (pairs[:, 1] >= 0) & (pairs[:, 1] < N)
    i, j = np.where(ok, pairs[:, 0], 0), np.where(ok, pairs[:, 1], 0)
    with np.errstate(invalid="ignore"):
        for s in range(S):
            for m in range(M):
                if N == 0:
                    continue
                r = pair_distances(frames[s, m], box)[i, j]
                c[m, :, s] = ok & (r < cut) & (r < cut_max)
    return c


def pack_bits(c):
    """bool [M, P, S] -> the header's words as int64 [M, P, ceil(S / 64)] (bit s % 64 of word s / 64)."""
    M, P, S = c.shape
    Wd = -(-S // 64)
    padded = np.zeros((M, P, Wd * 64), np.uint64)
    padded[..., :S] = c
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (padded.reshape(M, P, Wd, 64) * weights).sum(-1, dtype=np.uint64).view(np.int64)


def per_frame(c):
    """i32 [S, M]: the listed pairs in contact per frame."""
    return c.sum(1).T.astype(np.int32)


def correlation(c, lags):
    """(origins, both) i32 [M, P, L] from the bool series."""
    M, P, S = c.shape
    origins = np.zeros((M, P, len(lags)), np.int32)
    both = np.zeros((M, P, len(lags)), np.int32)
    for l, lag in enumerate(lags):
        assert 0 <= lag < S
        head = c[..., :S - lag]
        origins[..., l] = head.sum(-1)
        both[..., l] = (head & c[..., lag:]).sum(-1)
    return origins, both
