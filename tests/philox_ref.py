"""numpy restatement of csrc/philox.h for tests/test_noise_host.py and tests/test_gpu_noise.py (a helper module like
bf16_replica.py: no fixtures, no settings).  Written from the definition: Philox4x32-10 of Salmon et al. (SC'11) — ten
rounds of  (c0, c1, c2, c3) <- (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)),  the key bumped by the
Weyl constants after every round — and the library's counter layout and normal transform."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
ROLLOUT, TRAIN_WINDOW = 0, 1


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (broadcastable), any integer type holding 32-bit values -> uint32 [..., 4]."""
    ctr = np.asarray(ctr).astype(np.uint64) & MASK
    key = np.asarray(key).astype(np.uint64) & MASK
    c0, c1, c2, c3 = (ctr[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                  # 32 x 32 -> 64 bit products: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def noise_words(seed, stream_ids, index, n_elems, purpose):
    """The two Philox words of every element: uint32 [M, n_elems, 2] ([..., 0] makes u1, [..., 1] u2)."""
    seed, index = int(seed), int(index)
    assert 0 <= seed < 2 ** 64 and 0 <= index < 2 ** 48 and 0 <= purpose < 256
    sid = np.asarray(stream_ids, dtype=np.int64).reshape(-1, 1) & 0xFFFFFFFF
    el = np.arange(n_elems, dtype=np.int64).reshape(1, -1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    out = np.empty((sid.shape[0], n_elems, 2), dtype=np.uint32)
    for second in (0, 1):
        word3 = purpose | (second << 8) | ((index >> 32) << 16)
        ctr = np.stack(np.broadcast_arrays(sid, np.int64(index & 0xFFFFFFFF), el >> 2, np.int64(word3)), axis=-1)
        blocks = philox4x32_10(ctr, key)
        out[..., second] = np.take_along_axis(blocks, np.broadcast_to(el & 3, blocks.shape[:-1])[..., None], -1)[..., 0]
    return out


def uniform32(w):
    """u = ((w >> 8) + 0.5f) * 2^-24 as the definition has it: an fp32 quantity (the sum rounds to even from 2^23 on)."""
    return (((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float32)


def normals(words):
    """z in fp64 from the fp32 inputs of the definition (u1, u2 and the angle 6.2831853f * u2 are fp32 quantities; the
    logarithm, root and cosine are taken in double)."""
    u1, u2 = uniform32(words[..., 0]), uniform32(words[..., 1])
    angle = (np.float32(6.2831853) * u2).astype(np.float32)
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(angle.astype(np.float64))
