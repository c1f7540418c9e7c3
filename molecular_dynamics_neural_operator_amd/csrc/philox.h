// The one definition of the library's random numbers: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random
// numbers: as easy as 1, 2, 3", SC'11) as a counter-based generator, and the standard normal made from it.  Plain
// C++, callable on the device and on the host (the host build is what tests/test_noise_host.py compiles).
//
// A value depends only on what it is FOR, never on where, when or beside what it is drawn:
//     key      (seed_lo, seed_hi)                                 the 64-bit seed
//     counter  (stream_id, index_lo, element >> 2, purpose_word)
//       stream_id     global ensemble member (rollout) or the sample's index in its dataset (training)
//       index         absolute step number (rollout) or epoch (training), 0 <= index < 2^48
//       element       atom * 3 + component (rollout), (frame_in_window * N + atom) * 3 + component (training window),
//                     the draw's number (a training sample's rigid motion: rigid_rule.h)
//       purpose_word  purpose | second << 8 | index_hi << 16: purpose NOISE_ROLLOUT / NOISE_TRAIN_WINDOW / NOISE_TRAIN_MOTION (< 256),
//                     second = 0 for the block u1 is taken from and 1 for u2's, index_hi = index >> 32 (0 for every
//                     index below 2^32, so the word is then just purpose, or purpose | 0x100)
//     the element uses word (element & 3) of both blocks:
//       u = ((w >> 8) + 0.5f) * 2^-24  in (0, 1],    z = sqrtf(-2 logf(u1)) * cosf(6.2831853f * u2)
// One normal per element (Box-Muller's cosine branch only): 3 N values per member and step, simplicity over throughput.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MDNO_HD __host__ __device__ inline
#else
#include <math.h>
#define MDNO_HD inline
#endif

namespace mdno {

enum NoisePurpose { NOISE_ROLLOUT = 0, NOISE_TRAIN_WINDOW = 1, NOISE_TRAIN_MOTION = 2 };
constexpr long long kNoiseMaxIndex = 1ll << 48;

MDNO_HD uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

// ctr[0..4) -> ten rounds under key (k0, k1), in place
MDNO_HD void philox4x32_10(uint32_t ctr[4], uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = philox_mulhi(M0, ctr[0]), lo0 = M0 * ctr[0];
        const uint32_t hi1 = philox_mulhi(M1, ctr[2]), lo1 = M1 * ctr[2];
        const uint32_t n0 = hi1 ^ ctr[1] ^ k0, n2 = hi0 ^ ctr[3] ^ k1;
        ctr[0] = n0; ctr[1] = lo1; ctr[2] = n2; ctr[3] = lo0;
        k0 += W0;
        k1 += W1;
    }
}

MDNO_HD uint32_t noise_purpose_word(int purpose, long long index, int second) {
    return (uint32_t)purpose | ((uint32_t)second << 8) | ((uint32_t)((unsigned long long)index >> 32) << 16);
}

// the block of elements 4 * block .. 4 * block + 3 (second = 0: u1's words, 1: u2's)
MDNO_HD void noise_block(unsigned long long seed, uint32_t stream_id, long long index, uint32_t block, int purpose,
                         int second, uint32_t w[4]) {
    w[0] = stream_id;
    w[1] = (uint32_t)(unsigned long long)index;
    w[2] = block;
    w[3] = noise_purpose_word(purpose, index, second);
    philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
}

MDNO_HD float noise_uniform(uint32_t w) { return ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-8f; }      // 2^-24

MDNO_HD float noise_normal(uint32_t w1, uint32_t w2) {
    return sqrtf(-2.0f * logf(noise_uniform(w1))) * cosf(6.2831853f * noise_uniform(w2));
}

}  // namespace mdno

#undef MDNO_HD
