// The one definition of a sample's random rigid motion (include/mdno_augment.h repeats it in words; csrc/augment.hip
// runs it; tests/rigid_ref.py restates it in numpy and tests/test_augment_host.py compiles this file for the host).
// Plain C++, callable on the device and on the host like philox.h.  fp64 on fp32 inputs, + - x / sqrt only, every
// operation rounded on its own (the library is built with -ffp-contract=off, and so must any other user be), so the
// device, the host and numpy agree in every bit.
//
// One motion per (seed, sample index in its dataset, epoch) and nothing else: noise_block of philox.h with
// stream = sample, index = epoch, purpose NOISE_TRAIN_MOTION.  Element e gives the fp32 uniforms u1_e, u2_e (word e & 3
// of block e >> 2, second = 0 and 1) and from them
//     a_e = 2 (double)u1_e - 1,   b_e = 2 (double)u2_e - 1        exact, in (-1, 1], never 0
//   translation  t = T * (a_0, b_0, a_1)                          (b_1 is not used; T = 0 gives zeros)
//   rotation     Marsaglia (1972), a uniform point on S^3: for e = 2, 3, .., last_element ascending,
//                s_e = a_e a_e + b_e b_e (exact), element e ACCEPTED when s_e < 1; A = the first accepted element,
//                B = the second;  f = sqrt((1 - s_A) / s_B),  q = (w, x, y, z) = (a_A, b_A, a_B f, b_B f).
//                Fewer than two accepted: q = (1, 0, 0, 0) and attempts = (A or -1, -1).
//   matrix       n = ((w w + x x) + y y) + z z,  g = 2 / n, the standard matrix of a quaternion with g in place of 2
//                (rigid_matrix below writes the nine entries out): a proper rotation for any q != 0.
//   pivot        c = the centroid of the sample's first window frame (rigid_centroid: fp64 sum of the fp32
//                coordinates in an order fixed by N alone, divided by N), or 0.
//   apply        d = (double)p - c,  r_a = (R_a0 d_0 + R_a1 d_1) + R_a2 d_2,  p'_a = (float)((c_a + t_a) + r_a)
//   inverse      d' = (double)p' - (c + t),  p_a = (float)(c_a + ((R_0a d'_0 + R_1a d'_1) + R_2a d'_2))
#pragma once
#include <stddef.h>

#include "philox.h"

#if defined(__HIPCC__)
#define MDNO_HD __host__ __device__ inline
#else
#define MDNO_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mdno {

constexpr int kRigidFirstElement = 2;       // elements 0 and 1 make the translation
constexpr int kRigidLastElement = 65;       // 64 candidates: fewer than two accepted has probability ~ 1e-41
constexpr int kRigidCentroidLanes = 64;     // the centroid's partial sums (rigid_centroid)

// (a_e, b_e) of elements 4 * block .. 4 * block + 3
MDNO_HD void rigid_block(unsigned long long seed, uint32_t sample, long long epoch, uint32_t block, double a[4], double b[4]) {
    uint32_t w1[4], w2[4];
    noise_block(seed, sample, epoch, block, NOISE_TRAIN_MOTION, 0, w1);
    noise_block(seed, sample, epoch, block, NOISE_TRAIN_MOTION, 1, w2);
    for (int j = 0; j < 4; ++j) {
        a[j] = 2.0 * (double)noise_uniform(w1[j]) - 1.0;
        b[j] = 2.0 * (double)noise_uniform(w2[j]) - 1.0;
    }
}

MDNO_HD void rigid_shift(unsigned long long seed, uint32_t sample, long long epoch, double T, double t[3]) {
    double a[4], b[4];
    rigid_block(seed, sample, epoch, 0, a, b);
    t[0] = T * a[0];
    t[1] = T * b[0];
    t[2] = T * a[1];
}

// q and the two accepted elements (or -1); last_element in [kRigidFirstElement, kRigidLastElement]
MDNO_HD void rigid_quaternion(unsigned long long seed, uint32_t sample, long long epoch, int last_element, double q[4],
                              int attempts[2]) {
    double a[4], b[4], aA = 0.0, bA = 0.0, sA = 0.0;
    attempts[0] = attempts[1] = -1;
    q[0] = 1.0;
    q[1] = q[2] = q[3] = 0.0;
    for (int e = kRigidFirstElement; e <= last_element; ++e) {
        if (e == kRigidFirstElement || (e & 3) == 0) rigid_block(seed, sample, epoch, (uint32_t)(e >> 2), a, b);
        const double ae = a[e & 3], be = b[e & 3];
        const double s = ae * ae + be * be;
        if (!(s < 1.0)) continue;
        if (attempts[0] < 0) {
            attempts[0] = e;
            aA = ae; bA = be; sA = s;
        } else {
            attempts[1] = e;
            const double f = sqrt((1.0 - sA) / s);
            q[0] = aA;
            q[1] = bA;
            q[2] = ae * f;
            q[3] = be * f;
            return;
        }
    }
}

// R[3 * a + b] = R_ab
MDNO_HD void rigid_matrix(const double q[4], double R[9]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double n = ((w * w + x * x) + y * y) + z * z;
    const double g = 2.0 / n;
    R[0] = 1.0 - g * (y * y + z * z);
    R[1] = g * (x * y - w * z);
    R[2] = g * (x * z + w * y);
    R[3] = g * (x * y + w * z);
    R[4] = 1.0 - g * (x * x + z * z);
    R[5] = g * (y * z - w * x);
    R[6] = g * (x * z - w * y);
    R[7] = g * (y * z + w * x);
    R[8] = 1.0 - g * (x * x + y * y);
}

// ct = c + t, formed once per sample (rigid_pivot_shift) and used by both directions
MDNO_HD void rigid_pivot_shift(const double c[3], const double t[3], double ct[3]) {
    for (int a = 0; a < 3; ++a) ct[a] = c[a] + t[a];
}

MDNO_HD void rigid_apply_row(const double R[9], const double c[3], const double ct[3], const float p[3], float out[3]) {
    const double d0 = (double)p[0] - c[0], d1 = (double)p[1] - c[1], d2 = (double)p[2] - c[2];
    for (int a = 0; a < 3; ++a) {
        const double r = (R[3 * a] * d0 + R[3 * a + 1] * d1) + R[3 * a + 2] * d2;
        out[a] = (float)(ct[a] + r);
    }
}

MDNO_HD void rigid_invert_row(const double R[9], const double c[3], const double ct[3], const float p[3], float out[3]) {
    const double d0 = (double)p[0] - ct[0], d1 = (double)p[1] - ct[1], d2 = (double)p[2] - ct[2];
    for (int a = 0; a < 3; ++a) {
        const double r = (R[a] * d0 + R[3 + a] * d1) + R[6 + a] * d2;
        out[a] = (float)(c[a] + r);
    }
}

// The centroid's summation order, fixed by N alone: partial l (0 <= l < 64) adds rows l, l + 64, l + 128, .. in
// ascending order onto 0.0; then for off = 32, 16, 8, 4, 2, 1: partial l += partial l + off (l < off); c = partial 0 / N.
// (The device gives one lane a partial and folds with shuffles; this is the same order written serially.)
MDNO_HD void rigid_centroid(const float* x, int N, double c[3]) {
    for (int k = 0; k < 3; ++k) {
        double part[kRigidCentroidLanes];
        for (int l = 0; l < kRigidCentroidLanes; ++l) {
            double s = 0.0;
            for (int r = l; r < N; r += kRigidCentroidLanes) s = s + (double)x[3 * (size_t)r + k];
            part[l] = s;
        }
        for (int off = kRigidCentroidLanes / 2; off > 0; off >>= 1)
            for (int l = 0; l < off; ++l) part[l] = part[l] + part[l + off];
        c[k] = part[0] / (double)N;
    }
}

}  // namespace mdno

#undef MDNO_HD
