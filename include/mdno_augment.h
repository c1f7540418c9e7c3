/*
 * mdno_augment.h — public header of libmdno.so: random rigid motions of training samples on the device
 * (csrc/rigid_rule.h, csrc/augment.hip).  Additive: every other header and both ABI version numbers stay
 * as they are.  Conventions as in mdno.h: device pointers owned by the caller, explicit sizes, `stream` a hipStream_t
 * passed as void*, 0 or a negative MDNO_E* code (mdno_last_error() has the message); arguments are checked on the host
 * before any device work.  No atomics anywhere: two calls give the same bits.
 *
 * THE RULE (csrc/rigid_rule.h is its one definition in code, tests/rigid_ref.py its numpy restatement; fp64 on fp32
 * inputs, + - x / sqrt only, every operation rounded on its own, no fused multiply-add):
 *
 *   generator    One motion per (seed, sample index in its dataset, epoch); it depends on nothing else — not the batch,
 *                its size, the rank, the launch or what is drawn beside it.  The generator is mdno_noise.h's: stream =
 *                sample index, index = epoch (0 <= epoch < 2^48), purpose MDNO_NOISE_TRAIN_MOTION.  Element e gives the
 *                fp32 uniforms u1_e, u2_e (word e & 3 of block e >> 2, second = 0 and 1), and
 *                    a_e = 2 (double)u1_e - 1,  b_e = 2 (double)u2_e - 1:  exact, in (-1, 1], never 0.
 *   translation  t = T * (a_0, b_0, a_1), T = `translate` in Angstrom; T = 0 gives zeros; b_1 is not used.
 *   rotation     Marsaglia's (1972) uniform point on S^3.  For e = 2, 3, .., last_element ascending (default 65),
 *                s_e = a_e a_e + b_e b_e (exact in fp64); element e is accepted when s_e < 1.  With A the first and B
 *                the second accepted element:  f = sqrt((1 - s_A) / s_B),  q = (w, x, y, z) = (a_A, b_A, a_B f, b_B f).
 *                Fewer than two accepted: q = (1, 0, 0, 0), and the sample's `attempts` holds -1 for what is missing.
 *                rotate = 0: q = (1, 0, 0, 0), no element from 2 on is drawn, attempts = (-1, -1).
 *   matrix       n = ((w w + x x) + y y) + z z,  g = 2 / n,
 *                    R00 = 1 - g (y y + z z)   R01 = g (x y - w z)       R02 = g (x z + w y)
 *                    R10 = g (x y + w z)       R11 = 1 - g (x x + z z)   R12 = g (y z - w x)
 *                    R20 = g (x z - w y)       R21 = g (y z + w x)       R22 = 1 - g (x x + y y)
 *                a proper rotation for any q != 0.
 *   pivot        c = the centroid of the sample's first window frame: partial sum l (0 <= l < 64) adds the fp32
 *                coordinates of rows l, l + 64, l + 128, .. as doubles, ascending, onto 0.0; then for off = 32, 16, 8, 4,
 *                2, 1: partial l += partial (l + off) for l < off; c = partial 0 / (double)N.  Or c = 0 (no frame given).
 *   apply        d = (double)p - c,  r_a = (R_a0 d_0 + R_a1 d_1) + R_a2 d_2,  p'_a = (float)((c_a + t_a) + r_a):
 *                rounded to fp32 once.
 *   inverse      d' = (double)p' - (c + t),  p_a = (float)(c_a + ((R_0a d'_0 + R_1a d'_1) + R_2a d'_2)).
 *   non-finite   A non-finite coordinate in the first window frame makes the centroid non-finite and with it every row
 *                of that sample (other samples are not touched).  With c = 0 a NaN stays on its own atom (all three of
 *                its components: every r_a reads all of d); an infinite coordinate likewise makes its own atom NaN
 *                or infinite and no other.
 */
#ifndef MDNO_AUGMENT_H
#define MDNO_AUGMENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDNO_NOISE_TRAIN_MOTION 2 /* stream_id = sample index in its dataset, index = epoch, element = the draw's
                                     number: 0 and 1 the translation, 2 .. 65 the rotation's candidates */
#define MDNO_AUGMENT_LAST_ELEMENT 65

/* The motions of B samples: quaternion f64 [B, 4] (w, x, y, z), pivot f64 [B, 3] (c), shift f64 [B, 3] (t) and
 * attempts i32 [B, 2] (the two accepted elements, -1 for one that was not found or not drawn).  sample_ids i32 [B]
 * (device): every sample's index in its dataset.  rotate 0 / 1; translate finite and >= 0; last_element in [2, 65]
 * (below 65 only so that a test can reach the fallback).  pivot_frames f32 [B * N, 3]: the first window frame of the
 * collated batch, sample b owning rows b * N .. b * N + N - 1 (N >= 1), or NULL for c = 0 (N is then not used).
 * One wave per sample; B <= 65535. */
int mdnoaug_motions(uint64_t seed, const int32_t* sample_ids, int B, int64_t epoch, int rotate, double translate,
                    int last_element, const float* pivot_frames, int N, double* quaternion, double* pivot, double* shift,
                    int32_t* attempts, void* stream);

/* x_out = the motion (inverse != 0: its inverse) of x_in, both f32 [F, B * N, 3]; x_out may be x_in.  Sample b owns rows
 * b * N .. b * N + N - 1 of every frame and moves by quaternion[b], pivot[b], shift[b] (as mdnoaug_motions wrote
 * them, or the caller's own; the matrix is formed from q by the rule in every workgroup).  B <= 65535,
 * F * N < 2^31. */
int mdnoaug_apply(const double* quaternion, const double* pivot, const double* shift, int B, int N, int F, int inverse,
                  const float* x_in, float* x_out, void* stream);

/* attr_out f32 [E, 6]: row e = (x0[edge_index[0][e]], x0[edge_index[1][e]]) — the edge attributes the collation of
 * the samples gives, gathered again from a moved first window frame x0 f32 [R, 3]; edge_index i64 [2, E].  An index
 * outside [0, R) writes six NaN and reads nothing.  E = 0 launches nothing. */
int mdnoaug_edge_attr(const float* x0, const int64_t* edge_index, int64_t E, int64_t R, float* attr_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_AUGMENT_H */
