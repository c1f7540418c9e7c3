/*
 * mdno_observe.h — sixth public header of libmdno.so: structural observables of frames that already lie in device
 * memory (csrc/observe.hip) — the histogram of pair distances of every frame, from which g(r) of a
 * periodic box and p(r) of a protein are formed, and the per-frame radius of gyration.  Additive, like mdno_pbc.h:
 * include/mdno.h, include/mdno_train.h and their version numbers stay as they are, and no launch, captured graph or bit
 * of an existing entry point changes.  (This file is part of the library's content hash, and csrc/observe.hip includes
 * it, so a declaration that drifts from its definition does not compile; tests/test_cabi_tables.py holds it to
 * the ctypes table and the exports.)  Conventions as in mdno.h: device pointers owned by the caller, explicit sizes,
 * `stream` a hipStream_t passed as void*, 0 or a negative MDNO_E* code (mdno_last_error() has the message).
 *
 * THE RULE.  A frame x is f32 [N, 3].  r_max is f64, finite and > 0; n_bins is in 1 .. 4096; box is NULL or HOST
 * f64 [3] as in mdno_pbc.h (0 = open axis; every periodic axis needs L >= 2 * r_max — exactly the box check of
 * mdno_pbc.h with cutoff = r_max, so every counted pair has one image; an all-open box is the same as NULL).  For
 * every UNORDERED pair i < j (no self pairs), all in fp64 on the fp32 coordinates, no FMA contraction:
 *     d_a = (double)x_j[a] - (double)x_i[a]            reduced on a periodic axis as in mdno_pbc.h:
 *                                                      d_a -= rint(d_a * invL) * L, invL = 1.0 / L formed on the host
 *     s   = (dx*dx + dy*dy) + dz*dz,   r = sqrt(s)     (the summation order and the sqrt of the radius graph's test)
 *     the pair is counted iff r < r_max                (strict, as the graph's; a NaN or an Inf anywhere makes the
 *                                                      comparison false: the pair is not counted)
 *     b   = (long long)(r * inv_dr)                    inv_dr = (double)n_bins / r_max formed once on the host;
 *                                                      b == n_bins (rounding) is set to n_bins - 1
 *     counts[f, b] += 1
 * The rule is symmetric in i and j bit for bit (the differences change sign, rint is odd, the squares do not change),
 * so the orientation in which a kernel takes a pair does not matter.  counts is i64 [F, n_bins], ONE ROW PER FRAME,
 * of unordered pairs: the caller sums rows over steps, members or windows on the device (64,000 frames x 200 bins are
 * 102 MB).  Integers: both kernel forms, and any order of their adds, give the same bits.
 * Identity: with r_max = threshold and the same box, 2 * sum_b counts[f, b] + N is the "forecast" contact count of
 * mdno_forecast_score / mdno_forecast_score_pbc on that frame (ordered pairs, diagonal included).
 *
 * RADIUS OF GYRATION.  rg[f], f64: c = (sum_i x_i) / N, rg = sqrt(sum_i |x_i - c|^2 / N); two passes in fp64 in a fixed
 * order (the same bits for the same input on every run); NaN for a frame with a non-finite coordinate or N == 0;
 * independent of any box (frames are never wrapped).
 */
#ifndef MDNO_OBSERVE_H
#define MDNO_OBSERVE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch mdno_pair_histogram needs for F frames of N atoms in the given form (MDNO_FORECAST_AUTO / _LDS /
 * _TILED of mdno.h).  Neither form needs any today: 0. */
size_t mdno_pair_histogram_workspace_bytes(int64_t F, int N, int n_bins, int form);

/* frames f32 [F, N, 3] -> counts i64 [F, n_bins] by the rule above.  Two forms with the same counts: up to 2,048 atoms
 * ONE workgroup per frame stages the frame and a histogram in LDS and stores its own row (no atomics on memory, nothing
 * outside the row written); any N: 256 x 256 pair tiles that add their non-zero bins to the frame's row with integer
 * atomics, after the rows were zeroed on the same stream.  form: MDNO_FORECAST_AUTO (LDS up to 2,048 atoms, tiled
 * above), _LDS (more atoms: MDNO_EUNSUPPORTED) or _TILED.  MDNO_EINVAL before any device work for n_bins outside
 * 1 .. 4096, r_max not finite or <= 0, a bad box (the messages of mdno_pbc.h), a null frames (F * N > 0) or counts
 * (F > 0), a workspace smaller than stated.  F == 0: returns 0, touches nothing.  N == 0 or 1: all-zero rows. */
int mdno_pair_histogram(const float* frames, int64_t F, int N, double r_max, int n_bins, const double* box,
                        int64_t* counts, int form, void* workspace, size_t workspace_bytes, void* stream);

/* frames f32 [F, N, 3] -> rg f64 [F] as defined above: one workgroup per frame, any N. */
int mdno_radius_of_gyration(const float* frames, int64_t F, int N, double* rg, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_OBSERVE_H */
