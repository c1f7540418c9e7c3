/*
 * mdno_dynamics.h — seventh public header of libmdno.so: time-correlation statistics of a trajectory that already lies
 * in device memory (csrc/dynamics.hip) — the sums behind the mean squared displacement MSD(tau), the
 * non-Gaussian parameter and the self part of the van Hove function, the velocity autocorrelation of finite-difference
 * velocities, and a companion that unwraps frames which arrive wrapped into a periodic box.  Additive, like
 * mdno_observe.h: include/mdno.h, include/mdno_train.h and their version numbers stay as they are, and no launch,
 * captured graph or bit of an existing entry point changes.  (This file is part of the library's content hash, and
 * csrc/dynamics.hip includes it, so a declaration that drifts from its definition does not compile;
 * tests/test_cabi_tables.py holds it to the ctypes table and the exports.)  Conventions as in mdno.h: device pointers
 * owned by the caller, explicit sizes, `stream` a hipStream_t passed as void*, 0 or a negative MDNO_E* code
 * (mdno_last_error() has the message).
 *
 * FRAMES are f32 [S, M, N, 3], time-major and contiguous: the layout of a rollout's trajectory buffer; x_i(t) below is
 * atom i of member m at time t.  Frames are never wrapped in this project, so no box enters the statistics
 * (mdno_unwrap_frames is for data that arrives wrapped).
 *
 * LAGS AND ORIGINS.  lags is a HOST i32 [n_lags] array, n_lags in 1 .. 1024, every lag tau in 0 .. S - 1 (the velocity
 * autocorrelation: 0 .. S - 2); it is read before the call returns and may be freed or changed then.  origin_stride
 * is >= 1.  The origins of lag tau are t = 0, stride, 2 stride, ... while t + tau <= S - 1 (velocities: t + tau + 1
 * <= S - 1).
 *
 * THE RULE OF THE DISPLACEMENTS.  For every member m, lag index l, origin t and atom i, all in fp64 on the fp32
 * coordinates, no FMA contraction:
 *     d_a = (double)x_i(t + tau)[a] - (double)x_i(t)[a]
 *     remove_com != 0:  d_a = d_a - (c(t + tau)[a] - c(t)[a]),   c(t) the centroid of the member's frame: the fp64 sum of
 *                       the coordinates in a fixed order, divided by (double)N, formed once per frame into the workspace
 *     s   = (dx*dx + dy*dy) + dz*dz
 *     sum2[m, l] += s,   sum4[m, l] += s*s                 f64 [M, n_lags] each
 *     n_bins > 0:   r = sqrt(s); the sample is counted iff r < r_max (strict; a NaN compares false: not counted);
 *                   b = (long long)(r * inv_dr), inv_dr = (double)n_bins / r_max formed once on the host, b == n_bins
 *                   (rounding) is set to n_bins - 1; counts[m, l, b] += 1      i64 [M, n_lags, n_bins]
 *                   (the binning of mdno_pair_histogram)
 *     n_bins == 0:  no histogram; counts may be NULL and r_max is ignored.  Otherwise n_bins is in 1 .. 4096 and r_max
 *                   is finite and > 0.
 * The number of samples of (m, l) is n_origins(tau) * N with n_origins(tau) = (S - 1 - tau) / origin_stride + 1
 * (integer division): a host formula, not written by the kernels.
 *
 * THE ORDER OF THE SUMS is fixed by (S, M, N, lags, origin_stride) alone — never by the device, the grid or the run —
 * and there are no floating-point atomics.  A workgroup of 256 threads owns MDNO_DYN_ORIGIN_CHUNK consecutive origins
 * (the last chunk of a lag: the rest) times one tile of MDNO_DYN_ATOM_TILE consecutive atoms of one (m, l); thread k
 * adds the samples e = k, k + 256, ... of that block in ascending order (e = origin-in-chunk * atoms-in-tile + atom-
 * in-tile), the threads' sums are added over a wave by an xor butterfly and over the waves in wave order, and the
 * workgroup stores ONE partial into the workspace.  A second kernel adds the partials of (m, l) in ascending (chunk,
 * tile) order and stores the result.  The same input gives the same bits on every run, and member m's entries do not
 * depend on M or on the other members.  The histogram is integer: any order of its adds gives the same bits.
 *
 * NON-FINITE INPUT.  A NaN or Inf coordinate makes non-finite exactly the sum2 / sum4 / corr entries one of whose samples
 * touches it (with remove_com: every sample of a frame whose centroid it enters) and takes exactly those samples out of
 * counts.  No other member changes.
 *
 * VELOCITY AUTOCORRELATION.  v_i(t)[a] = (double)x_i(t + 1)[a] - (double)x_i(t)[a], with remove_com != 0 minus
 * (c(t + 1)[a] - c(t)[a]);  corr[m, l] = sum_t sum_i (vx*vx' + vy*vy') + vz*vz',  v' = v_i(t + tau);  f64 [M, n_lags].
 * Needs S >= 2.  Samples per (m, l): ((S - 2 - tau) / origin_stride + 1) * N.  Same chunks, same fixed order.
 *
 * UNWRAPPING.  frames f32 [S, M, N, 3] and a HOST box f64 [3] (0 = open axis; every entry finite and >= 0 as in
 * mdno_pbc.h, without a cutoff condition) -> out f32 of the same shape.  Per member, atom and axis with L > 0, with an
 * integer image count n (held as an integer-valued double) and no accumulated rounding:
 *     n(0) = 0, u(0) = x(0);   t >= 1:  d = ((double)x(t) - n(t-1) * L) - (double)u(t-1),  k = rint(d * invL),
 *     invL = 1.0 / L formed on the host,  n(t) = n(t-1) + k,  u(t) = (float)((double)x(t) - n(t) * L)
 * An axis with L == 0 is a copy.  A trajectory whose steps are all shorter than L / 2 and which never wrapped comes back
 * bit for bit.
 */
#ifndef MDNO_DYNAMICS_H
#define MDNO_DYNAMICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* origins per workgroup, and atoms per workgroup: they fix the order of the sums (above) */
#define MDNO_DYN_ORIGIN_CHUNK 64
#define MDNO_DYN_ATOM_TILE 256

/* Bytes of scratch mdno_displacement_stats needs: the centroids f64 [S, M, 3] and one partial per (m, l, chunk, tile),
 * sized for origin_stride == 1.  Non-decreasing in every argument. */
size_t mdno_displacement_stats_workspace_bytes(int S, int M, int N, int n_lags, int n_bins);

/* frames -> sum2, sum4 f64 [M, n_lags] and (n_bins > 0) counts i64 [M, n_lags, n_bins] by the rule above; counts is zeroed
 * on the same stream first.  MDNO_EINVAL before any device work for negative sizes, n_lags outside 1 .. 1024,
 * origin_stride < 1, n_bins outside 0 .. 4096, r_max not finite or <= 0 with n_bins > 0, a lag outside 0 .. S - 1, a null
 * frames (N > 0), lags, sum2, sum4 or (n_bins > 0) counts, a workspace smaller than stated; MDNO_EUNSUPPORTED for
 * M > 65535.  S == 0 or M == 0: returns 0, touches nothing.  N == 0: rows of zeros. */
int mdno_displacement_stats(const float* frames, int S, int M, int N, const int32_t* lags, int n_lags, int origin_stride,
                            int remove_com, double r_max, int n_bins, double* sum2, double* sum4, int64_t* counts,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of scratch mdno_velocity_autocorrelation needs (as above, one sum per partial instead of two). */
size_t mdno_velocity_autocorrelation_workspace_bytes(int S, int M, int N, int n_lags);

/* frames -> corr f64 [M, n_lags] as defined above.  Refusals as mdno_displacement_stats, lags in 0 .. S - 2 (S == 1:
 * every lag is refused). */
int mdno_velocity_autocorrelation(const float* frames, int S, int M, int N, const int32_t* lags, int n_lags,
                                  int origin_stride, int remove_com, double* corr, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* frames f32 [S, M, N, 3] -> out f32 [S, M, N, 3] unwrapped as defined above: one thread per (member, atom, axis) scans
 * over S.  MDNO_EINVAL for negative sizes, a null or bad box (the messages of mdno_pbc.h), null pointers, out == frames.
 * Nothing to do (S * M * N == 0): returns 0, touches nothing. */
int mdno_unwrap_frames(const float* frames, int S, int M, int N, const double* box, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_DYNAMICS_H */
