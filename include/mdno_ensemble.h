/*
 * mdno_ensemble.h — eighth public header of libmdno.so: verification of an ENSEMBLE forecast against the truth, on frames
 * that already lie in device memory (csrc/ensemble.hip) — per step, the sums behind the error of the
 * ensemble mean, the ensemble spread, the continuous ranked probability score (CRPS) and the rank (Talagrand) histogram.
 * Additive, like mdno_dynamics.h: include/mdno.h, include/mdno_train.h and their version numbers stay as they are, and no
 * launch, captured graph or bit of an existing entry point changes.  (This file is part of the library's content hash, and
 * csrc/ensemble.hip includes it, so a declaration that drifts from its definition does not compile;
 * tests/test_cabi_tables.py holds it to the ctypes table and the exports.)  Conventions as in mdno.h: device pointers
 * owned by the caller, explicit sizes, `stream` a hipStream_t passed as void*, 0 or a negative MDNO_E* code
 * (mdno_last_error() has the message).
 *
 * THE PREFIX.  The two entry points are named mdnoens_*, not mdno_*.  The prefix is kept because the names are ABI; nothing
 * else asks for it (names need only be unique over all headers, which tests/test_cabi_tables.py checks).
 * The functions live in the same library, under the same content hash and the same mdno_abi_version().
 *
 * FRAMES are f32 [S, M, N, 3], time-major and contiguous: the layout of a rollout's trajectory buffer, M members of one
 * ensemble.  TRUTH is f32 [S, N, 3].  1 <= M <= 1024.
 *
 * THE RULE.  A sample is one (step s, atom, component): n = 3 N samples per step, sample e of step s being
 * frames[s, m, e] over the members m and truth[s, e].  Everything in fp64 on the fp32 values, no FMA contraction:
 *     x_(0) <= ... <= x_(M-1)     the M members' fp32 values of the sample, sorted ascending (fp32 compare; -0 == +0)
 *     y                           the truth's value
 *     valid                       every x_m and y finite
 *     d_j  = (double)x_(j) - (double)y
 *     mean = (d_0 + d_1 + ... in ascending j) / (double)M
 *     q0 = mean * mean                                         squared error of the ensemble mean
 *     q1 = M >= 2: (sum_j (d_j - mean) * (d_j - mean), ascending j) / (double)(M - 1);   M == 1: 0      unbiased variance
 *     q2 = sum_j |d_j|, ascending j                            = sum_m |x_m - y|
 *     q3 = sum_j (double)(2 j - M + 1) * d_j, ascending j      = sum_{m<k} |x_m - x_k|, through the sort
 *     r  = #{j : x_(j) < y}  (fp32 compare)                    tie: some x_m == y
 *     valid:    sums[s, c] += q_c;  rank_hist[s, r] += 1;  n_ties[s] += tie
 *     invalid:  sums[s, 0..3] += NaN (the step's four sums come out NaN, as a NaN passes on everywhere in this project);
 *               the sample is left out of rank_hist and n_ties;  n_invalid[s] += 1
 * From these: RMSE of the mean = sqrt(sums0 / n), spread = sqrt(sums1 / n), CRPS = sums2 / (M n) - sums3 / (M^2 n), the
 * fair CRPS with M (M - 1) in the second term (forecast.py: EnsembleScore).
 *
 * MEMBER ORDER.  Every per-sample quantity is defined on the SORTED values, so no output depends on the order of the
 * members, bit for bit (only the sign of a zero may differ where -0 and +0 meet): the score does not depend on how the
 * members were sharded over ranks, grouped or gathered.
 *
 * THE ORDER OF THE SUMS over a step's n samples is fixed by (N, M) alone — never by the device, the grid, the form or the
 * run — and there are no floating-point atomics.  A workgroup of 256 threads owns one tile of MDNO_ENS_SAMPLE_TILE
 * consecutive samples of one step; sample k of the tile is thread k's term (a sample past n: 0), the threads' terms are
 * added over a wave by an xor butterfly and over the waves in wave order, and the workgroup stores ONE partial per sum
 * into the workspace.  A second kernel adds a step's partials in ascending tile order.  Step s's outputs depend on
 * nothing but step s.  rank_hist, n_invalid and n_ties are integers: any order of their adds gives the same bits.
 *
 * TWO FORMS, ONE RESULT.  form 0: auto; 1: registers (M <= 64: one thread per sample, the members' values in registers,
 * an unrolled sorting network); 2: LDS (M <= 1024: a workgroup stages [M, T] values and its threads share the columns'
 * sorting networks).  Both give the same bits for every M <= 64; auto takes registers there and LDS above.
 */
#ifndef MDNO_ENSEMBLE_H
#define MDNO_ENSEMBLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* samples per workgroup: fixes the order of the sums (above) */
#define MDNO_ENS_SAMPLE_TILE 256

#define MDNO_ENS_MAX_MEMBERS 1024
#define MDNO_ENS_MAX_REGISTER_MEMBERS 64

/* Bytes of scratch mdnoens_score needs: four partials f64 per (step, tile).  Non-decreasing in every argument; 0 for
 * S <= 0 or a negative M or N. */
size_t mdnoens_score_workspace_bytes(int S, int M, int N);

/* frames, truth -> sums f64 [S, 4], rank_hist i64 [S, M + 1], n_invalid i64 [S], n_ties i64 [S] by the rule above; the
 * three integer outputs are zeroed on the same stream first.  Before any device work: MDNO_EINVAL for negative sizes, a
 * form outside 0 .. 2, M outside 1 .. 1024 (with S > 0 and N > 0), a null frames or truth (N > 0), sums, rank_hist,
 * n_invalid or n_ties, a workspace that is null or smaller than stated; MDNO_EUNSUPPORTED for form 1 with M > 64 and
 * where S times the tiles of a step exceeds the launch grid.  S == 0: returns 0, touches nothing.  N == 0: rows of
 * zeros. */
int mdnoens_score(const float* frames, const float* truth, int S, int M, int N, double* sums, int64_t* rank_hist,
                  int64_t* n_invalid, int64_t* n_ties, int form, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_ENSEMBLE_H */
