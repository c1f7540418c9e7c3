/*
 * mdno_essential.h — tenth public header of libmdno.so: essential dynamics of a run, on frames that already lie in device
 * memory (csrc/essential.hip) — put every frame into one frame of reference (optimal rigid superposition
 * onto one structure, the rotated coordinates handed back), form the feature x feature second-moment matrix over the
 * frames at a time lag (lag 0: the covariance PCA diagonalises; lag > 0: the time-lagged matrix of TICA), and project the
 * frames onto chosen directions.  The eigen-solves themselves are the host's (forecast.py: pca, tica).  Additive, like
 * mdno_conformations.h: include/mdno.h, include/mdno_train.h and their version numbers stay as they are, and no launch,
 * captured graph or bit of an existing entry point changes.  (This file is part of the library's content hash, and
 * csrc/essential.hip includes it, so a declaration that drifts from its definition does not compile;
 * tests/test_cabi_tables.py holds it to the ctypes table and the exports.)  Conventions as in mdno.h: device pointers
 * owned by the caller, explicit sizes, `stream` a hipStream_t passed as void*, 0 or a negative MDNO_E* code
 * (mdno_last_error() has the message), every refusal before any device work.
 *
 * THE PREFIX.  The entry points are named mdnopca_*, not mdno_*.  The prefix is kept because the names are ABI;
 * nothing else asks for it (names need only be unique over all headers, which tests/test_cabi_tables.py checks).
 * The functions live in the same library, under the same content hash and the same
 * mdno_abi_version().
 *
 * ARITHMETIC.  Everything in fp64 on the fp32 inputs, no FMA contraction outside the matrix instruction, no floating-point
 * atomics.  The order of every sum is fixed by the shapes alone (below), so a call gives the same bits on every run.
 *
 * SUPERPOSITION (mdnopca_superpose).  For a frame p of N atoms and the reference q, with the centroid c, the centred
 * coordinates a_k = (double)p_k - c_p, b_k = (double)q_k - c_q and g as in mdno_conformations.h (FRAME ORDER: 64 partial
 * sums, partial t adds the terms of atoms t, t + 64, ... in ascending order; the partials are added pairwise by an xor
 * butterfly, t with t ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1):
 *     S_rc     = sum_k a_k[r] * b_k[c]      nine sums over the atoms, each in the FRAME ORDER
 *     G        = g_p + g_q
 *     (lambda, v) = the largest eigenvalue of Horn's 4 x 4 quaternion matrix of S and its eigenvector (csrc/superpose.h:
 *                the cyclic Jacobi sweeps of rmsd2_from_moments with the rotations accumulated; among equal diagonal
 *                entries the lowest index)
 *     R        = the rotation matrix of the quaternion v / |v|: a proper rotation whatever v is, never a reflection
 *     aligned_k = R a_k + c_q              in fp64, rounded once to fp32
 *     rmsd     = sqrt(max(0, G - 2 lambda) / N)
 * A degenerate largest eigenvalue (N <= 2, collinear frames, a frame identical to the reference's mirror image) gives one
 * of the optimal rotations, finite.  A frame with a non-finite coordinate gives NaN in its whole aligned frame and in its
 * rmsd; a non-finite reference gives NaN everywhere.  N == 0: nothing is written to `aligned`, every rmsd is 0.  The bits
 * of a frame's outputs depend on that frame, the reference and N alone.
 *
 * COLUMN SUMS (mdnopca_feature_sums).  X is f32 [R, D].  sum[a] = sum_r (double)X[r, a]: MDNO_PCA_SUM_PARTIALS partial
 * sums, partial t adds rows t, t + MDNO_PCA_SUM_PARTIALS, ... in ascending order, and the partials are added in ascending
 * t.  A column that holds a non-finite value gives NaN.  n_invalid = the number of rows that hold a non-finite value (an
 * integer count: exact in any order).  The host forms the mean, sum / R.
 *
 * COVARIANCE (mdnopca_covariance).  X is f32 [S, M, D], time-major like a rollout's trajectory buffer (a flat [S M, D]
 * matrix of rows), `mean` f64 [D], lag >= 0:
 *     C[a, b] = sum_m sum_{t = 0}^{S - 1 - lag} ((double)X[t, m, a] - mean[a]) * ((double)X[t + lag, m, b] - mean[b])
 * pooled over the members: K = M (S - lag) terms, term r = t M + m pairs row r of the flat matrix with row r + lag M.
 * lag >= S: K = 0 and C is zeros.  One fp64 GEMM over the rows on v_mfma_f64_16x16x4_f64; the rows are centred in fp64 on
 * their way into LDS and no fp64 copy of X reaches global memory.
 *   TILES.  C is cut into T x T tiles of MDNO_PCA_TILE x MDNO_PCA_TILE, T = ceil(D / MDNO_PCA_TILE).  lag == 0 computes
 *   the T (T + 1) / 2 tiles with tile row <= tile column and of those only the elements a <= b are kept; C[b, a] is a copy
 *   of C[a, b], so C is bitwise symmetric.  lag > 0 computes all T^2 tiles: C is not symmetric.
 *   ROW SPLIT (fixed by K, D and whether lag is 0, alone).  With `tiles` the number of computed tiles,
 *       want   = min(MDNO_PCA_MAX_SPLITS, max(1, ceil(MDNO_PCA_TARGET_WORKGROUPS / tiles)))
 *       L      = MDNO_PCA_ROW_CHUNK * ceil(K / (want * MDNO_PCA_ROW_CHUNK))          rows per split
 *       splits = ceil(K / L)                                                         (<= want)
 *   Split i owns the terms r = i L .. min(K, (i + 1) L) - 1.  One workgroup per (tile, split) walks its rows in ascending
 *   passes of MDNO_PCA_ROW_PASS, each pass in ascending groups of four; a group is ONE v_mfma_f64_16x16x4_f64 that adds its
 *   four products onto the running partial C[a, b] (rows past the split's end are zeros).  The partial tiles go to the
 *   workspace and a second kernel adds them in ascending split order, partial 0 first.
 *   WORKSPACE.  8 MDNO_PCA_TILE^2 bytes per (tile, split); since tiles * splits < MDNO_PCA_TARGET_WORKGROUPS + tiles and
 *   splits <= MDNO_PCA_MAX_SPLITS, the bound  8 MDNO_PCA_TILE^2 * min(T^2 MDNO_PCA_MAX_SPLITS, MDNO_PCA_TARGET_WORKGROUPS
 *   + T^2)  holds whatever K is: it depends on D alone.  The result does not depend on what the workspace held.
 *
 * PROJECTION (mdnopca_project).  X f32 [R, D], mean f64 [D], V f64 [D, k], 1 <= k <= MDNO_PCA_MAX_COMPONENTS:
 *     P[r, c] = sum_a ((double)X[r, a] - mean[a]) * V[a, c]       one running sum from zero, a ascending
 */
#ifndef MDNO_ESSENTIAL_H
#define MDNO_ESSENTIAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* features per side of a workgroup's tile of C */
#define MDNO_PCA_TILE 32
/* rows staged per pass */
#define MDNO_PCA_ROW_PASS 32
/* the row chunk: a split's length is a multiple of it */
#define MDNO_PCA_ROW_CHUNK 64
/* the row split aims at this many workgroups and stops at MDNO_PCA_MAX_SPLITS splits */
#define MDNO_PCA_TARGET_WORKGROUPS 2048
#define MDNO_PCA_MAX_SPLITS 256
/* partial sums per column of mdnopca_feature_sums */
#define MDNO_PCA_SUM_PARTIALS 16
/* the largest k of mdnopca_project */
#define MDNO_PCA_MAX_COMPONENTS 32

/* frames f32 [S, M, N, 3], reference f32 [N, 3] -> aligned f32 [S, M, N, 3] (or null), rmsd f64 [S, M] (or null), by the
 * rule above.  `aligned` may not overlap `frames`.  MDNO_EINVAL for negative sizes, both outputs null, a null frames or
 * reference with work to do (S M > 0 and N > 0); MDNO_EUNSUPPORTED where S M exceeds the launch grid (four frames per
 * workgroup).  S M == 0: returns 0 and touches nothing. */
int mdnopca_superpose(const float* frames, int S, int M, int N, const float* reference, float* aligned, double* rmsd,
                      void* stream);

/* x f32 [R, D] -> sum f64 [D], n_invalid i64 [1].  MDNO_EINVAL for negative sizes, a null n_invalid, a null sum with
 * D > 0, a null x with R D > 0.  R == 0: zeros. */
int mdnopca_feature_sums(const float* x, int64_t R, int D, double* sum, int64_t* n_invalid, void* stream);

/* The WORKSPACE bound above: a function of D alone, so non-decreasing in S, M and D; 0 for a negative size or lag;
 * SIZE_MAX where it does not fit a size_t. */
size_t mdnopca_covariance_workspace_bytes(int S, int M, int D, int lag);

/* x f32 [S, M, D], mean f64 [D], lag -> c f64 [D, D].  MDNO_EINVAL for negative sizes or lag, a null c with D > 0, a null x
 * or mean with work to do (K > 0 and D > 0), a workspace that is null or smaller than
 * mdnopca_covariance_workspace_bytes(S, M, D, lag) where there is work to do; MDNO_EUNSUPPORTED where tiles x splits
 * exceeds the launch grid.  K == 0: zeros, no workspace needed. */
int mdnopca_covariance(const float* x, int S, int M, int D, const double* mean, int lag, double* c, void* workspace,
                       size_t workspace_bytes, void* stream);

/* x f32 [R, D], mean f64 [D], v f64 [D, k] -> p f64 [R, k].  MDNO_EINVAL for negative sizes, k outside
 * 1 .. MDNO_PCA_MAX_COMPONENTS, a null p with R > 0, a null x, mean or v with R D > 0; MDNO_EUNSUPPORTED where R exceeds
 * the launch grid (16 rows per workgroup).  D == 0: zeros. */
int mdnopca_project(const float* x, int64_t R, int D, const double* mean, const double* v, int k, double* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_ESSENTIAL_H */
