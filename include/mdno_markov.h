/*
 * mdno_markov.h — eleventh public header of libmdno.so: the device half of a Markov state model of a run, on feature rows
 * that already lie in device memory (csrc/markov.hip) — assign every row to its nearest centre, seed
 * centres by farthest-point (k-centres) selection, sum the rows of every state (the Lloyd update of k-means) and count the
 * transitions between the states at a set of lags.  The models themselves (active set, transition matrix, spectrum,
 * Chapman–Kolmogorov) are the host's (forecast.py: markov_model).  Additive, like mdno_essential.h: include/mdno.h,
 * include/mdno_train.h and their version numbers stay as they are, and no launch, captured graph or bit of an existing
 * entry point changes.  (This file is part of the library's content hash, and csrc/markov.hip includes it, so a declaration
 * that drifts from its definition does not compile; tests/test_cabi_tables.py holds it to the ctypes table and the
 * exports.)  Conventions as in mdno.h: device pointers owned by the caller, explicit sizes, `stream` a hipStream_t passed
 * as void*, 0 or a negative MDNO_E* code (mdno_last_error() has the message), every refusal before any device work.
 *
 * THE PREFIX.  The entry points are named mdnomsm_*, not mdno_*.  The prefix is kept because the names are ABI;
 * nothing else asks for it (names need only be unique over all headers, which tests/test_cabi_tables.py checks).
 * The functions live in the same library, under the same content hash and the
 * same mdno_abi_version().
 *
 * ARITHMETIC.  Everything in fp64, no FMA contraction outside the matrix instruction, no floating-point atomics (the only
 * atomics add integers).  The order of every sum is fixed by the shapes alone (below), so a call gives the same bits on
 * every run, whatever the workspace held.
 *
 * FEATURE MATRICES are [R, D], row-major.  `dtype` chooses the element type of the rows AND of the centres: MDNO_MSM_F32
 * (frames, latents) or MDNO_MSM_F64 (what mdnopca_project returns).  A value is widened to fp64 when it is loaded; everything
 * after the load is the same code.  "Non-finite" means NaN or +-Inf in the stored value.
 *
 * ASSIGN (mdnomsm_assign).  x [R, D], centres [k, D], origin f64 [D] (null: zeros):
 *     x~_ra = (double)x_ra - origin_a          c~_ja = (double)c_ja - origin_a
 *     n_r   = sum_a x~_ra * x~_ra              one running sum from zero, a ascending
 *     m_j   = sum_a c~_ja * c~_ja              likewise
 *     g_rj  = sum_a x~_ra * c~_ja              on v_mfma_f64_16x16x4_f64, in ascending groups of four features: a group
 *                                              is ONE matrix instruction that adds its four products onto the running
 *                                              partial; features past D are zeros
 *     d2_rj = max(0, (n_r + m_j) - 2 g_rj)
 *   The bits of d2_rj depend on row r, centre j, origin and D alone — not on R, k, the tile the pair falls into or the run:
 *   two identical centres tie exactly.  The rows and centres are centred in fp64 on their way into LDS; no fp64 copy of x
 *   reaches global memory.
 *   label_r = the j with the smallest d2_rj among the centres that hold no non-finite value, the lowest j on a tie;
 *   dist2_r = that d2.  A candidate replaces the best so far only when it is strictly smaller, so a d2 that is NaN or +Inf
 *   (a non-finite origin, an overflow of fp64 inputs) is never chosen.  A row that holds a non-finite value, k == 0, or
 *   no centre left to choose: label -1, dist2 NaN.
 *   TILES.  A workgroup owns MDNO_MSM_ROW_TILE rows x MDNO_MSM_CENTRE_TILE centres and walks the features in passes of
 *   MDNO_MSM_FEATURE_PASS.  Within a tile the candidates of a row are compared in ascending j; every centre tile writes its
 *   best (value, index) per row to the workspace and a second kernel takes the minimum over the tiles in ascending tile
 *   order.  WORKSPACE: ceil(k / MDNO_MSM_CENTRE_TILE) * R entries of (f64, i32), each array rounded up to 256 bytes.
 *
 * K-CENTRES (mdnomsm_kcenters).  Farthest-point seeding; all k rounds are enqueued, nothing is read back in between.
 *     index[0] = first, radius[0] = +inf
 *     round i = 1 .. k - 1, with c = index[i - 1] read from device memory:
 *         e_r     = sum_a ((double)x_ra - (double)x_ca)^2      the direct form, one running sum from zero, a ascending
 *         mind2_r = min(mind2_r, e_r)                            (mind2_r = +inf before round 1; e_r replaces it only
 *                                                                 when strictly smaller, so a NaN e_r changes nothing)
 *         index[i]  = the r with the largest mind2_r among the rows without a non-finite value, the lowest r on a tie
 *         radius[i] = sqrt of that maximum: the covering radius BEFORE centre i was added
 *   Once every finite row is a centre every mind2 is 0 and the rule still holds: the lowest finite row, radius 0.  No
 *   finite row at all: index[i] = -1, radius[i] = NaN (and a round whose centre is -1 changes nothing).
 *   The argmax is a fixed two-stage reduction: one (value, row) per workgroup of MDNO_MSM_ARGMAX_TILE rows, then one
 *   workgroup over those; "larger value, then lower row" is a total order, so the result does not depend on the tree.
 *   WORKSPACE: mind2 f64 [R], and per workgroup one f64 and one i64.
 *
 * CENTROID SUMS (mdnomsm_centroid_sums).  x [R, D], label i32 [R]:
 *     sums[j, a] = sum of (double)x_ra over the rows with label_r == j;  counts[j] = their number
 *   MDNO_MSM_SUM_PARTIALS partial sums per (state, feature): partial t adds the rows t, t + MDNO_MSM_SUM_PARTIALS, ... whose
 *   label is that state, in ascending row order; the partials are added in ascending t.  A workgroup owns
 *   MDNO_MSM_SUM_FEATURES features x MDNO_MSM_SUM_STATES states; one thread owns a feature column of its partial's table
 *   in LDS, so no two threads add to the same cell.  Labels outside 0 .. k - 1 are skipped; an empty state is zeros.
 *   counts are integers (exact in any order).
 *
 * TRANSITION COUNTS (mdnomsm_transition_counts).  label i32 [S, M], time-major like a rollout's trajectory buffer.  For lag
 * l of `lags` (a HOST array of n_lags int32), member m and every origin t with t + lag < S:
 *     from = label[t, m], to = label[t + lag, m];  both in 0 .. n_states - 1: counts[l, m (or 0 when pooled), from, to] += 1
 *                                                  otherwise:                  n_skipped[l] += 1
 *   so counts[l].sum() + n_skipped[l] == M max(S - lag, 0).  Integer atomics only; n_states <= MDNO_MSM_LDS_STATES
 *   keeps a private table in LDS per workgroup.  A lag >= S gives zeros.
 */
#ifndef MDNO_MARKOV_H
#define MDNO_MARKOV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element types of a feature matrix */
#define MDNO_MSM_F32 0
#define MDNO_MSM_F64 1
/* the largest number of states (centres) of every entry point */
#define MDNO_MSM_MAX_STATES 1024
/* assign: rows and centres per workgroup, features staged per pass */
#define MDNO_MSM_ROW_TILE 64
#define MDNO_MSM_CENTRE_TILE 64
#define MDNO_MSM_FEATURE_PASS 32
/* k-centres: rows per workgroup of the first argmax stage */
#define MDNO_MSM_ARGMAX_TILE 64
/* centroid sums: partial sums per (state, feature); features and states per workgroup */
#define MDNO_MSM_SUM_PARTIALS 16
#define MDNO_MSM_SUM_FEATURES 16
#define MDNO_MSM_SUM_STATES 16
/* transition counts: the largest n_states whose n x n table is kept in LDS; the largest number of lags */
#define MDNO_MSM_LDS_STATES 64
#define MDNO_MSM_MAX_LAGS 1024

/* The WORKSPACE of mdnomsm_assign: non-decreasing in R and k, independent of D; 0 for a negative size or
 * k > MDNO_MSM_MAX_STATES (and where there is nothing to do); SIZE_MAX where it does not fit a size_t. */
size_t mdnomsm_assign_workspace_bytes(int64_t R, int k, int D);

/* x [R, D], centres [k, D] (both of `dtype`), origin f64 [D] or null -> label i32 [R] (or null), dist2 f64 [R] (or null).
 * MDNO_EINVAL for negative sizes, a dtype other than the two above, k > MDNO_MSM_MAX_STATES, both outputs null, a null x
 * with R D > 0, null centres with k D > 0 (and R > 0), a workspace that is null or smaller than
 * mdnomsm_assign_workspace_bytes(R, k, D) where R > 0 and k > 0; MDNO_EUNSUPPORTED where R exceeds the launch grid.
 * R == 0: returns 0 and touches nothing.  k == 0: every label -1, every dist2 NaN, no workspace needed. */
int mdnomsm_assign(const void* x, int64_t R, int D, int dtype, const void* centres, int k, const double* origin,
                   int32_t* label, double* dist2, void* workspace, size_t workspace_bytes, void* stream);

/* The WORKSPACE of mdnomsm_kcenters: non-decreasing in R, independent of D; 0 for a negative size; SIZE_MAX where it does
 * not fit. */
size_t mdnomsm_kcenters_workspace_bytes(int64_t R, int D);

/* x [R, D] of `dtype` -> index i64 [k], radius f64 [k].  MDNO_EINVAL for negative sizes, a bad dtype, k outside
 * 1 .. MDNO_MSM_MAX_STATES, k > R, first outside 0 .. R - 1, a null index or radius, a null x with D > 0, a workspace that
 * is null or too small; MDNO_EUNSUPPORTED where R exceeds the launch grid. */
int mdnomsm_kcenters(const void* x, int64_t R, int D, int dtype, int k, int64_t first, int64_t* index, double* radius,
                     void* workspace, size_t workspace_bytes, void* stream);

/* x [R, D] of `dtype`, label i32 [R] -> sums f64 [k, D], counts i64 [k].  MDNO_EINVAL for negative sizes, a bad dtype, k
 * outside 1 .. MDNO_MSM_MAX_STATES, a null counts, a null sums with D > 0, a null label with R > 0, a null x with
 * R D > 0. */
int mdnomsm_centroid_sums(const void* x, int64_t R, int D, int dtype, const int32_t* label, int k, double* sums,
                          int64_t* counts, void* stream);

/* label i32 [S, M] (device), lags int32 [n_lags] (HOST) -> counts i64 [n_lags, pooled ? 1 : M, n_states, n_states],
 * n_skipped i64 [n_lags].  MDNO_EINVAL for negative sizes, n_lags outside 1 .. MDNO_MSM_MAX_LAGS, a null lags, a lag < 1,
 * n_states outside 1 .. MDNO_MSM_MAX_STATES, a null counts (with M > 0 or pooled) or n_skipped, a null label with
 * S M > 0; MDNO_EUNSUPPORTED where S or M exceeds the launch grid. */
int mdnomsm_transition_counts(const int32_t* label, int S, int M, int n_states, const int32_t* lags, int n_lags, int pooled,
                              int64_t* counts, int64_t* n_skipped, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_MARKOV_H */
