/*
 * mdno_conformations.h — ninth public header of libmdno.so: structural coverage of a run, on frames that already lie in
 * device memory (csrc/conformations.hip) — the superposed RMSD of EVERY produced frame against EVERY
 * reference frame, and its row and column minima: the nearest reference frame of each produced frame (precision) and the
 * nearest produced frame of each reference frame, per member (coverage).  Additive, like mdno_ensemble.h: include/mdno.h,
 * include/mdno_train.h and their version numbers stay as they are, and no launch, captured graph or bit of an existing
 * entry point changes.  (This file is part of the library's content hash, and csrc/conformations.hip includes it, so a
 * declaration that drifts from its definition does not compile; tests/test_cabi_tables.py holds it to the ctypes
 * table and the exports.)  Conventions as in mdno.h: device pointers owned by the caller, explicit sizes, `stream` a
 * hipStream_t passed as void*, 0 or a negative MDNO_E* code (mdno_last_error() has the message).
 *
 * THE PREFIX.  The two entry points are named mdnoconf_*, not mdno_*.  The prefix is kept because the names are
 * ABI; nothing else asks for it (names need only be unique over all headers, which tests/test_cabi_tables.py checks).
 * The functions live in the same library, under the same content hash and the same
 * mdno_abi_version().
 *
 * INPUTS.  A is f32 [S, M, N, 3], time-major and contiguous: the layout of a rollout's trajectory buffer, M members (a plain
 * stack [F, N, 3] is M = 1).  B is f32 [Fb, N, 3], the reference frames.  Row (s, m) is compared with column j.  A and B may
 * be the same buffer (the self matrix); its symmetry is not exploited (below).
 *
 * THE RULE.  Everything in fp64 on the fp32 coordinates, no FMA contraction outside the matrix instruction.  For a frame p
 * of N atoms p_0 .. p_(N-1):
 *     c_p      = (sum_k (double)p_k, in the FRAME ORDER below) / (double)N                 the centroid
 *     a_k      = (double)p_k - c_p
 *     g_p      = sum_k ((a_k[0]^2 + a_k[1]^2) + a_k[2]^2), in the FRAME ORDER
 *     valid(p) = every coordinate of p is finite
 * and for a pair of valid frames p (of A, centred: a) and q (of B, centred: b):
 *     S_rc     = sum_k a_k[r] * b_k[c]      nine sums over the atoms, in the PAIR ORDER below
 *     G        = g_p + g_q
 *     lambda   = the largest eigenvalue of Horn's 4 x 4 quaternion matrix of S (csrc/superpose.h: cyclic Jacobi, the
 *                eigen-solve mdno_forecast_score uses, one definition)
 *     rmsd^2   = max(0, G - 2 lambda) / N
 *     matrix[s, m, j] = sqrt(rmsd^2)
 * A pair with an invalid frame on either side is NaN in `matrix`.  N == 0: every frame is valid and every rmsd is 0.
 *     nearest[s, m]       = min_j matrix[s, m, j] over the valid j;  nearest_index[s, m] = the LOWEST j that attains it.
 *                           Frame (s, m) invalid, or no valid j (Fb == 0 among them): NaN and -1.
 *     cover[m, j]         = min_s matrix[s, m, j] over member m's valid steps;  cover_step[m, j] = the LOWEST such s.
 *                           Frame j invalid, or no valid step of member m (S == 0 among them): NaN and -1.
 * A minimum is exact: apart from ties, which the lowest index settles, no order matters, and there are no floating-point
 * atomics.
 *
 * FRAME ORDER (fixed by N alone).  64 partial sums: partial t adds the terms of atoms t, t + 64, t + 128, ... in ascending
 * order; the partials are then added pairwise, t with t ^ 32, then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1 (an xor butterfly).
 *
 * PAIR ORDER (fixed by N alone).  The atoms are walked in ascending chunks of MDNO_CONF_ATOM_CHUNK, each chunk in ascending
 * groups of four; a group is ONE v_mfma_f64_16x16x4_f64 that adds its four products a_k[r] * b_k[c] onto the running S_rc
 * (the atoms past N in the last chunk are zeros).  No sum is split over the atoms across workgroups.
 *
 * POSITION INDEPENDENCE.  The bits of matrix[s, m, j] depend only on the coordinates of the two frames and on N: not on S,
 * M, Fb, the pair's position in a tile, which outputs were asked for, or the run.  A member scored alone has the bits it
 * has inside any batch, and a sub-selection of steps, members or reference frames gives the sub-block of the full matrix.
 * This is why the self matrix is computed in full: S and its transpose give Horn matrices that are equal in exact
 * arithmetic only, so matrix[i, j] and matrix[j, i] may differ in the last bits, and copying one half would make an
 * element's bits depend on where it lies.
 *
 * TILES.  A workgroup scores MDNO_CONF_FRAME_TILE consecutive STEPS of ONE member against MDNO_CONF_FRAME_TILE consecutive
 * reference frames; it leaves one (minimum, index) per row and per column of its tile in the workspace, and two small
 * kernels take the minima over the tiles in ascending tile order.
 */
#ifndef MDNO_CONFORMATIONS_H
#define MDNO_CONFORMATIONS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* frames per side of a workgroup's tile of pairs */
#define MDNO_CONF_FRAME_TILE 32
/* atoms staged per pass: fixes the PAIR ORDER together with the four-atom groups */
#define MDNO_CONF_ATOM_CHUNK 32

/* Bytes of scratch mdnoconf_cross_rmsd needs: {c[3], g, valid} f64 per frame of A and of B, one (f64, i32) per (row,
 * column tile) and, with want_cover != 0, one per (member, row tile, column).  Non-decreasing in every argument; 0 for a
 * negative size; SIZE_MAX where the count does not fit (such a call is refused as MDNO_EUNSUPPORTED). */
size_t mdnoconf_cross_rmsd_workspace_bytes(int S, int M, int N, int64_t Fb, int want_cover);

/* a f32 [S, M, N, 3], b f32 [Fb, N, 3] -> by the rule above, each output optional:
 *     matrix f64 [S, M, Fb]                              or null
 *     nearest f64 [S, M], nearest_index i64 [S, M]       both or neither
 *     cover f64 [M, Fb], cover_step i64 [M, Fb]          both or neither
 * Before any device work: MDNO_EINVAL for negative sizes, half a pair of outputs, all outputs null, a null a or b with
 * work to do (S M > 0, Fb > 0, N > 0), a workspace that is null or smaller than
 * mdnoconf_cross_rmsd_workspace_bytes(S, M, N, Fb, cover != null) where there is work to do; MDNO_EUNSUPPORTED where
 * M x row tiles x column tiles exceeds the launch grid.  S M == 0 or Fb == 0: returns 0; the outputs that have no
 * counterpart (nearest with Fb == 0, cover with S == 0) are filled with NaN and -1, nothing is written where an output is
 * empty, and no workspace is needed.  N == 0: zeros, index 0. */
int mdnoconf_cross_rmsd(const float* a, int S, int M, const float* b, int64_t Fb, int N, double* matrix, double* nearest,
                        int64_t* nearest_index, double* cover, int64_t* cover_step, void* workspace, size_t workspace_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_CONFORMATIONS_H */
