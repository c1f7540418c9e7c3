/*
 * mdno_surface.h — public header of libmdno.so: the solvent-accessible surface of frames that already lie in
 * device memory (csrc/surface.hip) — per atom and frame the number of points of a sphere table that no
 * other atom's expanded sphere covers (Shrake and Rupley's count), from which the per-atom, per-residue and total area
 * follow on the caller's side as 4 pi R_i^2 * count / P.  Additive, like mdno_observe.h: include/mdno.h,
 * include/mdno_train.h and their version numbers stay as they are, and no launch, captured graph or bit of an existing
 * entry point changes.  (This file is part of the library's content hash, and csrc/surface.hip includes it, so a
 * declaration that drifts from its definition does not compile; tests/test_cabi_tables.py holds it to the ctypes table
 * and the exports.)  Conventions as in mdno.h: device pointers owned by the caller, explicit sizes, `stream` a
 * hipStream_t passed as void*, 0 or a negative MDNO_E* code (mdno_last_error() has the message), every refusal before
 * any device work.  The entry points are named mdnosa_*.
 *
 * THE RULE.  frames is f32 [F, N, 3].  R is f64 [N] on the device: the EXPANDED radii r_i + probe, formed by the caller
 * in fp64, finite and > 0.  U is f64 [P, 3] on the device, P in 1 .. MDNOSA_MAX_POINTS: the point table.  It is data: no
 * kernel calls sin or cos, and none cares whether the rows are unit vectors.  box is NULL or HOST f64 [3] as in
 * mdno_pbc.h (0 = open axis; an all-open box is the same as NULL).  reach is f64, 2 * max_i R_i, formed by the caller:
 * every periodic axis needs L >= 2 * reach — the box check of mdno_pbc.h with cutoff = reach — so a pair has one image
 * inside R_i + R_j.  A reach that lies gives wrong numbers, never an access outside the buffers.  For atom i of frame
 * f, all in fp64 on the fp32 coordinates, no FMA contraction:
 *   1. a coordinate of x_i is not finite:  counts[f, i] = -1.
 *   2. for every j != i:
 *        d_a = (double)x_j[a] - (double)x_i[a]          reduced on a periodic axis as in mdno_pbc.h:
 *                                                       d_a -= rint(d_a * invL) * L, invL = 1.0 / L formed on the host
 *        s   = (dx*dx + dy*dy) + dz*dz
 *        j is a NEIGHBOUR iff sqrt(s) < R_i + R_j       (strict; a NaN or an Inf anywhere makes it false)
 *      The neighbour filter is part of the rule, not an optimisation that may be widened.
 *   3. for every point p:  q_a = R_i * U[p, a];  p is BURIED iff some neighbour j has t < R_j * R_j, where
 *        e_a = q_a - d_a,  t = (ex*ex + ey*ey) + ez*ez  (strict)
 *   4. counts[f, i] = the number of points that are not buried.  counts is i32 [F, N].
 * "Buried" is an OR over the neighbours: their order, any chunking, an early exit, the kernel form and the batch cannot
 * change a value.  Integers; no atomics at all; every element of counts is stored exactly once.  N == 1 gives P.
 */
#ifndef MDNO_SURFACE_H
#define MDNO_SURFACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDNOSA_MAX_POINTS 1024     /* the largest point table: 16 points per lane of a wave */
#define MDNOSA_STAGED_ATOMS 2048   /* the largest N of the staged form (the frame and R lie in LDS as fp64: 32 N bytes) */
#define MDNOSA_TILE 256            /* atoms per tile of the global form */
#define MDNOSA_CHUNK 64            /* neighbours a wave collects before it tests its points against them */

/* Bytes of scratch mdnosa_exposed_points needs for F frames of N atoms and P points in the given form
 * (MDNO_FORECAST_AUTO / _LDS / _TILED of mdno.h).  Neither form needs any today: 0. */
size_t mdnosa_workspace_bytes(int64_t F, int N, int P, int form);

/* frames f32 [F, N, 3], R f64 [N], U f64 [P, 3] -> counts i32 [F, N] by the rule above.  One wave per atom: its lanes
 * stride over j, the neighbours are compacted by the wave-wide ballot into the wave's LDS chunk (d and R_j^2,
 * MDNOSA_CHUNK of them), lane l owns the points l, l + 64, .. with one buried bit each, a buried point is skipped and a
 * wave whose points are all buried stops; chunks repeat until the neighbours are exhausted (their number has no cap).
 * Two forms with the same counts: the STAGED form holds the whole frame and R in LDS as fp64 (N <=
 * MDNOSA_STAGED_ATOMS), the GLOBAL form walks MDNOSA_TILE-atom tiles of the frame from memory, any N.  form:
 * MDNO_FORECAST_AUTO (staged up to MDNOSA_STAGED_ATOMS atoms, global above), _LDS (the staged form; more atoms:
 * MDNO_EUNSUPPORTED) or _TILED (the global form).  MDNO_EINVAL before any device work for a negative size, a form that
 * is none of the three, P outside 1 .. MDNOSA_MAX_POINTS, reach not finite or <= 0, a bad box (the messages of
 * mdno_pbc.h), a workspace smaller than stated, a null pointer where sizes are non-zero; MDNO_EUNSUPPORTED for F above
 * the launch grid (2^31 - 2).  F == 0: returns 0, touches nothing. */
int mdnosa_exposed_points(const float* frames, int64_t F, int N, const double* R, const double* U, int P, const double* box,
                          double reach, int32_t* counts, int form, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_SURFACE_H */
