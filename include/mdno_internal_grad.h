/*
 * mdno_internal_grad.h — thirteenth public header of libmdno.so: the adjoint of mdnoic_features (include/mdno_internal.h)
 * in its default mode — given the gradient g [F, D] with respect to the features of F frames, the gradient [F, N, 3] with
 * respect to their positions (csrc/internal_grad.hip).  It is what makes
 * forecast.internal_coordinates differentiable and training.StructureLoss a training signal.  Additive, like
 * mdno_internal.h: include/mdno.h, include/mdno_train.h and their version numbers stay as they are, and no launch, captured
 * graph or bit of an existing entry point changes (csrc/internal.hip takes its bond, dot and cross product from
 * csrc/internal_rule.h now, the same text in another file).  This file is part of the library's content hash, and
 * csrc/internal_grad.hip includes it, so a declaration that drifts from its definition does not compile;
 * tests/test_cabi_tables.py holds it to the ctypes table and the exports.  Conventions as in mdno.h: device pointers
 * owned by the caller, explicit sizes, `stream` a hipStream_t passed as void*, 0 or a negative MDNO_E* code
 * (mdno_last_error() has the message), every refusal before any device work.
 *
 * THE PREFIX.  The entry point is named mdnoicg_*, neither mdno_* nor mdnoic_*.  The prefix is kept because the name
 * is ABI; nothing else asks for it (names need only be unique over all headers, which tests/test_cabi_tables.py checks).
 * The function lives in
 * the same library, under the same content hash and the same mdno_abi_version().  The element types, the forms,
 * MDNO_IC_WORKGROUP, MDNO_IC_LDS_ATOMS and MDNO_IC_FRAMES_PER_GROUP(N) are mdno_internal.h's.
 *
 * ARGUMENTS.  frames f32 [F, N, 3]; pairs i32 [P, 2], triples [A, 3], quads [T, 4] (null where the count is 0); box NULL
 * or HOST f64 [3]; g [F, D] row-major of `g_dtype`, D = P + A + 2 T in the forward's column order (P distances, A angle
 * cosines, then (cos, sin) per dihedral), converted to fp64 on load; grad [F, N, 3] of `grad_dtype`.  Radians mode has no
 * gradient here: any bit in `flags` is refused, MDNO_IC_RADIANS with a message that says so.
 *
 * THE RULE.  fp64 on the fp32 coordinates; + - x / sqrt rint only, each rounded once (no FMA contraction), in exactly this
 * order.  v(a->b), p . q and p x q are mdno_internal.h's, minimum image included (rint has zero derivative: the image is
 * held fixed).  Every clamp of the forward is treated as the identity.  -(e) is a sign flip (exact).  Per ITEM (one index
 * tuple; items count the pairs, then the triples, then the quads) and component c:
 *   distance (i, j), incoming g:   v = v(i->j);  r = sqrt(v . v);  s = g / r;  t_c = s * v_c.
 *                 Atom j receives t_c, atom i receives -(t_c).  r == 0: the item contributes nothing (the subgradient, as
 *                 torch.linalg.norm gives it).
 *   angle (i, j, k), incoming g:   u = v(j->i), w = v(j->k);  uu = u . u, ww = w . w;  den = sqrt(uu) * sqrt(ww);
 *                 c = (u . w) / den (unclamped);
 *                 di_c = (w_c / den) - ((c * u_c) / uu);   dk_c = (u_c / den) - ((c * w_c) / ww).
 *                 Atom i receives g * di_c, atom k receives g * dk_c, atom j receives -(g * (di_c + dk_c)).
 *   dihedral (i, j, k, l), incoming (gc, gs) for its (cos, sin) columns:   b1, b2, b3, n1, n2, x, y, h are the forward's;
 *                 bb = b2 . b2, lb = sqrt(bb);   gphi = gs * (x / h) - gc * (y / h);
 *                 fi_c = -((lb / (n1 . n1)) * n1_c);   fl_c = (lb / (n2 . n2)) * n2_c;
 *                 p = (b1 . b2) / bb;   q = (b3 . b2) / bb;
 *                 fj_c = (-fi_c - p * fi_c) + q * fl_c;   fk_c = (-fl_c + p * fi_c) - q * fl_c.
 *                 Atoms i, j, k, l receive gphi * fi_c, gphi * fj_c, gphi * fk_c, gphi * fl_c.
 *                 (cos = x / h and sin = y / h are functions of the angle phi alone, d cos = -sin d phi, d sin = cos d phi:
 *                 gphi is the gradient with respect to phi, and f are the textbook derivatives of phi, IUPAC sign.)
 *   ZERO GRADIENT.  An item whose incoming gradient is exactly zero (+0 or -0; both columns for a dihedral) is skipped, not
 *                 evaluated: a degenerate feature that the caller masked out yields 0, not 0 * NaN.  A NaN g is not zero
 *                 and propagates.
 *   AN INDEX outside 0 .. N - 1 in a tuple: the item contributes nothing and reads nothing.
 *   DEGENERATE GEOMETRY with non-zero g gives NaN or Inf through the arithmetic (0 / 0, x / 0), as the forward gives NaN.
 *   NON-FINITE COORDINATES reach, through the arithmetic, exactly the atoms that share a non-skipped item with them.
 *
 * THE SUM IS A GATHER.  grad[f, a, c] is ONE accumulation chain acc = acc + contribution starting from +0.0, over atom a's
 * incidences in ascending (item, slot) order, slot = the position in the tuple (a tuple that names an atom twice gives it
 * two entries).  One thread owns one (frame, atom); nothing is summed across threads and there are no float atomics.  The
 * bits of grad[f, a, :] depend on frame f, row g[f, :], the index arrays, the box and N alone — not on F, the form, the
 * launch geometry or the run.  f32 output is the fp64 value rounded once.  Every element of grad is written: an atom in no
 * item gets +0.0.
 *
 * THE INCIDENCE TABLE is a CSR by atom that the host builds once per (index set, N): atom_ptr i32 [N + 1], inc i32 [n_inc],
 * inc[e] = item * 4 + slot, ascending within an atom's range atom_ptr[a] .. atom_ptr[a + 1] - 1 (hence P + A + T < 2^29).
 * The kernel does not trust it: an atom's range is clamped into [0, n_inc]; an entry is skipped if its item is >= P + A + T
 * (a negative entry included), its slot is >= the tuple's width, or the tuple's slot does not name this atom.  A wrong
 * table gives wrong numbers, never a read or a write outside the buffers given.
 *
 * FORMS AND GRID.  The forward's two forms.  MDNO_IC_FORM_LDS (N <= MDNO_IC_LDS_ATOMS): a workgroup of MDNO_IC_WORKGROUP
 * threads copies G = MDNO_IC_FRAMES_PER_GROUP(N) consecutive whole frames into LDS as they lie in memory and gathers the
 * coordinates from there; MDNO_IC_FORM_GLOBAL (any N) gathers them from global memory; MDNO_IC_FORM_AUTO: LDS where N
 * allows it.  Both call one arithmetic function.  The grid is (frame groups, atom chunks): a workgroup owns G frames x C
 * consecutive atoms and its threads walk (frame, atom) in strides of the workgroup, the atom fastest (consecutive lanes own
 * consecutive atoms: the staged coordinates 12 bytes apart fall on distinct LDS banks, grad is stored coalesced).  C starts
 * at N and is halved (rounding up) while the grid has fewer than MDNO_ICG_TARGET_GROUPS workgroups and G C exceeds
 * MDNO_ICG_MIN_THREADS: a training batch of 128 frames x 28 atoms runs as 8 x 7 workgroups rather than 8, a long run as one
 * atom chunk per frame group (no frame staged twice).  The bits do not depend on C.
 */
#ifndef MDNO_INTERNAL_GRAD_H
#define MDNO_INTERNAL_GRAD_H

#include <stddef.h>
#include <stdint.h>

#include "mdno_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the item count P + A + T stays below this (an incidence is item * 4 + slot in an int32) */
#define MDNO_ICG_MAX_ITEMS (1 << 29)
/* the atom chunk is halved while the grid has fewer workgroups than this and a workgroup more (frame, atom) than that */
#define MDNO_ICG_TARGET_GROUPS 1024
#define MDNO_ICG_MIN_THREADS 64

/* frames f32 [F, N, 3], pairs i32 [P, 2], triples i32 [A, 3], quads i32 [T, 4], atom_ptr i32 [N + 1], inc i32 [n_inc],
 * g [F, P + A + 2 T] of g_dtype (device), box NULL or HOST f64 [3] -> grad [F, N, 3] of grad_dtype.  MDNO_EINVAL for
 * negative sizes, a g_dtype, a grad_dtype or a form other than mdno_internal.h's, any bit in flags (MDNO_IC_RADIANS: not
 * differentiable here), MDNO_IC_FORM_LDS with N > MDNO_IC_LDS_ATOMS, P + A + T >= MDNO_ICG_MAX_ITEMS, a box entry that is
 * negative or not finite, a null index array whose count is > 0, a null atom_ptr, inc (n_inc > 0), frames, g (D > 0) or
 * grad; MDNO_EUNSUPPORTED where F exceeds the launch grid.  F == 0 or N == 0: returns 0 and touches nothing.  D == 0:
 * zeros grad. */
int mdnoicg_features_bwd(const float* frames, int64_t F, int N, const int32_t* pairs, int P, const int32_t* triples, int A,
                         const int32_t* quads, int T, const int32_t* atom_ptr, const int32_t* inc, int64_t n_inc,
                         const double* box, int flags, const void* g, int g_dtype, void* grad, int grad_dtype, int form,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_INTERNAL_GRAD_H */
