/*
 * mdno_constrain.h — public header of libmdno.so: distance-constraint projection on the device (csrc/constrain.hip,
 * csrc/engine.hip).  The inference-time counterpart of the structure loss: a SHAKE-style sweep that puts
 * every listed pair distance back into its band, for any stack of frames (mdnocst_project) and as an opt-in launch at the
 * end of a rollout step (mdnocst_rollout_plan_set_constraints), so that the frame the next window and the next radius
 * graph read lies on the manifold the truth lives on.  Additive: include/mdno.h, include/mdno_train.h and their version
 * numbers stay as they are, and with no constraints given no launch, captured graph or bit of the library changes.  Every
 * name starts with mdnocst_, the plan's setter included: the prefix is kept because the names are ABI, nothing else asks for
 * it (as mdno_ensemble.h says of mdnoens_).  This file is part of the library's content hash; csrc/constrain.hip
 * and csrc/engine.hip include it, and tests/test_cabi_tables.py holds it to the ctypes table and the exports.
 * Conventions as in mdno.h: device pointers owned by the caller, explicit sizes, `stream` a hipStream_t passed as void*,
 * 0 or a negative MDNO_E* code (mdno_last_error() has the message).
 *
 * THE RULE.  A constraint c is a pair (i, j), i != j, with a band lo_c <= hi_c: both f64, lo >= 0, hi = +inf allowed,
 * lo == hi an equality.  Optional per-atom weights w (f32 [N], finite and >= 0, NULL means 1 everywhere) play the role
 * of inverse masses; w = 0 pins an atom.  All arithmetic is fp64 on the fp32 coordinates with + - x / sqrt rint only,
 * every operation rounded once (the library is built with -ffp-contract=off).  For one constraint on the state x:
 *
 *     r_a  = x_i[a] - x_j[a]             under a box: r_a = r_a - rint(r_a * invL_a) * L_a  (the minimum image of
 *                                        mdno_pbc.h: invL_a = 1.0 / L_a formed once; nothing on an open axis, L_a = 0)
 *     len  = sqrt((r_x*r_x + r_y*r_y) + r_z*r_z)
 *     t    = len < lo ? lo : (len > hi ? hi : len)
 *     SKIP the constraint if: an index is outside [0, N) (nothing is read), len is not finite, len == 0, t == len,
 *                             or w_i + w_j == 0
 *     g    = ((len - t) / len) / (w_i + w_j)
 *     x_i[a] = x_i[a] - (w_i * g) * r_a ;   x_j[a] = x_j[a] + (w_j * g) * r_a          a = x, y, z
 *
 * ORDER.  The host colours the constraints greedily: in list order, each takes the lowest colour that neither of its atoms
 * has yet; it then stable-sorts them by colour into pairs i32 [C, 2], lo f64 [C], hi f64 [C] and
 * colour_ptr i32 [n_colours + 1] (colour k owns constraints colour_ptr[k] .. colour_ptr[k + 1] - 1; colour_ptr[0] = 0,
 * colour_ptr[n_colours] = C).  One SWEEP walks the colours in ascending order; within a colour no two constraints share an
 * atom, so they are applied in parallel and the result does not depend on how.  Per frame:
 *
 *     v = measure()            max over the non-skipped constraints of |len - t|, 0 if there is none
 *     viol_in = v; sweeps = 0
 *     while sweeps < iterations and v > tol:  sweep(); sweeps += 1; v = measure()
 *     viol_out = v
 *
 * The state is widened to fp64 when it is loaded, stays fp64 through every sweep and every measure, and is rounded to
 * fp32 once when it is stored; viol_out is measured on the fp64 state.  A frame already inside every band comes back with
 * the same bits and sweeps = 0; iterations = 0 measures only.  A NaN or Inf coordinate stays on its own atom: every
 * constraint that names the atom is skipped.  A colour table that lies (two constraints of one colour sharing an atom, a
 * colour_ptr that is not ascending within [0, C]) gives unspecified numbers, never an access outside the buffers: entries
 * of colour_ptr are clamped to [0, C] and indices are tested against N before anything is read.  No atomics on floating
 * point values, no dependence on F, on the launch geometry or on graph replay: two calls give the same bits.
 *
 * FORM.  One workgroup of MDNOCST_WORKGROUP threads owns MDNOCST_FRAMES_PER_GROUP(N) whole frames for all sweeps: the
 * frames are staged in LDS as fp64 (24 bytes per atom) and a workgroup barrier separates the colours.  The early exit is
 * per frame, but every barrier is reached by the whole workgroup: a frame that is done idles while its neighbours go on,
 * and the workgroup leaves the loop when none of its frames has work left.  N <= MDNOCST_MAX_ATOMS (the LDS of one compute
 * unit holds 160 KiB); a larger N is MDNO_EINVAL before any device work.
 */
#ifndef MDNO_CONSTRAIN_H
#define MDNO_CONSTRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDNOCST_WORKGROUP 256            /* threads of a workgroup */
#define MDNOCST_MAX_ATOMS 6144           /* the largest N: 6,144 x 24 B = 147,456 B of the 163,840 B of LDS */
#define MDNOCST_GROUP_ATOMS 1024         /* atoms of all the frames one workgroup holds when N is small (24 KiB) */
#define MDNOCST_MAX_GROUP_FRAMES 16      /* and the most frames it holds */
#define MDNOCST_MAX_CONSTRAINTS (1 << 26)
#define MDNOCST_FRAMES_PER_GROUP(N) \
    ((N) <= 0 || MDNOCST_GROUP_ATOMS / (N) < 1 ? 1 : (MDNOCST_GROUP_ATOMS / (N) < MDNOCST_MAX_GROUP_FRAMES ? MDNOCST_GROUP_ATOMS / (N) : MDNOCST_MAX_GROUP_FRAMES))

typedef struct mdno_rollout_plan mdno_rollout_plan;

/* out f32 [F, N, 3] = the projection of in f32 [F, N, 3] (out may be in; otherwise the two must not overlap).  The table:
 * pairs i32 [C, 2], lo and hi f64 [C], colour_ptr i32 [n_colours + 1] and weights f32 [N] (or NULL) are DEVICE arrays,
 * sorted by colour as above; box is a HOST pointer to three doubles (0 = open axis) or NULL.  0 <= C <=
 * MDNOCST_MAX_CONSTRAINTS, 0 <= N <= MDNOCST_MAX_ATOMS, iterations >= 0, tol >= 0 (not NaN).  Per frame: sweeps i32 [F]
 * (or NULL), viol_in and viol_out f64 [F] (or NULL, each).  C = 0: out = in, sweeps = 0, viol = 0; C > 0 needs
 * n_colours >= 1. */
int mdnocst_project(const float* in, float* out, int64_t F, int N, const int32_t* pairs, const double* lo, const double* hi,
                    int64_t C, const int32_t* colour_ptr, int n_colours, const float* weights, const double* box,
                    int iterations, double tol, int32_t* sweeps, double* viol_in, double* viol_out, void* stream);

/* Constrained rollout: from the next mdno_rollout_plan_run on, the frame a step produces is projected where it lies — after
 * the noise launch of mdno_rollout_plan_set_noise, before anything else reads it: the stored frame, the next windows and
 * the next radius graph all see the projected frame.  The step is the one the noise addresses, *t_dev - 1 (the absolute
 * step number, whatever launched it); the box is the plan's own (mdno_rollout_plan_set_box, before or after this call: either
 * setter captures the step as the plan then is).  The table (device arrays as above, N = the plan's) must stay valid as long as the plan.
 * sweeps i32, viol_in and viol_out f64 [max_steps, M] are caller-owned (or NULL, each): row `step` is written by that step.
 * Valid before the first mdno_rollout_plan_run after the plan was created (or its trajectory reset); a plan created with
 * use_graph re-captures its steps on the stream it was created with, exactly as set_noise and set_box do.  C = 0 or a NULL
 * table restores the plain step: the launch sequence and the captured graph of a plan that never had constraints. */
int mdnocst_rollout_plan_set_constraints(mdno_rollout_plan* plan, const int32_t* pairs, const double* lo, const double* hi,
                                         int64_t C, const int32_t* colour_ptr, int n_colours, const float* weights,
                                         int iterations, double tol, int32_t* sweeps, double* viol_in, double* viol_out);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_CONSTRAIN_H */
