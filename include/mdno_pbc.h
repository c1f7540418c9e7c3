/*
 * mdno_pbc.h — fifth public header of libmdno.so: orthorhombic periodic boundary conditions (csrc/pbc.h, csrc/pbc.hip;
 * DESIGN.md §4.12).  Additive: include/mdno.h, include/mdno_train.h and their version numbers stay as they are, and
 * with no box given every launch, captured graph and bit of the library is what it was.  (A header of its own, like
 * mdno_noise.h: the entry points of mdno.h that write caller memory are pinned, name by name, by that header's
 * guard-band table in tests/test_gpu_bounds.py; these have their table in tests/test_gpu_pbc.py.  This file is part of
 * the library's content hash, and csrc/pbc.hip, csrc/engine.hip and csrc/forecast.hip include it, so a declaration that
 * drifts from its definition does not compile; tests/test_cabi_tables.py holds it to the ctypes table and the exports.)
 * Conventions as in mdno.h: device pointers owned by the caller, explicit sizes, `stream` a hipStream_t passed as
 * void*, 0 or a negative MDNO_E* code (mdno_last_error() has the message).
 *
 * THE RULE.  box = (Lx, Ly, Lz), HOST f64 [3], one box for all members of a call.  L == 0: that axis is open.  Every
 * periodic axis needs L >= 2 * cutoff (a pair then has at most one image inside the strict cutoff); a negative, NaN or
 * Inf entry or a shorter periodic axis is MDNO_EINVAL before any device work.  For destination i, source j and axis a,
 * all in fp64 on the fp32 coordinates, with invL = 1.0 / L formed once on the host:
 *     d  = (double)x_j - (double)x_i
 *     k  = rint(d * invL)        (round-half-even; k = 0 on an open axis)
 *     d' = d - k * L
 * and the pair is kept iff sqrt((dx'*dx' + dy'*dy') + dz'*dz') < cutoff: strict, self-loops kept, the summation order
 * of mdno_radius_graph_csr, no FMA contraction.  rint is odd, so the graph is symmetric.  The edge attribute row is
 *     [ (float)((double)x_j - k * L) for the three axes,  x_i ]
 * — the source's image next to the destination, then the destination as stored: the reference's [A, B] with A moved
 * to the image that was tested.  With a box so large that no pair wraps, k = 0 everywhere and the CSR and the
 * attributes are bit-identical to the open graph and to cat(pos[src], pos[dst]).
 * Frames are never wrapped: coordinates stay continuous in time and the model sees them as stored.  (fp32 coordinates
 * of atoms that have drifted many box lengths lose precision: at |x| = 1000 A one ulp is 6e-5 A.)
 */
#ifndef MDNO_PBC_H
#define MDNO_PBC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mdno_rollout_plan mdno_rollout_plan;

/* Periodic radius graph of pos f32 [M, N, 3] -> destination-sorted CSR with sources ascending within a row, exactly
 * as mdno_radius_graph_csr (row_ptr i32 [M*N + 1], src i32 [edge_cap], dst i32 [edge_cap] or NULL, num_edges i32 [1],
 * status i32 [1] or NULL; edge_cap >= M*N), plus edge_attr f32 [edge_cap, 6], the attribute row of every edge beside
 * src[p] (NULL: topology only).  More than edge_cap edges: MDNO_STATUS_EDGE_OVERFLOW is set in *status, the list is
 * truncated, nothing is written at or past edge_cap.  Brute force (N^2 pair tests per member, one wave per
 * destination row) at every size. */
int mdno_radius_graph_pbc(const float* pos, int M, int N, double cutoff, const double* box, int32_t* row_ptr,
                          int32_t* src, int32_t* dst, float* edge_attr, int64_t edge_cap, int32_t* num_edges,
                          int32_t* status, void* stream);

/* Periodic rollout: from the next mdno_rollout_plan_run on, every step builds the periodic graph of its newest frame
 * (cutoff = the plan's threshold) into the plan's CSR and into edge_attr f32 [edge_cap, 6] (caller-owned, valid as long
 * as the plan), and the forward reads edge_attr as its edge source.  The plan's workspace and conv formulation stay as
 * created; the model must have ker_in == 6.  Valid before the first mdno_rollout_plan_run after the plan was created
 * (or its trajectory reset); a plan created with use_graph re-captures its steps on the stream it was created with.
 * box == NULL or all zero restores the plain step: the launch sequence and the captured graph of a plan that never had
 * a box (edge_attr may then be NULL).  Composes with mdno_rollout_plan_set_noise: the new frame is perturbed after the
 * step, as without a box. */
int mdno_rollout_plan_set_box(mdno_rollout_plan* plan, const double* box, float* edge_attr);

/* mdno_contact_maps / mdno_forecast_score (mdno.h) with contacts counted under the rule above: the same kernels on the
 * periodic pair test.  mse, rmsd and first_nonfinite do not depend on the box.  Workspace:
 * mdno_forecast_score_workspace_bytes.  box == NULL: MDNO_EINVAL. */
int mdno_forecast_score_pbc(const float* frames, const float* truth, int truth_per_member, int S, int M, int N,
                            double cutoff, const double* box, double* mse, double* rmsd, int64_t* counts,
                            int32_t* first_nonfinite, int form, void* workspace, size_t workspace_bytes, void* stream);
int mdno_contact_maps_pbc(const float* frames, int64_t F, int N, double cutoff, const double* box, uint8_t* maps,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_PBC_H */
