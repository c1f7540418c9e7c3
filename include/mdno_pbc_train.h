/*
 * mdno_pbc_train.h — public header of libmdno.so for TRAINING under an orthorhombic periodic box (csrc/pbc_train.hip;
 * DESIGN.md §4.12 "Training under a box").  Additive: include/mdno.h, include/mdno_train.h, include/mdno_pbc.h and the
 * two version numbers stay as they are, and with no box given every launch, captured graph and bit of the library is
 * what it was.  This file is part of the library's content hash, and csrc/pbc_train.hip includes it, so a declaration
 * that drifts from its definition does not compile; tests/test_cabi_tables.py holds it to the ctypes table
 * (_lib.PBC_TRAIN_SIGNATURES) and the exports.  The name starts with mdnopbt_, not mdno_: the prefix is kept because the
 * name is ABI, nothing else asks for it.  The guard-band table of this header is in
 * tests/test_gpu_pbc_train.py.
 * Conventions as in mdno.h: device pointers owned by the caller, explicit sizes, `stream` a hipStream_t passed as
 * void*, 0 or a negative MDNO_E* code (mdno_last_error() has the message), arguments validated before any device work.
 *
 * THE RULE is include/mdno_pbc.h's: box = (Lx, Ly, Lz), HOST f64 [3], L == 0 an open axis, every periodic axis
 * L >= 2 * cutoff; k = rint(d / L) round-half-even in fp64 on the fp32 coordinates, no FMA contraction.
 *
 * THE ADJOINT.  The shift k * L of an edge is a constant of that edge: k is piecewise constant in the positions, and
 * no gradient goes through it, just as none goes through the topology.  So
 *     d edge_attr[p][0:3] / d pos[src[p]] = I,   d edge_attr[p][3:6] / d pos[dst[p]] = I
 * exactly as without a box, and the exact adjoint of mdnopbt_edge_attr_from_pos is mdno_edge_attr_pos_bwd
 * (include/mdno_unroll.h) as it is.  There is no backward entry here.
 */
#ifndef MDNO_PBC_TRAIN_H
#define MDNO_PBC_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Edge attributes as a function of positions under a box: for the edge at CSR position p, s = src[p], d = dst[p],
 *   edge_attr[p] = [ (float)((double)x_s[a] - k_a * L[a]) for a in 0..2,  x_d[0..2] ]      (f32 [edge_cap, 6])
 * with k_a = rint(((double)x_s[a] - (double)x_d[a]) / L[a]) (0 on an open axis): the source's image next to the
 * destination, then the destination as stored (pos f32 [num_rows, 3]).  Rows 0 .. min(*num_edges, edge_cap) - 1 are
 * written (num_edges i32 [1], device); rows past the count stay untouched; an endpoint outside [0, num_rows) is
 * clamped into it; edge_cap == 0 launches nothing.  edge_attr must be 8-byte aligned.  box == NULL, or a box that
 * mdno_radius_graph_pbc refuses for this cutoff, is MDNO_EINVAL.  With an all-zero box the rows are bit-identical to
 * mdno_edge_attr_from_pos; for a graph made by mdno_radius_graph_pbc on the same pos, cutoff and box they are
 * bit-identical to the attribute rows that call wrote (the same inputs, the same rule).  The list itself may be any
 * directed list: pairs beyond the cutoff, self-loops and repeated pairs need nothing special. */
int mdnopbt_edge_attr_from_pos(const float* pos, const int32_t* src, const int32_t* dst, const int32_t* num_edges,
                               int64_t edge_cap, int num_rows, double cutoff, const double* box, float* edge_attr,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_PBC_TRAIN_H */
