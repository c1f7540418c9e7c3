/*
 * mdno_unroll.h — fourth public header of libmdno.so: gradients with respect to the model's INPUTS (window frames and
 * edge attributes) and the pieces an unrolled training step needs (csrc/input_grad.hip, csrc/train_nodes.hip;
 * DESIGN.md §4.11).  Additive, like mdno_noise.h: include/mdno.h, include/mdno_train.h and their version numbers stay
 * as they are; this file is part of the library's content hash (and csrc/input_grad.hip and csrc/train_nodes.hip
 * include it, so a declaration that drifts from its definition does not compile; tests/test_cabi_tables.py holds it
 * to the ctypes table and the exports; the entries that write caller memory have their guard-band table in
 * tests/test_gpu_unroll.py).
 * Conventions as in mdno.h: device pointers owned by the caller, explicit sizes, `stream` a hipStream_t passed as
 * void*, 0 or a negative MDNO_E* code (mdno_last_error() has the message), arguments validated before any device
 * work.  All storage fp32.  Fixed summation orders, no atomics: two calls give the same bits.
 */
#ifndef MDNO_UNROLL_H
#define MDNO_UNROLL_H

#include <stddef.h>
#include <stdint.h>

#include "mdno.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Input gradient of the edge-MLP's first layer: d_edge_attr f32 [edge_cap, ker_in] = gz1 . W0 for
 *   gz1 f32 [edge_cap, ker_width]  the masked gradient at the first hidden layer ((h1 > 0) * dLoss/dh1), CSR edge order
 *   w0  f32 [ker_width, ker_in]    the layer's weight (torch Linear layout)
 * Rows 0 .. min(*num_edges, edge_cap) - 1 are written (num_edges i32 [1], device); rows past the count stay
 * untouched.  ker_in 1..8, any ker_width >= 1; edge_cap = 0 is legal (nothing is launched).  One pass over gz1:
 * a row's columns are added per lane in ascending order (lane l owns columns 4 l .. 4 l + 3 of every 256 where
 * ker_width % 4 == 0, column l of every 64 otherwise), the 64 lanes of the wave by a fixed tree. */
int mdno_edge_mlp_input_bwd(const float* gz1, const float* w0, const int32_t* num_edges, int64_t edge_cap,
                            int ker_width, int ker_in, float* d_edge_attr, void* stream);

/* Edge attributes as a function of positions: for the edge at CSR position p,
 *   edge_attr[p] = [pos[src[p]], pos[dst[p]]]   (f32 [edge_cap, 6]; pos f32 [num_rows, 3])
 * — what the forward forms from edge_pos for the same edge (mdno_edge_mlp_fwd / mdno_kernelnn_fwd without edge_attr).
 * Rows 0 .. min(*num_edges, edge_cap) - 1 are written; an endpoint outside [0, num_rows) is clamped into it. */
int mdno_edge_attr_from_pos(const float* pos, const int32_t* src, const int32_t* dst, const int32_t* num_edges,
                            int64_t edge_cap, int num_rows, float* edge_attr, void* stream);

/* Its exact adjoint: d_pos f32 [num_rows, 3], every row written,
 *   d_pos[a] = sum_{p: src[p] = a} d_edge_attr[p][0:3] + sum_{p: dst[p] = a} d_edge_attr[p][3:6]
 * the first sum over atom a's out-edges in the order of the by-source list (mdno_csr_by_source: row_ptr_s [R + 1],
 * eid_s [E] = CSR position of the edge: ascending p), the second over its in-edges row_ptr[a] .. row_ptr[a + 1] - 1
 * of the destination-sorted CSR in ascending p; the two partial sums are then added.  Self-loops, repeated pairs,
 * directed lists and atoms without in- or out-edges need nothing special.  The edge count is row_ptr[num_rows]. */
int mdno_edge_attr_pos_bwd(const float* d_edge_attr, const int32_t* row_ptr, const int32_t* row_ptr_s,
                           const int32_t* eid_s, int num_rows, float* d_pos, void* stream);

/* mdno_node_prologue_bwd (mdno.h; same arguments, same workspace size, the same parameter gradients bit for bit)
 * that also writes d_frames f32 [W, M, N, 3] = dLoss/dframes: W_ih^T . dpre_t of every LSTM step, or — notebook-era
 * model without LSTM — the coordinate part of d feat for the last frame and 0 for the frames before it. */
int mdno_node_prologue_bwd_frames(const mdno_kernelnn_params* p, const float* frames, int M, int W, int N,
                                  const int64_t* x_aminoacid, int aa_per_member, const float* x0, const float* g0,
                                  float* d_lstm, float* d_emb, float* d_fc1_w, float* d_fc1_b, float* d_frames,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* Targets of an unrolled training step: y f32 [K, B * N, 3], step k of sample b = frame
 * meta[b] + W + horizon - 1 + k of pos f32 [num_frames, N, 3] (meta: the table of mdno_collate_samples, whose first
 * B entries are the samples' first window frames).  A frame outside [0, num_frames) is not read: those rows of y
 * are left as they are (the caller checks its indices on the host, where it owns the table). */
int mdno_collate_targets(const float* pos, int64_t num_frames, const int64_t* meta, int B, int N, int W, int horizon,
                         int K, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_UNROLL_H */
