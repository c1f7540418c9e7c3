/*
 * mdno_train.h — second public header of libmdno.so: training on dense graphs through the factored
 * ("edge moment") formulation of the kernel-integral block (csrc/train_moment.hip).
 * Versioned on its own (mdno_train_abi_version) so that include/mdno.h and its ABI number stay as they are.
 * Conventions as in mdno.h: device pointers owned by the caller, explicit sizes, a workspace sized by the
 * matching *_workspace_bytes function, `stream` a hipStream_t passed as void*, 0 or a negative MDNO_E* code
 * (mdno_last_error() has the message).  Width 64, ker_width a multiple of 128, mean aggregation, fp32 storage.
 *
 * The block:  x_a = relu(conv(x_{a-1})),  a = 1 .. 2*depth, conv1's root / bias for a <= depth and conv2's
 * after, every application with the same edge-MLP; H = relu(L1(relu(L0(edge_attr)))) is the MLP's last hidden
 * activation, kept as the k-tiled fp32 image [ceil(E/128)][ker_width/32][128][32] (element (e, c) at
 * ((e/128)*(k/32) + c/32)*4096 + (e%128)*32 + c%32).  No per-edge 64 x 64 object is formed in either direction.
 */
#ifndef MDNO_TRAIN_H
#define MDNO_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDNO_TRAIN_ABI_VERSION 1

int mdno_train_abi_version(void);

/* Floats of the H image for `num_edges` edges (whole 128-edge tiles). */
size_t mdno_train_moment_h_floats(int64_t num_edges, int ker_width);

/* Forward: the edge-MLP up to H (edge_attr f32 [E, ker_in] in the caller's edge order, perm[p] = the input edge
 * at CSR position p, or NULL; num_edges: the device count; edge_cap = max(E, 1)) and the 2*depth applications.
 * x_stack f32 [2*depth+1, num_rows, 64]: layer 0 given, layers 1 .. 2*depth written.  h_tiled: the H image
 * (mdno_train_moment_h_floats), written for edges < E.  gemm_mode as the inference forward (MDNO_GEMM_*): the
 * rows of x_stack are bitwise what mdno_kernelnn_fwd computes with conv_mode MDNO_CONV_FACTORED. */
size_t mdno_train_moment_fwd_workspace_bytes(int num_rows, int ker_width, int64_t edge_cap, int gemm_mode);
int mdno_train_moment_fwd(const float* edge_attr, const int32_t* perm, const int32_t* num_edges, int64_t edge_cap,
                          int ker_in, int ker_width, int gemm_mode, const float* w0, const float* b0,
                          const float* w1, const float* b1, const float* w2, const float* b2,
                          const int32_t* row_ptr, const int32_t* src, const int32_t* dst, int num_rows,
                          const float* root1, const float* bias1, const float* root2, const float* bias2, int depth,
                          float* x_stack, float* h_tiled, void* workspace, size_t workspace_bytes, void* stream);

/* Backward through the 2*depth applications, given g_out = dLoss/dx_{2*depth} [num_rows, 64], the stack and the H
 * image of the forward, the CSR and the same edges by source (mdno_csr_by_source: srow_ptr, sperm):
 *   gz    [2*depth, num_rows, 64]  (x_a > 0) * dLoss/dx_a per application (operand of mdno_nnconv_bwd_root_pair)
 *   g_in  [num_rows, 64]           dLoss/dx_0
 *   gz2   [num_edges, ker_width]   (H > 0) * dLoss/dH, row-major in CSR edge order (the edge-MLP backward goes on
 *                                  from here with the existing ops)
 *   d_w2  [4096, ker_width], d_b2 [4096]   gradients of the MLP's last layer
 * Per application and per chunk of 512 destinations: S recomputed (K1), dW3R += S^T gs, D = gs W3R^T, then per
 * destination dH += x_src D and the per-edge messages D h_e, gathered by source.  fp32 fmaf chains in fixed
 * orders, no atomics: two calls give the same bits.  gemm_mode selects how S is recomputed (MDNO_GEMM_F32: the
 * fp32 MFMA; otherwise three bf16 planes). */
size_t mdno_train_moment_bwd_workspace_bytes(int num_rows, int ker_width, int64_t num_edges);
int mdno_train_moment_bwd(const float* g_out, const float* x_stack, const float* h_tiled, const int32_t* row_ptr,
                          const int32_t* src, const int32_t* srow_ptr, const int32_t* sperm, int num_rows,
                          int64_t num_edges, int ker_width, int depth, int gemm_mode, const float* w2,
                          const float* b2, const float* root1, const float* root2, float* gz, float* g_in,
                          float* gz2, float* d_w2, float* d_b2, void* workspace, size_t workspace_bytes,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_TRAIN_H */
