// Backward of a stand-alone NNConv_old (graph_kernel.py:125-214, with torch_geometric's MessagePassing.propagate) and of a
// DenseNet (:217-242) for any channel counts and every aggregation the forward has — what autograd gives the reference's
// users when they build their own models from these two classes.  The model's own training path (train.hip) covers
// KernelNN's 64x64 mean convs only.
//
// Conv forward, destination-sorted (CSR) edge order:  y[t] = A_{e->t}(m_e) + x[t].root + bias,  m_e = x[src e] . W_e,
// W_e [Cin, Cout] row-major.  Given g = dL/dy [R, Cout]:
//     gm_e   = dL/dm_e:  add  g[dst e];  mean  g[dst e] / max(deg, 1);
//                        max  g[t][o] / ties for the edges whose message reaches the row's maximum in channel o, 0 for
//                             the others (torch's scatter_reduce "amax" backward: ties share evenly)    (nnconv_msg_grad)
//     dx[s]  = g[s].root^T + sum_{e: src e = s} W_e . gm_e                                          (nnconv_bwd_x_edges)
//     dW_e   = x[src e] (x) gm_e                                                                    (nnconv_bwd_we_edges)
// d root = x^T g and d bias = colsum(g) are mdno_gemm_atb / mdno_colsum; the DenseNet's products are mdno_linear_fwd and
// mdno_gemm_atb, its ReLU masks relu_mask_bwd below.  No atomics: every sum runs in one fixed order (bitwise
// reproducible); the edge count is read from row_ptr[num_rows] on the device, so nothing here waits for the host.
#include <cmath>

#include "kernels.h"

namespace mdno {
namespace {

constexpr int kGridStrideBlocks = 4096;     // edge-parallel kernels: a fixed grid walks all edges

// gm[p][o] for add / mean: one wave per destination row, lanes along the output channels (coalesced rows of gm)
__global__ __launch_bounds__(256) void msg_grad_sum_kernel(const int* __restrict__ row_ptr, const float* __restrict__ g,
                                                           float* __restrict__ gm, int num_rows, int Cout, int mean) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= num_rows) return;
    const int beg = row_ptr[row], end = row_ptr[row + 1];
    const float d = mean ? (float)(end - beg > 1 ? end - beg : 1) : 1.f;
    for (int o = lane; o < Cout; o += 64) {
        const float v = g[(size_t)row * Cout + o] / d;
        for (int p = beg; p < end; ++p) gm[(size_t)p * Cout + o] = v;
    }
}

// m[p][o] = sum_i x[src p][i] * W_e[p][i][o], i ascending (the order of nnconv.hip's generic forward kernel): one wave
// per edge, lanes along the output channels
__global__ __launch_bounds__(256) void msg_values_kernel(const float* __restrict__ x, const int* __restrict__ row_ptr,
                                                         const int* __restrict__ src, const float* __restrict__ w_e,
                                                         float* __restrict__ m, int num_rows, int Cin, int Cout) {
    const long long E = row_ptr[num_rows];
    const int lane = threadIdx.x & 63;
    const size_t cc = (size_t)Cin * Cout;
    for (long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); p < E; p += (long long)gridDim.x * 4) {
        const float* xs = x + (size_t)src[p] * Cin;
        const float* w = w_e + (size_t)p * cc;
        for (int o = lane; o < Cout; o += 64) {
            float s = 0.f;
#pragma unroll 8
            for (int i = 0; i < Cin; ++i) s = fmaf(xs[i], w[(size_t)i * Cout + o], s);
            m[(size_t)p * Cout + o] = s;
        }
    }
}

// max: gm holds the messages on entry.  Per row and channel: the maximum and how many edges reach it (edges in CSR
// order), then each of those edges gets g / ties and every other edge 0 — in place
__global__ __launch_bounds__(256) void msg_grad_max_kernel(const int* __restrict__ row_ptr, const float* __restrict__ g,
                                                           float* __restrict__ gm, int num_rows, int Cout) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= num_rows) return;
    const int beg = row_ptr[row], end = row_ptr[row + 1];
    if (beg >= end) return;
    for (int o = lane; o < Cout; o += 64) {
        float mx = gm[(size_t)beg * Cout + o];
        int ties = 1;
        for (int p = beg + 1; p < end; ++p) {
            const float v = gm[(size_t)p * Cout + o];
            if (v > mx) {
                mx = v;
                ties = 1;
            } else if (v == mx) {
                ++ties;
            }
        }
        const float share = g[(size_t)row * Cout + o] / (float)ties;
        for (int p = beg; p < end; ++p) {
            float* at = gm + (size_t)p * Cout + o;
            *at = *at == mx ? share : 0.f;
        }
    }
}

// dx[s][i] = sum_o (sum_{e: src e = s} W_e[i][o] gm_e[o] + root[i][o] g[s][o]): one workgroup per source row.  The
// workgroup holds up to kChunk elements of the [Cin, Cout] product in registers (thread t: elements 4t + 1024j + u with
// VEC, t + 256j without), adds the row's out-edges in their fixed order and the root term last, then sums every row i
// over o in LDS, o ascending.  Chunks are whole rows of W_e (kChunk / Cout of them).
constexpr int kChunk = 4096;

template <bool VEC>
__global__ __launch_bounds__(256) void bwd_x_edges_kernel(const float* __restrict__ gm, const float* __restrict__ g,
                                                          const int* __restrict__ row_ptr_s, const int* __restrict__ eid_s,
                                                          const float* __restrict__ w_e, const float* __restrict__ root,
                                                          float* __restrict__ dx, int num_rows, int Cin, int Cout) {
    __shared__ float red[kChunk];
    const int row = blockIdx.x;
    if (row >= num_rows) return;
    const int tid = threadIdx.x;
    const int beg = row_ptr_s[row], end = row_ptr_s[row + 1];
    const size_t cc = (size_t)Cin * Cout;
    const int rows_per_chunk = kChunk / Cout;
    for (int i0 = 0; i0 < Cin; i0 += rows_per_chunk) {
        const int i1 = i0 + rows_per_chunk < Cin ? i0 + rows_per_chunk : Cin;
        const int n = (i1 - i0) * Cout;                 // elements in this chunk
        const size_t c0 = (size_t)i0 * Cout;
        float acc[16];
        int oo[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            acc[j] = 0.f;
            const int k = VEC ? 4 * tid + 1024 * (j >> 2) + (j & 3) : tid + 256 * j;
            oo[j] = k < n ? k % Cout : -1;
        }
        for (int p = beg; p < end; ++p) {
            const size_t e = (size_t)eid_s[p];
            const float* wrow = w_e + e * cc + c0;
            const float* grow = gm + e * Cout;
            if (VEC) {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int k = 4 * tid + 1024 * jj;
                    if (k < n) {
                        const float4 w = *reinterpret_cast<const float4*>(wrow + k);
                        const float4 gv = *reinterpret_cast<const float4*>(grow + oo[4 * jj]);
                        acc[4 * jj + 0] = fmaf(w.x, gv.x, acc[4 * jj + 0]);
                        acc[4 * jj + 1] = fmaf(w.y, gv.y, acc[4 * jj + 1]);
                        acc[4 * jj + 2] = fmaf(w.z, gv.z, acc[4 * jj + 2]);
                        acc[4 * jj + 3] = fmaf(w.w, gv.w, acc[4 * jj + 3]);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (oo[j] >= 0) acc[j] = fmaf(wrow[tid + 256 * j], grow[oo[j]], acc[j]);
            }
        }
        if (root != nullptr) {
            const float* rrow = root + c0;
            const float* grow = g + (size_t)row * Cout;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int k = VEC ? 4 * tid + 1024 * (j >> 2) + (j & 3) : tid + 256 * j;
                if (oo[j] >= 0) acc[j] = fmaf(rrow[k], grow[oo[j]], acc[j]);
            }
        }
        __syncthreads();            // (the previous chunk's row sums have read red)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = VEC ? 4 * tid + 1024 * (j >> 2) + (j & 3) : tid + 256 * j;
            if (oo[j] >= 0) red[k] = acc[j];
        }
        __syncthreads();
        for (int il = tid; il < i1 - i0; il += 256) {
            float s = 0.f;
            for (int o = 0; o < Cout; ++o) s += red[il * Cout + o];
            dx[(size_t)row * Cin + i0 + il] = s;
        }
    }
}

// dW_e[p][i][o] = x[src p][i] * gm[p][o]: a pure stream of E*Cin*Cout*4 bytes out.  Thread slots are fixed elements of the
// [Cin, Cout] block (4 adjacent ones with VEC: one 16-B store), so (i, o) is computed once per slot; the workgroups walk
// the edges with a fixed grid stride.
template <bool VEC>
__global__ __launch_bounds__(256) void bwd_we_edges_kernel(const float* __restrict__ x, const float* __restrict__ gm,
                                                           const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                           float* __restrict__ d_we, int num_rows, int Cin, int Cout) {
    const long long E = row_ptr[num_rows];
    const int cc = Cin * Cout;
    const int step = VEC ? 1024 : 256;
    for (int k = VEC ? 4 * threadIdx.x : threadIdx.x; k < cc; k += step) {
        const int i = k / Cout, o = k - i * Cout;
        for (long long p = blockIdx.x; p < E; p += gridDim.x) {
            const float xv = x[(size_t)src[p] * Cin + i];
            float* out = d_we + (size_t)p * cc + k;
            if (VEC) {
                const float4 gv = *reinterpret_cast<const float4*>(gm + (size_t)p * Cout + o);
                *reinterpret_cast<float4*>(out) = make_float4(xv * gv.x, xv * gv.y, xv * gv.z, xv * gv.w);
            } else {
                *out = xv * gm[(size_t)p * Cout + o];
            }
        }
    }
}

__global__ __launch_bounds__(256) void scale_rows_kernel(const float* __restrict__ a, const float* __restrict__ scale,
                                                         float* __restrict__ out, long long rows, int n) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= rows * n) return;
    out[id] = a[id] * scale[id / n];
}

// torch's ReLU backward (threshold_backward on the output): g where y > 0, else 0 — any element count
__global__ __launch_bounds__(256) void relu_mask_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                            float* __restrict__ out, long long count) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= count) return;
    out[id] = y[id] > 0.f ? g[id] : 0.f;
}

__global__ __launch_bounds__(256) void scatter_rows_kernel(const float* __restrict__ in, const int* __restrict__ perm,
                                                           long long rows, int width, float* __restrict__ out) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= rows * width) return;
    const long long p = id / width;
    out[(size_t)perm[p] * width + (int)(id - p * width)] = in[id];
}

bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" int mdno_nnconv_msg_grad(const float* x, const int32_t* row_ptr, const int32_t* src, int num_rows,
                                    const float* w_e, const float* g, int Cin, int Cout, int aggr, float* gm,
                                    void* stream) {
    MDNO_REQUIRE(row_ptr && g && gm && num_rows > 0 && Cin > 0 && Cout > 0, MDNO_EINVAL,
                 "mdno_nnconv_msg_grad: bad arguments");
    MDNO_REQUIRE(aggr == MDNO_AGGR_ADD || aggr == MDNO_AGGR_MEAN || aggr == MDNO_AGGR_MAX, MDNO_EUNSUPPORTED,
                 "mdno_nnconv_msg_grad: aggr %d (add, mean, max)", aggr);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 rows_grid((unsigned)((num_rows + 3) / 4));
    if (aggr == MDNO_AGGR_MAX) {
        MDNO_REQUIRE(x && src && w_e, MDNO_EINVAL, "mdno_nnconv_msg_grad: max needs x, src and w_e");
        hipLaunchKernelGGL(msg_values_kernel, dim3(kGridStrideBlocks), dim3(256), 0, s, x, row_ptr, src, w_e, gm, num_rows,
                           Cin, Cout);
        hipLaunchKernelGGL(msg_grad_max_kernel, rows_grid, dim3(256), 0, s, row_ptr, g, gm, num_rows, Cout);
    } else {
        hipLaunchKernelGGL(msg_grad_sum_kernel, rows_grid, dim3(256), 0, s, row_ptr, g, gm, num_rows, Cout,
                           aggr == MDNO_AGGR_MEAN ? 1 : 0);
    }
    return check_launch("mdno_nnconv_msg_grad");
}

extern "C" int mdno_nnconv_bwd_x_edges(const float* gm, const float* g, const int32_t* row_ptr_s, const int32_t* eid_s,
                                       int num_rows, const float* w_e, const float* root, int Cin, int Cout, float* dx,
                                       void* stream) {
    MDNO_REQUIRE(gm && row_ptr_s && eid_s && w_e && dx && num_rows > 0 && Cin > 0 && Cout > 0, MDNO_EINVAL,
                 "mdno_nnconv_bwd_x_edges: bad arguments");
    MDNO_REQUIRE(root == nullptr || g != nullptr, MDNO_EINVAL, "mdno_nnconv_bwd_x_edges: root needs g");
    MDNO_REQUIRE(Cout <= kChunk, MDNO_EUNSUPPORTED, "mdno_nnconv_bwd_x_edges: Cout %d > %d", Cout, kChunk);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool vec = Cout % 4 == 0 && aligned16(w_e, gm, root);
    if (vec)
        hipLaunchKernelGGL(bwd_x_edges_kernel<true>, dim3(num_rows), dim3(256), 0, s, gm, g, row_ptr_s, eid_s, w_e, root, dx,
                           num_rows, Cin, Cout);
    else
        hipLaunchKernelGGL(bwd_x_edges_kernel<false>, dim3(num_rows), dim3(256), 0, s, gm, g, row_ptr_s, eid_s, w_e, root,
                           dx, num_rows, Cin, Cout);
    return check_launch("mdno_nnconv_bwd_x_edges");
}

extern "C" int mdno_nnconv_bwd_we_edges(const float* x, const float* gm, const int32_t* row_ptr, const int32_t* src,
                                        int num_rows, int Cin, int Cout, float* d_we, void* stream) {
    MDNO_REQUIRE(x && gm && row_ptr && src && d_we && num_rows > 0 && Cin > 0 && Cout > 0, MDNO_EINVAL,
                 "mdno_nnconv_bwd_we_edges: bad arguments");
    MDNO_REQUIRE((long long)Cin * Cout < (1ll << 30), MDNO_EUNSUPPORTED, "mdno_nnconv_bwd_we_edges: Cin*Cout too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (Cout % 4 == 0 && aligned16(gm, d_we))
        hipLaunchKernelGGL(bwd_we_edges_kernel<true>, dim3(kGridStrideBlocks), dim3(256), 0, s, x, gm, row_ptr, src, d_we,
                           num_rows, Cin, Cout);
    else
        hipLaunchKernelGGL(bwd_we_edges_kernel<false>, dim3(kGridStrideBlocks), dim3(256), 0, s, x, gm, row_ptr, src, d_we,
                           num_rows, Cin, Cout);
    return check_launch("mdno_nnconv_bwd_we_edges");
}

extern "C" int mdno_scale_rows(const float* a, const float* scale, int64_t rows, int n, float* out, void* stream) {
    MDNO_REQUIRE(a && scale && out && rows > 0 && n > 0, MDNO_EINVAL, "mdno_scale_rows: bad arguments");
    const long long count = (long long)rows * n;
    hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a, scale, out, (long long)rows, n);
    return check_launch("mdno_scale_rows");
}

extern "C" int mdno_relu_mask_bwd(const float* g, const float* y, int64_t count, float* out, void* stream) {
    MDNO_REQUIRE(count >= 0, MDNO_EINVAL, "mdno_relu_mask_bwd: count %lld", (long long)count);
    if (count == 0) return MDNO_OK;
    MDNO_REQUIRE(g && y && out, MDNO_EINVAL, "mdno_relu_mask_bwd: null pointer");
    hipLaunchKernelGGL(relu_mask_bwd_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), g, y, out, (long long)count);
    return check_launch("mdno_relu_mask_bwd");
}

extern "C" int mdno_scatter_rows(const float* in, const int32_t* perm, int64_t rows, int width, float* out, void* stream) {
    MDNO_REQUIRE(rows >= 0 && width > 0, MDNO_EINVAL, "mdno_scatter_rows: rows=%lld width=%d", (long long)rows, width);
    if (rows == 0) return MDNO_OK;
    MDNO_REQUIRE(in && perm && out && in != out, MDNO_EINVAL, "mdno_scatter_rows: null pointer (or in == out)");
    const long long n = (long long)rows * width;
    hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), in, perm, (long long)rows, width, out);
    return check_launch("mdno_scatter_rows");
}
