// Training through the factored conv (include/mdno_train.h; the forward is moment.hip's K1/K2/K3 as it stands).
// Backward of one application y = relu(z / max(deg, 1) + x root + bias), z_t = W3R^T [S_t; s0_t], given g = dLoss/dy:
//     gz_t = (y_t > 0) g_t,  gs_t = gz_t / max(deg_t, 1)
//     dW3R[kappa][o] += sum_t S_t[kappa] gs_t[o]                    (tm_dw3r_kernel: S recomputed per chunk by K1)
//     D_t[kappa]      = sum_o W3R[kappa][o] gs_t[o]                  (tm_d_kernel: an image of S's shape; kappa >= 64 k: d0_t)
//     dH_e[c]        += sum_i x_src(e)[i] D_t[i k + c]               (tm_edge_kernel, t = destination of e)
//     m_e[i]          = sum_c D_t[i k + c] h_e[c] + d0_t[i]          (tm_edge_kernel: partials per 256 hidden units)
//     dx_j[i]         = sum_{e: src(e) = j} m_e[i] + sum_o root[i][o] gz_j[o]      (tm_gather_kernel, by source)
// All products are fp32 fmaf chains in a fixed order; every output element has one owner (dW3R and dH are added in
// place across chunks and applications by that owner, launches in stream order): no atomics, same bits every run.
// S is not kept between forward and backward (R 64 k 4 B per application): K1 runs again per chunk.
#include "kernels.h"
#include "moment_layout.h"
#include "../../include/mdno_train.h"

namespace mdno {
namespace {

__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// gz = (y > 0) g, gs = gz / max(deg, 1): one float4 per thread
__global__ __launch_bounds__(256) void tm_mask_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                      const int* __restrict__ row_ptr, int num_rows,
                                                      float* __restrict__ gz, float* __restrict__ gs) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)num_rows * 16) return;
    const int r = (int)(id >> 4);
    const float4 gv = reinterpret_cast<const float4*>(g)[id], yv = reinterpret_cast<const float4*>(y)[id];
    const int deg = row_ptr[r + 1] - row_ptr[r];
    const float d = (float)(deg > 1 ? deg : 1);
    const float4 z = make_float4(yv.x > 0.f ? gv.x : 0.f, yv.y > 0.f ? gv.y : 0.f, yv.z > 0.f ? gv.z : 0.f,
                                 yv.w > 0.f ? gv.w : 0.f);
    reinterpret_cast<float4*>(gz)[id] = z;
    reinterpret_cast<float4*>(gs)[id] = make_float4(z.x / d, z.y / d, z.z / d, z.w / d);
}

constexpr int TM_GLD = 65;      // LDS row of 64 gs values + 1: rows fall into different banks

// rows rb .. rb + 127 of the chunk's gs (zeros past the chunk's last destination) -> Gs[128][TM_GLD]
__device__ __forceinline__ void tm_stage_gs(const float* __restrict__ gs, int row0, int n, float* __restrict__ Gs) {
    for (int u = threadIdx.x; u < 128 * 16; u += 256) {
        const int row = u >> 4, q = u & 15;
        const float4 v = row < n ? *reinterpret_cast<const float4*>(gs + (size_t)(row0 + row) * 64 + 4 * q) : f4zero();
        float* d = Gs + row * TM_GLD + 4 * q;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
}

// dW3R[kt][o][kl] += sum over the chunk's destinations r of gs[r][o] * S[r][kt*32 + kl], in destination order.
// Workgroup = one k-tile of W3R (64 o x 32 kappa); thread (o, 8 kappa) owns its 8 sums.
__global__ __launch_bounds__(256) void tm_dw3r_kernel(const float* __restrict__ S, const float* __restrict__ gs,
                                                      float* __restrict__ dw3r, int nkt, int r0, int cnt) {
    __shared__ __attribute__((aligned(16))) float Ss[128 * 32];
    __shared__ float Gs[128 * TM_GLD];
    const int kt = blockIdx.x, tid = threadIdx.x;
    const int o = tid >> 2, kl0 = (tid & 3) * 8;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int rb = 0; rb < cnt; rb += 128) {
        const int n = cnt - rb < 128 ? cnt - rb : 128;
        const float4* St = reinterpret_cast<const float4*>(S + ((size_t)(rb >> 7) * nkt + kt) * 4096);
        __syncthreads();
        for (int u = tid; u < 128 * 8; u += 256)      // (rows K1 did not write are not read)
            reinterpret_cast<float4*>(Ss)[u] = (u >> 3) < n ? St[u] : f4zero();
        tm_stage_gs(gs, r0 + rb, n, Gs);
        __syncthreads();
        for (int r = 0; r < n; ++r) {
            const float gv = Gs[r * TM_GLD + o];
            const float4 s0 = *reinterpret_cast<const float4*>(&Ss[r * 32 + kl0]);
            const float4 s1 = *reinterpret_cast<const float4*>(&Ss[r * 32 + kl0 + 4]);
            acc[0] = fmaf(gv, s0.x, acc[0]); acc[1] = fmaf(gv, s0.y, acc[1]);
            acc[2] = fmaf(gv, s0.z, acc[2]); acc[3] = fmaf(gv, s0.w, acc[3]);
            acc[4] = fmaf(gv, s1.x, acc[4]); acc[5] = fmaf(gv, s1.y, acc[5]);
            acc[6] = fmaf(gv, s1.z, acc[6]); acc[7] = fmaf(gv, s1.w, acc[7]);
        }
    }
    float* d = dw3r + (size_t)kt * 2048 + o * 32 + kl0;
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] += acc[j];
}

// D[rt][kt][row][kl] = sum_o gs[r0 + 128 rt + row][o] * W3R[kt][o][kl], o ascending.  Workgroup = one tile of the image
// (128 destinations x 32 kappa); thread (row, 16 kappa).  Rows past the chunk's last destination get zeros.
__global__ __launch_bounds__(256) void tm_d_kernel(const float* __restrict__ w3r, const float* __restrict__ gs,
                                                   float* __restrict__ D, int nkt, int r0, int cnt) {
    __shared__ __attribute__((aligned(16))) float Ws[64 * 32];
    __shared__ float Gs[128 * TM_GLD];
    const int kt = blockIdx.x, rt = blockIdx.y, tid = threadIdx.x;
    const int n = cnt - rt * 128 < 128 ? cnt - rt * 128 : 128;
    for (int u = tid; u < 64 * 8; u += 256)
        reinterpret_cast<float4*>(Ws)[u] = reinterpret_cast<const float4*>(w3r + (size_t)kt * 2048)[u];
    tm_stage_gs(gs, r0 + rt * 128, n, Gs);
    __syncthreads();
    const int row = tid >> 1, kl0 = (tid & 1) * 16;
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    for (int o = 0; o < 64; ++o) {
        const float gv = Gs[row * TM_GLD + o];
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
            const float4 w = *reinterpret_cast<const float4*>(&Ws[o * 32 + kl0 + 4 * j4]);
            acc[4 * j4 + 0] = fmaf(gv, w.x, acc[4 * j4 + 0]); acc[4 * j4 + 1] = fmaf(gv, w.y, acc[4 * j4 + 1]);
            acc[4 * j4 + 2] = fmaf(gv, w.z, acc[4 * j4 + 2]); acc[4 * j4 + 3] = fmaf(gv, w.w, acc[4 * j4 + 3]);
        }
    }
    float4* d = reinterpret_cast<float4*>(D + ((size_t)rt * nkt + kt) * 4096 + row * 32 + kl0);
#pragma unroll
    for (int j4 = 0; j4 < 4; ++j4) d[j4] = make_float4(acc[4 * j4], acc[4 * j4 + 1], acc[4 * j4 + 2], acc[4 * j4 + 3]);
}

// Per destination, shaped like K1: workgroup = (256 of the k hidden units, destination t of the chunk), stages of 16
// of t's in-edges.  The workgroup's slice of D_t (64 features x 256 hidden units) sits in registers twice:
//   thread c        (one hidden unit)             Dc[i] = D_t[i][c]:  dH_e[c] += sum_i x_src(e)[i] Dc[i]   (read-modify-
//                                                 write of the dH image: (e, c) belongs to this thread alone)
//   thread (cg, i)  (wave cg = 64 hidden units)   Dr[j] = D_t[i][64 cg + j]:  the edge's message partial over the
//                                                 wave's 64 units; the four waves are added in wave order and stored as
//                                                 msg[e][cq][i] (cq = 0 starts from d0_t[i], the b3 term)
constexpr int TE_EDGES = 16;

__global__ __launch_bounds__(256) void tm_edge_kernel(const float* __restrict__ D, const float* __restrict__ Hm,
                                                      float* __restrict__ dHm, const float* __restrict__ x,
                                                      const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                      float* __restrict__ msg, int K, int r0, int nqc) {
    __shared__ __attribute__((aligned(16))) float xs[TE_EDGES * 64];
    __shared__ __attribute__((aligned(16))) float hs[TE_EDGES * MO_CQ];
    __shared__ __attribute__((aligned(16))) float ms[TE_EDGES * 4 * 64];
    const int cq = blockIdx.x, tl = blockIdx.y, t = r0 + tl;
    const int beg = row_ptr[t], end = row_ptr[t + 1];
    if (beg == end) return;
    const int tid = threadIdx.x;
    const int c = cq * MO_CQ + tid;
    const bool live_c = c < K;
    const float* Dt = D + (size_t)(tl >> 7) * moment_nkt(K) * 4096 + (tl & 127) * 32;
    float Dc[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const size_t kappa = (size_t)i * K + c;
        Dc[i] = live_c ? Dt[(kappa >> 5) * 4096 + (kappa & 31)] : 0.f;
    }
    const int cg = tid >> 6, fi = tid & 63;
    const int cb = cq * MO_CQ + cg * 64;
    const bool live_g = cb < K;
    float Dr[64];
#pragma unroll
    for (int j4 = 0; j4 < 16; ++j4) {      // (i K + cb is a multiple of 64: two whole 32-kappa runs)
        const size_t kappa = (size_t)fi * K + cb + 4 * j4;
        const float4 v = live_g ? *reinterpret_cast<const float4*>(Dt + (kappa >> 5) * 4096 + (kappa & 31)) : f4zero();
        Dr[4 * j4] = v.x; Dr[4 * j4 + 1] = v.y; Dr[4 * j4 + 2] = v.z; Dr[4 * j4 + 3] = v.w;
    }
    float d0 = 0.f;
    if (cq == 0 && cg == 0) d0 = Dt[((size_t)64 * K / 32 + (fi >> 5)) * 4096 + (fi & 31)];
    const int er = tid >> 4, q = tid & 15;
    for (int e0 = beg; e0 < end; e0 += TE_EDGES) {
        const int n = end - e0 < TE_EDGES ? end - e0 : TE_EDGES;
        __syncthreads();      // (the previous stage's reads of xs / hs / ms are done)
        float4 xv = f4zero();
        if (er < n) xv = *reinterpret_cast<const float4*>(x + (size_t)src[e0 + er] * 64 + 4 * q);
        *reinterpret_cast<float4*>(&xs[er * 64 + 4 * q]) = xv;
        for (int u = 0; u < n; ++u) hs[u * MO_CQ + tid] = live_c ? Hm[h_image_offset(e0 + u, c, K)] : 0.f;
        __syncthreads();
        if (live_c) {
            for (int u = 0; u < n; ++u) {
                float a = 0.f;
#pragma unroll
                for (int i = 0; i < 64; ++i) a = fmaf(xs[u * 64 + i], Dc[i], a);
                float* p = dHm + h_image_offset(e0 + u, c, K);
                *p += a;
            }
        }
        for (int u = 0; u < n; ++u) {
            float m = d0;
            if (live_g) {
#pragma unroll
                for (int j = 0; j < 64; ++j) m = fmaf(Dr[j], hs[u * MO_CQ + cg * 64 + j], m);
            }
            ms[(u * 4 + cg) * 64 + fi] = m;
        }
        __syncthreads();
        if (er < n) {
            float4 v = *reinterpret_cast<const float4*>(&ms[(er * 4 + 0) * 64 + 4 * q]);
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const float4 a = *reinterpret_cast<const float4*>(&ms[(er * 4 + w) * 64 + 4 * q]);
                v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
            }
            *reinterpret_cast<float4*>(msg + ((size_t)(e0 + er) * nqc + cq) * 64 + 4 * q) = v;
        }
    }
}

// g_prev[j][i] = sum over j's out-edges (by-source order) of sum_cq msg[e][cq][i]  +  sum_o root[i][o] gz[j][o].
// Workgroup = source j; wave w takes out-edges w, w + 4, ..; the four waves are added in wave order.
__global__ __launch_bounds__(256) void tm_gather_kernel(const float* __restrict__ msg, int nqc,
                                                        const int* __restrict__ srow_ptr, const int* __restrict__ sperm,
                                                        const float* __restrict__ root, const float* __restrict__ gz,
                                                        float* __restrict__ g_prev) {
    __shared__ float red[4][64];
    __shared__ float gzs[64];
    const int j = blockIdx.x, w = threadIdx.x >> 6, i = threadIdx.x & 63;
    const int beg = srow_ptr[j], end = srow_ptr[j + 1];
    if (w == 0) gzs[i] = gz[(size_t)j * 64 + i];
    float a = 0.f;
    for (int p = beg + w; p < end; p += 4) {
        const float* m = msg + (size_t)sperm[p] * nqc * 64 + i;
        float e = m[0];
        for (int cq = 1; cq < nqc; ++cq) e += m[(size_t)cq * 64];
        a += e;
    }
    red[w][i] = a;
    __syncthreads();
    if (w != 0) return;
    float s = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
    float r = 0.f;
#pragma unroll 8
    for (int o = 0; o < 64; ++o) r = fmaf(root[i * 64 + o], gzs[o], r);
    g_prev[(size_t)j * 64 + i] = s + r;
}

// dW3R tiled -> d_w2 [4096, k], d_b2 [4096]: the inverse of w3_moment_kernel's map
__global__ __launch_bounds__(256) void tm_untile_w_kernel(const float* __restrict__ dw3r, int k, float* __restrict__ d_w2,
                                                          float* __restrict__ d_b2) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;      // over (kappa tile, o, kappa & 31), as W3R
    const long long total = (long long)(64 * k + 64) * 64;
    if (id >= total) return;
    const int kl = (int)(id & 31), o = (int)((id >> 5) & 63);
    const long long kappa = (id >> 11) * 32 + kl;
    if (kappa >= (long long)64 * k) {
        d_b2[(kappa - (long long)64 * k) * 64 + o] = dw3r[id];
        return;
    }
    const int i = (int)(kappa / k), c = (int)(kappa - (long long)i * k);
    d_w2[((size_t)i * 64 + o) * k + c] = dw3r[id];
}

// gz2[e][c] = H[e][c] > 0 ? dH[e][c] : 0, images -> row-major [E, k]; one float4 of a row per thread
__global__ __launch_bounds__(256) void tm_untile_h_kernel(const float* __restrict__ Hm, const float* __restrict__ dHm,
                                                          long long E, int K, float* __restrict__ gz2) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    const int k4 = K >> 2;
    if (id >= E * k4) return;
    const long long e = id / k4;
    const int c = (int)(id - e * k4) * 4;
    const size_t off = h_image_offset(e, c, K);
    const float4 h = *reinterpret_cast<const float4*>(Hm + off), d = *reinterpret_cast<const float4*>(dHm + off);
    reinterpret_cast<float4*>(gz2)[id] = make_float4(h.x > 0.f ? d.x : 0.f, h.y > 0.f ? d.y : 0.f, h.z > 0.f ? d.z : 0.f,
                                                     h.w > 0.f ? d.w : 0.f);
}

size_t h_image_floats(long long num_edges, int ker_width) {
    return (size_t)((num_edges + 127) / 128 * 128) * (size_t)ker_width;
}
int tm_nqc(int ker_width) { return (ker_width + MO_CQ - 1) / MO_CQ; }

struct TrainMomentWs {
    void* moment;       // moment_carve's region (W3R, the S chunk, K2's partials, ..)
    void* mlp;          // forward: the edge-MLP's workspace
    size_t mlp_bytes;
    float *gs, *g[2];   // backward: gs of the current application, dLoss/dx ping-pong
    float *d, *dw3r;    //           the D chunk (S's shape), dW3R (W3R's shape)
    float *dh, *msg;    //           the dH image, the per-edge messages [E][k/256][64]
};

// ONE carve for the sizes and the pointers of both directions (Carver(nullptr) only counts)
TrainMomentWs tm_carve(Carver& cv, int num_rows, int ker_width, long long edges, int gemm_mode, bool backward) {
    TrainMomentWs f{};
    f.moment = cv.take<char>(moment_workspace_bytes(num_rows, ker_width));
    if (!backward) {
        f.mlp_bytes = mdno_edge_mlp_workspace_bytes(ker_width, ker_width, edges, gemm_mode);
        f.mlp = cv.take<char>(f.mlp_bytes);
        return f;
    }
    const size_t rows64 = (size_t)num_rows * 64;
    f.gs = cv.take<float>(rows64);
    f.g[0] = cv.take<float>(rows64);
    f.g[1] = cv.take<float>(rows64);
    f.d = cv.take<float>((size_t)(moment_chunk_rows(num_rows) / 128) * moment_nkt(ker_width) * 4096);
    f.dw3r = cv.take<float>((size_t)(64 * ker_width + 64) * 64);
    f.dh = cv.take<float>(h_image_floats(edges, ker_width));
    f.msg = cv.take<float>((size_t)edges * tm_nqc(ker_width) * 64);
    return f;
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" int mdno_train_abi_version(void) { return MDNO_TRAIN_ABI_VERSION; }

extern "C" size_t mdno_train_moment_h_floats(int64_t num_edges, int ker_width) {
    if (num_edges < 0 || ker_width <= 0) return 0;
    return h_image_floats(num_edges > 0 ? num_edges : 1, ker_width);
}

extern "C" size_t mdno_train_moment_fwd_workspace_bytes(int num_rows, int ker_width, int64_t edge_cap, int gemm_mode) {
    if (num_rows <= 0 || edge_cap <= 0 || !moment_supported(64, ker_width)) return 0;
    Carver cv(nullptr);
    (void)tm_carve(cv, num_rows, ker_width, edge_cap, gemm_mode, false);
    return cv.used();
}

extern "C" int mdno_train_moment_fwd(const float* edge_attr, const int32_t* perm, const int32_t* num_edges, int64_t edge_cap,
                                     int ker_in, int ker_width, int gemm_mode, const float* w0, const float* b0,
                                     const float* w1, const float* b1, const float* w2, const float* b2,
                                     const int32_t* row_ptr, const int32_t* src, const int32_t* dst, int num_rows,
                                     const float* root1, const float* bias1, const float* root2, const float* bias2,
                                     int depth, float* x_stack, float* h_tiled, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    MDNO_REQUIRE(edge_attr && num_edges && w0 && b0 && w1 && b1 && w2 && b2 && row_ptr && src && root1 && bias1 && root2 &&
                     bias2 && x_stack && h_tiled && workspace, MDNO_EINVAL, "mdno_train_moment_fwd: null pointer");
    MDNO_REQUIRE(num_rows > 0 && edge_cap > 0 && depth >= 1, MDNO_EINVAL, "mdno_train_moment_fwd: num_rows=%d edge_cap=%lld depth=%d",
                 num_rows, (long long)edge_cap, depth);
    MDNO_REQUIRE(moment_supported(64, ker_width), MDNO_EUNSUPPORTED, "mdno_train_moment_fwd: ker_width=%d (x128)", ker_width);
    MDNO_REQUIRE(gemm_mode == MDNO_GEMM_SPLIT_BF16 || gemm_mode == MDNO_GEMM_F32 || gemm_mode == MDNO_GEMM_SPLIT_F16, MDNO_EINVAL,
                 "mdno_train_moment_fwd: gemm_mode=%d", gemm_mode);
    const size_t need = mdno_train_moment_fwd_workspace_bytes(num_rows, ker_width, edge_cap, gemm_mode);
    MDNO_REQUIRE(workspace_bytes >= need, MDNO_EWORKSPACE, "mdno_train_moment_fwd: workspace %zu < %zu", workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Carver cv(workspace);
    const TrainMomentWs ws = tm_carve(cv, num_rows, ker_width, edge_cap, gemm_mode, false);
    const MomentWs mw = moment_carve(ws.moment, num_rows, ker_width);
    const size_t layer = (size_t)num_rows * 64;
    // the inference forward's own sequence (engine.hip forward_impl, factored branch): the same kernels, the same bits
    MDNO_TRY(moment_prepare_graph(row_ptr, num_rows, mw, s));
    if (gemm_mode == MDNO_GEMM_SPLIT_F16) MDNO_TRY(moment_row_absmax(x_stack, num_rows, mw, s));
    const EdgeSource es{nullptr, 0, nullptr, num_rows, src, dst, edge_attr, perm, num_edges, (long long)edge_cap};
    const EdgeMlpWeights w{w0, b0, w1, b1, w2, b2};
    MDNO_TRY(edge_mlp(es, ker_in, ker_width, gemm_mode, w, EdgeMlpOut::hidden(h_tiled), ws.mlp, ws.mlp_bytes, s, WP_BOTH));
    MDNO_TRY(moment_prepare_weights(w2, b2, ker_width, mw, s, gemm_mode));
    for (int a = 0; a < 2 * depth; ++a)
        MDNO_TRY(moment_conv(x_stack + a * layer, h_tiled, row_ptr, src, num_rows, ker_width, a < depth ? root1 : root2,
                             a < depth ? bias1 : bias2, MDNO_AGGR_MEAN, /*relu=*/1, x_stack + (a + 1) * layer, mw, s, gemm_mode, a));
    return MDNO_OK;
}

extern "C" size_t mdno_train_moment_bwd_workspace_bytes(int num_rows, int ker_width, int64_t num_edges) {
    if (num_rows <= 0 || num_edges < 0 || !moment_supported(64, ker_width)) return 0;
    Carver cv(nullptr);
    (void)tm_carve(cv, num_rows, ker_width, num_edges > 0 ? num_edges : 1, MDNO_GEMM_F32, true);
    return cv.used();
}

extern "C" int mdno_train_moment_bwd(const float* g_out, const float* x_stack, const float* h_tiled, const int32_t* row_ptr,
                                     const int32_t* src, const int32_t* srow_ptr, const int32_t* sperm, int num_rows,
                                     int64_t num_edges, int ker_width, int depth, int gemm_mode, const float* w2,
                                     const float* b2, const float* root1, const float* root2, float* gz, float* g_in,
                                     float* gz2, float* d_w2, float* d_b2, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    MDNO_REQUIRE(g_out && x_stack && h_tiled && row_ptr && src && srow_ptr && sperm && w2 && b2 && root1 && root2 && gz && g_in &&
                     gz2 && d_w2 && d_b2 && workspace, MDNO_EINVAL, "mdno_train_moment_bwd: null pointer");
    MDNO_REQUIRE(num_rows > 0 && num_edges >= 0 && depth >= 1, MDNO_EINVAL, "mdno_train_moment_bwd: num_rows=%d num_edges=%lld depth=%d",
                 num_rows, (long long)num_edges, depth);
    MDNO_REQUIRE(moment_supported(64, ker_width), MDNO_EUNSUPPORTED, "mdno_train_moment_bwd: ker_width=%d (x128)", ker_width);
    const size_t need = mdno_train_moment_bwd_workspace_bytes(num_rows, ker_width, num_edges);
    MDNO_REQUIRE(workspace_bytes >= need, MDNO_EWORKSPACE, "mdno_train_moment_bwd: workspace %zu < %zu", workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long E = num_edges;
    Carver cv(workspace);
    const TrainMomentWs ws = tm_carve(cv, num_rows, ker_width, E > 0 ? E : 1, MDNO_GEMM_F32, true);
    const MomentWs mw = moment_carve(ws.moment, num_rows, ker_width);
    const int K = ker_width, L = 2 * depth, nkt = (int)moment_nkt(K), nqc = tm_nqc(K);
    const size_t layer = (size_t)num_rows * 64;
    const size_t w3r_floats = (size_t)(64 * K + 64) * 64;
    // W3R and the chunks' visiting order as the forward had them (plain fp32 W3R: MDNO_GEMM_SPLIT_BF16's preparation)
    MDNO_TRY(moment_prepare_graph(row_ptr, num_rows, mw, s));
    MDNO_TRY(moment_prepare_weights(w2, b2, K, mw, s, MDNO_GEMM_SPLIT_BF16));
    MDNO_HIP(hipMemsetAsync(ws.dw3r, 0, w3r_floats * sizeof(float), s));
    MDNO_HIP(hipMemsetAsync(ws.dh, 0, h_image_floats(E > 0 ? E : 1, K) * sizeof(float), s));
    const unsigned mask_blocks = (unsigned)(((long long)num_rows * 16 + 255) / 256);
    const float* g = g_out;
    for (int a = L; a >= 1; --a) {
        const float* x = x_stack + (size_t)(a - 1) * layer;
        float* gz_a = gz + (size_t)(a - 1) * layer;
        hipLaunchKernelGGL(tm_mask_kernel, dim3(mask_blocks), dim3(256), 0, s, g, x_stack + (size_t)a * layer, row_ptr, num_rows,
                           gz_a, ws.gs);
        if (E > 0) {
            for (int r0 = 0; r0 < num_rows; r0 += kMomentChunkRows) {
                const int cnt = num_rows - r0 < kMomentChunkRows ? num_rows - r0 : kMomentChunkRows;
                MDNO_TRY(moment_s_chunk(x, h_tiled, row_ptr, src, K, r0, cnt, mw, s, gemm_mode == MDNO_GEMM_F32));
                hipLaunchKernelGGL(tm_dw3r_kernel, dim3(nkt), dim3(256), 0, s, (const float*)mw.s, (const float*)ws.gs, ws.dw3r,
                                   nkt, r0, cnt);
                hipLaunchKernelGGL(tm_d_kernel, dim3(nkt, (cnt + 127) / 128), dim3(256), 0, s, (const float*)mw.w3r,
                                   (const float*)ws.gs, ws.d, nkt, r0, cnt);
                hipLaunchKernelGGL(tm_edge_kernel, dim3(nqc, cnt), dim3(256), 0, s, (const float*)ws.d, h_tiled, ws.dh, x, row_ptr,
                                   src, ws.msg, K, r0, nqc);
            }
        }
        float* g_prev = a == 1 ? g_in : ws.g[a & 1];
        hipLaunchKernelGGL(tm_gather_kernel, dim3(num_rows), dim3(256), 0, s, (const float*)ws.msg, nqc, srow_ptr, sperm,
                           a <= depth ? root1 : root2, (const float*)gz_a, g_prev);
        g = g_prev;
    }
    hipLaunchKernelGGL(tm_untile_w_kernel, dim3((unsigned)((w3r_floats + 255) / 256)), dim3(256), 0, s, (const float*)ws.dw3r, K,
                       d_w2, d_b2);
    if (E > 0)
        hipLaunchKernelGGL(tm_untile_h_kernel, dim3((unsigned)((E * (K / 4) + 255) / 256)), dim3(256), 0, s, h_tiled,
                           (const float*)ws.dh, E, K, gz2);
    return check_launch("mdno_train_moment_bwd");
}
