// Training (BASELINE.json configs[3]): the materialised 64x64 conv's training kernels — the 2*depth conv applications of
// the kernel-integral block, forward and backward, for W_e / dW_e stored in fp32 or in bf16.  Replaces what autograd +
// torch_geometric do for graph_kernel.py:445-474 (train) on the path :299-302 / :194-209 / :239-242.  The Linear
// layers of the shared edge-MLP are train.hip (fp32) and train_bf16.hip (bf16).
//
// Forward (materialised) per application a = 1..L:  z_a = mean_{e->t} x_{a-1}[src e] . W_e + x_{a-1}.root + bias,
// x_a = relu(z_a), W_e = reshape(L2(relu(L1(relu(L0 attr_e))))).  Given g_a = dLoss/dx_a:
//     gz_a      = g_a * (x_a > 0)                          gs_a[t] = gz_a[t] / max(deg_t, 1)
//     g_{a-1}   = gz_a . root^T + sum_{e: src e = r} W_e . gs_a[dst e]                 (nnconv_bwd_x)
//     d root    = sum_a x_{a-1}^T . gz_a,   d bias = sum_a colsum(gz_a)               (nnconv_bwd_root)
//     d W_e     = sum_a x_{a-1}[src e] (x) gs_a[dst e]                                (nnconv_bwd_we)
// Each kernel is ONE body with a template parameter for the stored type; the lane mapping and the association of the
// sums are conv64.h's, shared with the inference kernels (nnconv.hip), so bf16 W_e that holds bf16-representable
// weights gives the bits of the fp32 path.  Node features, conv outputs and every reduction are fp32; reductions over
// rows / edges use fixed-order partial sums (no float atomics), so gradients are bitwise reproducible.
#include <type_traits>

#include "conv64.h"
#include "kernels.h"
#include "reduce.h"
#include "split_mma.h"

namespace mdno {
namespace {

__global__ __launch_bounds__(256) void inv_degree_kernel(const int* __restrict__ row_ptr, int rows, int mean,
                                                         float* __restrict__ inv) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int d = row_ptr[r + 1] - row_ptr[r];
    inv[r] = mean ? 1.0f / (float)(d > 1 ? d : 1) : 1.0f;
}

// ---------------------------------------------------------------- conv forward, bf16 W_e
// The row kernel of nnconv.hip for W_e stored in bf16 (8-B loads of four bf16, widened exactly): same lane map, same 16
// summation chains, fp32 accumulation.  Kept as its own body on purpose, NOT merged into nnconv64_row_kernel: that
// one carries max aggregation and the output-layer tail (FcTail) and sits at 106-108 VGPRs where this one sits at
// 72-82, and it is the benchmark's kernel.
// WAVES = 16: a wave per summation chain; WAVES = 4: a wave owns chains w, w+4, w+8, w+12, one after the other (same
// chains, same order of additions: same bits) — four times as many workgroups resident per CU
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void nnconv64_bf16w_kernel(const float* __restrict__ x, const int* __restrict__ row_ptr,
                                                              const int* __restrict__ src,
                                                              const __bf16* __restrict__ w_e,
                                                              const float* __restrict__ root,
                                                              const float* __restrict__ bias, float* __restrict__ y,
                                                              int num_rows, int aggr, int relu) {
    __shared__ float red[CHAINS][64];
    __shared__ float rootred[64];
    const int row = blockIdx.x;
    if (row >= num_rows) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, q = lane & 15;
    const int beg = row_ptr[row], end = row_ptr[row + 1], deg = end - beg;
#pragma unroll
    for (int u = 0; u < CHAINS / WAVES; ++u) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int p = beg + wave + u * WAVES; p < end; p += CHAINS)
            edge_accumulate64<__bf16, true>(acc, x + (size_t)src[p] * 64, w_e + (size_t)p * 4096, g, q);
        acc = reduce_over_g(acc);
        if (lane < 16) *reinterpret_cast<float4*>(&red[wave + u * WAVES][4 * lane]) = acc;
    }
    const bool root_wave = root != nullptr && wave == (deg % WAVES);
    float4 racc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (root_wave) edge_accumulate64<float, false>(racc, x + (size_t)row * 64, root, g, q);
    racc = reduce_over_g(racc);
    if (root_wave && lane < 16) *reinterpret_cast<float4*>(&rootred[4 * lane]) = racc;
    __syncthreads();
    if (tid < 64) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CHAINS; ++c) s += red[c][tid];
        if (aggr == MDNO_AGGR_MEAN) s = s / (float)(deg > 1 ? deg : 1);
        if (root != nullptr) s += rootred[tid];
        if (bias != nullptr) s += bias[tid];
        if (relu) s = relu_f(s);
        y[(size_t)row * 64 + tid] = s;
    }
}

// ---------------------------------------------------------------- conv backward: input gradient
// g_prev[r] = gz[r] . root^T + sum_{p in out-edges of r} W_e[eid[p]] . gs[dst[p]]   (64x64 only; WT = float or __bf16)
// One workgroup (4 waves) per source row r; its out-edges (positions in the dst-sorted edge array)
// come from the src-sorted CSR (row_ptr_s, eid_s, dst_s).  An edge's W_e is streamed, root is not (conv64.h).
// y_below != NULL: the gradient leaves through the ReLU of the application below (whose output is y_below) —
// gz_below = g_prev * (y_below > 0), gs_below = gz_below * inv_deg[row] are written instead of g_prev: what
// mdno_relu_bwd2 would make of g_prev in a launch of its own, same arithmetic
template <class WT>
__global__ __launch_bounds__(256) void nnconv_bwd_x_kernel(const float* __restrict__ gz, const float* __restrict__ gs,
                                                           const int* __restrict__ row_ptr_s,
                                                           const int* __restrict__ eid_s, const int* __restrict__ dst_s,
                                                           const WT* __restrict__ w_e, const float* __restrict__ root,
                                                           float* __restrict__ g_prev, int num_rows,
                                                           const float* __restrict__ y_below,
                                                           const float* __restrict__ inv_deg,
                                                           float* __restrict__ gz_below, float* __restrict__ gs_below) {
    __shared__ float red[4][64];
    const int row = blockIdx.x;
    if (row >= num_rows) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, q = lane & 15;
    const int beg = row_ptr_s[row], end = row_ptr_s[row + 1];
    float acc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int p = beg + wave; p < end; p += 4)
        wg_accumulate<WT, true>(acc, w_e + (size_t)eid_s[p] * 4096, gs + (size_t)dst_s[p] * 64, g, q);
    if (root != nullptr && wave == ((end - beg) & 3)) wg_accumulate<float, false>(acc, root, gz + (size_t)row * 64, g, q);
    // reduce over the 16 q-lanes of each group: xor 1,2,4,8
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float v = acc[r];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        v += __shfl_xor(v, 8);
        acc[r] = v;
    }
    if (q == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave][16 * g + r] = acc[r];
    }
    __syncthreads();
    if (tid < 64) {
        const float v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        const size_t at = (size_t)row * 64 + tid;
        if (y_below != nullptr) {
            const bool on = y_below[at] > 0.f;
            gz_below[at] = on ? v : 0.f;
            gs_below[at] = on ? v * inv_deg[row] : 0.f;
        } else {
            g_prev[at] = v;
        }
    }
}

// ---------------------------------------------------------------- conv backward: d root, d bias
// d root[i][o] (+)= sum_{l, r} x_l[r][i] * gz_l[r][o];  d bias[o] (+)= sum_{l, r} gz_l[r][o]
// x, gz: [L, R, 64] stacked layers.  Block b takes a slice of the L*R rows -> partials, then reduce.
__device__ __forceinline__ void bwd_root_slice(const float* __restrict__ x, const float* __restrict__ gz, long long r0, long long r1,
                                               int slot, float* __restrict__ part_root, float* __restrict__ part_bias) {
    __shared__ float xs[64][65], gsx[64][65];
    const int tid = threadIdx.x;
    const int i0 = (tid >> 4) * 4, o0 = (tid & 15) * 4;    // 4x4 outputs per thread
    float acc[4][4] = {};
    float bsum = 0.f;
    for (long long rb = r0; rb < r1; rb += 64) {
        __syncthreads();
        for (int t = tid; t < 64 * 64; t += 256) {
            const int rr = t >> 6, c = t & 63;
            const bool ok = rb + rr < r1;
            xs[rr][c] = ok ? x[(rb + rr) * 64 + c] : 0.f;
            gsx[rr][c] = ok ? gz[(rb + rr) * 64 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int rr = 0; rr < 64; ++rr) {
            float xv[4], gv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { xv[a] = xs[rr][i0 + a]; gv[a] = gsx[rr][o0 + a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(xv[a], gv[b], acc[a][b]);
        }
        if (tid < 64)
            for (int rr = 0; rr < 64; ++rr) bsum += gsx[rr][tid];
    }
    float* pr = part_root + (size_t)slot * 4096;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) pr[(i0 + a) * 64 + o0 + b] = acc[a][b];
    if (tid < 64) part_bias[(size_t)slot * 64 + tid] = bsum;
}

__global__ __launch_bounds__(256) void nnconv_bwd_root_kernel(const float* __restrict__ x, const float* __restrict__ gz,
                                                              long long rows, long long slice_rows,
                                                              float* __restrict__ part_root,
                                                              float* __restrict__ part_bias) {
    const long long r0 = (long long)blockIdx.x * slice_rows;
    long long r1 = r0 + slice_rows;
    if (r1 > rows) r1 = rows;
    bwd_root_slice(x, gz, r0, r1, blockIdx.x, part_root, part_bias);
}

__global__ __launch_bounds__(256) void nnconv_bwd_root_pair_kernel(const float* __restrict__ x, const float* __restrict__ gz,
                                                                   long long rows_each, long long slice_rows, int per_half,
                                                                   float* __restrict__ part_root, float* __restrict__ part_bias) {
    const int half = (int)blockIdx.x / per_half, b = (int)blockIdx.x - half * per_half;
    const long long base = (long long)half * rows_each;
    const long long r0 = base + (long long)b * slice_rows;
    long long r1 = r0 + slice_rows;
    if (r1 > base + rows_each) r1 = base + rows_each;
    bwd_root_slice(x, gz, r0, r1, blockIdx.x, part_root, part_bias);
}

// ---------------------------------------------------------------- conv backward: d W_e, FMA loop
// dW_e[p][i][o] (+)= sum_l x_l[src[p]][i] * gs_l[dst[p]][o];  x, gs: [L, R, 64].  One wave per edge,
// lane (g, q) owns rows 16g..16g+15 x columns 4q..4q+3.  OUT = float: written as 16 coalesced 16-B stores, optionally
// on top of what dwe holds (`accumulate`); OUT = __bf16: rounded once, at the end, and written as 8-B stores
// (`accumulate` is not read).
template <class OUT>
__global__ __launch_bounds__(256) void nnconv_bwd_we_kernel(const float* __restrict__ x, const float* __restrict__ gs,
                                                            const int* __restrict__ src, const int* __restrict__ dst,
                                                            long long E, int L, long long layer_stride,
                                                            OUT* __restrict__ dwe, int accumulate) {
    constexpr bool F32 = std::is_same<OUT, float>::value;
    const int lane = threadIdx.x & 63, g = lane >> 4, q = lane & 15;
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= E) return;
    const float* xs = x + (size_t)src[p] * 64 + 16 * g;
    const float* gq = gs + (size_t)dst[p] * 64 + 4 * q;
    float4 acc[16];
    OUT* out = dwe + (size_t)p * 4096 + (16 * g) * 64 + 4 * q;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if constexpr (F32) acc[r] = accumulate ? *reinterpret_cast<const float4*>(out + r * 64) : make_float4(0.f, 0.f, 0.f, 0.f);
        else acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int l = 0; l < L; ++l) {
        const float4 gv = *reinterpret_cast<const float4*>(gq + (size_t)l * layer_stride);
        const float* xl = xs + (size_t)l * layer_stride;
        const float4 x0 = *reinterpret_cast<const float4*>(xl), x1 = *reinterpret_cast<const float4*>(xl + 4);
        const float4 x2 = *reinterpret_cast<const float4*>(xl + 8), x3 = *reinterpret_cast<const float4*>(xl + 12);
        const float xv[16] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w,
                              x2.x, x2.y, x2.z, x2.w, x3.x, x3.y, x3.z, x3.w};
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[r].x = fmaf(xv[r], gv.x, acc[r].x);
            acc[r].y = fmaf(xv[r], gv.y, acc[r].y);
            acc[r].z = fmaf(xv[r], gv.z, acc[r].z);
            acc[r].w = fmaf(xv[r], gv.w, acc[r].w);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if constexpr (F32) *reinterpret_cast<float4*>(out + r * 64) = acc[r];
        else *reinterpret_cast<uint2*>(out + r * 64) = pack4_bf16(acc[r].x, acc[r].y, acc[r].z, acc[r].w);
    }
}

// ---------------------------------------------------------------- d W_e + its column sums, on the matrix pipe
// dW_e[p] = sum_l gs_l[dst p] (x) x_l[src p] is a [64 x L] . [L x 64] product per edge: with L <= 16 ONE k-step of
// v_mfma_f32_32x32x16_bf16 per 32 x 32 quadrant.  The kernel above spends 768 FMAs per lane and edge on it (115 us at
// cfg4, twice what writing the 358 MB takes); here both fp32 operands are split exactly into three bf16 planes in
// registers and the six leading plane products accumulated in fp32 (fp32 accuracy, as everywhere in this library):
// 24 MFMAs per edge.  One wave per edge at a time, edges p = wave, wave + W, ..: the next edge's 32 operand words are
// fetched before this edge's MFMAs.
//   A = G (rows o): lane (l31, h) holds gs_l[dst][32 ob + l31], l = 8 h .. 8 h + 7;  B = X (columns i): x_l[src][32 ib + l31]
//   acc[ob][ib][e] = dW_e[i = 32 ib + l31][o = 32 ob + (e & 3) + 8 (e >> 2) + 4 h]: four consecutive o -> one 8-B LDS write
// and the rounded tile goes out through LDS row by row: 16 B per lane, 1 KiB contiguous per store instruction.
// The column sums (the last layer's bias gradient: sum over edges of the ROUNDED dW_e, what mdno_colsum_bf16 computes
// from the stored tensor in a second pass over its 358 MB) are taken on the way: every lane owns 64 fixed (i, o)
// positions of the tile, adds each edge's rounded values in edge order, the four waves of a workgroup are added in wave
// order through LDS and the workgroups by reduce_slices: fixed association, no atomics.
// BF16 = false: the fp32 training path's dW_e (nnconv_bwd_we_kernel<float>: 180 us + a 96 us column-sum pass over
// 716 MB at cfg4) through the same loop, the tile staged as fp32 and its column sums taken from the stored values.
constexpr int WE_WGS = 512;                              // workgroups of the launch (whatever E: the association of the sums is fixed)
template <bool BF16> struct WeTile {
    static constexpr int ROW = BF16 ? 136 : 272;         // LDS bytes per row of 64 outputs (+8 / +16: the 32 rows a write touches spread over the banks)
    static constexpr int BYTES = 64 * ROW;               // 8,704 / 17,408 B per wave
};

template <bool BF16>
__global__ __launch_bounds__(256, 2) void nnconv_bwd_we_mfma_kernel(const float* __restrict__ x, const float* __restrict__ gs,
                                                                   const int* __restrict__ src, const int* __restrict__ dst,
                                                                   long long E, int L, long long layer_stride,
                                                                   void* __restrict__ dwe_, float* __restrict__ part) {
    constexpr int ROW = WeTile<BF16>::ROW, TILE = WeTile<BF16>::BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * TILE > 4096 * 4 ? 4 * TILE : 4096 * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    // read-back role: 16 B per lane; bf16: 8 rows x 128 B per pass (8 passes), fp32: 4 rows x 256 B (16 passes)
    constexpr int PASSES = BF16 ? 8 : 16, RPP = 64 / PASSES, PER = BF16 ? 8 : 4;
    const int rr = BF16 ? lane >> 3 : lane >> 4, rc = BF16 ? lane & 7 : lane & 15;
    unsigned char* tile = lds + wave * TILE;
    const long long W = (long long)gridDim.x * 4;
    float cs[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) cs[j] = 0.f;
    float ga[2][8], xb[2][8];                            // this edge's operand words; next edge's while the MFMAs run
    // (every load unconditional — a layer past L re-reads layer 0 and is zeroed by a select — so that the loop body is
    // straight-line code: with `on ? load : 0` the compiler built a branch around each of the 32 loads)
    auto fetch = [&](long long p, float (&g_)[2][8], float (&x_)[2][8]) {
        const float* gq = gs + (size_t)dst[p] * 64 + l31;
        const float* xq = x + (size_t)src[p] * 64 + l31;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int l = 8 * h + j;
            const size_t off = (size_t)(l < L ? l : 0) * layer_stride;
            g_[0][j] = gq[off];
            g_[1][j] = gq[off + 32];
            x_[0][j] = xq[off];
            x_[1][j] = xq[off + 32];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (8 * h + j >= L) { g_[0][j] = 0.f; g_[1][j] = 0.f; x_[0][j] = 0.f; x_[1][j] = 0.f; }
    };
    auto split3 = [](const float (&v)[8], bf16x8 (&pl)[3]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const __bf16 hi = (__bf16)v[j];
            const float r1 = v[j] - (float)hi;
            const __bf16 mid = (__bf16)r1;
            const __bf16 lo = (__bf16)(r1 - (float)mid);
            pl[0][j] = hi; pl[1][j] = mid; pl[2][j] = lo;
        }
    };
    long long p = (long long)blockIdx.x * 4 + wave;
    if (p < E) fetch(p, ga, xb);
    for (; p < E; p += W) {
        bf16x8 a[2][3], b[2][3];
        split3(ga[0], a[0]); split3(ga[1], a[1]);
        split3(xb[0], b[0]); split3(xb[1], b[1]);
        if (p + W < E) fetch(p + W, ga, xb);
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc[2][2];
#pragma unroll
        for (int ob = 0; ob < 2; ++ob)
#pragma unroll
            for (int ib = 0; ib < 2; ++ib) {
                // (a constant zero: the first product's C operand is the inline 0, no accumulator is cleared)
                acc[ob][ib] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                mma6_bf16(a[ob], b[ib], acc[ob][ib]);
            }
        // tile -> LDS [i][o] (a wave's own tile: no workgroup barrier); four consecutive o per write
#pragma unroll
        for (int ob = 0; ob < 2; ++ob)
#pragma unroll
            for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x16& c = acc[ob][ib];
                    unsigned char* wp = tile + (32 * ib + l31) * ROW + (32 * ob + 8 * g + 4 * h) * (BF16 ? 2 : 4);
                    if (BF16) *reinterpret_cast<uint2*>(wp) = pack4_bf16(c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]);
                    else *reinterpret_cast<float4*>(wp) = make_float4(c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]);
                }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
            const unsigned char* rp = tile + (RPP * ps + rr) * ROW + rc * 16;
            const size_t at = (size_t)p * 4096 + (RPP * ps + rr) * 64 + PER * rc;
            if (BF16) {
                const uint2 u0 = *reinterpret_cast<const uint2*>(rp), u1 = *reinterpret_cast<const uint2*>(rp + 8);
                *reinterpret_cast<uint4*>(static_cast<__bf16*>(dwe_) + at) = make_uint4(u0.x, u0.y, u1.x, u1.y);
                const unsigned w4[4] = {u0.x, u0.y, u1.x, u1.y};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    cs[8 * ps + 2 * j] += __builtin_bit_cast(float, w4[j] << 16);
                    cs[8 * ps + 2 * j + 1] += __builtin_bit_cast(float, w4[j] & 0xffff0000u);
                }
            } else {
                const float4 v = *reinterpret_cast<const float4*>(rp);
                *reinterpret_cast<float4*>(static_cast<float*>(dwe_) + at) = v;
                cs[4 * ps] += v.x; cs[4 * ps + 1] += v.y; cs[4 * ps + 2] += v.z; cs[4 * ps + 3] += v.w;
            }
        }
        __builtin_amdgcn_wave_barrier();      // the tile is rewritten by the next edge
    }
    // column sums: the four waves in wave order through LDS -> part[workgroup][4096]
    float* red = reinterpret_cast<float*>(lds);
    __syncthreads();
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int ps = 0; ps < PASSES; ++ps)
#pragma unroll
                for (int j = 0; j < PER; ++j) {
                    const int idx = (RPP * ps + rr) * 64 + PER * rc + j;
                    red[idx] = w == 0 ? cs[PER * ps + j] : red[idx] + cs[PER * ps + j];
                }
        }
        __syncthreads();
    }
    float* po = part + (size_t)blockIdx.x * 4096;
    for (int i = threadIdx.x; i < 1024; i += 256)
        reinterpret_cast<float4*>(po)[i] = reinterpret_cast<const float4*>(red)[i];
}

// rows per workgroup of nnconv_bwd_root_kernel: 256 (four 64-row passes) — 1,024 left cfg4's 21,504 stacked
// rows to 21 workgroups on 256 CUs (174 us per call); 128 moved the time into the serial slice sums
constexpr long long kRootSliceRows = 256;

// ---------------------------------------------------------------- host side: one launch site per kernel
// y_below == NULL: the input gradient itself -> g_prev; else through the ReLU below -> gz_below, gs_below
template <class WT>
void launch_bwd_x(hipStream_t s, const float* gz, const float* gs, const int* row_ptr_s, const int* eid_s, const int* dst_s,
                  int num_rows, const void* w_e, const float* root, float* g_prev, const float* y_below = nullptr,
                  const float* inv_deg = nullptr, float* gz_below = nullptr, float* gs_below = nullptr) {
    hipLaunchKernelGGL(nnconv_bwd_x_kernel<WT>, dim3(num_rows), dim3(256), 0, s, gz, gs, row_ptr_s, eid_s, dst_s,
                       static_cast<const WT*>(w_e), root, g_prev, num_rows, y_below, inv_deg, gz_below, gs_below);
}

template <class WT>
int bwd_x(const char* what, const float* gz, const float* gs, const int32_t* row_ptr_s, const int32_t* eid_s,
          const int32_t* dst_s, int num_rows, const void* w_e, const float* root, int Cin, int Cout, float* g_prev,
          void* stream) {
    MDNO_REQUIRE(gz && gs && row_ptr_s && eid_s && dst_s && w_e && g_prev && num_rows > 0, MDNO_EINVAL, "%s: bad arguments", what);
    MDNO_REQUIRE(Cin == 64 && Cout == 64, MDNO_EUNSUPPORTED, "%s: only 64x64 channels", what);
    launch_bwd_x<WT>(static_cast<hipStream_t>(stream), gz, gs, row_ptr_s, eid_s, dst_s, num_rows, w_e, root, g_prev);
    return check_launch(what);
}

template <class OUT>
int bwd_we(const char* what, const float* x, const float* gs, const int32_t* src, const int32_t* dst, int64_t E, int L,
           int64_t layer_stride, void* d_we, int accumulate, void* stream) {
    hipLaunchKernelGGL(nnconv_bwd_we_kernel<OUT>, dim3((unsigned)((E + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x, gs, src, dst, (long long)E, L, (long long)layer_stride, static_cast<OUT*>(d_we), accumulate);
    return check_launch(what);
}

template <bool BF16>
int bwd_we_colsum(const char* what, const float* x, const float* gs, const int32_t* src, const int32_t* dst, int64_t E, int L,
                  int64_t layer_stride, void* d_we, float* colsum, void* workspace, size_t workspace_bytes, void* stream) {
    MDNO_REQUIRE(x && gs && src && dst && d_we && colsum && workspace && E >= 0 && L > 0, MDNO_EINVAL, "%s: bad arguments", what);
    MDNO_REQUIRE(L <= 16, MDNO_EUNSUPPORTED, "%s: %d conv applications (one MFMA k-step holds 16)", what, L);
    MDNO_REQUIRE(workspace_bytes >= mdno_nnconv_bwd_we_colsum_workspace_bytes(), MDNO_EWORKSPACE, "%s: workspace too small", what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(nnconv_bwd_we_mfma_kernel<BF16>, dim3(WE_WGS), dim3(256), 0, s, x, gs, src, dst, (long long)E, L,
                       (long long)layer_stride, d_we, static_cast<float*>(workspace));
    launch_reduce_slices(static_cast<const float*>(workspace), WE_WGS, 4096, colsum, 0, s);
    return check_launch(what);
}

// The conv applications of a training step as ONE call.  `apply(x_in, root, bias, x_out)`: one application with
// mean aggregation and ReLU — mdno_nnconv_fwd or mdno_nnconv_bf16w_fwd on the chain's W_e.
template <class Apply>
int chain_fwd(const char* what, float* x_layers, const int32_t* row_ptr, const int32_t* src, int num_rows, const void* w_e,
              const float* root1, const float* bias1, const float* root2, const float* bias2, int depth, Apply apply) {
    MDNO_REQUIRE(x_layers && row_ptr && src && w_e && num_rows > 0 && depth > 0, MDNO_EINVAL, "%s: bad arguments", what);
    const size_t stride = (size_t)num_rows * 64;
    for (int a = 1; a <= 2 * depth; ++a)
        MDNO_TRY(apply(x_layers + (a - 1) * stride, a <= depth ? root1 : root2, a <= depth ? bias1 : bias2, x_layers + a * stride));
    return MDNO_OK;
}

template <class WT>
int chain_bwd(const char* what, const float* g_out, const float* x_layers, const float* inv_deg, const int32_t* row_ptr_s,
              const int32_t* eid_s, const int32_t* dst_s, int num_rows, const void* w_e, const float* root1, const float* root2,
              int depth, float* gz, float* gs, float* g_in, void* stream) {
    MDNO_REQUIRE(g_out && x_layers && inv_deg && row_ptr_s && eid_s && dst_s && w_e && gz && gs && g_in && num_rows > 0 &&
                     depth > 0, MDNO_EINVAL, "%s: bad arguments", what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int L = 2 * depth;
    const size_t stride = (size_t)num_rows * 64;
    // the gradient enters through the ReLU of application L; every later ReLU is the epilogue of the kernel above it
    MDNO_TRY(mdno_relu_bwd2(g_out, x_layers + L * stride, inv_deg, num_rows, 64, gz + (L - 1) * stride, gs + (L - 1) * stride,
                            stream));
    for (int a = L; a >= 1; --a) {
        const float* root = a <= depth ? root1 : root2;
        const float *gz_a = gz + (a - 1) * stride, *gs_a = gs + (a - 1) * stride;
        if (a > 1)
            launch_bwd_x<WT>(s, gz_a, gs_a, row_ptr_s, eid_s, dst_s, num_rows, w_e, root, nullptr, x_layers + (a - 1) * stride,
                             inv_deg, gz + (a - 2) * stride, gs + (a - 2) * stride);
        else
            launch_bwd_x<WT>(s, gz_a, gs_a, row_ptr_s, eid_s, dst_s, num_rows, w_e, root, g_in);
    }
    return check_launch(what);
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" int mdno_inv_degree(const int32_t* row_ptr, int rows, int aggr, float* inv, void* stream) {
    MDNO_REQUIRE(row_ptr && inv && rows > 0, MDNO_EINVAL, "mdno_inv_degree: bad arguments");
    hipLaunchKernelGGL(inv_degree_kernel, dim3((rows + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       row_ptr, rows, aggr == MDNO_AGGR_MEAN ? 1 : 0, inv);
    return check_launch("mdno_inv_degree");
}

extern "C" int mdno_nnconv_bf16w_fwd(const float* x, const int32_t* row_ptr, const int32_t* src, int num_rows,
                                     const void* w_e, const float* root, const float* bias, int aggr, int relu,
                                     float* y, void* stream) {
    MDNO_REQUIRE(x && row_ptr && src && w_e && y && num_rows > 0, MDNO_EINVAL, "mdno_nnconv_bf16w_fwd: bad arguments");
    MDNO_REQUIRE(aggr == MDNO_AGGR_ADD || aggr == MDNO_AGGR_MEAN, MDNO_EUNSUPPORTED, "mdno_nnconv_bf16w_fwd: aggr %d", aggr);
    // many short rows (a training batch: 3,584 rows of ~12 edges): four waves per row keep four times as many rows
    // resident per CU — 30.4k instead of 29.5k samples/s on cfg4; few rows: a wave per chain
    if (num_rows >= 2048)
        hipLaunchKernelGGL(nnconv64_bf16w_kernel<4>, dim3(num_rows), dim3(256), 0, static_cast<hipStream_t>(stream), x, row_ptr,
                           src, static_cast<const __bf16*>(w_e), root, bias, y, num_rows, aggr, relu);
    else
        hipLaunchKernelGGL(nnconv64_bf16w_kernel<16>, dim3(num_rows), dim3(1024), 0, static_cast<hipStream_t>(stream), x,
                           row_ptr, src, static_cast<const __bf16*>(w_e), root, bias, y, num_rows, aggr, relu);
    return check_launch("nnconv64_bf16w_kernel");
}

extern "C" int mdno_nnconv_bwd_x(const float* gz, const float* gs, const int32_t* row_ptr_s, const int32_t* eid_s,
                                 const int32_t* dst_s, int num_rows, const float* w_e, const float* root,
                                 int Cin, int Cout, float* g_prev, void* stream) {
    return bwd_x<float>("mdno_nnconv_bwd_x", gz, gs, row_ptr_s, eid_s, dst_s, num_rows, w_e, root, Cin, Cout, g_prev, stream);
}

extern "C" int mdno_nnconv_bwd_x_bf16w(const float* gz, const float* gs, const int32_t* row_ptr_s, const int32_t* eid_s,
                                       const int32_t* dst_s, int num_rows, const void* w_e, const float* root,
                                       float* g_prev, void* stream) {
    return bwd_x<__bf16>("mdno_nnconv_bwd_x_bf16w", gz, gs, row_ptr_s, eid_s, dst_s, num_rows, w_e, root, 64, 64, g_prev, stream);
}

extern "C" size_t mdno_nnconv_bwd_root_workspace_bytes(int64_t rows) {
    const long long blocks = (rows + kRootSliceRows - 1) / kRootSliceRows;
    return align_up((size_t)blocks * (4096 + 64) * sizeof(float), 256);
}

extern "C" int mdno_nnconv_bwd_root(const float* x, const float* gz, int64_t rows, int Cin, int Cout, float* d_root,
                                    float* d_bias, int accumulate, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    MDNO_REQUIRE(x && gz && rows > 0 && workspace, MDNO_EINVAL, "mdno_nnconv_bwd_root: bad arguments");
    MDNO_REQUIRE(Cin == 64 && Cout == 64, MDNO_EUNSUPPORTED, "mdno_nnconv_bwd_root: only 64x64 channels");
    MDNO_REQUIRE(workspace_bytes >= mdno_nnconv_bwd_root_workspace_bytes(rows), MDNO_EWORKSPACE,
                 "mdno_nnconv_bwd_root: workspace");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long slice_rows = kRootSliceRows;
    const int blocks = (int)((rows + slice_rows - 1) / slice_rows);
    float* part_root = static_cast<float*>(workspace);
    float* part_bias = part_root + (size_t)blocks * 4096;
    hipLaunchKernelGGL(nnconv_bwd_root_kernel, dim3(blocks), dim3(256), 0, s, x, gz, (long long)rows, slice_rows,
                       part_root, part_bias);
    if (d_root)
        launch_reduce_slices((const float*)part_root, blocks, 4096ll, d_root, accumulate, s);
    if (d_bias)
        launch_reduce_slices((const float*)part_bias, blocks, 64ll, d_bias, accumulate, s);
    return check_launch("mdno_nnconv_bwd_root");
}

// conv1's and conv2's root / bias gradients in ONE launch: x, gz [2 * rows_each, 64], the first rows_each rows conv1's
// stacked layers, the rest conv2's (they are adjacent in the training step's layer stack).  The slices of a half never
// cross into the other, and each half's partial sums are the ones mdno_nnconv_bwd_root forms for it alone (same slice
// boundaries, same order): bitwise the two single calls, one 36 us launch less per batch.
extern "C" size_t mdno_nnconv_bwd_root_pair_workspace_bytes(int64_t rows_each) {
    const long long blocks = 2 * ((rows_each + kRootSliceRows - 1) / kRootSliceRows);
    return align_up((size_t)blocks * (4096 + 64) * sizeof(float), 256);
}

extern "C" int mdno_nnconv_bwd_root_pair(const float* x, const float* gz, int64_t rows_each, float* d_root1, float* d_bias1,
                                         float* d_root2, float* d_bias2, void* workspace, size_t workspace_bytes, void* stream) {
    MDNO_REQUIRE(x && gz && rows_each > 0 && workspace && d_root1 && d_bias1 && d_root2 && d_bias2, MDNO_EINVAL,
                 "mdno_nnconv_bwd_root_pair: bad arguments");
    MDNO_REQUIRE(workspace_bytes >= mdno_nnconv_bwd_root_pair_workspace_bytes(rows_each), MDNO_EWORKSPACE,
                 "mdno_nnconv_bwd_root_pair: workspace");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int per_half = (int)((rows_each + kRootSliceRows - 1) / kRootSliceRows);
    float* part_root = static_cast<float*>(workspace);
    float* part_bias = part_root + (size_t)2 * per_half * 4096;
    hipLaunchKernelGGL(nnconv_bwd_root_pair_kernel, dim3(2 * per_half), dim3(256), 0, s, x, gz, (long long)rows_each,
                       (long long)kRootSliceRows, per_half, part_root, part_bias);
    launch_reduce_slices((const float*)part_root, per_half, 4096ll, d_root1, 0, s);
    launch_reduce_slices((const float*)part_root + (size_t)per_half * 4096, per_half, 4096ll, d_root2, 0, s);
    launch_reduce_slices((const float*)part_bias, per_half, 64ll, d_bias1, 0, s);
    launch_reduce_slices((const float*)part_bias + (size_t)per_half * 64, per_half, 64ll, d_bias2, 0, s);
    return check_launch("mdno_nnconv_bwd_root_pair");
}

extern "C" int mdno_nnconv_bwd_we(const float* x, const float* gs, const int32_t* src, const int32_t* dst, int64_t E,
                                  int layers, int64_t layer_stride, int Cin, int Cout, float* d_we, int accumulate,
                                  void* stream) {
    MDNO_REQUIRE(x && gs && src && dst && d_we && E > 0 && layers > 0, MDNO_EINVAL, "mdno_nnconv_bwd_we: bad arguments");
    MDNO_REQUIRE(Cin == 64 && Cout == 64, MDNO_EUNSUPPORTED, "mdno_nnconv_bwd_we: only 64x64 channels");
    return bwd_we<float>("mdno_nnconv_bwd_we", x, gs, src, dst, E, layers, layer_stride, d_we, accumulate, stream);
}

extern "C" int mdno_nnconv_bwd_we_bf16(const float* x, const float* gs, const int32_t* src, const int32_t* dst, int64_t E,
                                       int L, int64_t layer_stride, void* d_we, void* stream) {
    MDNO_REQUIRE(x && gs && src && dst && d_we && E >= 0 && L > 0, MDNO_EINVAL, "mdno_nnconv_bwd_we_bf16: bad arguments");
    if (E == 0) return MDNO_OK;
    return bwd_we<__bf16>("mdno_nnconv_bwd_we_bf16", x, gs, src, dst, E, L, layer_stride, d_we, 0, stream);
}

extern "C" size_t mdno_nnconv_bwd_we_colsum_workspace_bytes(void) { return align_up((size_t)WE_WGS * 4096 * sizeof(float), 256); }
extern "C" size_t mdno_nnconv_bwd_we_bf16_colsum_workspace_bytes(void) { return mdno_nnconv_bwd_we_colsum_workspace_bytes(); }

extern "C" int mdno_nnconv_bwd_we_bf16_colsum(const float* x, const float* gs, const int32_t* src, const int32_t* dst, int64_t E,
                                              int L, int64_t layer_stride, void* d_we, float* colsum, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    return bwd_we_colsum<true>("mdno_nnconv_bwd_we_bf16_colsum", x, gs, src, dst, E, L, layer_stride, d_we, colsum, workspace,
                               workspace_bytes, stream);
}

extern "C" int mdno_nnconv_bwd_we_colsum(const float* x, const float* gs, const int32_t* src, const int32_t* dst, int64_t E, int L,
                                         int64_t layer_stride, float* d_we, float* colsum, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    return bwd_we_colsum<false>("mdno_nnconv_bwd_we_colsum", x, gs, src, dst, E, L, layer_stride, d_we, colsum, workspace,
                                workspace_bytes, stream);
}

extern "C" int mdno_nnconv_chain_fwd(float* x_layers, const int32_t* row_ptr, const int32_t* src, int num_rows,
                                     const float* w_e, const float* root1, const float* bias1, const float* root2,
                                     const float* bias2, int depth, void* stream) {
    return chain_fwd("mdno_nnconv_chain_fwd", x_layers, row_ptr, src, num_rows, w_e, root1, bias1, root2, bias2, depth,
                     [=](const float* xi, const float* root, const float* bias, float* xo) {
                         return mdno_nnconv_fwd(xi, row_ptr, src, num_rows, w_e, root, bias, 64, 64, MDNO_AGGR_MEAN, 1, xo, stream);
                     });
}

extern "C" int mdno_nnconv_chain_bf16w_fwd(float* x_layers, const int32_t* row_ptr, const int32_t* src, int num_rows,
                                           const void* w_e, const float* root1, const float* bias1, const float* root2,
                                           const float* bias2, int depth, void* stream) {
    return chain_fwd("mdno_nnconv_chain_bf16w_fwd", x_layers, row_ptr, src, num_rows, w_e, root1, bias1, root2, bias2, depth,
                     [=](const float* xi, const float* root, const float* bias, float* xo) {
                         return mdno_nnconv_bf16w_fwd(xi, row_ptr, src, num_rows, w_e, root, bias, MDNO_AGGR_MEAN, 1, xo, stream);
                     });
}

extern "C" int mdno_nnconv_chain_bwd(const float* g_out, const float* x_layers, const float* inv_deg,
                                     const int32_t* row_ptr_s, const int32_t* eid_s, const int32_t* dst_s, int num_rows,
                                     const float* w_e, const float* root1, const float* root2, int depth, float* gz,
                                     float* gs, float* g_in, void* stream) {
    return chain_bwd<float>("mdno_nnconv_chain_bwd", g_out, x_layers, inv_deg, row_ptr_s, eid_s, dst_s, num_rows, w_e, root1,
                            root2, depth, gz, gs, g_in, stream);
}

extern "C" int mdno_nnconv_chain_bf16w_bwd(const float* g_out, const float* x_layers, const float* inv_deg,
                                           const int32_t* row_ptr_s, const int32_t* eid_s, const int32_t* dst_s,
                                           int num_rows, const void* w_e, const float* root1, const float* root2, int depth,
                                           float* gz, float* gs, float* g_in, void* stream) {
    return chain_bwd<__bf16>("mdno_nnconv_chain_bf16w_bwd", g_out, x_layers, inv_deg, row_ptr_s, eid_s, dst_s, num_rows, w_e,
                             root1, root2, depth, gz, gs, g_in, stream);
}
