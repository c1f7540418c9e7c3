// Training (BASELINE.json configs[3]): the Linear-layer ops of the fp32 training path — the shared edge-MLP of the
// kernel-integral block, forward and backward, as individually callable ops: C = act(A . Bt^T + bias) (linear_fwd),
// C = A^T . B over rows (gemm_atb), column sums, ReLU masks and a transpose.  The conv applications and their
// gradients are train_conv.hip.  Replaces what autograd does for graph_kernel.py:445-474 (train) on the path
// :299-302 / :239-242.  Everything is fp32; reductions over rows/edges use fixed-order partial sums
// (no float atomics), so gradients are bitwise reproducible.
#include "kernels.h"
#include "mfma_f32.h"
#include "reduce.h"
#include "split_mma.h"

namespace mdno {
namespace {

using f32mma::mma_64x64;
constexpr int BK = f32mma::BK, LD = f32mma::LD;

// ---------------------------------------------------------------- C = act(A . Bt^T + bias), any M
// A [M,K], Bt [N,K], C [M,N]; N % 128 == 0, K % 32 == 0 (MFMA path).  128x128x32 tile, 4 waves.
template <bool RELU>
__global__ __launch_bounds__(256, 2) void linear_mfma_kernel(const float* __restrict__ A, const float* __restrict__ Bt,
                                                             const float* __restrict__ bias, float* __restrict__ Cm,
                                                             int rows, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;
    float* Bs = smem + 2 * 128 * LD;
    const int bm = blockIdx.y * 128, bn = blockIdx.x * 128;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, h = lane >> 5;
    const int srow = tid >> 3, scol = (tid & 7) * 4;
    const size_t ldk = (size_t)K;
    auto arow = [&](int r) { const int rr = bm + r; return (size_t)(rr < rows ? rr : rows - 1); };
    const float* A0 = A + arow(srow) * ldk + scol;
    const float* A1 = A + arow(srow + 32) * ldk + scol;
    const float* A2 = A + arow(srow + 64) * ldk + scol;
    const float* A3 = A + arow(srow + 96) * ldk + scol;
    const float* Bg = Bt + (size_t)(bn + srow) * ldk + scol;
    float4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;
#define MDNO_LOAD(KOFF)                                                  \
    ra0 = *reinterpret_cast<const float4*>(A0 + (KOFF));                 \
    ra1 = *reinterpret_cast<const float4*>(A1 + (KOFF));                 \
    ra2 = *reinterpret_cast<const float4*>(A2 + (KOFF));                 \
    ra3 = *reinterpret_cast<const float4*>(A3 + (KOFF));                 \
    rb0 = *reinterpret_cast<const float4*>(Bg + (KOFF));                 \
    rb1 = *reinterpret_cast<const float4*>(Bg + 32 * ldk + (KOFF));      \
    rb2 = *reinterpret_cast<const float4*>(Bg + 64 * ldk + (KOFF));      \
    rb3 = *reinterpret_cast<const float4*>(Bg + 96 * ldk + (KOFF));
    float* a_st = As + srow * LD + scol;
    float* b_st = Bs + srow * LD + scol;
#define MDNO_STORE(BUF)                                                            \
    *reinterpret_cast<float4*>(a_st + (BUF) * 128 * LD) = ra0;                     \
    *reinterpret_cast<float4*>(a_st + (BUF) * 128 * LD + 32 * LD) = ra1;           \
    *reinterpret_cast<float4*>(a_st + (BUF) * 128 * LD + 64 * LD) = ra2;           \
    *reinterpret_cast<float4*>(a_st + (BUF) * 128 * LD + 96 * LD) = ra3;           \
    *reinterpret_cast<float4*>(b_st + (BUF) * 128 * LD) = rb0;                     \
    *reinterpret_cast<float4*>(b_st + (BUF) * 128 * LD + 32 * LD) = rb1;           \
    *reinterpret_cast<float4*>(b_st + (BUF) * 128 * LD + 64 * LD) = rb2;           \
    *reinterpret_cast<float4*>(b_st + (BUF) * 128 * LD + 96 * LD) = rb3;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const float* a_rd = As + (wm * 64 + l31) * LD + 4 * h;
    const float* b_rd = Bs + (wn * 64 + l31) * LD + 4 * h;
    const int nk = K / BK;
    MDNO_LOAD(0)
    MDNO_STORE(0)
    __syncthreads();
    for (int kt = 0; kt < nk - 1; ++kt) {
        MDNO_LOAD((size_t)(kt + 1) * BK)
        mma_64x64(acc, a_rd + (kt & 1) * 128 * LD, b_rd + (kt & 1) * 128 * LD);
        MDNO_STORE((kt & 1) ^ 1)
        __syncthreads();
    }
    mma_64x64(acc, a_rd + ((nk - 1) & 1) * 128 * LD, b_rd + ((nk - 1) & 1) * 128 * LD);
#undef MDNO_LOAD
#undef MDNO_STORE
    // bias loaded once and pinned (sunk into the predicated store blocks it serialises the stores)
    float bv0 = 0.f, bv1 = 0.f;
    if (bias) {
        bv0 = bias[bn + wn * 64 + l31];
        bv1 = bias[bn + wn * 64 + 32 + l31];
    }
    asm volatile("" : "+v"(bv0), "+v"(bv1));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = bn + wn * 64 + j * 32 + l31;
        const float bv = j ? bv1 : bv0;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = mfma32_row(e, h, bm + wm * 64 + i * 32);
                if (m < rows) {
                    float v = acc[i][j][e] + bv;
                    if (RELU) v = relu_f(v);
                    Cm[(size_t)m * N + n] = v;
                }
            }
    }
}

// any shape (small fixtures, K = 6 first layer): one thread per output element
template <bool RELU>
__global__ __launch_bounds__(256) void linear_generic_kernel(const float* __restrict__ A, const float* __restrict__ Bt,
                                                             const float* __restrict__ bias, float* __restrict__ Cm,
                                                             long long rows, int N, int K) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= rows * N) return;
    const long long m = id / N;
    const int n = (int)(id % N);
    const float* a = A + m * K;
    const float* b = Bt + (size_t)n * K;
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf(a[k], b[k], s);
    s += bias ? bias[n] : 0.f;
    if (RELU) s = relu_f(s);
    Cm[id] = s;
}

// ---------------------------------------------------------------- C[N1,N2] = A^T . B over rows
// A [K,N1], B [K,N2] row-major (K = number of rows, e.g. edges), partial sums per K-slice:
// part[slice][N1][N2]; a second kernel adds the slices in order.  Tile 128x128, k-tile 32 rows.
// LDS holds the tiles k-major ([k][n]); MFMA fragments are 4-byte LDS reads (lanes along n).
constexpr int LDT = 128 + 4;
__global__ __launch_bounds__(256, 2) void gemm_atb_mfma_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                               float* __restrict__ part, long long K, int N1, int N2,
                                                               long long kslice) {
    __shared__ __attribute__((aligned(16))) float As[BK * LDT];
    __shared__ __attribute__((aligned(16))) float Bs[BK * LDT];
    const int bm = blockIdx.y * 128, bn = blockIdx.x * 128, slice = blockIdx.z;
    const long long k0 = (long long)slice * kslice;
    long long k1 = k0 + kslice;
    if (k1 > K) k1 = K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, h = lane >> 5;
    // staging: 32 rows x 128 floats per operand = 1024 float4 -> 4 per thread; thread covers row tid>>5 + 8*i
    const int srow = tid >> 5, scol = (tid & 31) * 4;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    for (long long kt = k0; kt < k1; kt += BK) {
        float4 ra[4], rb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long r = kt + srow + 8 * i;
            if (r < k1) {
                ra[i] = *reinterpret_cast<const float4*>(A + r * N1 + bm + scol);
                rb[i] = *reinterpret_cast<const float4*>(B + r * N2 + bn + scol);
            } else {
                ra[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                rb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        __syncthreads();   // previous tile fully consumed
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<float4*>(As + (srow + 8 * i) * LDT + scol) = ra[i];
            *reinterpret_cast<float4*>(Bs + (srow + 8 * i) * LDT + scol) = rb[i];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            const float* ar = As + (2 * s + h) * LDT + wm * 64 + l31;
            const float* br = Bs + (2 * s + h) * LDT + wn * 64 + l31;
            const float a0 = ar[0], a1 = ar[32], b0 = br[0], b1 = br[32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    float* P = part + (size_t)slice * N1 * N2;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = bn + wn * 64 + j * 32 + l31;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = mfma32_row(e, h, bm + wm * 64 + i * 32);
                P[(size_t)m * N2 + n] = acc[i][j][e];
            }
    }
}

// any N1, N2 (e.g. N2 = 6): thread per output element, loops over its K-slice
__global__ __launch_bounds__(256) void gemm_atb_generic_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                               float* __restrict__ part, long long K, int N1, int N2,
                                                               long long kslice) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= N1 * N2) return;
    const int m = id / N2, n = id % N2, slice = blockIdx.y;
    const long long k0 = (long long)slice * kslice;
    long long k1 = k0 + kslice;
    if (k1 > K) k1 = K;
    float s = 0.f;
    for (long long r = k0; r < k1; ++r) s = fmaf(A[r * N1 + m], B[r * N2 + n], s);
    part[(size_t)slice * N1 * N2 + id] = s;
}

// N2 <= 8 (the first edge-MLP layer's weight gradient: N2 = 6 edge attributes): thread per column of A, so that a
// row of A is read as whole lines (the kernel above reads each element of A from N2 threads and 172 B of every
// KiB of a row per wave); four rows in flight per thread.  Each (m, n) sum runs over its slice's rows in ascending
// order, as above.
__global__ __launch_bounds__(256) void gemm_atb_smalln_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                              float* __restrict__ part, long long K, int N1, int N2,
                                                              long long kslice) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= N1) return;
    const int slice = blockIdx.y;
    const long long k0 = (long long)slice * kslice;
    long long k1 = k0 + kslice;
    if (k1 > K) k1 = K;
    float s[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) s[n] = 0.f;
    long long r = k0;
    for (; r + 4 <= k1; r += 4) {
        float a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = A[(r + u) * N1 + m];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int n = 0; n < 8; ++n)
                if (n < N2) s[n] = fmaf(a[u], B[(r + u) * N2 + n], s[n]);
    }
    for (; r < k1; ++r) {
        const float a = A[r * N1 + m];
#pragma unroll
        for (int n = 0; n < 8; ++n)
            if (n < N2) s[n] = fmaf(a, B[r * N2 + n], s[n]);
    }
#pragma unroll
    for (int n = 0; n < 8; ++n)
        if (n < N2) part[((size_t)slice * N1 + m) * N2 + n] = s[n];
}

// column sums of A [K,N] in fixed order: part[slice][N] then reduce_slices
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ A, float* __restrict__ part, long long K,
                                                     int N, long long kslice) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int slice = blockIdx.y;
    const long long k0 = (long long)slice * kslice;
    long long k1 = k0 + kslice;
    if (k1 > K) k1 = K;
    float s = 0.f;
    for (long long r = k0; r < k1; ++r) s += A[r * N + n];
    part[(size_t)slice * N + n] = s;
}

// the same sums (each column over its slice's rows, ascending) with four adjacent columns per thread — 16-B loads —
// and four rows in flight: N % 4 == 0, 16-byte aligned A
__global__ __launch_bounds__(256) void colsum4_kernel(const float* __restrict__ A, float* __restrict__ part, long long K,
                                                      int N, long long kslice) {
    const int n = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (n >= N) return;
    const int slice = blockIdx.y;
    const long long k0 = (long long)slice * kslice;
    long long k1 = k0 + kslice;
    if (k1 > K) k1 = K;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    long long r = k0;
    for (; r + 4 <= k1; r += 4) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(A + (size_t)(r + u) * N + n);
#pragma unroll
        for (int u = 0; u < 4; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
    }
    for (; r < k1; ++r) {
        const float4 v = *reinterpret_cast<const float4*>(A + (size_t)r * N + n);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(part + (size_t)slice * N + n) = s;
}

// out = g * (y > 0) [* scale[row]]
__global__ __launch_bounds__(256) void relu_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                       const float* __restrict__ row_scale, float* __restrict__ out,
                                                       long long rows, int N) {
    const long long id = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (id >= rows * N) return;
    const float4 gv = *reinterpret_cast<const float4*>(g + id);
    const float4 yv = *reinterpret_cast<const float4*>(y + id);
    const float sc = row_scale ? row_scale[id / N] : 1.f;
    float4 o;
    o.x = yv.x > 0.f ? gv.x * sc : 0.f;
    o.y = yv.y > 0.f ? gv.y * sc : 0.f;
    o.z = yv.z > 0.f ? gv.z * sc : 0.f;
    o.w = yv.w > 0.f ? gv.w * sc : 0.f;
    *reinterpret_cast<float4*>(out + id) = o;
}

// the same for a row length that is not a multiple of 4 (an edge-MLP of any ker_width): one element per thread
__global__ __launch_bounds__(256) void relu_bwd_scalar_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                              const float* __restrict__ row_scale, float* __restrict__ out,
                                                              long long rows, int N) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= rows * N) return;
    const float sc = row_scale ? row_scale[id / N] : 1.f;
    out[id] = y[id] > 0.f ? g[id] * sc : 0.f;
}

// both at once: gz = g * (y > 0) and gs = gz * scale[row] — what the conv backward needs of one application
// (d root, d bias read gz; the input and edge-weight gradients read gs = gz / max(deg,1)); same arithmetic as two calls
__global__ __launch_bounds__(256) void relu_bwd2_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                        const float* __restrict__ row_scale, float* __restrict__ gz,
                                                        float* __restrict__ gs, long long rows, int N) {
    const long long id = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (id >= rows * N) return;
    const float4 gv = *reinterpret_cast<const float4*>(g + id);
    const float4 yv = *reinterpret_cast<const float4*>(y + id);
    const float sc = row_scale[id / N];
    float4 a, b;
    a.x = yv.x > 0.f ? gv.x : 0.f; b.x = yv.x > 0.f ? gv.x * sc : 0.f;
    a.y = yv.y > 0.f ? gv.y : 0.f; b.y = yv.y > 0.f ? gv.y * sc : 0.f;
    a.z = yv.z > 0.f ? gv.z : 0.f; b.z = yv.z > 0.f ? gv.z * sc : 0.f;
    a.w = yv.w > 0.f ? gv.w : 0.f; b.w = yv.w > 0.f ? gv.w * sc : 0.f;
    *reinterpret_cast<float4*>(gz + id) = a;
    *reinterpret_cast<float4*>(gs + id) = b;
}

__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ A, float* __restrict__ At, int R, int Cc) {
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int i = ty; i < 32; i += 8)
        if (by + i < R && bx + tx < Cc) tile[i][tx] = A[(size_t)(by + i) * Cc + bx + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (bx + i < Cc && by + tx < R) At[(size_t)(bx + i) * R + by + tx] = tile[tx][i];
}

constexpr int kSlices = 16;      // fixed K-split of the A^T.B reductions (partials added in slice order)
constexpr int kColSlices = 128;  // column sums: many more slices (the reduction is a pure stream)

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" int mdno_linear_fwd(const float* a, const float* w, const float* bias, int64_t rows, int n, int k,
                               int relu, float* c, void* stream) {
    MDNO_REQUIRE(a && w && c && rows > 0 && n > 0 && k > 0, MDNO_EINVAL, "mdno_linear_fwd: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool mfma = n % 128 == 0 && k % 32 == 0 && rows < (1ll << 31) &&
                      ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(w)) & 15) == 0;
    if (mfma) {
        const size_t lds = sizeof(float) * 2 * 256 * LD;
        static std::atomic<unsigned long long> raised_relu{0}, raised_plain{0};
        MDNO_TRY(raise_dynamic_lds(reinterpret_cast<const void*>(&linear_mfma_kernel<true>), (int)lds, raised_relu));
        MDNO_TRY(raise_dynamic_lds(reinterpret_cast<const void*>(&linear_mfma_kernel<false>), (int)lds, raised_plain));
        dim3 grid(n / 128, (unsigned)((rows + 127) / 128));
        if (relu) hipLaunchKernelGGL(linear_mfma_kernel<true>, grid, dim3(256), lds, s, a, w, bias, c, (int)rows, n, k);
        else hipLaunchKernelGGL(linear_mfma_kernel<false>, grid, dim3(256), lds, s, a, w, bias, c, (int)rows, n, k);
    } else {
        const unsigned nb = (unsigned)((rows * n + 255) / 256);
        if (relu) hipLaunchKernelGGL(linear_generic_kernel<true>, dim3(nb), dim3(256), 0, s, a, w, bias, c, (long long)rows, n, k);
        else hipLaunchKernelGGL(linear_generic_kernel<false>, dim3(nb), dim3(256), 0, s, a, w, bias, c, (long long)rows, n, k);
    }
    return check_launch("mdno_linear_fwd");
}

extern "C" size_t mdno_linear_split_workspace_bytes(int64_t rows, int n, int k) {
    return rows > 0 && n > 0 && k > 0 ? split_linear_workspace_bytes((long long)rows, n, k) : 0;
}

extern "C" int mdno_linear_split_fwd(const float* a, const float* w, const float* bias, int64_t rows, int n, int k,
                                     int relu, float* c, void* workspace, size_t workspace_bytes, void* stream) {
    MDNO_REQUIRE(a && w && c && workspace && rows > 0 && n > 0 && k > 0, MDNO_EINVAL,
                 "mdno_linear_split_fwd: bad arguments");
    MDNO_REQUIRE(split_linear_supported((long long)rows, n, k) &&
                     ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(w)) & 15) == 0,
                 MDNO_EUNSUPPORTED, "mdno_linear_split_fwd: needs k %% 32 == 0, n %% 128 == 0, 16-byte aligned operands "
                 "(rows=%lld n=%d k=%d); use mdno_linear_fwd", (long long)rows, n, k);
    MDNO_REQUIRE(workspace_bytes >= split_linear_workspace_bytes((long long)rows, n, k), MDNO_EWORKSPACE,
                 "mdno_linear_split_fwd: workspace");
    return split_linear(a, w, bias, (long long)rows, n, k, relu, c, workspace, static_cast<hipStream_t>(stream));
}

extern "C" size_t mdno_linear_split_f16_workspace_bytes(int64_t rows, int n, int k) {
    return rows > 0 && n > 0 && k > 0 ? split_linear_f16_workspace_bytes((long long)rows, n, k) : 0;
}

extern "C" int mdno_linear_split_f16_fwd(const float* a, const float* w, const float* bias, int64_t rows, int n, int k,
                                         int relu, float* c, void* workspace, size_t workspace_bytes, void* stream) {
    MDNO_REQUIRE(a && w && c && workspace && rows > 0 && n > 0 && k > 0, MDNO_EINVAL,
                 "mdno_linear_split_f16_fwd: bad arguments");
    MDNO_REQUIRE(split_linear_supported((long long)rows, n, k) &&
                     ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(w)) & 15) == 0,
                 MDNO_EUNSUPPORTED, "mdno_linear_split_f16_fwd: needs k %% 32 == 0, n %% 128 == 0, 16-byte aligned "
                 "operands (rows=%lld n=%d k=%d); use mdno_linear_fwd", (long long)rows, n, k);
    MDNO_REQUIRE(workspace_bytes >= split_linear_f16_workspace_bytes((long long)rows, n, k), MDNO_EWORKSPACE,
                 "mdno_linear_split_f16_fwd: workspace");
    return split_linear_f16(a, w, bias, (long long)rows, n, k, relu, c, workspace, static_cast<hipStream_t>(stream));
}

extern "C" int mdno_gemm_atb_split_f16_supported(int64_t rows, int n1, int n2) {
    return gemm_atb_f16_supported((long long)rows, n1, n2) ? 1 : 0;
}

extern "C" size_t mdno_gemm_atb_split_f16_workspace_bytes(int64_t rows, int n1, int n2) {
    return gemm_atb_f16_supported((long long)rows, n1, n2) ? gemm_atb_f16_workspace_bytes((long long)rows, n1, n2) : 0;
}

extern "C" int mdno_gemm_atb_split_f16(const float* a, const float* b, int64_t rows, int n1, int n2, float* c, int accumulate,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    MDNO_REQUIRE(a && b && c && workspace && rows > 0, MDNO_EINVAL, "mdno_gemm_atb_split_f16: bad arguments");
    MDNO_REQUIRE(gemm_atb_f16_supported((long long)rows, n1, n2) &&
                     ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0,
                 MDNO_EUNSUPPORTED, "mdno_gemm_atb_split_f16: needs n1 %% 256 == 0, n2 %% 256 == 0, 16-byte aligned operands "
                 "(rows=%lld n1=%d n2=%d); use mdno_gemm_atb", (long long)rows, n1, n2);
    MDNO_REQUIRE(workspace_bytes >= gemm_atb_f16_workspace_bytes((long long)rows, n1, n2), MDNO_EWORKSPACE,
                 "mdno_gemm_atb_split_f16: workspace");
    return gemm_atb_f16(a, b, (long long)rows, n1, n2, c, accumulate, workspace, static_cast<hipStream_t>(stream));
}

extern "C" size_t mdno_reduce_workspace_bytes(int n1, int n2) {
    if (n2 <= 1) return align_up((size_t)kColSlices * (size_t)n1 * sizeof(float), 256);
    if (n2 <= 8) return align_up((size_t)kColSlices * (size_t)n1 * (size_t)n2 * sizeof(float), 256);   // gemm_atb_smalln_kernel
    return align_up((size_t)kSlices * (size_t)n1 * (size_t)n2 * sizeof(float), 256);
}

extern "C" int mdno_gemm_atb(const float* a, const float* b, int64_t rows, int n1, int n2, float* c, int accumulate,
                             void* workspace, size_t workspace_bytes, void* stream) {
    MDNO_REQUIRE(a && b && c && workspace && rows > 0 && n1 > 0 && n2 > 0, MDNO_EINVAL, "mdno_gemm_atb: bad arguments");
    MDNO_REQUIRE(workspace_bytes >= mdno_reduce_workspace_bytes(n1, n2), MDNO_EWORKSPACE, "mdno_gemm_atb: workspace");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(workspace);
    long long kslice = (rows + kSlices - 1) / kSlices;
    kslice = (kslice + BK - 1) / BK * BK;
    const bool mfma = n1 % 128 == 0 && n2 % 128 == 0 &&
                      ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
    if (!mfma && n2 <= 8) {      // few columns of B: a stream over A, many more slices
        const long long ks = (rows + kColSlices - 1) / kColSlices;
        hipLaunchKernelGGL(gemm_atb_smalln_kernel, dim3((n1 + 255) / 256, kColSlices), dim3(256), 0, s, a, b, part,
                           (long long)rows, n1, n2, ks);
        const long long cnt = (long long)n1 * n2;
        launch_reduce_slices((const float*)part, kColSlices, cnt, c, accumulate, s);
        return check_launch("mdno_gemm_atb");
    }
    if (mfma)
        hipLaunchKernelGGL(gemm_atb_mfma_kernel, dim3(n2 / 128, n1 / 128, kSlices), dim3(256), 0, s, a, b, part,
                           (long long)rows, n1, n2, kslice);
    else
        hipLaunchKernelGGL(gemm_atb_generic_kernel, dim3((n1 * n2 + 255) / 256, kSlices), dim3(256), 0, s, a, b, part,
                           (long long)rows, n1, n2, kslice);
    const long long count = (long long)n1 * n2;
    launch_reduce_slices((const float*)part, kSlices, count, c, accumulate, s);
    return check_launch("mdno_gemm_atb");
}

extern "C" int mdno_colsum(const float* a, int64_t rows, int n, float* out, int accumulate, void* workspace,
                           size_t workspace_bytes, void* stream) {
    MDNO_REQUIRE(a && out && workspace && rows > 0 && n > 0, MDNO_EINVAL, "mdno_colsum: bad arguments");
    MDNO_REQUIRE(workspace_bytes >= mdno_reduce_workspace_bytes(n, 1), MDNO_EWORKSPACE, "mdno_colsum: workspace");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(workspace);
    const long long kslice = (rows + kColSlices - 1) / kColSlices;
    if (n % 4 == 0 && (reinterpret_cast<uintptr_t>(a) & 15) == 0)
        hipLaunchKernelGGL(colsum4_kernel, dim3((n / 4 + 255) / 256, kColSlices), dim3(256), 0, s, a, part, (long long)rows, n,
                           kslice);
    else
        hipLaunchKernelGGL(colsum_kernel, dim3((n + 255) / 256, kColSlices), dim3(256), 0, s, a, part, (long long)rows, n,
                           kslice);
    launch_reduce_slices((const float*)part, kColSlices, (long long)n, out, accumulate, s);
    return check_launch("mdno_colsum");
}

extern "C" int mdno_relu_bwd(const float* g, const float* y, const float* row_scale, int64_t rows, int n, float* out,
                             void* stream) {
    MDNO_REQUIRE(g && y && out && rows > 0 && n > 0, MDNO_EINVAL, "mdno_relu_bwd: bad arguments");
    if (n % 4 || ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out)) & 15)) {
        const long long count = rows * n;
        hipLaunchKernelGGL(relu_bwd_scalar_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), g, y, row_scale, out, (long long)rows, n);
        return check_launch("mdno_relu_bwd");
    }
    const long long quads = rows * n / 4;
    hipLaunchKernelGGL(relu_bwd_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), g, y, row_scale, out, (long long)rows, n);
    return check_launch("mdno_relu_bwd");
}

extern "C" int mdno_relu_bwd2(const float* g, const float* y, const float* row_scale, int64_t rows, int n, float* gz,
                              float* gs, void* stream) {
    MDNO_REQUIRE(g && y && row_scale && gz && gs && rows > 0 && n > 0 && n % 4 == 0, MDNO_EINVAL,
                 "mdno_relu_bwd2: bad arguments (n % 4)");
    // the kernel reads and writes 16 bytes at a time and has no one-element form: refuse before any launch
    MDNO_REQUIRE(((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(gz) |
                   reinterpret_cast<uintptr_t>(gs)) & 15) == 0,
                 MDNO_EINVAL, "mdno_relu_bwd2: g, y, gz and gs must be 16-byte aligned");
    const long long quads = rows * n / 4;
    hipLaunchKernelGGL(relu_bwd2_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), g, y, row_scale, gz, gs, (long long)rows, n);
    return check_launch("mdno_relu_bwd2");
}

extern "C" int mdno_transpose(const float* a, int rows, int cols, float* at, void* stream) {
    MDNO_REQUIRE(a && at && rows > 0 && cols > 0, MDNO_EINVAL, "mdno_transpose: bad arguments");
    hipLaunchKernelGGL(transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a, at, rows, cols);
    return check_launch("mdno_transpose");
}
