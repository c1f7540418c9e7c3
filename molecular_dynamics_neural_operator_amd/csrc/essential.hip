// Essential dynamics on the device (include/mdno_essential.h states the rules and every summation order):
// superposition onto one reference with the rotated frames handed back, column sums, the feature x feature second-moment
// matrix at a time lag, and the projection onto chosen directions (forecast.py: superpose, covariance, pca, tica, project).
//
//   pca_superpose_kernel   one wave per frame: centroids, g and the nine cross moments in the FRAME ORDER (lane partials,
//                          xor butterfly), rotation_from_moments of superpose.h on every lane (the same bits), then the
//                          lanes rotate their atoms.
//   pca_sums_kernel        a workgroup owns 16 columns: thread (column c, partial t) adds rows t, t + 16, ...; the 16 partials
//                          of a column are added in ascending t.  pca_rows_kernel counts the rows with a non-finite value
//                          (one wave per row at a time; an integer atomic, exact in any order).
//   pca_cov_kernel         THE HOT KERNEL.  A workgroup of four waves owns one kTile x kTile tile of C and one split of the
//                          rows.  Per pass of kPass rows every thread reads fp32 values of ONE feature per side (one pass
//                          ahead, into registers: the read's latency passes under the MFMAs), centres them in fp64 on the
//                          way and writes them to LDS, lds[side][row of the pass][feature of the tile] (rows past the
//                          split's end and features past D as zeros); no centred fp64 copy of a row ever reaches global
//                          memory.  Side A is row r, side B row r + lag M of the flat [S M, D] matrix.  Wave (wr, wc) owns
//                          the 16 x 16 elements of tile rows 16 wr .. and tile columns 16 wc ..: per group of four rows it
//                          reads one A value and one B value per lane (A operand: feature lane & 15, row lane >> 4 of the
//                          group; B the same) and issues one MFMA.  The f64 C/D map is col = lane & 15,
//                          row = (lane >> 4) + 4 reg — NOT the f32 one.  The partial tile goes to the workspace,
//                          part[tile][split][row][col].
//   pca_cov_sum_kernel     one workgroup per tile: each thread adds the partials of four elements in ascending split order
//                          and writes C; at lag 0 only the elements a <= b, each to C[a, b] and C[b, a].
//   pca_project_kernel     a workgroup owns 16 rows: 64 features at a time are centred into LDS, thread (row, c) adds the
//                          terms of components c and c + 16 in ascending feature order.
// LDS of the hot kernel: 2 sides x 32 rows x 48 (32 + padding: the four row groups of an operand read fall on disjoint
// banks per half wave) x 8 B = 24 KiB.
#include "common.h"
#include "reduce.h"
#include "superpose.h"
#include "../../include/mdno_essential.h"

namespace mdno {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = MDNO_PCA_TILE;
constexpr int kPass = MDNO_PCA_ROW_PASS;
constexpr int kLd = kTile + 16;                           // LDS row stride in doubles
constexpr int kSumPartials = MDNO_PCA_SUM_PARTIALS;
constexpr int kSumCols = kThreads / kSumPartials;         // columns per workgroup of pca_sums_kernel
constexpr int kProjRows = 16, kProjFeat = 64;
static_assert(kTile == 32 && kThreads == 256, "four waves, each 16 x 16 elements of a 32 x 32 tile");
static_assert(kPass % 4 == 0 && kTile * kPass == 4 * kThreads, "a thread stages four rows of one feature per side and pass");
static_assert(MDNO_PCA_ROW_CHUNK % kPass == 0, "a split is a whole number of passes");
static_assert(kSumCols == 16 && MDNO_PCA_MAX_COMPONENTS == 32, "thread maps of pca_sums_kernel and pca_project_kernel");

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef unsigned __int128 u128;

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ double nan_d() { return __longlong_as_double(0x7ff8000000000000ll); }

// ------------------------------------------------------------------------------------------------ superposition
// one wave per frame (flat (s, m)); aligned and rmsd may each be null
__global__ __launch_bounds__(kThreads) void pca_superpose_kernel(const float* __restrict__ frames, long long F, int N,
                                                                 const float* __restrict__ ref, float* __restrict__ aligned,
                                                                 double* __restrict__ rmsd) {
    const int lane = threadIdx.x & 63;
    const long long id = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (id >= F) return;                                  // (the whole wave)
    const float* p = frames + (size_t)id * N * 3;
    double sp[3] = {0.0, 0.0, 0.0}, sq[3] = {0.0, 0.0, 0.0};
    int bad = 0;
    for (int k = lane; k < N; k += 64) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float v = p[3 * (size_t)k + d], w = ref[3 * (size_t)k + d];
            bad |= !finite_f(v) || !finite_f(w);
            sp[d] += (double)v;
            sq[d] += (double)w;
        }
    }
    double cp[3], cq[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        cp[d] = wave_reduce_add(sp[d]) / (double)N;
        cq[d] = wave_reduce_add(sq[d]) / (double)N;
    }
    double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double gp = 0.0, gq = 0.0;
    for (int k = lane; k < N; k += 64) {
        double a[3], b[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            a[d] = (double)p[3 * (size_t)k + d] - cp[d];
            b[d] = (double)ref[3 * (size_t)k + d] - cq[d];
        }
        gp += (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
        gq += (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) s[3 * r + c] += a[r] * b[c];
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) s[e] = wave_reduce_add(s[e]);
    gp = wave_reduce_add(gp);
    gq = wave_reduce_add(gq);
    bad = wave_reduce_add(bad);
    double rot[9];
    const double lam = rotation_from_moments(s, rot);
    if (rmsd != nullptr && lane == 0) {
        const double r2 = ((gp + gq) - 2.0 * lam) / (double)N;
        rmsd[id] = bad ? nan_d() : sqrt(r2 < 0.0 ? 0.0 : r2);
    }
    if (aligned == nullptr) return;
    float* o = aligned + (size_t)id * N * 3;
    for (int k = lane; k < N; k += 64) {
        double a[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) a[d] = (double)p[3 * (size_t)k + d] - cp[d];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double v = ((rot[3 * d] * a[0] + rot[3 * d + 1] * a[1]) + rot[3 * d + 2] * a[2]) + cq[d];
            o[3 * (size_t)k + d] = bad ? __int_as_float(0x7fc00000) : (float)v;
        }
    }
}

__global__ __launch_bounds__(kThreads) void pca_fill_kernel(double* __restrict__ v, long long count, double value) {
    for (long long id = (long long)blockIdx.x * kThreads + threadIdx.x; id < count; id += (long long)gridDim.x * kThreads) v[id] = value;
}

// ------------------------------------------------------------------------------------------------ column sums
// grid ceil(D / 16): thread (c = tid & 15, t = tid >> 4)
__global__ __launch_bounds__(kThreads) void pca_sums_kernel(const float* __restrict__ x, long long R, int D, double* __restrict__ sum) {
    __shared__ double part[kSumPartials][kSumCols];
    __shared__ int flag[kSumPartials][kSumCols];
    const int c = threadIdx.x & (kSumCols - 1), t = threadIdx.x >> 4;
    const long long col = (long long)blockIdx.x * kSumCols + c;
    double acc = 0.0;
    int bad = 0;
    if (col < D) {
        long long r = t;
        for (; r + 3 * kSumPartials < R; r += 4 * kSumPartials) {       // four loads in flight, added in row order
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = x[(size_t)(r + u * kSumPartials) * D + col];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bad |= !finite_f(v[u]);
                acc += (double)v[u];
            }
        }
        for (; r < R; r += kSumPartials) {
            const float v = x[(size_t)r * D + col];
            bad |= !finite_f(v);
            acc += (double)v;
        }
    }
    part[t][c] = acc;
    flag[t][c] = bad;
    __syncthreads();
    if (t == 0 && col < D) {
        double total = part[0][c];
        int any = flag[0][c];
        for (int u = 1; u < kSumPartials; ++u) {
            total += part[u][c];
            any |= flag[u][c];
        }
        sum[col] = any ? nan_d() : total;
    }
}

// rows with a non-finite value: a wave per row at a time, one integer atomic per workgroup
__global__ __launch_bounds__(kThreads) void pca_rows_kernel(const float* __restrict__ x, long long R, int D,
                                                            unsigned long long* __restrict__ n_invalid) {
    __shared__ unsigned long long slots[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long count = 0;
    for (long long r = (long long)blockIdx.x * (kThreads / 64) + wave; r < R; r += (long long)gridDim.x * (kThreads / 64)) {
        int bad = 0;
        for (int a = lane; a < D; a += 64) bad |= !finite_f(x[(size_t)r * D + a]);
        bad = wave_reduce_add(bad);
        count += bad != 0;
    }
    if (lane == 0) slots[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (int w = 0; w < kThreads / 64; ++w) total += slots[w];
        if (total) atomicAdd(n_invalid, total);
    }
}

// ------------------------------------------------------------------------------------------------ covariance
struct CovPlan {
    long long K = 0, T = 0, tiles = 0, L = 0, splits = 0;
    bool fits = true;                                     // tiles * splits is a launch grid
    CovPlan(int S, int M, int D, int lag) {
        K = lag < S ? (long long)M * (S - lag) : 0;
        T = ((long long)D + kTile - 1) / kTile;
        tiles = lag == 0 ? T * (T + 1) / 2 : T * T;
        if (K == 0 || tiles == 0) return;
        long long want = (MDNO_PCA_TARGET_WORKGROUPS + tiles - 1) / tiles;
        want = want < 1 ? 1 : want > MDNO_PCA_MAX_SPLITS ? MDNO_PCA_MAX_SPLITS : want;
        const long long unit = want * MDNO_PCA_ROW_CHUNK;
        L = MDNO_PCA_ROW_CHUNK * ((K + unit - 1) / unit);
        splits = (K + L - 1) / L;
        fits = (u128)tiles * (u128)splits < ((u128)1 << 31) - 1;
    }
};

size_t cov_workspace_bound(int D) {
    const u128 T = ((u128)D + kTile - 1) / kTile, t2 = T * T;
    const u128 a = t2 * MDNO_PCA_MAX_SPLITS, b = t2 + MDNO_PCA_TARGET_WORKGROUPS;
    const u128 bytes = (a < b ? a : b) * (u128)(kTile * kTile * sizeof(double));
    return bytes > (u128)SIZE_MAX ? SIZE_MAX : (size_t)bytes;
}

// grid tiles * splits (split fastest).  x is the flat [rows, D] matrix; term r of the split pairs row r with row r + shift.
__global__ __launch_bounds__(kThreads) void pca_cov_kernel(const float* __restrict__ x, int D, const double* __restrict__ mean,
                                                           long long K, long long shift, long long L, int splits, int T,
                                                           int upper, double* __restrict__ part) {
    __shared__ double lds[2 * kPass * kLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int split = blockIdx.x % splits;
    int t = blockIdx.x / splits, ta = 0, tb = 0;
    if (upper) {                                          // tile t of the upper triangle, row by row
        while (t >= T - ta) t -= T - ta, ++ta;
        tb = ta + t;
    } else {
        ta = t / T, tb = t % T;
    }
    const long long r0 = (long long)split * L, r1 = r0 + L < K ? r0 + L : K;

    // staging role: feature f of the tile on both sides, rows g0 .. g0 + 3 of every pass
    const int f = tid & (kTile - 1), g0 = (tid >> 5) * 4;
    const long long fa = (long long)ta * kTile + f, fb = (long long)tb * kTile + f;
    const bool use_a = fa < D, use_b = fb < D;
    const double ma = use_a ? mean[fa] : 0.0, mb = use_b ? mean[fb] : 0.0;
    const float* pa = x + (use_a ? fa : 0);
    const float* pb = x + (size_t)shift * D + (use_b ? fb : 0);

    // MFMA role
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    double* la = lds;
    double* lb = lds + kPass * kLd;

    // the fp32 values of a pass are read one pass ahead, so that their latency passes under the MFMAs
    float ra[4], rb[4];
    auto fetch = [&](long long k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long r = k0 + g0 + i;
            ra[i] = use_a && r < r1 ? pa[(size_t)r * D] : 0.f;
            rb[i] = use_b && r < r1 ? pb[(size_t)r * D] : 0.f;
        }
    };
    fetch(r0);
    for (long long k0 = r0; k0 < r1; k0 += kPass) {
        __syncthreads();                                  // the last pass's operands have been read
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = k0 + g0 + i < r1;
            la[(g0 + i) * kLd + f] = use_a && in ? (double)ra[i] - ma : 0.0;
            lb[(g0 + i) * kLd + f] = use_b && in ? (double)rb[i] - mb : 0.0;
        }
        fetch(k0 + kPass);                                // (past the end: zeros, never used)
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kPass / 4; ++kk) {
            const int k = kk * 4 + l4;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(la[k * kLd + wr * 16 + l15], lb[k * kLd + wc * 16 + l15], acc, 0, 0, 0);
        }
    }
    // register slot i: the element (row l4 + 4 i, column l15) of the wave's 16 x 16
    double* out = part + (size_t)blockIdx.x * (kTile * kTile);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[(wr * 16 + l4 + 4 * i) * kTile + wc * 16 + l15] = acc[i];
}

// grid tiles: thread -> row tid >> 3, columns (tid & 7) * 4 .. + 3 of the tile
__global__ __launch_bounds__(kThreads) void pca_cov_sum_kernel(const double* __restrict__ part, int D, int splits, int T, int upper,
                                                               double* __restrict__ c) {
    int t = blockIdx.x, ta = 0, tb = 0;
    if (upper) {
        while (t >= T - ta) t -= T - ta, ++ta;
        tb = ta + t;
    } else {
        ta = t / T, tb = t % T;
    }
    const int row = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * 4;
    const double* src = part + (size_t)blockIdx.x * splits * (kTile * kTile) + row * kTile + c0;
    double s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = src[q];
    for (int i = 1; i < splits; ++i) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += src[(size_t)i * (kTile * kTile) + q];
    }
    const long long a = (long long)ta * kTile + row;
    if (a >= D) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long long b = (long long)tb * kTile + c0 + q;
        if (b >= D || (upper && b < a)) continue;
        c[(size_t)a * D + b] = s[q];
        if (upper) c[(size_t)b * D + a] = s[q];
    }
}

// ------------------------------------------------------------------------------------------------ projection
// grid ceil(R / 16): thread (row tid >> 4, components tid & 15 and (tid & 15) + 16)
__global__ __launch_bounds__(kThreads) void pca_project_kernel(const float* __restrict__ x, long long R, int D,
                                                               const double* __restrict__ mean, const double* __restrict__ v, int k,
                                                               double* __restrict__ p) {
    __shared__ double xs[kProjRows][kProjFeat + 1];
    const int tid = threadIdx.x, row = tid >> 4, c = tid & 15;
    const long long r_base = (long long)blockIdx.x * kProjRows;
    double acc0 = 0.0, acc1 = 0.0;
    for (int a0 = 0; a0 < D; a0 += kProjFeat) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kProjRows * kProjFeat / kThreads; ++i) {
            const int e = i * kThreads + tid, rr = e / kProjFeat, ff = e % kProjFeat;
            const long long r = r_base + rr;
            const int a = a0 + ff;
            xs[rr][ff] = r < R && a < D ? (double)x[(size_t)r * D + a] - mean[a] : 0.0;
        }
        __syncthreads();
        const int n = D - a0 < kProjFeat ? D - a0 : kProjFeat;
        for (int ff = 0; ff < n; ++ff) {
            const double xv = xs[row][ff];
            const double* vr = v + (size_t)(a0 + ff) * k;
            if (c < k) acc0 += xv * vr[c];
            if (c + 16 < k) acc1 += xv * vr[c + 16];
        }
    }
    const long long r = r_base + row;
    if (r < R) {
        if (c < k) p[(size_t)r * k + c] = acc0;
        if (c + 16 < k) p[(size_t)r * k + c + 16] = acc1;
    }
}

unsigned capped_blocks(long long count, long long per) {
    const long long blocks = (count + per - 1) / per;
    return (unsigned)(blocks < 1 ? 1 : blocks < (1 << 20) ? blocks : (1 << 20));
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" int mdnopca_superpose(const float* frames, int S, int M, int N, const float* reference, float* aligned, double* rmsd,
                                 void* stream) {
    const char* who = "superpose";
    MDNO_REQUIRE(S >= 0 && M >= 0 && N >= 0, MDNO_EINVAL, "%s: S=%d M=%d N=%d", who, S, M, N);
    MDNO_REQUIRE(aligned || rmsd, MDNO_EINVAL, "%s: no output was asked for", who);
    const long long F = (long long)S * M;
    if (F == 0) return MDNO_OK;
    MDNO_REQUIRE((frames && reference) || N == 0, MDNO_EINVAL, "%s: null pointer (frames or reference)", who);
    const long long blocks = (F + 3) / 4;
    MDNO_REQUIRE(blocks < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "%s: %lld frames exceed the launch grid", who, F);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (N == 0) {       // frames without atoms: nothing to rotate, every rmsd 0
        if (rmsd == nullptr) return MDNO_OK;
        hipLaunchKernelGGL(pca_fill_kernel, dim3(capped_blocks(F, kThreads)), dim3(kThreads), 0, st, rmsd, F, 0.0);
        return check_launch(who);
    }
    hipLaunchKernelGGL(pca_superpose_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, frames, F, N, reference, aligned, rmsd);
    return check_launch(who);
}

extern "C" int mdnopca_feature_sums(const float* x, int64_t R, int D, double* sum, int64_t* n_invalid, void* stream) {
    const char* who = "feature_sums";
    MDNO_REQUIRE(R >= 0 && D >= 0, MDNO_EINVAL, "%s: R=%lld D=%d", who, (long long)R, D);
    MDNO_REQUIRE(n_invalid != nullptr, MDNO_EINVAL, "%s: null pointer (n_invalid)", who);
    MDNO_REQUIRE(sum || D == 0, MDNO_EINVAL, "%s: null pointer (sum)", who);
    MDNO_REQUIRE(x || R == 0 || D == 0, MDNO_EINVAL, "%s: null pointer (x)", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    MDNO_HIP(hipMemsetAsync(n_invalid, 0, sizeof(int64_t), st));
    if (D == 0) return MDNO_OK;
    hipLaunchKernelGGL(pca_sums_kernel, dim3((unsigned)((D + kSumCols - 1) / kSumCols)), dim3(kThreads), 0, st, x, (long long)R, D, sum);
    MDNO_TRY(check_launch(who));
    if (R == 0) return MDNO_OK;
    hipLaunchKernelGGL(pca_rows_kernel, dim3(capped_blocks(R, 4 * 8)), dim3(kThreads), 0, st, x, (long long)R, D,
                       reinterpret_cast<unsigned long long*>(n_invalid));
    return check_launch(who);
}

extern "C" size_t mdnopca_covariance_workspace_bytes(int S, int M, int D, int lag) {
    if (S < 0 || M < 0 || D < 0 || lag < 0) return 0;
    return cov_workspace_bound(D);
}

extern "C" int mdnopca_covariance(const float* x, int S, int M, int D, const double* mean, int lag, double* c, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    const char* who = "covariance";
    MDNO_REQUIRE(S >= 0 && M >= 0 && D >= 0 && lag >= 0, MDNO_EINVAL, "%s: S=%d M=%d D=%d lag=%d", who, S, M, D, lag);
    MDNO_REQUIRE(c || D == 0, MDNO_EINVAL, "%s: null pointer (c)", who);
    if (D == 0) return MDNO_OK;
    const CovPlan plan(S, M, D, lag);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (plan.K == 0) {
        MDNO_REQUIRE((u128)D * (u128)D < ((u128)1 << 56), MDNO_EUNSUPPORTED, "%s: D=%d is too large", who, D);
        MDNO_HIP(hipMemsetAsync(c, 0, (size_t)D * (size_t)D * sizeof(double), st));
        return MDNO_OK;
    }
    MDNO_REQUIRE(x && mean, MDNO_EINVAL, "%s: null pointer (x or mean)", who);
    MDNO_REQUIRE(plan.fits, MDNO_EUNSUPPORTED, "%s: %lld tiles x %lld splits exceed the launch grid", who, plan.tiles, plan.splits);
    const size_t need = cov_workspace_bound(D);
    MDNO_REQUIRE(workspace && workspace_bytes >= need, MDNO_EINVAL, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    double* part = static_cast<double*>(workspace);
    const int upper = lag == 0;
    hipLaunchKernelGGL(pca_cov_kernel, dim3((unsigned)(plan.tiles * plan.splits)), dim3(kThreads), 0, st, x, D, mean, plan.K,
                       (long long)lag * M, plan.L, (int)plan.splits, (int)plan.T, upper, part);
    MDNO_TRY(check_launch(who));
    hipLaunchKernelGGL(pca_cov_sum_kernel, dim3((unsigned)plan.tiles), dim3(kThreads), 0, st, part, D, (int)plan.splits, (int)plan.T,
                       upper, c);
    return check_launch(who);
}

extern "C" int mdnopca_project(const float* x, int64_t R, int D, const double* mean, const double* v, int k, double* p, void* stream) {
    const char* who = "project";
    MDNO_REQUIRE(R >= 0 && D >= 0, MDNO_EINVAL, "%s: R=%lld D=%d", who, (long long)R, D);
    MDNO_REQUIRE(k >= 1 && k <= MDNO_PCA_MAX_COMPONENTS, MDNO_EINVAL, "%s: k=%d outside 1 .. %d", who, k, MDNO_PCA_MAX_COMPONENTS);
    MDNO_REQUIRE(p || R == 0, MDNO_EINVAL, "%s: null pointer (p)", who);
    MDNO_REQUIRE((x && mean && v) || R == 0 || D == 0, MDNO_EINVAL, "%s: null pointer (x, mean or v)", who);
    if (R == 0) return MDNO_OK;
    const long long blocks = (R + kProjRows - 1) / kProjRows;
    MDNO_REQUIRE(blocks < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "%s: R=%lld rows exceed the launch grid", who, (long long)R);
    hipLaunchKernelGGL(pca_project_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), x, (long long)R,
                       D, mean, v, k, p);
    return check_launch(who);
}
