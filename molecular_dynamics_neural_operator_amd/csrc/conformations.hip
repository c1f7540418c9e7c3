// Structural coverage on the device (include/mdno_conformations.h states THE RULE, the two summation orders and the
// position independence): the superposed RMSD of every frame of A f32 [S, M, N, 3] against every frame of
// B f32 [Fb, N, 3], and its row and per-member column minima (forecast.py: CrossRmsd).
//
// The nine cross-covariance sums of all pairs are one fp64 GEMM, [3 Fa, N] . [N, 3 Fb], on v_mfma_f64_16x16x4_f64; the
// eigen-solve per pair is rmsd2_from_moments of superpose.h, the one forecast.hip uses.  Three kernels:
//   conf_stats_kernel   one wave per frame of A and of B: {c[3], g, valid} into the workspace (FRAME ORDER of the header).
//   conf_pairs_kernel   a workgroup of four waves owns kTile = 32 consecutive STEPS of one member x 32 consecutive reference
//                       frames.  It walks the atoms in ascending chunks of kChunk = 32: every thread reads fp32 coordinates
//                       of one frame per side (one chunk ahead, into registers: the read's latency passes under the
//                       MFMAs), centres them in fp64 on the way and writes them PLANAR BY COMPONENT into
//                       LDS, lds[side][component][atom of the chunk][frame of the tile] (rows, columns and atoms past the
//                       end, and invalid frames, as zeros); no centred fp64 copy of a frame ever reaches global memory.
//                       Wave (wr, wc) owns the 16 x 16 pairs of rows 16 wr .. and columns 16 wc ..: per group of four atoms
//                       it reads three A values and three B values per lane (A operand: frame lane & 15, atom lane >> 4 of
//                       the group; B the same) and issues nine MFMAs, accumulator tile (r, c) = A_r . B_c^T = S_rc.  The
//                       f64 C/D map is col = lane & 15, row = (lane >> 4) + 4 reg — NOT the f32 one — so register slot i of
//                       a lane's nine accumulators holds all nine S_rc of ONE pair and the lane solves its four pairs with
//                       no lane movement.  The 32 x 32 results go through LDS: coalesced rows of `matrix`, and one
//                       (minimum, index) per row and per column of the tile, scanned in ascending order with a strict <, so
//                       the lowest index wins a tie.
//   conf_rows_kernel / conf_cols_kernel   the minima over the column tiles of a row, over the row tiles of a (member,
//                       column), in ascending tile order with a strict <.
// LDS: 2 sides x 3 components x 32 atoms x 32 frames x 8 B = 48 KiB, reused for the 32 x 33 result tile; two workgroups
// per CU (by registers: 114 VGPRs + 72 AGPRs), so one's staging and eigen-solves run under the other's MFMAs.
#include "common.h"
#include "reduce.h"
#include "superpose.h"
#include "../../include/mdno_conformations.h"

#include <limits>

namespace mdno {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = MDNO_CONF_FRAME_TILE;
constexpr int kChunk = MDNO_CONF_ATOM_CHUNK;
constexpr int kStat = 5;                                  // {c[3], g, valid} per frame
static_assert(kTile == 32 && kThreads == 256, "four waves, each 16 x 16 pairs of a 32 x 32 tile");
static_assert(kChunk % 4 == 0 && kTile * kChunk == 4 * kThreads, "a thread stages four atoms of one frame per side and chunk");

typedef double f64x4 __attribute__((ext_vector_type(4)));

// Measurement aid for scripts/micro/build_exp.sh (EXPERIMENTS.md says what it showed), 0 in the library: 1 leaves the
// eigen-solves out (a sum of the nine moments instead), 2 issues the MFMAs of one group of four atoms per chunk only.
#ifndef MDNO_EXP_CONF_SKIP
#define MDNO_EXP_CONF_SKIP 0
#endif

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ double nan_d() { return __longlong_as_double(0x7ff8000000000000ll); }

// one wave per frame: frames 0 .. FA-1 of a (flat (s, m)), then FB frames of b
__global__ __launch_bounds__(kThreads) void conf_stats_kernel(const float* __restrict__ a, long long FA, const float* __restrict__ b,
                                                              long long FB, int N, double* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const long long id = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (id >= FA + FB) return;                            // (the whole wave)
    const float* p = id < FA ? a + (size_t)id * N * 3 : b + (size_t)(id - FA) * N * 3;
    double sum[3] = {0.0, 0.0, 0.0};
    int bad = 0;
    for (int k = lane; k < N; k += 64) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float v = p[3 * (size_t)k + d];
            bad |= !finite_f(v);
            sum[d] += (double)v;
        }
    }
    double c[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) c[d] = wave_reduce_add(sum[d]) / (double)N;
    double g = 0.0;
    for (int k = lane; k < N; k += 64) {
        const double ax = (double)p[3 * (size_t)k] - c[0], ay = (double)p[3 * (size_t)k + 1] - c[1],
                     az = (double)p[3 * (size_t)k + 2] - c[2];
        g += (ax * ax + ay * ay) + az * az;
    }
    g = wave_reduce_add(g);
    bad = wave_reduce_add(bad);
    if (lane == 0) {
        double* o = stats + (size_t)id * kStat;
        o[0] = c[0];
        o[1] = c[1];
        o[2] = c[2];
        o[3] = g;
        o[4] = bad ? 0.0 : 1.0;
    }
}

// grid M * row_tiles * col_tiles (column tile fastest).  row_v/row_i [S M, col_tiles], col_v/col_i [M, row_tiles, Fb]; each
// of matrix, row_v (with row_i) and col_v (with col_i) may be null.  row_i: the column inside the tile, col_i: the step; -1
// where no pair of the row (column) is valid.
__global__ __launch_bounds__(kThreads) void conf_pairs_kernel(const float* __restrict__ A, int S, int M, const float* __restrict__ B,
                                                              long long Fb, int N, const double* __restrict__ stats, int row_tiles,
                                                              long long col_tiles, double* __restrict__ matrix,
                                                              double* __restrict__ row_v, int* __restrict__ row_i,
                                                              double* __restrict__ col_v, int* __restrict__ col_i) {
    __shared__ double lds[2 * 3 * kChunk * kTile];
    __shared__ double g_of[2 * kTile];
    __shared__ int ok_of[2 * kTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long ct = blockIdx.x % col_tiles, rest = blockIdx.x / col_tiles;
    const int rt = (int)(rest % row_tiles), m = (int)(rest / row_tiles);
    const long long SM = (long long)S * M;

    // staging role: frame f of the tile on both sides, atoms a0 .. a0 + 3 of every chunk
    const int f = tid & (kTile - 1), a0 = (tid >> 5) * 4;
    const long long sf = (long long)rt * kTile + f, jf = ct * kTile + f;
    const long long ida = sf * M + m, idb = SM + jf;
    double ca[3] = {0.0, 0.0, 0.0}, cb[3] = {0.0, 0.0, 0.0};
    double ga = 0.0, gb = 0.0;
    bool use_a = false, use_b = false;
    if (sf < S) {
        const double* st = stats + (size_t)ida * kStat;
        ca[0] = st[0], ca[1] = st[1], ca[2] = st[2], ga = st[3];
        use_a = st[4] != 0.0;
    }
    if (jf < Fb) {
        const double* st = stats + (size_t)idb * kStat;
        cb[0] = st[0], cb[1] = st[1], cb[2] = st[2], gb = st[3];
        use_b = st[4] != 0.0;
    }
    if (tid < kTile) {
        g_of[f] = ga;
        g_of[kTile + f] = gb;
        ok_of[f] = use_a;
        ok_of[kTile + f] = use_b;
    }
    const float* pa = A + (size_t)(use_a ? ida : 0) * N * 3;
    const float* pb = B + (size_t)(use_b ? jf : 0) * N * 3;

    // MFMA role
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    f64x4 acc[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[r][c] = f64x4{0.0, 0.0, 0.0, 0.0};
    double* la = lds;
    double* lb = lds + 3 * kChunk * kTile;

    // the fp32 coordinates of a chunk are read one chunk ahead, so that their latency passes under the MFMAs
    float ra[4][3], rb[4][3];
    auto fetch = [&](long long k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long atom = k0 + a0 + i;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                ra[i][d] = use_a && atom < N ? pa[3 * (size_t)atom + d] : 0.f;
                rb[i][d] = use_b && atom < N ? pb[3 * (size_t)atom + d] : 0.f;
            }
        }
    };
    fetch(0);
    for (long long k0 = 0; k0 < N; k0 += kChunk) {
        __syncthreads();                                  // the last chunk's operands have been read
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = k0 + a0 + i < N;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                la[(d * kChunk + a0 + i) * kTile + f] = use_a && in ? (double)ra[i][d] - ca[d] : 0.0;
                lb[(d * kChunk + a0 + i) * kTile + f] = use_b && in ? (double)rb[i][d] - cb[d] : 0.0;
            }
        }
        fetch(k0 + kChunk);                               // (past the end: zeros, never used)
        __syncthreads();
#pragma unroll 2
        for (int kk = 0; kk < (MDNO_EXP_CONF_SKIP == 2 ? 1 : kChunk / 4); ++kk) {
            const int k = kk * 4 + l4;
            double av[3], bv[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                av[d] = la[(d * kChunk + k) * kTile + wr * 16 + l15];
                bv[d] = lb[(d * kChunk + k) * kTile + wc * 16 + l15];
            }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[r], bv[c], acc[r][c], 0, 0, 0);
        }
    }
    __syncthreads();                                      // g_of / ok_of are written; the operands are no longer needed

    // register slot i of the nine accumulators: the pair (row l4 + 4 i, column l15) of the wave's 16 x 16
    double* tile = lds;                                   // [kTile][kTile + 1]
    const double n = (double)N;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = wr * 16 + l4 + 4 * i, col = wc * 16 + l15;
        double v = nan_d();
        if (ok_of[row] && ok_of[kTile + col]) {
            double s[9];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) s[3 * r + c] = acc[r][c][i];
            if (MDNO_EXP_CONF_SKIP == 1) {
                v = g_of[row] + g_of[kTile + col];
#pragma unroll
                for (int e = 0; e < 9; ++e) v += fabs(s[e]);
            } else {
                v = sqrt(rmsd2_from_moments(s, g_of[row] + g_of[kTile + col], n));
            }
        }
        tile[row * (kTile + 1) + col] = v;
    }
    __syncthreads();

    if (matrix != nullptr) {
        const int row = tid >> 3, c0 = (tid & 7) * 4;
        const long long s = (long long)rt * kTile + row;
        if (s < S) {
            double* out = matrix + ((size_t)s * M + m) * (size_t)Fb;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long long j = ct * kTile + c0 + q;
                if (j < Fb) out[j] = tile[row * (kTile + 1) + c0 + q];
            }
        }
    }
    if (row_v != nullptr && wave == 0 && lane < kTile) {
        const long long s = (long long)rt * kTile + lane;
        if (s < S) {
            double best = 0.0;
            int at = -1;
            for (int c = 0; c < kTile; ++c) {
                const double v = tile[lane * (kTile + 1) + c];
                if (at < 0 ? v == v : v < best) best = v, at = c;
            }
            const size_t o = ((size_t)s * M + m) * (size_t)col_tiles + (size_t)ct;
            row_v[o] = best;
            row_i[o] = at;
        }
    }
    if (col_v != nullptr && wave == 1 && lane < kTile) {
        const long long j = ct * kTile + lane;
        if (j < Fb) {
            double best = 0.0;
            int at = -1;
            for (int r = 0; r < kTile; ++r) {
                const double v = tile[r * (kTile + 1) + lane];
                if (at < 0 ? v == v : v < best) best = v, at = r;
            }
            const size_t o = ((size_t)m * row_tiles + rt) * (size_t)Fb + (size_t)j;
            col_v[o] = best;
            col_i[o] = at < 0 ? -1 : rt * kTile + at;
        }
    }
}

// one thread per row (s, m): the minimum over its column tiles in ascending order
__global__ __launch_bounds__(kThreads) void conf_rows_kernel(const double* __restrict__ row_v, const int* __restrict__ row_i,
                                                             long long rows, long long col_tiles, double* __restrict__ nearest,
                                                             long long* __restrict__ nearest_index) {
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= rows) return;
    double best = 0.0;
    long long at = -1;
    for (long long t = 0; t < col_tiles; ++t) {
        const int i = row_i[(size_t)id * col_tiles + t];
        const double v = row_v[(size_t)id * col_tiles + t];
        if (i >= 0 && (at < 0 || v < best)) best = v, at = t * kTile + i;
    }
    nearest[id] = at < 0 ? nan_d() : best;
    nearest_index[id] = at;
}

// one thread per (m, j): the minimum over the row tiles in ascending order
__global__ __launch_bounds__(kThreads) void conf_cols_kernel(const double* __restrict__ col_v, const int* __restrict__ col_i,
                                                             long long count, long long Fb, int row_tiles,
                                                             double* __restrict__ cover, long long* __restrict__ cover_step) {
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= count) return;
    const long long m = id / Fb, j = id - m * Fb;
    double best = 0.0;
    long long at = -1;
    for (int t = 0; t < row_tiles; ++t) {
        const size_t o = ((size_t)m * row_tiles + t) * (size_t)Fb + (size_t)j;
        const int i = col_i[o];
        const double v = col_v[o];
        if (i >= 0 && (at < 0 || v < best)) best = v, at = i;
    }
    cover[id] = at < 0 ? nan_d() : best;
    cover_step[id] = at;
}

// v[i] = value, idx[i] = index for i < count
__global__ __launch_bounds__(kThreads) void conf_fill_kernel(double* __restrict__ v, long long* __restrict__ idx, long long count,
                                                             double value, long long index) {
    for (long long id = (long long)blockIdx.x * kThreads + threadIdx.x; id < count; id += (long long)gridDim.x * kThreads) {
        v[id] = value;
        if (idx != nullptr) idx[id] = index;
    }
}

typedef unsigned __int128 u128;

struct ConfCarve {
    double *stats = nullptr, *row_v = nullptr, *col_v = nullptr;
    int *row_i = nullptr, *col_i = nullptr;
    long long row_tiles = 0, col_tiles = 0;
    bool fits = true;
    size_t total = 0;
    ConfCarve(void* ws, int S, int M, long long Fb, bool want_cover) {
        row_tiles = ((long long)S + kTile - 1) / kTile;
        col_tiles = Fb / kTile + (Fb % kTile != 0);
        const u128 SM = (u128)S * (u128)M;
        const u128 frames = SM + (u128)Fb, rows = SM * (u128)col_tiles, cols = (u128)M * (u128)row_tiles * (u128)Fb;
        const u128 limit = (u128)1 << 56;
        if (frames > limit || rows > limit || cols > limit) {
            fits = false;
            total = SIZE_MAX;
            return;
        }
        Carver c(ws);
        stats = c.take<double>((size_t)frames * kStat);
        row_v = c.take<double>((size_t)rows);
        row_i = c.take<int>((size_t)rows);
        if (want_cover) {
            col_v = c.take<double>((size_t)cols);
            col_i = c.take<int>((size_t)cols);
        }
        total = c.used();
    }
};

double nan_host() { return std::numeric_limits<double>::quiet_NaN(); }

unsigned blocks_for(long long count) { return (unsigned)((count + kThreads - 1) / kThreads); }

int fill(double* v, long long* idx, long long count, double value, long long index, hipStream_t st, const char* who) {
    if (count == 0 || v == nullptr) return MDNO_OK;
    const long long blocks = (count + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(conf_fill_kernel, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(kThreads), 0, st, v, idx, count,
                       value, index);
    return check_launch(who);
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" size_t mdnoconf_cross_rmsd_workspace_bytes(int S, int M, int N, int64_t Fb, int want_cover) {
    if (S < 0 || M < 0 || N < 0 || Fb < 0) return 0;
    return ConfCarve(nullptr, S, M, (long long)Fb, want_cover != 0).total;
}

extern "C" int mdnoconf_cross_rmsd(const float* a, int S, int M, const float* b, int64_t Fb, int N, double* matrix, double* nearest,
                                   int64_t* nearest_index, double* cover, int64_t* cover_step, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    const char* who = "cross_rmsd";
    MDNO_REQUIRE(S >= 0 && M >= 0 && N >= 0 && Fb >= 0, MDNO_EINVAL, "%s: S=%d M=%d N=%d Fb=%lld", who, S, M, N, (long long)Fb);
    MDNO_REQUIRE((nearest != nullptr) == (nearest_index != nullptr), MDNO_EINVAL, "%s: nearest and nearest_index go together", who);
    MDNO_REQUIRE((cover != nullptr) == (cover_step != nullptr), MDNO_EINVAL, "%s: cover and cover_step go together", who);
    MDNO_REQUIRE(matrix || nearest || cover, MDNO_EINVAL, "%s: no output was asked for", who);
    const long long SM = (long long)S * M;
    const bool work = SM > 0 && Fb > 0;
    ConfCarve c(work ? workspace : nullptr, S, M, (long long)Fb, cover != nullptr);
    if (work) {
        MDNO_REQUIRE(c.fits && (u128)M * (u128)c.row_tiles * (u128)c.col_tiles < ((u128)1 << 31) - 1, MDNO_EUNSUPPORTED,
                     "%s: M=%d members of %lld x %lld tiles exceed the launch grid", who, M, c.row_tiles, c.col_tiles);
        MDNO_REQUIRE((a && b) || N == 0, MDNO_EINVAL, "%s: null pointer (a or b)", who);
        MDNO_REQUIRE(workspace && workspace_bytes >= c.total, MDNO_EINVAL, "%s: workspace %zu < %zu", who, workspace_bytes, c.total);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    long long* near_i = reinterpret_cast<long long*>(nearest_index);
    long long* cover_i = reinterpret_cast<long long*>(cover_step);
    if (!work) {        // no pairs: what has no counterpart is NaN and -1
        MDNO_TRY(fill(nearest, near_i, SM, nan_host(), -1, st, who));
        return fill(cover, cover_i, S == 0 ? (long long)M * Fb : 0, nan_host(), -1, st, who);
    }
    if (N == 0) {       // frames without atoms: every frame valid, every rmsd 0, the lowest index
        MDNO_TRY(fill(matrix, nullptr, SM * Fb, 0.0, 0, st, who));
        MDNO_TRY(fill(nearest, near_i, SM, 0.0, 0, st, who));
        return fill(cover, cover_i, (long long)M * Fb, 0.0, 0, st, who);
    }
    const long long frames = SM + Fb;
    hipLaunchKernelGGL(conf_stats_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(kThreads), 0, st, a, SM, b, (long long)Fb, N, c.stats);
    MDNO_TRY(check_launch(who));
    const unsigned blocks = (unsigned)((long long)M * c.row_tiles * c.col_tiles);
    hipLaunchKernelGGL(conf_pairs_kernel, dim3(blocks), dim3(kThreads), 0, st, a, S, M, b, (long long)Fb, N, c.stats, (int)c.row_tiles,
                       c.col_tiles, matrix, nearest ? c.row_v : nullptr, c.row_i, cover ? c.col_v : nullptr, c.col_i);
    MDNO_TRY(check_launch(who));
    if (nearest) {
        hipLaunchKernelGGL(conf_rows_kernel, dim3(blocks_for(SM)), dim3(kThreads), 0, st, c.row_v, c.row_i, SM, c.col_tiles, nearest,
                           near_i);
        MDNO_TRY(check_launch(who));
    }
    if (cover) {
        const long long count = (long long)M * Fb;
        hipLaunchKernelGGL(conf_cols_kernel, dim3(blocks_for(count)), dim3(kThreads), 0, st, c.col_v, c.col_i, count, (long long)Fb,
                           (int)c.row_tiles, cover, cover_i);
        MDNO_TRY(check_launch(who));
    }
    return MDNO_OK;
}
