// Markov state models on the device (include/mdno_markov.h states the rules and every summation order):
// nearest-centre assignment, farthest-point (k-centres) seeding, the per-state row sums of a Lloyd round and the transition
// counts at a set of lags (forecast.py: assign, kcenters, kmeans, discretize, transition_counts, markov_model).
//
//   msm_assign_kernel      THE HOT KERNEL.  A workgroup of four waves owns kRows rows x kCentres centres.  Per pass of kPass
//                          features every thread reads eight values of ONE feature per side (one pass ahead, into
//                          registers), centres them in fp64 on the way and writes them to LDS, lds[side][feature of the
//                          pass][row of the tile] (rows past R, centres past k and features past D as zeros); no fp64 copy
//                          of a row reaches global memory.  Thread tid & 127 = one row or centre adds the squares of the
//                          staged values to the running norms n_r and m_j (features ascending; between the MFMAs, and waves
//                          2 and 3 repeat what waves 0 and 1 keep).  Wave (wr, wc) owns
//                          the 32 x 32 pairs of rows 32 wr .. and centres 32 wc ..: four 16 x 16 accumulators, per group of
//                          four features two A values and two B values per lane (operand: row lane & 15, feature lane >> 4
//                          of the group) and four MFMAs.  The f64 C/D map is col = lane & 15, row = (lane >> 4) + 4 reg —
//                          NOT the f32 one.  d2 = max(0, (n + m) - 2 g) goes to LDS centre-major; thread (row, quarter)
//                          scans 16 centres in ascending order, the four quarters are merged in ascending order, and the
//                          tile's best (value, index) per row goes to the workspace.
//   msm_assign_min_kernel  one thread per row: the minimum over the centre tiles in ascending tile order.
//   msm_kc_round_kernel    a workgroup owns kArgRows rows: kKcFeat features at a time are read (one pass ahead, into
//                          registers) and widened into LDS; wave 0, thread = row, adds the squared differences to the last
//                          centre in ascending feature order and updates mind2, and the workgroup reduces (larger value,
//                          then lower row) to one candidate.
//   msm_kc_pick_kernel     one workgroup reduces the candidates and writes index[i], radius[i].
//   msm_sums_kernel        a workgroup owns kSumFeat features x kSumStates states: thread (feature f, partial t) walks the
//                          rows t, t + kSumPartials, ... and adds into ITS column of the LDS table [partial][state][feature].
//   msm_counts_kernel      the state populations: an integer table in LDS per workgroup, flushed with integer atomics.
//   msm_trans_kernel       one launch per lag, grid (origin blocks, members): integer atomics into a private n x n table in
//                          LDS (n <= kLdsStates) or straight into global memory.
// LDS of the hot kernel: 2 sides x 32 features x 81 (64 + padding: odd, so the staging writes of 32 features fall on
// distinct banks, and 17 mod 32, so the two feature rows of an operand read per half wave overlap in one bank only) x 8 B =
// 40.5 KiB, reused for the 64 x 65 d2 tile.
#include "common.h"
#include "../../include/mdno_markov.h"

namespace mdno {
namespace {

constexpr int kThreads = 256;
constexpr int kRows = MDNO_MSM_ROW_TILE, kCentres = MDNO_MSM_CENTRE_TILE, kPass = MDNO_MSM_FEATURE_PASS;
constexpr int kLd = kRows + 17;                            // LDS stride of a feature's row in doubles
constexpr int kD2Ld = kRows + 1;                           // stride of a centre's row of the d2 tile
constexpr int kStage = kRows * kPass / kThreads;           // values a thread stages per side and pass
constexpr int kArgRows = MDNO_MSM_ARGMAX_TILE, kKcFeat = 64;
constexpr int kSumPartials = MDNO_MSM_SUM_PARTIALS, kSumFeat = MDNO_MSM_SUM_FEATURES, kSumStates = MDNO_MSM_SUM_STATES;
constexpr int kLdsStates = MDNO_MSM_LDS_STATES;
static_assert(kRows == 64 && kCentres == 64 && kThreads == 256, "four waves, each 32 x 32 pairs of a 64 x 64 tile");
static_assert(kPass == 32 && kStage == 8, "a thread stages eight rows of one feature per side and pass");
static_assert(kCentres * kD2Ld <= 2 * kPass * kLd, "the d2 tile reuses the staging buffers");
static_assert(kArgRows == 64 && kKcFeat == 64, "k-centres: wave 0 sums, one thread per row; a thread stages 16 values per pass");
static_assert(kSumPartials * kSumFeat == kThreads && kSumStates * kSumFeat == kThreads, "thread maps of msm_sums_kernel");
static_assert(MDNO_MSM_MAX_STATES <= 1024, "msm_counts_kernel keeps MDNO_MSM_MAX_STATES counters in LDS");

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef unsigned __int128 u128;
typedef unsigned long long u64;

__device__ __forceinline__ bool finite_v(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool finite_v(double v) {
    return ((u64)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
__device__ __forceinline__ double nan_d() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double inf_d() { return __longlong_as_double(0x7ff0000000000000ll); }

constexpr int kRowBad = -2;                                // a tile's index entry for a row that holds a non-finite value

// ------------------------------------------------------------------------------------------------ assign
// grid (row tiles, centre tiles)
template <class T>
__global__ __launch_bounds__(kThreads) void msm_assign_kernel(const T* __restrict__ x, long long R, int D,
                                                              const T* __restrict__ cen, int k,
                                                              const double* __restrict__ origin, double* __restrict__ part_val,
                                                              int* __restrict__ part_idx) {
    __shared__ double lds[2 * kPass * kLd];
    __shared__ double nrm[kRows + kCentres];
    __shared__ int bad[kRows + kCentres];
    __shared__ double qv[4][kRows];
    __shared__ int qi[4][kRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r_base = (long long)blockIdx.x * kRows;
    const int c_base = blockIdx.y * kCentres;
    if (tid < kRows + kCentres) bad[tid] = 0;
    __syncthreads();

    // staging role: feature a of the pass on both sides, rows (centres) g, g + 8, ..., g + 56 of the tile
    const int a = tid & (kPass - 1), g = tid >> 5;
    double* la = lds;
    double* lb = lds + kPass * kLd;
    T ra[kStage], rb[kStage];
    double ro = 0.0;
    auto fetch = [&](int a0) {
        const int fa = a0 + a;
        const bool in = fa < D;
        ro = in && origin != nullptr ? origin[fa] : 0.0;
#pragma unroll
        for (int i = 0; i < kStage; ++i) {
            const long long r = r_base + g + 8 * i;
            const int c = c_base + g + 8 * i;
            ra[i] = in && r < R ? x[(size_t)r * D + fa] : (T)0;
            rb[i] = in && c < k ? cen[(size_t)c * D + fa] : (T)0;
        }
    };

    // MFMA role
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    double norm = 0.0;                                     // tid < 64: n of row tid; 64 <= tid < 128: m of centre tid - 64

    if (D > 0) fetch(0);
    for (int a0 = 0; a0 < D; a0 += kPass) {
        __syncthreads();                                   // the last pass's operands have been read
        const bool in = a0 + a < D;
#pragma unroll
        for (int i = 0; i < kStage; ++i) {
            const int slot = g + 8 * i;
            const bool use_r = in && r_base + slot < R, use_c = in && c_base + slot < k;
            if (use_r && !finite_v(ra[i])) bad[slot] = 1;
            if (use_c && !finite_v(rb[i])) bad[kRows + slot] = 1;
            la[a * kLd + slot] = use_r ? (double)ra[i] - ro : 0.0;
            lb[a * kLd + slot] = use_c ? (double)rb[i] - ro : 0.0;
        }
        if (a0 + kPass < D) fetch(a0 + kPass);
        __syncthreads();
        // the norms' serial chain runs in the same straight-line code as the MFMAs, so its adds issue between them (waves 2
        // and 3 repeat the chains of waves 0 and 1 and drop the result: no branch)
        const double* nsrc = (tid & 127) < kRows ? la + (tid & 127) : lb + ((tid & 127) - kRows);
#pragma unroll
        for (int kk = 0; kk < kPass / 4; ++kk) {
            const int f = kk * 4 + l4;
            const double a0v = la[f * kLd + wr * 32 + l15], a1v = la[f * kLd + wr * 32 + 16 + l15];
            const double b0v = lb[f * kLd + wc * 32 + l15], b1v = lb[f * kLd + wc * 32 + 16 + l15];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0v, b0v, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0v, b1v, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1v, b0v, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1v, b1v, acc[1][1], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double v = nsrc[(kk * 4 + u) * kLd];
                norm += v * v;                             // (features ascending; those past D are zeros: they add +0)
            }
        }
    }
    __syncthreads();                                       // every wave is done with the operands: the buffers are free
    if (tid < kRows + kCentres) nrm[tid] = norm;
    __syncthreads();
    // register slot q of accumulator (i, j): the pair (row 32 wr + 16 i + l4 + 4 q, centre 32 wc + 16 j + l15)
    double* d2t = lds;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = wr * 32 + 16 * i + l4 + 4 * q, col = wc * 32 + 16 * j + l15;
                const double d = (nrm[row] + nrm[kRows + col]) - 2.0 * acc[i][j][q];
                d2t[col * kD2Ld + row] = d < 0.0 ? 0.0 : d;
            }
    __syncthreads();
    {   // thread (row, quarter): 16 centres in ascending order, strictly smaller replaces
        const int row = tid & (kRows - 1), quarter = tid >> 6;
        double best = inf_d();
        int bi = -1;
        for (int jj = 0; jj < kCentres / 4; ++jj) {
            const int j = quarter * (kCentres / 4) + jj;
            if (c_base + j < k && !bad[kRows + j]) {
                const double v = d2t[j * kD2Ld + row];
                if (v < best) best = v, bi = c_base + j;
            }
        }
        qv[quarter][row] = best;
        qi[quarter][row] = bi;
    }
    __syncthreads();
    if (tid < kRows && r_base + tid < R) {
        double best = qv[0][tid];
        int bi = qi[0][tid];
#pragma unroll
        for (int u = 1; u < 4; ++u)
            if (qv[u][tid] < best) best = qv[u][tid], bi = qi[u][tid];
        const size_t at = (size_t)blockIdx.y * (size_t)R + (size_t)(r_base + tid);
        part_val[at] = best;
        part_idx[at] = bad[tid] ? kRowBad : bi;
    }
}

__global__ __launch_bounds__(kThreads) void msm_assign_min_kernel(const double* __restrict__ part_val, const int* __restrict__ part_idx,
                                                                  long long R, int tiles, int* __restrict__ label,
                                                                  double* __restrict__ dist2) {
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    double best = inf_d();
    int bi = -1;
    bool row_bad = false;
    for (int t = 0; t < tiles; ++t) {
        const size_t at = (size_t)t * (size_t)R + (size_t)r;
        const int i = part_idx[at];
        const double v = part_val[at];
        if (i == kRowBad) row_bad = true;
        else if (i >= 0 && v < best) best = v, bi = i;
    }
    if (row_bad) bi = -1;
    if (label != nullptr) label[r] = bi;
    if (dist2 != nullptr) dist2[r] = bi < 0 ? nan_d() : best;
}

__global__ __launch_bounds__(kThreads) void msm_unassigned_kernel(long long R, int* __restrict__ label, double* __restrict__ dist2) {
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    if (label != nullptr) label[r] = -1;
    if (dist2 != nullptr) dist2[r] = nan_d();
}

// ------------------------------------------------------------------------------------------------ k-centres
struct Cand {
    double v;
    long long i;
};
// larger value first, then the lower row; a candidate without a row (i < 0) loses to every other
__device__ __forceinline__ bool better(const Cand& p, const Cand& q) {
    return p.i >= 0 && (q.i < 0 || p.v > q.v || (p.v == q.v && p.i < q.i));
}

__device__ __forceinline__ Cand block_best(Cand mine, double* rv, long long* ri) {
    const int tid = threadIdx.x;
    rv[tid] = mine.v;
    ri[tid] = mine.i;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const Cand p{rv[tid], ri[tid]}, q{rv[tid + s], ri[tid + s]};
            if (better(q, p)) rv[tid] = q.v, ri[tid] = q.i;
        }
        __syncthreads();
    }
    return Cand{rv[0], ri[0]};
}

__global__ void msm_kc_init_kernel(long long first, long long* __restrict__ index, double* __restrict__ radius) {
    index[0] = first;
    radius[0] = inf_d();
}

// grid ceil(R / kArgRows): thread = row
template <class T>
__global__ __launch_bounds__(kThreads) void msm_kc_round_kernel(const T* __restrict__ x, long long R, int D,
                                                                const long long* __restrict__ index, int round,
                                                                double* __restrict__ mind2, double* __restrict__ blk_val,
                                                                long long* __restrict__ blk_idx) {
    __shared__ double xs[kArgRows][kKcFeat + 1];
    __shared__ double cs[kKcFeat];
    __shared__ double rv[kThreads];
    __shared__ long long ri[kThreads];
    constexpr int kLoads = kArgRows * kKcFeat / kThreads;  // values a thread stages per pass: row tid / 64 + 4 i, feature tid % 64
    const int tid = threadIdx.x, ff = tid % kKcFeat, rr0 = tid / kKcFeat;
    const long long r_base = (long long)blockIdx.x * kArgRows, r = r_base + tid;
    const long long c = index[round - 1];
    const bool centre_ok = c >= 0 && c < R;
    // the values of a pass are read one pass ahead, so that their latency passes under the sums
    T pv[kLoads], pc = (T)0;
    auto fetch = [&](int a0) {
        const bool in = a0 + ff < D;
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const long long row = r_base + rr0 + (kThreads / kKcFeat) * i;
            pv[i] = in && row < R ? x[(size_t)row * D + a0 + ff] : (T)0;
        }
        if (tid < kKcFeat) pc = in && centre_ok ? x[(size_t)c * D + a0 + ff] : (T)0;
    };
    double e = 0.0;
    bool row_bad = false;
    if (D > 0) fetch(0);
    for (int a0 = 0; a0 < D; a0 += kKcFeat) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kLoads; ++i) xs[rr0 + (kThreads / kKcFeat) * i][ff] = (double)pv[i];
        if (tid < kKcFeat) cs[tid] = (double)pc;
        if (a0 + kKcFeat < D) fetch(a0 + kKcFeat);
        __syncthreads();
        if (tid < kArgRows) {                              // (wave 0, whole): thread = row, features ascending
            const int n = D - a0 < kKcFeat ? D - a0 : kKcFeat;
            for (int f = 0; f < n; ++f) {
                const double v = xs[tid][f];
                row_bad |= !finite_v(v);
                const double diff = v - cs[f];
                e += diff * diff;
            }
        }
    }
    Cand mine{-1.0, -1};
    if (tid < kArgRows && r < R) {
        const double prev = round == 1 ? inf_d() : mind2[r];
        const double m = row_bad ? -1.0 : (centre_ok && e < prev ? e : prev);
        mind2[r] = m;
        if (!row_bad) mine = Cand{m, r};
    }
    const Cand best = block_best(mine, rv, ri);
    if (tid == 0) {
        blk_val[blockIdx.x] = best.v;
        blk_idx[blockIdx.x] = best.i;
    }
}

__global__ __launch_bounds__(kThreads) void msm_kc_pick_kernel(const double* __restrict__ blk_val, const long long* __restrict__ blk_idx,
                                                               long long blocks, int round, long long* __restrict__ index,
                                                               double* __restrict__ radius) {
    __shared__ double rv[kThreads];
    __shared__ long long ri[kThreads];
    Cand mine{-1.0, -1};
    for (long long b = threadIdx.x; b < blocks; b += kThreads) {
        const Cand q{blk_val[b], blk_idx[b]};
        if (better(q, mine)) mine = q;
    }
    const Cand best = block_best(mine, rv, ri);
    if (threadIdx.x == 0) {
        index[round] = best.i;
        radius[round] = best.i < 0 ? nan_d() : sqrt(best.v);
    }
}

// ------------------------------------------------------------------------------------------------ centroid sums
// grid (ceil(D / kSumFeat), ceil(k / kSumStates)): thread (f = tid & 15, t = tid >> 4)
template <class T>
__global__ __launch_bounds__(kThreads) void msm_sums_kernel(const T* __restrict__ x, long long R, int D,
                                                            const int* __restrict__ label, int k, double* __restrict__ sums) {
    __shared__ double table[kSumPartials][kSumStates][kSumFeat];
    const int f = threadIdx.x & (kSumFeat - 1), t = threadIdx.x >> 4;
    const long long col = (long long)blockIdx.x * kSumFeat + f;
    const int k0 = blockIdx.y * kSumStates;
    const int k1 = k0 + kSumStates < k ? k0 + kSumStates : k;
    for (int s = 0; s < kSumStates; ++s) table[t][s][f] = 0.0;
    if (col < D) {
        long long r = t;
        for (; r + 3 * kSumPartials < R; r += 4 * kSumPartials) {       // four loads in flight, added in row order
            int lab[4];
            T v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) lab[u] = label[r + u * kSumPartials];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                v[u] = lab[u] >= k0 && lab[u] < k1 ? x[(size_t)(r + u * kSumPartials) * D + col] : (T)0;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (lab[u] >= k0 && lab[u] < k1) table[t][lab[u] - k0][f] += (double)v[u];
        }
        for (; r < R; r += kSumPartials) {
            const int lab = label[r];
            if (lab >= k0 && lab < k1) table[t][lab - k0][f] += (double)x[(size_t)r * D + col];
        }
    }
    __syncthreads();
    const int s = t;                                       // now thread (state s, feature f)
    if (col < D && k0 + s < k) {
        double total = table[0][s][f];
        for (int u = 1; u < kSumPartials; ++u) total += table[u][s][f];
        sums[(size_t)(k0 + s) * D + col] = total;
    }
}

__global__ __launch_bounds__(kThreads) void msm_counts_kernel(const int* __restrict__ label, long long R, int k, u64* __restrict__ counts) {
    __shared__ u64 tab[MDNO_MSM_MAX_STATES];
    for (int s = threadIdx.x; s < k; s += kThreads) tab[s] = 0;
    __syncthreads();
    for (long long r = (long long)blockIdx.x * kThreads + threadIdx.x; r < R; r += (long long)gridDim.x * kThreads) {
        const int lab = label[r];
        if (lab >= 0 && lab < k) atomicAdd(&tab[lab], 1ull);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < k; s += kThreads)
        if (tab[s]) atomicAdd(&counts[s], tab[s]);
}

// ------------------------------------------------------------------------------------------------ transition counts
// grid (origin blocks, M): `out` is the lag's [Mo, n, n] block, `skipped` the lag's counter
__global__ __launch_bounds__(kThreads) void msm_trans_kernel(const int* __restrict__ label, int S, int M, int n, int lag, int pooled,
                                                             u64* __restrict__ out, u64* __restrict__ skipped) {
    __shared__ unsigned tab[kLdsStates * kLdsStates];
    __shared__ unsigned skip_s;
    const bool use_lds = n <= kLdsStates;
    const int m = blockIdx.y, tid = threadIdx.x;
    const long long T = (long long)S - lag;
    u64* dst = out + (pooled ? (size_t)0 : (size_t)m * n * n);
    if (use_lds)
        for (int e = tid; e < n * n; e += kThreads) tab[e] = 0;
    if (tid == 0) skip_s = 0;
    __syncthreads();
    unsigned skip = 0;
    for (long long t = (long long)blockIdx.x * kThreads + tid; t < T; t += (long long)gridDim.x * kThreads) {
        const int from = label[(size_t)t * M + m], to = label[(size_t)(t + lag) * M + m];
        if (from >= 0 && from < n && to >= 0 && to < n) {
            if (use_lds) atomicAdd(&tab[from * n + to], 1u);
            else atomicAdd(&dst[(size_t)from * n + to], 1ull);
        } else {
            ++skip;
        }
    }
    if (skip) atomicAdd(&skip_s, skip);
    __syncthreads();
    if (use_lds)
        for (int e = tid; e < n * n; e += kThreads)
            if (tab[e]) atomicAdd(&dst[e], (u64)tab[e]);
    if (tid == 0 && skip_s) atomicAdd(skipped, (u64)skip_s);
}

size_t assign_workspace(long long R, int k) {
    if (R <= 0 || k <= 0) return 0;
    const u128 tiles = ((u128)k + kCentres - 1) / kCentres;
    const u128 entries = tiles * (u128)R;
    const u128 bytes = (entries * 8 + 255) / 256 * 256 + (entries * 4 + 255) / 256 * 256;
    return bytes > (u128)SIZE_MAX ? SIZE_MAX : (size_t)bytes;
}

size_t kcenters_workspace(long long R) {
    if (R <= 0) return 0;
    const u128 blocks = ((u128)R + kArgRows - 1) / kArgRows;
    const u128 bytes = ((u128)R * 8 + 255) / 256 * 256 + 2 * ((blocks * 8 + 255) / 256 * 256);
    return bytes > (u128)SIZE_MAX ? SIZE_MAX : (size_t)bytes;
}

bool dtype_ok(int dtype) { return dtype == MDNO_MSM_F32 || dtype == MDNO_MSM_F64; }

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" size_t mdnomsm_assign_workspace_bytes(int64_t R, int k, int D) {
    if (R < 0 || k < 0 || D < 0 || k > MDNO_MSM_MAX_STATES) return 0;
    return assign_workspace((long long)R, k);
}

extern "C" int mdnomsm_assign(const void* x, int64_t R, int D, int dtype, const void* centres, int k, const double* origin,
                              int32_t* label, double* dist2, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "msm_assign";
    MDNO_REQUIRE(R >= 0 && D >= 0 && k >= 0, MDNO_EINVAL, "%s: R=%lld D=%d k=%d", who, (long long)R, D, k);
    MDNO_REQUIRE(dtype_ok(dtype), MDNO_EINVAL, "%s: dtype=%d is neither f32 (0) nor f64 (1)", who, dtype);
    MDNO_REQUIRE(k <= MDNO_MSM_MAX_STATES, MDNO_EINVAL, "%s: k=%d outside 0 .. %d", who, k, MDNO_MSM_MAX_STATES);
    MDNO_REQUIRE(label || dist2, MDNO_EINVAL, "%s: no output was asked for", who);
    if (R == 0) return MDNO_OK;
    MDNO_REQUIRE(x || D == 0, MDNO_EINVAL, "%s: null pointer (x)", who);
    MDNO_REQUIRE(centres || D == 0 || k == 0, MDNO_EINVAL, "%s: null pointer (centres)", who);
    const long long row_tiles = ((long long)R + kRows - 1) / kRows;
    MDNO_REQUIRE(row_tiles < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "%s: R=%lld rows exceed the launch grid", who, (long long)R);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned row_blocks = (unsigned)(((long long)R + kThreads - 1) / kThreads);
    if (k == 0) {
        hipLaunchKernelGGL(msm_unassigned_kernel, dim3(row_blocks), dim3(kThreads), 0, st, (long long)R, label, dist2);
        return check_launch(who);
    }
    const size_t need = assign_workspace((long long)R, k);
    MDNO_REQUIRE(need != SIZE_MAX, MDNO_EUNSUPPORTED, "%s: the workspace does not fit a size_t", who);
    MDNO_REQUIRE(workspace && workspace_bytes >= need, MDNO_EINVAL, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    const int tiles = (k + kCentres - 1) / kCentres;
    Carver carve(workspace);
    double* part_val = carve.take<double>((size_t)tiles * (size_t)R);
    int* part_idx = carve.take<int>((size_t)tiles * (size_t)R);
    const dim3 grid((unsigned)row_tiles, (unsigned)tiles);
    if (dtype == MDNO_MSM_F32)
        hipLaunchKernelGGL(msm_assign_kernel<float>, grid, dim3(kThreads), 0, st, static_cast<const float*>(x), (long long)R, D,
                           static_cast<const float*>(centres), k, origin, part_val, part_idx);
    else
        hipLaunchKernelGGL(msm_assign_kernel<double>, grid, dim3(kThreads), 0, st, static_cast<const double*>(x), (long long)R, D,
                           static_cast<const double*>(centres), k, origin, part_val, part_idx);
    MDNO_TRY(check_launch(who));
    hipLaunchKernelGGL(msm_assign_min_kernel, dim3(row_blocks), dim3(kThreads), 0, st, part_val, part_idx, (long long)R, tiles, label,
                       dist2);
    return check_launch(who);
}

extern "C" size_t mdnomsm_kcenters_workspace_bytes(int64_t R, int D) {
    if (R < 0 || D < 0) return 0;
    return kcenters_workspace((long long)R);
}

extern "C" int mdnomsm_kcenters(const void* x, int64_t R, int D, int dtype, int k, int64_t first, int64_t* index, double* radius,
                                void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "msm_kcenters";
    MDNO_REQUIRE(R >= 0 && D >= 0, MDNO_EINVAL, "%s: R=%lld D=%d", who, (long long)R, D);
    MDNO_REQUIRE(dtype_ok(dtype), MDNO_EINVAL, "%s: dtype=%d is neither f32 (0) nor f64 (1)", who, dtype);
    MDNO_REQUIRE(k >= 1 && k <= MDNO_MSM_MAX_STATES, MDNO_EINVAL, "%s: k=%d outside 1 .. %d", who, k, MDNO_MSM_MAX_STATES);
    MDNO_REQUIRE(k <= R, MDNO_EINVAL, "%s: k=%d centres of R=%lld rows", who, k, (long long)R);
    MDNO_REQUIRE(first >= 0 && first < R, MDNO_EINVAL, "%s: first=%lld outside 0 .. %lld", who, (long long)first, (long long)R - 1);
    MDNO_REQUIRE(index && radius, MDNO_EINVAL, "%s: null pointer (index or radius)", who);
    MDNO_REQUIRE(x || D == 0, MDNO_EINVAL, "%s: null pointer (x)", who);
    const long long blocks = ((long long)R + kArgRows - 1) / kArgRows;
    MDNO_REQUIRE(blocks < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "%s: R=%lld rows exceed the launch grid", who, (long long)R);
    const size_t need = kcenters_workspace((long long)R);
    MDNO_REQUIRE(need != SIZE_MAX, MDNO_EUNSUPPORTED, "%s: the workspace does not fit a size_t", who);
    MDNO_REQUIRE(workspace && workspace_bytes >= need, MDNO_EINVAL, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    Carver carve(workspace);
    double* mind2 = carve.take<double>((size_t)R);
    double* blk_val = carve.take<double>((size_t)blocks);
    long long* blk_idx = carve.take<long long>((size_t)blocks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    long long* idx = reinterpret_cast<long long*>(index);
    hipLaunchKernelGGL(msm_kc_init_kernel, dim3(1), dim3(1), 0, st, (long long)first, idx, radius);
    MDNO_TRY(check_launch(who));
    for (int round = 1; round < k; ++round) {
        if (dtype == MDNO_MSM_F32)
            hipLaunchKernelGGL(msm_kc_round_kernel<float>, dim3((unsigned)blocks), dim3(kThreads), 0, st, static_cast<const float*>(x),
                               (long long)R, D, idx, round, mind2, blk_val, blk_idx);
        else
            hipLaunchKernelGGL(msm_kc_round_kernel<double>, dim3((unsigned)blocks), dim3(kThreads), 0, st, static_cast<const double*>(x),
                               (long long)R, D, idx, round, mind2, blk_val, blk_idx);
        MDNO_TRY(check_launch(who));
        hipLaunchKernelGGL(msm_kc_pick_kernel, dim3(1), dim3(kThreads), 0, st, blk_val, blk_idx, blocks, round, idx, radius);
        MDNO_TRY(check_launch(who));
    }
    return MDNO_OK;
}

extern "C" int mdnomsm_centroid_sums(const void* x, int64_t R, int D, int dtype, const int32_t* label, int k, double* sums,
                                     int64_t* counts, void* stream) {
    const char* who = "msm_centroid_sums";
    MDNO_REQUIRE(R >= 0 && D >= 0, MDNO_EINVAL, "%s: R=%lld D=%d", who, (long long)R, D);
    MDNO_REQUIRE(dtype_ok(dtype), MDNO_EINVAL, "%s: dtype=%d is neither f32 (0) nor f64 (1)", who, dtype);
    MDNO_REQUIRE(k >= 1 && k <= MDNO_MSM_MAX_STATES, MDNO_EINVAL, "%s: k=%d outside 1 .. %d", who, k, MDNO_MSM_MAX_STATES);
    MDNO_REQUIRE(counts != nullptr, MDNO_EINVAL, "%s: null pointer (counts)", who);
    MDNO_REQUIRE(sums || D == 0, MDNO_EINVAL, "%s: null pointer (sums)", who);
    MDNO_REQUIRE(label || R == 0, MDNO_EINVAL, "%s: null pointer (label)", who);
    MDNO_REQUIRE(x || R == 0 || D == 0, MDNO_EINVAL, "%s: null pointer (x)", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    MDNO_HIP(hipMemsetAsync(counts, 0, (size_t)k * sizeof(int64_t), st));
    if (R > 0) {
        const long long want = ((long long)R + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(msm_counts_kernel, dim3((unsigned)(want < 256 ? want : 256)), dim3(kThreads), 0, st, label, (long long)R, k,
                           reinterpret_cast<u64*>(counts));
        MDNO_TRY(check_launch(who));
    }
    if (D == 0) return MDNO_OK;
    const dim3 grid((unsigned)((D + kSumFeat - 1) / kSumFeat), (unsigned)((k + kSumStates - 1) / kSumStates));
    if (dtype == MDNO_MSM_F32)
        hipLaunchKernelGGL(msm_sums_kernel<float>, grid, dim3(kThreads), 0, st, static_cast<const float*>(x), (long long)R, D, label, k,
                           sums);
    else
        hipLaunchKernelGGL(msm_sums_kernel<double>, grid, dim3(kThreads), 0, st, static_cast<const double*>(x), (long long)R, D, label, k,
                           sums);
    return check_launch(who);
}

extern "C" int mdnomsm_transition_counts(const int32_t* label, int S, int M, int n_states, const int32_t* lags, int n_lags,
                                         int pooled, int64_t* counts, int64_t* n_skipped, void* stream) {
    const char* who = "msm_transition_counts";
    MDNO_REQUIRE(S >= 0 && M >= 0, MDNO_EINVAL, "%s: S=%d M=%d", who, S, M);
    MDNO_REQUIRE(n_lags >= 1 && n_lags <= MDNO_MSM_MAX_LAGS, MDNO_EINVAL, "%s: n_lags=%d outside 1 .. %d", who, n_lags, MDNO_MSM_MAX_LAGS);
    MDNO_REQUIRE(n_states >= 1 && n_states <= MDNO_MSM_MAX_STATES, MDNO_EINVAL, "%s: n_states=%d outside 1 .. %d", who, n_states,
                 MDNO_MSM_MAX_STATES);
    MDNO_REQUIRE(lags != nullptr, MDNO_EINVAL, "%s: null pointer (lags)", who);
    for (int l = 0; l < n_lags; ++l) MDNO_REQUIRE(lags[l] >= 1, MDNO_EINVAL, "%s: lag %d (entry %d) is below 1", who, lags[l], l);
    const size_t members = pooled ? 1 : (size_t)M;
    MDNO_REQUIRE(n_skipped != nullptr, MDNO_EINVAL, "%s: null pointer (n_skipped)", who);
    MDNO_REQUIRE(counts || members == 0, MDNO_EINVAL, "%s: null pointer (counts)", who);
    MDNO_REQUIRE(label || S == 0 || M == 0, MDNO_EINVAL, "%s: null pointer (label)", who);
    MDNO_REQUIRE(M <= 65535, MDNO_EUNSUPPORTED, "%s: M=%d members exceed the launch grid", who, M);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t block = members * (size_t)n_states * (size_t)n_states;
    if (block) MDNO_HIP(hipMemsetAsync(counts, 0, (size_t)n_lags * block * sizeof(int64_t), st));
    MDNO_HIP(hipMemsetAsync(n_skipped, 0, (size_t)n_lags * sizeof(int64_t), st));
    if (M == 0) return MDNO_OK;
    for (int l = 0; l < n_lags; ++l) {
        if (lags[l] >= S) continue;
        const long long want = ((long long)S - lags[l] + kThreads - 1) / kThreads;
        const dim3 grid((unsigned)(want < 1024 ? want : 1024), (unsigned)M);
        hipLaunchKernelGGL(msm_trans_kernel, grid, dim3(kThreads), 0, st, label, S, M, n_states, lags[l], pooled,
                           reinterpret_cast<u64*>(counts) + (size_t)l * block, reinterpret_cast<u64*>(n_skipped) + l);
        MDNO_TRY(check_launch(who));
    }
    return MDNO_OK;
}
