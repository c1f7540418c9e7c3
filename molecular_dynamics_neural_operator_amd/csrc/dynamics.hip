// Time-correlation statistics of a trajectory that lies in device memory (include/mdno_dynamics.h states THE RULE and
// the order of the sums): the displacement sums behind MSD(tau), the non-Gaussian parameter and the self
// van Hove histogram (forecast.py: DisplacementStats), the velocity autocorrelation, and the unwrapping of frames that
// arrive wrapped.
//
// One kernel template, two accumulate functors (Displacement, Velocity).  grid (chunk * tiles + tile, lag of the batch,
// member): a workgroup owns MDNO_DYN_ORIGIN_CHUNK origins x MDNO_DYN_ATOM_TILE atoms of one (m, l), walks its samples
// with the flat index e = origin * atoms + atom (full waves whatever N is), reduces the threads' fp64 sums with
// block_reduce_add and stores one partial; dynamics_finish_kernel adds the partials of (m, l) in ascending order.  No
// float atomics: the same bits on every run.  The displacement histogram is a u32 histogram in LDS per workgroup whose
// non-zero bins are added to the zeroed row with integer atomics, as observe.hip's tiled form does.
//
// The lags are a HOST array the caller may free when the call returns, so they travel BY VALUE in the kernel
// arguments, kLagBatch at a time (the default set of 33 lags is one launch): no copy whose completion the caller
// would have to wait for.
#include "pbc.h"
#include "reduce.h"
#include "../../include/mdno_dynamics.h"

#include <cmath>

namespace mdno {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kChunk = MDNO_DYN_ORIGIN_CHUNK;
constexpr int kAtomTile = MDNO_DYN_ATOM_TILE;
constexpr int kLagBatch = 256;
constexpr int kMaxLags = 1024;
constexpr int kMaxBins = 4096;             // as observe.hip's

struct LagBatch {
    int tau[kLagBatch];
};

// the trajectory and, where the centroid's motion is removed, the centroids f64 [S, M, 3] (nullptr: not removed)
struct Frames {
    const float* x;
    const double* com;
    int S, M, N;
    // d = x_i(t1) - x_i(t0) of member m, in fp64, minus the centroid's displacement
    __device__ __forceinline__ void diff(long long t1, long long t0, int m, int i, double d[3]) const {
        const float* p1 = x + (((size_t)t1 * M + m) * N + i) * 3;
        const float* p0 = x + (((size_t)t0 * M + m) * N + i) * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = (double)p1[a] - (double)p0[a];
        if (com != nullptr) {
            const double* c1 = com + ((size_t)t1 * M + m) * 3;
            const double* c0 = com + ((size_t)t0 * M + m) * 3;
#pragma unroll
            for (int a = 0; a < 3; ++a) d[a] = d[a] - (c1[a] - c0[a]);
        }
    }
};

// sum2 += |d|^2, sum4 += |d|^4, and the histogram of |d|
struct Displacement {
    static constexpr int K = 2;            // sums per partial
    static constexpr int span = 0;         // frames needed beyond t + tau
    double r_max, inv_dr;
    int n_bins;                            // 0: no histogram
    __device__ __forceinline__ void operator()(const Frames& f, long long t, int tau, int m, int i, double (&v)[K],
                                               unsigned int* hist) const {
        double d[3];
        f.diff(t + tau, t, m, i, d);
        const double s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
        v[0] += s;
        v[1] += s * s;
        if (n_bins > 0) {
            const double r = sqrt(s);
            if (r < r_max) {               // false for a NaN or an Inf
                int b = (int)(r * inv_dr); // 0 <= r * inv_dr < n_bins + 1: the value (long long) gives
                b = b < n_bins ? b : n_bins - 1;
                atomicAdd(hist + b, 1u);
            }
        }
    }
};

// corr += v(t) . v(t + tau) of the finite-difference velocities
struct Velocity {
    static constexpr int K = 1;
    static constexpr int span = 1;
    static constexpr int n_bins = 0;
    __device__ __forceinline__ void operator()(const Frames& f, long long t, int tau, int m, int i, double (&v)[K],
                                               unsigned int*) const {
        double a[3], b[3];
        f.diff(t + 1, t, m, i, a);
        f.diff(t + tau + 1, t + tau, m, i, b);
        v[0] += (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    }
};

__host__ __device__ inline int origins_of(int S, int tau, int span, int stride) {
    const int last = S - 1 - span - tau;   // the largest t with t + tau + span <= S - 1
    return last < 0 ? 0 : last / stride + 1;
}
__host__ __device__ inline int chunks_of(int n_origins) { return (n_origins + kChunk - 1) / kChunk; }

// ---------------------------------------------------------------------------------------------- centroids
// one workgroup per frame (t, m): com[(t, m), a] = (fp64 sum over the atoms in a fixed order) / N
__global__ __launch_bounds__(kThreads) void centroid_kernel(const float* __restrict__ frames, int N, double* __restrict__ com) {
    __shared__ double slots[kWaves * 3];
    const size_t f = blockIdx.x;
    const float* P = frames + f * N * 3;
    double c[3] = {0, 0, 0};
    for (int i = threadIdx.x; i < N; i += kThreads) {
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] += (double)P[3 * (size_t)i + a];
    }
    block_reduce_add<kWaves>(c, slots);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) com[f * 3 + a] = c[a] / (double)N;
    }
}

// ---------------------------------------------------------------------------------------------- partial sums
// grid (P, lags of this batch, M), P = (chunks of the smallest lag possible) * tiles: a workgroup beyond its lag's chunks
// leaves at once.  part f64 [M, n_lags, P, K]; counts u64 [M, n_lags, n_bins], zero when this starts.  dynamic LDS: the
// histogram u32 [n_bins].
template <class Acc>
__global__ __launch_bounds__(kThreads) void dynamics_partial_kernel(const Frames f, const Acc acc, const LagBatch lags,
                                                                    int lag0, int n_lags, int stride, int tiles, int P,
                                                                    double* __restrict__ part,
                                                                    unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned int hist[];
    __shared__ double slots[kWaves * Acc::K];
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x / tiles, tile = blockIdx.x - chunk * tiles;
    const int l = lag0 + blockIdx.y, m = blockIdx.z;
    const int tau = lags.tau[blockIdx.y];
    const int n_origins = origins_of(f.S, tau, Acc::span, stride);
    if (chunk >= chunks_of(n_origins)) return;
    const int o0 = chunk * kChunk, no = min(n_origins - o0, kChunk);
    const int a0 = tile * kAtomTile, na = min(f.N - a0, kAtomTile);
    for (int k = tid; k < acc.n_bins; k += kThreads) hist[k] = 0u;
    if (acc.n_bins > 0) __syncthreads();
    double v[Acc::K];
#pragma unroll
    for (int k = 0; k < Acc::K; ++k) v[k] = 0.0;
    for (int e = tid; e < no * na; e += kThreads) {
        const int o = e / na, i = e - o * na;
        acc(f, (long long)(o0 + o) * stride, tau, m, a0 + i, v, hist);
    }
    block_reduce_add<kWaves>(v, slots);     // (starts and ends with a barrier: the histogram is complete after it)
    const size_t row = (size_t)m * n_lags + l;
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < Acc::K; ++k) part[(row * P + blockIdx.x) * Acc::K + k] = v[k];
    }
    if (acc.n_bins > 0) {
        unsigned long long* c = counts + row * acc.n_bins;
        for (int b = tid; b < acc.n_bins; b += kThreads) {
            if (hist[b]) atomicAdd(c + b, (unsigned long long)hist[b]);
        }
    }
}

// one thread per (m, lag of this batch, k): out_k[m, l] = the partials of (m, l) added in ascending order
template <int K, int SPAN>
__global__ __launch_bounds__(kThreads) void dynamics_finish_kernel(const double* __restrict__ part, const LagBatch lags,
                                                                   int lag0, int batch, int n_lags, int S, int M, int stride,
                                                                   int tiles, int P, double* __restrict__ out0,
                                                                   double* __restrict__ out1) {
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= (long long)M * batch * K) return;
    const int k = (int)(id % K);
    const int j = (int)((id / K) % batch);
    const int m = (int)(id / ((long long)K * batch));
    const int np = chunks_of(origins_of(S, lags.tau[j], SPAN, stride)) * tiles;
    const size_t row = (size_t)m * n_lags + lag0 + j;
    const double* p = part + row * P * K + k;
    double s = 0.0;
    for (int q = 0; q < np; ++q) s += p[(size_t)q * K];
    (k == 0 ? out0 : out1)[row] = s;
}

// ---------------------------------------------------------------------------------------------- unwrap
// one thread per (m, atom, axis): a scan over the frames (consecutive threads read consecutive floats of every frame)
__global__ __launch_bounds__(kThreads) void unwrap_kernel(const float* __restrict__ frames, int S, long long per_frame,
                                                          const PbcBox box, float* __restrict__ out) {
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (j >= per_frame) return;
    const int a = (int)(j % 3);
    const double L = box.L[a], invL = box.inv[a];
    float u = frames[j];
    out[j] = u;
    double n = 0.0;
    for (int t = 1; t < S; ++t) {
        const double x = (double)frames[(size_t)t * per_frame + j];
        if (L > 0.0) {
            const double d = (x - n * L) - (double)u;
            n = n + rint(d * invL);
            u = (float)(x - n * L);
        } else {
            u = (float)x;
        }
        out[(size_t)t * per_frame + j] = u;
    }
}

int tiles_of(int N) { return N > 0 ? (N + kAtomTile - 1) / kAtomTile : 1; }

// partials per (m, l): sized for origin_stride == 1 and lag 0, the most chunks a lag can have
int partials_of(int S, int N) { return (chunks_of(S) > 0 ? chunks_of(S) : 1) * tiles_of(N); }

size_t workspace_bytes(int S, int M, int N, int n_lags, int K) {
    if (S <= 0 || M <= 0 || N < 0 || n_lags <= 0) return 0;
    Carver c(nullptr);
    c.take<double>((size_t)S * M * 3);
    c.take<double>((size_t)M * n_lags * partials_of(S, N) * K);
    return c.used();
}

// what both statistics check alike, before any device work; *done: nothing to compute
int check_common(const char* who, const void* frames, int S, int M, int N, const int32_t* lags, int n_lags, int stride,
                 int span, bool* done) {
    *done = false;
    MDNO_REQUIRE(S >= 0 && M >= 0 && N >= 0, MDNO_EINVAL, "%s: S=%d M=%d N=%d", who, S, M, N);
    MDNO_REQUIRE(n_lags >= 1 && n_lags <= kMaxLags, MDNO_EINVAL, "%s: n_lags=%d is outside 1 .. %d", who, n_lags, kMaxLags);
    MDNO_REQUIRE(stride >= 1, MDNO_EINVAL, "%s: origin_stride=%d is not >= 1", who, stride);
    if (S == 0 || M == 0) {
        *done = true;
        return MDNO_OK;
    }
    MDNO_REQUIRE(lags != nullptr, MDNO_EINVAL, "%s: null pointer (lags)", who);
    for (int l = 0; l < n_lags; ++l) {
        MDNO_REQUIRE(lags[l] >= 0 && lags[l] <= S - 1 - span, MDNO_EINVAL, "%s: lag[%d] = %d is outside 0 .. %d (S=%d)", who, l,
                     lags[l], S - 1 - span, S);
    }
    MDNO_REQUIRE(frames != nullptr || N == 0, MDNO_EINVAL, "%s: null pointer (frames)", who);
    MDNO_REQUIRE(M <= 65535 && (long long)S * M < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "%s: S=%d M=%d exceed the launch grid", who,
                 S, M);
    return MDNO_OK;
}

// centroids (where asked for), partial sums and their ordered sum; counts was zeroed by the caller
template <class Acc>
int run_statistic(const char* who, const float* frames, int S, int M, int N, const int32_t* lags, int n_lags, int stride,
                  int remove_com, const Acc& acc, double* out0, double* out1, int64_t* counts, void* workspace,
                  hipStream_t st) {
    Carver c(workspace);
    double* com = c.take<double>((size_t)S * M * 3);
    const int tiles = tiles_of(N), P = partials_of(S, N);
    double* part = c.take<double>((size_t)M * n_lags * P * Acc::K);
    if (remove_com && N > 0) {
        hipLaunchKernelGGL(centroid_kernel, dim3((unsigned)((size_t)S * M)), dim3(kThreads), 0, st, frames, N, com);
        MDNO_TRY(check_launch(who));
    }
    const Frames f{frames, remove_com && N > 0 ? com : nullptr, S, M, N};
    for (int lag0 = 0; lag0 < n_lags; lag0 += kLagBatch) {
        const int batch = n_lags - lag0 < kLagBatch ? n_lags - lag0 : kLagBatch;
        LagBatch lb{};
        int most = 0;                      // the most origins of a lag of this batch
        for (int j = 0; j < batch; ++j) {
            lb.tau[j] = lags[lag0 + j];
            const int n = origins_of(S, lb.tau[j], Acc::span, stride);
            most = n > most ? n : most;
        }
        if (most > 0 && N > 0) {
            hipLaunchKernelGGL(dynamics_partial_kernel<Acc>, dim3((unsigned)(chunks_of(most) * tiles), batch, M), dim3(kThreads),
                               (size_t)acc.n_bins * 4, st, f, acc, lb, lag0, n_lags, stride, tiles, P, part,
                               reinterpret_cast<unsigned long long*>(counts));
            MDNO_TRY(check_launch(who));
        }
        const long long threads = (long long)M * batch * Acc::K;
        hipLaunchKernelGGL((dynamics_finish_kernel<Acc::K, Acc::span>), dim3((unsigned)((threads + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, st, part, lb, lag0, batch, n_lags, S, M, stride, N > 0 ? tiles : 0, P, out0, out1);
        MDNO_TRY(check_launch(who));
    }
    return MDNO_OK;
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" size_t mdno_displacement_stats_workspace_bytes(int S, int M, int N, int n_lags, int n_bins) {
    (void)n_bins;      // the histogram lives in LDS and in the caller's counts
    return workspace_bytes(S, M, N, n_lags, Displacement::K);
}

extern "C" size_t mdno_velocity_autocorrelation_workspace_bytes(int S, int M, int N, int n_lags) {
    return workspace_bytes(S, M, N, n_lags, Velocity::K);
}

extern "C" int mdno_displacement_stats(const float* frames, int S, int M, int N, const int32_t* lags, int n_lags,
                                       int origin_stride, int remove_com, double r_max, int n_bins, double* sum2, double* sum4,
                                       int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "displacement_stats";
    MDNO_REQUIRE(n_bins >= 0 && n_bins <= kMaxBins, MDNO_EINVAL, "%s: n_bins=%d is outside 0 .. %d", who, n_bins, kMaxBins);
    MDNO_REQUIRE(n_bins == 0 || (std::isfinite(r_max) && r_max > 0.0), MDNO_EINVAL,
                 "%s: r_max %g is not a finite positive number", who, r_max);
    bool done = false;
    MDNO_TRY(check_common(who, frames, S, M, N, lags, n_lags, origin_stride, Displacement::span, &done));
    if (done) return MDNO_OK;
    MDNO_REQUIRE(sum2 && sum4 && (counts || n_bins == 0), MDNO_EINVAL, "%s: null pointer (sum2, sum4 or counts)", who);
    const size_t need = mdno_displacement_stats_workspace_bytes(S, M, N, n_lags, n_bins);
    MDNO_REQUIRE(workspace && workspace_bytes >= need, MDNO_EINVAL, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_bins > 0) MDNO_HIP(hipMemsetAsync(counts, 0, (size_t)M * n_lags * n_bins * sizeof(int64_t), st));
    const Displacement acc{r_max, n_bins > 0 ? (double)n_bins / r_max : 0.0, n_bins};
    return run_statistic(who, frames, S, M, N, lags, n_lags, origin_stride, remove_com, acc, sum2, sum4, counts, workspace, st);
}

extern "C" int mdno_velocity_autocorrelation(const float* frames, int S, int M, int N, const int32_t* lags, int n_lags,
                                             int origin_stride, int remove_com, double* corr, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    const char* who = "velocity_autocorrelation";
    bool done = false;
    MDNO_TRY(check_common(who, frames, S, M, N, lags, n_lags, origin_stride, Velocity::span, &done));
    if (done) return MDNO_OK;
    MDNO_REQUIRE(corr, MDNO_EINVAL, "%s: null pointer (corr)", who);
    const size_t need = mdno_velocity_autocorrelation_workspace_bytes(S, M, N, n_lags);
    MDNO_REQUIRE(workspace && workspace_bytes >= need, MDNO_EINVAL, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    return run_statistic(who, frames, S, M, N, lags, n_lags, origin_stride, remove_com, Velocity{}, corr, nullptr, nullptr,
                         workspace, static_cast<hipStream_t>(stream));
}

extern "C" int mdno_unwrap_frames(const float* frames, int S, int M, int N, const double* box, float* out, void* stream) {
    MDNO_REQUIRE(S >= 0 && M >= 0 && N >= 0, MDNO_EINVAL, "unwrap_frames: S=%d M=%d N=%d", S, M, N);
    PbcBox b{};
    MDNO_TRY(pbc_box_from(box, 0.0, &b, "mdno_unwrap_frames"));
    const long long per_frame = (long long)M * N * 3;
    if (S == 0 || per_frame == 0) return MDNO_OK;
    MDNO_REQUIRE(frames && out, MDNO_EINVAL, "unwrap_frames: null pointer");
    const size_t total = (size_t)S * per_frame;
    MDNO_REQUIRE(out + total <= frames || frames + total <= out, MDNO_EINVAL, "unwrap_frames: out overlaps frames");
    const long long blocks = (per_frame + kThreads - 1) / kThreads;
    MDNO_REQUIRE(blocks < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "unwrap_frames: M * N = %lld exceeds the launch grid",
                 per_frame / 3);
    hipLaunchKernelGGL(unwrap_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), frames, S,
                       per_frame, b, out);
    return check_launch("unwrap_frames");
}
