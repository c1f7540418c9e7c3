// Structural observables of frames that lie in device memory (include/mdno_observe.h states THE RULE):
// the histogram of pair distances of every frame — the numerator of g(r) and p(r) (forecast.py: PairHistogram) — and the
// per-frame radius of gyration.  The pairs are those forecast.hip walks for its contact counts, and the distance is the
// one its pair test takes the root of (pbc.h: dist2 of OpenPair / PbcPair, the minimum image under a box); here every
// pair inside r_max is binned instead of counted.
//
// Two forms of the histogram, as in forecast.hip.  Up to kLdsAtoms atoms ONE workgroup stages the frame in LDS (12 N
// bytes), walks the pairs i < j with rows r and N-1-r taken together (N - 1 pairs: every wave iteration is full), adds 1
// to a u32 histogram in LDS per counted pair, and stores its own row of counts as i64: no atomics on memory, no zeroing
// pass, nothing outside the row written.  Any N: 256 x 256 pair tiles for bi <= bj (a diagonal tile takes i < j, the
// others every pair once), a u32 histogram in LDS per workgroup, non-zero bins added to the frame's row with integer
// atomics after the entry point zeroed the rows on the same stream.  Integers: any order of the adds gives the same bits.
//
// ONE histogram per workgroup.  Replicas of it (thread t adding into copy t % R, bin-major so that the lanes of a wave that
// hit one bin spread over R banks) were built and timed at R = 4, 16 and 64: no faster at 8 or 200 bins, slower at 64
// (occupancy) — the fp64 pair arithmetic, not the LDS add, is what the kernels wait for (EXPERIMENTS.md).
#include "pbc.h"
#include "reduce.h"
#include "../../include/mdno_observe.h"

#include <cmath>

namespace mdno {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kLdsAtoms = 2048;            // as forecast.hip's LDS form
constexpr int kPairTile = 256;             // atoms per side of a pair tile, as forecast.hip's
constexpr int kMaxBins = 4096;

// counts the pair in `hist` if it lies inside r_max = pair.cutoff
template <class Pair>
__device__ __forceinline__ void bin_pair(const Pair& pair, double xi, double yi, double zi, const float* __restrict__ pj,
                                         double inv_dr, int n_bins, unsigned int* hist) {
    const double r = sqrt(pair.dist2(xi, yi, zi, pj));
    if (r < pair.cutoff) {                 // false for a NaN or an Inf
        int b = (int)(r * inv_dr);         // 0 <= r * inv_dr < n_bins + 1: the value (long long) gives
        b = b < n_bins ? b : n_bins - 1;
        atomicAdd(hist + b, 1u);
    }
}

// ---------------------------------------------------------------------------------------------- LDS form
// dynamic LDS: the frame f32 [3 N], then the histogram u32 [n_bins]
template <class Pair>
__global__ __launch_bounds__(kThreads) void pair_histogram_lds_kernel(const float* __restrict__ frames, int N,
                                                                      const Pair pair, double inv_dr, int n_bins,
                                                                      long long* __restrict__ counts) {
    extern __shared__ float lds[];
    float* p = lds;
    unsigned int* hist = reinterpret_cast<unsigned int*>(lds + (size_t)N * 3);
    const long long f = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* P = frames + (size_t)f * N * 3;
    for (int k = tid; k < 3 * N; k += kThreads) p[k] = P[k];
    for (int k = tid; k < n_bins; k += kThreads) hist[k] = 0u;
    __syncthreads();
    // rows r and N-1-r together hold N-1 pairs with j > i (the middle row of an odd N stands alone)
    const int half = (N + 1) / 2;
    for (int r = wave; r < half; r += kWaves) {
        const int i2 = N - 1 - r;
        const int n1 = N - 1 - r, n2 = i2 != r ? r : 0;
        const double x1 = p[3 * r], y1 = p[3 * r + 1], z1 = p[3 * r + 2];
        const double x2 = p[3 * i2], y2 = p[3 * i2 + 1], z2 = p[3 * i2 + 2];
        for (int c = lane; c < n1 + n2; c += 64) {
            const bool first = c < n1;
            const int j = first ? r + 1 + c : i2 + 1 + (c - n1);
            bin_pair(pair, first ? x1 : x2, first ? y1 : y2, first ? z1 : z2, p + 3 * j, inv_dr, n_bins, hist);
        }
    }
    __syncthreads();
    long long* row = counts + (size_t)f * n_bins;
    for (int b = tid; b < n_bins; b += kThreads) row[b] = (long long)hist[b];
}

// ---------------------------------------------------------------------------------------------- tiled form
// grid (F, T2, T2), workgroups with bj < bi leave at once: thread t owns atom bi*256 + t and walks the atoms of tile bj
// from LDS.  dynamic LDS: the histogram u32 [n_bins].  The rows of counts are zero when this starts.
template <class Pair>
__global__ __launch_bounds__(kThreads) void pair_histogram_tile_kernel(const float* __restrict__ frames, int N,
                                                                       const Pair pair, double inv_dr, int n_bins,
                                                                       unsigned long long* __restrict__ counts) {
    const int bi = blockIdx.y, bj = blockIdx.z;
    if (bj < bi) return;
    extern __shared__ float lds[];
    __shared__ float pj[kPairTile * 3];
    unsigned int* hist = reinterpret_cast<unsigned int*>(lds);
    const long long f = blockIdx.x;
    const int tid = threadIdx.x;
    const float* P = frames + (size_t)f * N * 3;
    const int j0 = bj * kPairTile, nj = min(N - j0, kPairTile);
    for (int k = tid; k < 3 * nj; k += kThreads) pj[k] = P[3 * (size_t)j0 + k];
    for (int k = tid; k < n_bins; k += kThreads) hist[k] = 0u;
    __syncthreads();
    const int i = bi * kPairTile + tid;
    if (i < N) {
        const double xi = P[3 * (size_t)i], yi = P[3 * (size_t)i + 1], zi = P[3 * (size_t)i + 2];
        for (int j = bi == bj ? tid + 1 : 0; j < nj; ++j) bin_pair(pair, xi, yi, zi, pj + 3 * j, inv_dr, n_bins, hist);
    }
    __syncthreads();
    unsigned long long* row = counts + (size_t)f * n_bins;
    for (int b = tid; b < n_bins; b += kThreads) {
        if (hist[b]) atomicAdd(row + b, (unsigned long long)hist[b]);
    }
}

// ---------------------------------------------------------------------------------------------- radius of gyration
__global__ __launch_bounds__(kThreads) void radius_of_gyration_kernel(const float* __restrict__ frames, int N,
                                                                      double* __restrict__ rg) {
    __shared__ double slots_d[kWaves * 3];
    const long long f = blockIdx.x;
    const float* P = frames + (size_t)f * N * 3;
    double c[3] = {0, 0, 0};
    for (int i = threadIdx.x; i < N; i += kThreads) {
#pragma unroll
        for (int d = 0; d < 3; ++d) c[d] += (double)P[3 * (size_t)i + d];
    }
    block_reduce_add<kWaves>(c, slots_d);
    const double n = (double)N;
#pragma unroll
    for (int d = 0; d < 3; ++d) c[d] /= n;
    double q[1] = {0};
    for (int i = threadIdx.x; i < N; i += kThreads) {
        const double dx = (double)P[3 * (size_t)i] - c[0], dy = (double)P[3 * (size_t)i + 1] - c[1],
                     dz = (double)P[3 * (size_t)i + 2] - c[2];
        q[0] += (dx * dx + dy * dy) + dz * dz;
    }
    block_reduce_add<kWaves>(q, slots_d);
    if (threadIdx.x == 0) rg[f] = sqrt(q[0] / n);      // N == 0: 0 / 0; an Inf coordinate: Inf - Inf
}

int tiles(int N, int tile) { return (N + tile - 1) / tile; }

bool form_ok(int form) { return form >= MDNO_FORECAST_AUTO && form <= MDNO_FORECAST_TILED; }

bool use_lds_form(int N, int form) { return form == MDNO_FORECAST_LDS || (form == MDNO_FORECAST_AUTO && N <= kLdsAtoms); }

template <class Pair>
int pair_histogram_impl(const float* frames, int64_t F, int N, const Pair& pair, double inv_dr, int n_bins, int64_t* counts,
                        bool lds, hipStream_t st) {
    if (lds) {
        hipLaunchKernelGGL(pair_histogram_lds_kernel<Pair>, dim3((unsigned)F), dim3(kThreads),
                           (size_t)N * 12 + (size_t)n_bins * 4, st, frames, N, pair, inv_dr, n_bins,
                           reinterpret_cast<long long*>(counts));      // at most 24 KiB + 16 KiB of LDS
    } else {
        MDNO_HIP(hipMemsetAsync(counts, 0, (size_t)F * n_bins * sizeof(int64_t), st));
        if (N < 2) return MDNO_OK;         // no pair
        const int T2 = tiles(N, kPairTile);
        hipLaunchKernelGGL(pair_histogram_tile_kernel<Pair>, dim3((unsigned)F, T2, T2), dim3(kThreads),
                           (size_t)n_bins * 4, st, frames, N, pair, inv_dr, n_bins,
                           reinterpret_cast<unsigned long long*>(counts));
    }
    return check_launch("pair_histogram");
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" size_t mdno_pair_histogram_workspace_bytes(int64_t F, int N, int n_bins, int form) {
    (void)F, (void)N, (void)n_bins, (void)form;
    return 0;      // the LDS form stores whole rows, the tiled form adds into rows the entry point zeroes
}

extern "C" int mdno_pair_histogram(const float* frames, int64_t F, int N, double r_max, int n_bins, const double* box,
                                   int64_t* counts, int form, void* workspace, size_t workspace_bytes, void* stream) {
    MDNO_REQUIRE(F >= 0 && N >= 0, MDNO_EINVAL, "pair_histogram: F=%lld N=%d", (long long)F, N);
    MDNO_REQUIRE(form_ok(form), MDNO_EINVAL, "pair_histogram: form=%d", form);
    MDNO_REQUIRE(n_bins >= 1 && n_bins <= kMaxBins, MDNO_EINVAL, "pair_histogram: n_bins=%d is outside 1 .. %d", n_bins, kMaxBins);
    MDNO_REQUIRE(std::isfinite(r_max) && r_max > 0.0, MDNO_EINVAL, "pair_histogram: r_max %g is not a finite positive number",
                 r_max);
    PbcBox b{};
    if (box != nullptr) MDNO_TRY(pbc_box_from(box, r_max, &b, "mdno_pair_histogram"));
    const size_t need = mdno_pair_histogram_workspace_bytes(F, N, n_bins, form);
    MDNO_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), MDNO_EINVAL, "pair_histogram: workspace %zu < %zu",
                 workspace_bytes, need);
    if (F == 0) return MDNO_OK;
    MDNO_REQUIRE(counts && (frames || N == 0), MDNO_EINVAL, "pair_histogram: null pointer");
    const bool lds = use_lds_form(N, form);
    MDNO_REQUIRE(!lds || N <= kLdsAtoms, MDNO_EUNSUPPORTED, "pair_histogram: the LDS form holds at most %d atoms (N=%d)",
                 kLdsAtoms, N);
    MDNO_REQUIRE(F < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "pair_histogram: F = %lld exceeds the launch grid", (long long)F);
    MDNO_REQUIRE(lds || tiles(N, kPairTile) <= 65535, MDNO_EUNSUPPORTED, "pair_histogram: N=%d exceeds the tiled form's grid", N);
    const double inv_dr = (double)n_bins / r_max;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (b.any()) return pair_histogram_impl(frames, F, N, PbcPair{r_max, b}, inv_dr, n_bins, counts, lds, st);
    return pair_histogram_impl(frames, F, N, OpenPair{r_max}, inv_dr, n_bins, counts, lds, st);
}

extern "C" int mdno_radius_of_gyration(const float* frames, int64_t F, int N, double* rg, void* stream) {
    MDNO_REQUIRE(F >= 0 && N >= 0, MDNO_EINVAL, "radius_of_gyration: F=%lld N=%d", (long long)F, N);
    if (F == 0) return MDNO_OK;
    MDNO_REQUIRE(rg && (frames || N == 0), MDNO_EINVAL, "radius_of_gyration: null pointer");
    MDNO_REQUIRE(F < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "radius_of_gyration: F = %lld exceeds the launch grid", (long long)F);
    hipLaunchKernelGGL(radius_of_gyration_kernel, dim3((unsigned)F), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       frames, N, rg);
    return check_launch("radius_of_gyration");
}
