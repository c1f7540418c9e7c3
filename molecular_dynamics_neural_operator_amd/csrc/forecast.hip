// Scoring a rollout against the true trajectory on the device (forecast.py): what the reference does on the host after
// every epoch — the contact map of a forecast beside the real one (make_propagation_movie / get_contact_map,
// graph_kernel.py:416-443), the per-step MSE of the notebook's propogate (bba_analysis.ipynb:351) and the structural
// distance its plots are coloured by (dataset.py:118) — for frames f32 [S, M, N, 3] against truth f32 [S, N, 3] (shared
// by the members) or [S, M, N, 3].  Per (step s, member m):
//     mse     mean over the 3N coordinates of (frame - truth)^2, differences and sum in fp64
//     rmsd    after the optimal RIGID superposition (centroids removed, proper rotations only): with a = p - mean(p),
//             b = q - mean(q), G = sum |a|^2 + sum |b|^2 and lambda the largest eigenvalue of Horn's 4 x 4 quaternion
//             matrix of the cross-covariance sum a b^T, rmsd^2 = max(0, G - 2 lambda) / N.  Everything is accumulated in
//             fp64; the eigenvalue is taken by cyclic Jacobi sweeps (a fixed number of them; exact zeros are skipped,
//             so identical, planar, collinear and one- or two-atom frames need no special case)
//     counts  i64 {contacts of the forecast, of the truth, of both} over all ORDERED pairs (i, j), diagonal included:
//             the non-zeros of the dense map get_contact_map builds.  The pair test is within() of graph_small.h (fp64,
//             strict <, the radius graph's own), evaluated for i <= j and counted twice off the diagonal — within() is
//             symmetric in its two atoms bit for bit (the differences change sign, their squares do not).  A NaN or
//             Inf coordinate is in no contact (the comparison is false).
//     first_nonfinite[m]  the first step whose forecast frame holds a NaN or Inf (-1: none); that (s, m) gets
//             mse = rmsd = NaN, its counts stay as defined above, no other (s, m) is touched.
// No atomics anywhere: every (s, m) is computed by its own workgroup(s) with fixed-order reductions (reduce.h), so a
// member scored alone has the bits it has inside any batch.
//
// Two forms.  Up to kLdsAtoms atoms ONE workgroup stages both frames in LDS (24 N bytes) and does all of the above;
// the pair tests of rows i and N-1-i are taken together (N + 1 tests: every wave iteration is full).  Larger frames
// are split: per-tile partial sums (1,024 atoms), centroids from the partials in tile order, per-tile partial
// covariances, 256 x 256 pair-test tiles for bi <= bj, and one finishing workgroup per (s, m) that adds the partials
// in tile order.  Counts are integers: both forms give the same ones.
//
// mdno_contact_maps: the dense u8 [F, N, N] maps themselves, sixteen pair tests per thread, one 16-byte store each.
//
// The kernels that test pairs are templated on the pair test (pbc.h): OpenPair is within() itself, PbcPair the
// minimum-image test of a periodic box (mdno_forecast_score_pbc / mdno_contact_maps_pbc, include/mdno_pbc.h) — symmetric
// in its two atoms bit for bit as well (rint is odd), so the i <= j counting holds for both.
#include "pbc.h"
#include "reduce.h"
#include "superpose.h"
#include "../../include/mdno_pbc.h"

#include <cmath>

namespace mdno {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kLdsAtoms = 2048;        // 2 frames x 2,048 atoms x 12 B = 48 KiB of LDS
constexpr int kSumTile = 1024;         // atoms per workgroup in the tiled sums
constexpr int kPairTile = 256;         // atoms per side of a pair-test tile

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and Inf

// ---------------------------------------------------------------------------------------------- LDS form
template <class Pair>
__global__ __launch_bounds__(kThreads) void forecast_score_lds_kernel(const float* __restrict__ frames,
                                                                      const float* __restrict__ truth,
                                                                      int truth_per_member, int M, int N, const Pair pair,
                                                                      double* __restrict__ mse, double* __restrict__ rmsd,
                                                                      int* __restrict__ flags,
                                                                      long long* __restrict__ counts) {
    extern __shared__ float lds[];
    __shared__ double slots_d[kWaves * 10];
    __shared__ int slots_i[kWaves * 3];
    float* p = lds;
    float* q = lds + (size_t)N * 3;
    const long long sm = blockIdx.x;
    const long long s = sm / M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* P = frames + (size_t)sm * N * 3;
    const float* Q = truth + (size_t)(truth_per_member ? sm : s) * N * 3;
    int bad = 0;
    for (int k = tid; k < 3 * N; k += kThreads) {
        const float pv = P[k];
        p[k] = pv;
        q[k] = Q[k];
        bad |= !finite_f(pv);
    }
    bad = __syncthreads_or(bad);
    // sums of the coordinates and of the squared differences
    double v7[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < N; i += kThreads) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double pd = p[3 * i + d], qd = q[3 * i + d], df = pd - qd;
            v7[d] += pd;
            v7[3 + d] += qd;
            v7[6] += df * df;
        }
    }
    block_reduce_add<kWaves>(v7, slots_d);
    const double n = (double)N;
    double cp[3], cq[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        cp[d] = v7[d] / n;
        cq[d] = v7[3 + d] / n;
    }
    // cross-covariance and G about the centroids
    double v10[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < N; i += kThreads) {
        double a[3], b[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            a[d] = (double)p[3 * i + d] - cp[d];
            b[d] = (double)q[3 * i + d] - cq[d];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v10[3 * r + c] += a[r] * b[c];
            v10[9] += a[r] * a[r] + b[r] * b[r];
        }
    }
    block_reduce_add<kWaves>(v10, slots_d);
    // pair tests: rows r and N-1-r together hold N+1 pairs with j >= i
    int cnt[3] = {0, 0, 0};
    const int half = (N + 1) / 2;
    for (int r = wave; r < half; r += kWaves) {
        const int i2 = N - 1 - r;
        const int n1 = N - r, n2 = i2 != r ? r + 1 : 0;
        const double p1x = p[3 * r], p1y = p[3 * r + 1], p1z = p[3 * r + 2];
        const double q1x = q[3 * r], q1y = q[3 * r + 1], q1z = q[3 * r + 2];
        const double p2x = p[3 * i2], p2y = p[3 * i2 + 1], p2z = p[3 * i2 + 2];
        const double q2x = q[3 * i2], q2y = q[3 * i2 + 1], q2z = q[3 * i2 + 2];
        for (int c = lane; c < n1 + n2; c += 64) {
            const bool first = c < n1;
            const int i = first ? r : i2;
            const int j = first ? r + c : i2 + (c - n1);
            const bool in_f = pair(first ? p1x : p2x, first ? p1y : p2y, first ? p1z : p2z, p + 3 * j);
            const bool in_t = pair(first ? q1x : q2x, first ? q1y : q2y, first ? q1z : q2z, q + 3 * j);
            const int w = j == i ? 1 : 2;
            cnt[0] += in_f ? w : 0;
            cnt[1] += in_t ? w : 0;
            cnt[2] += (in_f && in_t) ? w : 0;
        }
    }
    block_reduce_add<kWaves>(cnt, slots_i);
    if (tid == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        mse[sm] = bad ? nan : v7[6] / (3.0 * n);
        const double r2 = rmsd2_from_moments(v10, v10[9], n);
        rmsd[sm] = bad ? nan : sqrt(r2);
        flags[sm] = bad;
        counts[sm * 3 + 0] = cnt[0];
        counts[sm * 3 + 1] = cnt[1];
        counts[sm * 3 + 2] = cnt[2];
    }
}

// ---------------------------------------------------------------------------------------------- tiled form
// part1 [SM, T, 8]: sums of p (3), of q (3), of the squared differences, and 1.0 if a forecast coordinate is not finite
__global__ __launch_bounds__(kThreads) void forecast_tile_sums_kernel(const float* __restrict__ frames,
                                                                      const float* __restrict__ truth,
                                                                      int truth_per_member, int M, int N,
                                                                      double* __restrict__ part1) {
    __shared__ double slots_d[kWaves * 8];
    const long long sm = blockIdx.x, s = sm / M;
    const int tile = blockIdx.y, T = gridDim.y;
    const float* P = frames + (size_t)sm * N * 3;
    const float* Q = truth + (size_t)(truth_per_member ? sm : s) * N * 3;
    const int i1 = min(N, (tile + 1) * kSumTile);
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tile * kSumTile + threadIdx.x; i < i1; i += kThreads) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float pf = P[3 * (size_t)i + d];
            const double pd = pf, qd = Q[3 * (size_t)i + d], df = pd - qd;
            v[d] += pd;
            v[3 + d] += qd;
            v[6] += df * df;
            if (!finite_f(pf)) v[7] = 1.0;
        }
    }
    block_reduce_add<kWaves>(v, slots_d);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) part1[((size_t)sm * T + tile) * 8 + k] = v[k];
    }
}

// part2 [SM, T, 10]: the tile's share of the cross-covariance (9) and of G, about centroids every workgroup takes
// from part1 in tile order
__global__ __launch_bounds__(kThreads) void forecast_tile_cov_kernel(const float* __restrict__ frames,
                                                                     const float* __restrict__ truth,
                                                                     int truth_per_member, int M, int N,
                                                                     const double* __restrict__ part1,
                                                                     double* __restrict__ part2) {
    __shared__ double slots_d[kWaves * 10];
    const long long sm = blockIdx.x, s = sm / M;
    const int tile = blockIdx.y, T = gridDim.y;
    const float* P = frames + (size_t)sm * N * 3;
    const float* Q = truth + (size_t)(truth_per_member ? sm : s) * N * 3;
    double c6[6] = {0, 0, 0, 0, 0, 0};
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int k = 0; k < 6; ++k) c6[k] += part1[((size_t)sm * T + t) * 8 + k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) c6[k] /= (double)N;
    const int i1 = min(N, (tile + 1) * kSumTile);
    double v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tile * kSumTile + threadIdx.x; i < i1; i += kThreads) {
        double a[3], b[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            a[d] = (double)P[3 * (size_t)i + d] - c6[d];
            b[d] = (double)Q[3 * (size_t)i + d] - c6[3 + d];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 * r + c] += a[r] * b[c];
            v[9] += a[r] * a[r] + b[r] * b[r];
        }
    }
    block_reduce_add<kWaves>(v, slots_d);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 10; ++k) part2[((size_t)sm * T + tile) * 10 + k] = v[k];
    }
}

// cpart [SM, T2, T2, 3] (entries with bj < bi are never written nor read): thread t owns atom bi*256 + t and walks the
// atoms of tile bj from LDS.  A diagonal tile counts its ordered pairs directly, the others twice.
template <class Pair>
__global__ __launch_bounds__(kThreads) void forecast_tile_contacts_kernel(const float* __restrict__ frames,
                                                                          const float* __restrict__ truth,
                                                                          int truth_per_member, int M, int N,
                                                                          const Pair pair, int* __restrict__ cpart) {
    const int bi = blockIdx.y, bj = blockIdx.z, T2 = gridDim.y;
    if (bj < bi) return;
    __shared__ float pj[kPairTile * 3], qj[kPairTile * 3];
    __shared__ int slots_i[kWaves * 3];
    const long long sm = blockIdx.x, s = sm / M;
    const float* P = frames + (size_t)sm * N * 3;
    const float* Q = truth + (size_t)(truth_per_member ? sm : s) * N * 3;
    const int j0 = bj * kPairTile, nj = min(N - j0, kPairTile);
    for (int k = threadIdx.x; k < 3 * nj; k += kThreads) {
        pj[k] = P[3 * (size_t)j0 + k];
        qj[k] = Q[3 * (size_t)j0 + k];
    }
    __syncthreads();
    const int i = bi * kPairTile + threadIdx.x;
    int cnt[3] = {0, 0, 0};
    if (i < N) {
        const double px = P[3 * (size_t)i], py = P[3 * (size_t)i + 1], pz = P[3 * (size_t)i + 2];
        const double qx = Q[3 * (size_t)i], qy = Q[3 * (size_t)i + 1], qz = Q[3 * (size_t)i + 2];
        const int w = bi == bj ? 1 : 2;
        for (int j = 0; j < nj; ++j) {
            const bool in_f = pair(px, py, pz, pj + 3 * j);
            const bool in_t = pair(qx, qy, qz, qj + 3 * j);
            cnt[0] += in_f ? w : 0;
            cnt[1] += in_t ? w : 0;
            cnt[2] += (in_f && in_t) ? w : 0;
        }
    }
    block_reduce_add<kWaves>(cnt, slots_i);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) cpart[(((size_t)sm * T2 + bi) * T2 + bj) * 3 + k] = cnt[k];
    }
}

__global__ __launch_bounds__(kThreads) void forecast_tile_finish_kernel(const double* __restrict__ part1,
                                                                        const double* __restrict__ part2,
                                                                        const int* __restrict__ cpart, int N, int T, int T2,
                                                                        double* __restrict__ mse, double* __restrict__ rmsd,
                                                                        int* __restrict__ flags,
                                                                        long long* __restrict__ counts) {
    __shared__ long long slots_l[kWaves * 3];
    const long long sm = blockIdx.x;
    long long cnt[3] = {0, 0, 0};
    for (int e = threadIdx.x; e < T2 * T2; e += kThreads) {
        if (e % T2 < e / T2) continue;
        const int* c = cpart + ((size_t)sm * T2 * T2 + e) * 3;
        cnt[0] += c[0];
        cnt[1] += c[1];
        cnt[2] += c[2];
    }
    block_reduce_add<kWaves>(cnt, slots_l);
    if (threadIdx.x == 0) {
        double sq = 0.0, bad = 0.0, v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int t = 0; t < T; ++t) {
            sq += part1[((size_t)sm * T + t) * 8 + 6];
            bad += part1[((size_t)sm * T + t) * 8 + 7];
#pragma unroll
            for (int k = 0; k < 10; ++k) v[k] += part2[((size_t)sm * T + t) * 10 + k];
        }
        const double n = (double)N, nan = __longlong_as_double(0x7ff8000000000000ll);
        const double r2 = rmsd2_from_moments(v, v[9], n);
        mse[sm] = bad != 0.0 ? nan : sq / (3.0 * n);
        rmsd[sm] = bad != 0.0 ? nan : sqrt(r2);
        flags[sm] = bad != 0.0;
        counts[sm * 3 + 0] = cnt[0];
        counts[sm * 3 + 1] = cnt[1];
        counts[sm * 3 + 2] = cnt[2];
    }
}

// first[m] = the smallest s with flags[s, m] set, -1 for none (flags == nullptr: no step was looked at); one wave per member
__global__ __launch_bounds__(64) void forecast_first_flag_kernel(const int* __restrict__ flags, int S, int M,
                                                                 int* __restrict__ first) {
    const int m = blockIdx.x;
    int best = 0x7fffffff;
    if (flags != nullptr)
        for (int s = threadIdx.x; s < S; s += 64)
            if (flags[(size_t)s * M + m] && s < best) best = s;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_xor(best, off));
    if (threadIdx.x == 0) first[m] = best == 0x7fffffff ? -1 : best;
}

// ---------------------------------------------------------------------------------------------- dense maps
// maps u8 [F*N*N] flat, 16 consecutive bytes per thread as one 16-byte store (the tail of the last thread by bytes)
template <class Pair>
__global__ __launch_bounds__(kThreads) void contact_maps_kernel(const float* __restrict__ frames, long long F, int N,
                                                                const Pair pair, unsigned char* __restrict__ maps) {
    const long long nn = (long long)N * N, total = F * nn;
    const long long base = ((long long)blockIdx.x * kThreads + threadIdx.x) * 16;
    if (base >= total) return;
    long long f = base / nn;
    const long long rem = base - f * nn;
    int i = (int)(rem / N), j = (int)(rem - (long long)i * N);
    const int count = total - base < 16 ? (int)(total - base) : 16;
    unsigned int word[4] = {0, 0, 0, 0};
    const float* pos = frames + (size_t)f * N * 3;
    double xi = pos[3 * (size_t)i], yi = pos[3 * (size_t)i + 1], zi = pos[3 * (size_t)i + 2];
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        if (b < count) {
            if (pair(xi, yi, zi, pos + 3 * (size_t)j)) word[b >> 2] |= 1u << (8 * (b & 3));
            if (++j == N) {
                j = 0;
                if (++i == N) {
                    i = 0;
                    ++f;
                }
                if (b + 1 < count) {
                    pos = frames + (size_t)f * N * 3;
                    xi = pos[3 * (size_t)i], yi = pos[3 * (size_t)i + 1], zi = pos[3 * (size_t)i + 2];
                }
            }
        }
    }
    if (count == 16) {
        *reinterpret_cast<uint4*>(maps + base) = make_uint4(word[0], word[1], word[2], word[3]);
    } else {
        for (int b = 0; b < count; ++b) maps[base + b] = (unsigned char)((word[b >> 2] >> (8 * (b & 3))) & 0xffu);
    }
}

int tiles(int N, int tile) { return (N + tile - 1) / tile; }

bool use_lds_form(int N, int form) { return form == MDNO_FORECAST_LDS || (form == MDNO_FORECAST_AUTO && N <= kLdsAtoms); }

struct ScoreCarve {
    int* flags;
    double *part1 = nullptr, *part2 = nullptr;
    int* cpart = nullptr;
    size_t total;
    ScoreCarve(void* ws, long long SM, int N, bool lds) {
        Carver c(ws);
        flags = c.take<int>((size_t)SM);
        if (!lds) {
            const size_t T = tiles(N, kSumTile), T2 = tiles(N, kPairTile);
            part1 = c.take<double>((size_t)SM * T * 8);
            part2 = c.take<double>((size_t)SM * T * 10);
            cpart = c.take<int>((size_t)SM * T2 * T2 * 3);
        }
        total = c.used();
    }
};

bool cutoff_ok(double c) { return std::isfinite(c) && c >= 0.0; }

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" size_t mdno_forecast_score_workspace_bytes(int S, int M, int N, int form) {
    if (S <= 0 || M <= 0 || N <= 0 || form < MDNO_FORECAST_AUTO || form > MDNO_FORECAST_TILED) return 0;
    return ScoreCarve(nullptr, (long long)S * M, N, use_lds_form(N, form)).total;
}

template <class Pair>
static int forecast_score_impl(const float* frames, const float* truth, int truth_per_member, int S, int M, int N,
                               const Pair& pair, double* mse, double* rmsd, int64_t* counts, int32_t* first_nonfinite,
                               int form, void* workspace, size_t workspace_bytes, void* stream) {
    MDNO_REQUIRE(form >= MDNO_FORECAST_AUTO && form <= MDNO_FORECAST_TILED, MDNO_EINVAL, "forecast_score: form=%d", form);
    MDNO_REQUIRE(M == 0 || first_nonfinite, MDNO_EINVAL, "forecast_score: null pointer (first_nonfinite)");
    const long long SM = (long long)S * M;
    const bool empty = SM == 0 || N == 0;
    MDNO_REQUIRE(empty || (frames && truth && mse && rmsd && counts), MDNO_EINVAL, "forecast_score: null pointer");
    MDNO_REQUIRE(SM < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "forecast_score: S*M = %lld exceeds the launch grid", SM);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (empty) {        // nothing to score: no member was ever non-finite
        if (M == 0) return MDNO_OK;
        hipLaunchKernelGGL(forecast_first_flag_kernel, dim3(M), dim3(64), 0, st, nullptr, 0, M, first_nonfinite);
        return check_launch("forecast_score");
    }
    const bool lds = use_lds_form(N, form);
    MDNO_REQUIRE(!lds || N <= kLdsAtoms, MDNO_EUNSUPPORTED, "forecast_score: the LDS form holds at most %d atoms (N=%d)",
                 kLdsAtoms, N);
    const int T = tiles(N, kSumTile), T2 = tiles(N, kPairTile);
    MDNO_REQUIRE(lds || T2 <= 65535, MDNO_EUNSUPPORTED, "forecast_score: N=%d exceeds the tiled form's grid", N);
    MDNO_REQUIRE(workspace, MDNO_EINVAL, "forecast_score: null pointer (workspace)");
    ScoreCarve c(workspace, SM, N, lds);
    MDNO_REQUIRE(workspace_bytes >= c.total, MDNO_EWORKSPACE, "forecast_score: workspace %zu < %zu", workspace_bytes, c.total);
    long long* cnt = reinterpret_cast<long long*>(counts);
    if (lds) {
        hipLaunchKernelGGL(forecast_score_lds_kernel<Pair>, dim3((unsigned)SM), dim3(kThreads), (size_t)N * 24, st, frames, truth,
                           truth_per_member, M, N, pair, mse, rmsd, c.flags, cnt);
    } else {
        hipLaunchKernelGGL(forecast_tile_sums_kernel, dim3((unsigned)SM, T), dim3(kThreads), 0, st, frames, truth,
                           truth_per_member, M, N, c.part1);
        hipLaunchKernelGGL(forecast_tile_cov_kernel, dim3((unsigned)SM, T), dim3(kThreads), 0, st, frames, truth,
                           truth_per_member, M, N, c.part1, c.part2);
        hipLaunchKernelGGL(forecast_tile_contacts_kernel<Pair>, dim3((unsigned)SM, T2, T2), dim3(kThreads), 0, st, frames, truth,
                           truth_per_member, M, N, pair, c.cpart);
        hipLaunchKernelGGL(forecast_tile_finish_kernel, dim3((unsigned)SM), dim3(kThreads), 0, st, c.part1, c.part2, c.cpart,
                           N, T, T2, mse, rmsd, c.flags, cnt);
    }
    hipLaunchKernelGGL(forecast_first_flag_kernel, dim3(M), dim3(64), 0, st, c.flags, S, M, first_nonfinite);
    return check_launch("forecast_score");
}

extern "C" int mdno_forecast_score(const float* frames, const float* truth, int truth_per_member, int S, int M, int N,
                                   double cutoff, double* mse, double* rmsd, int64_t* counts, int32_t* first_nonfinite,
                                   int form, void* workspace, size_t workspace_bytes, void* stream) {
    MDNO_REQUIRE(S >= 0 && M >= 0 && N >= 0, MDNO_EINVAL, "forecast_score: S=%d M=%d N=%d", S, M, N);
    MDNO_REQUIRE(cutoff_ok(cutoff), MDNO_EINVAL, "forecast_score: cutoff %g is not a finite non-negative number", cutoff);
    return forecast_score_impl(frames, truth, truth_per_member, S, M, N, OpenPair{cutoff}, mse, rmsd, counts, first_nonfinite,
                               form, workspace, workspace_bytes, stream);
}

extern "C" int mdno_forecast_score_pbc(const float* frames, const float* truth, int truth_per_member, int S, int M, int N,
                                       double cutoff, const double* box, double* mse, double* rmsd, int64_t* counts,
                                       int32_t* first_nonfinite, int form, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    MDNO_REQUIRE(S >= 0 && M >= 0 && N >= 0, MDNO_EINVAL, "forecast_score_pbc: S=%d M=%d N=%d", S, M, N);
    PbcPair pair{cutoff, {}};
    MDNO_TRY(pbc_box_from(box, cutoff, &pair.box, "mdno_forecast_score_pbc"));
    return forecast_score_impl(frames, truth, truth_per_member, S, M, N, pair, mse, rmsd, counts, first_nonfinite, form,
                               workspace, workspace_bytes, stream);
}

template <class Pair>
static int contact_maps_impl(const float* frames, int64_t F, int N, const Pair& pair, uint8_t* maps, void* stream) {
    if (F == 0 || N == 0) return MDNO_OK;
    MDNO_REQUIRE(frames && maps, MDNO_EINVAL, "contact_maps: null pointer");
    MDNO_REQUIRE((reinterpret_cast<uintptr_t>(maps) & 15) == 0, MDNO_EINVAL, "contact_maps: maps not 16-B aligned");
    const long long total = (long long)F * N * N;
    const long long blocks = (total + 16ll * kThreads - 1) / (16ll * kThreads);
    MDNO_REQUIRE(blocks < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "contact_maps: %lld bytes exceed one launch", total);
    hipLaunchKernelGGL(contact_maps_kernel<Pair>, dim3((unsigned)blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       frames, (long long)F, N, pair, maps);
    return check_launch("contact_maps");
}

extern "C" int mdno_contact_maps(const float* frames, int64_t F, int N, double cutoff, uint8_t* maps, void* stream) {
    MDNO_REQUIRE(F >= 0 && N >= 0, MDNO_EINVAL, "contact_maps: F=%lld N=%d", (long long)F, N);
    MDNO_REQUIRE(cutoff_ok(cutoff), MDNO_EINVAL, "contact_maps: cutoff %g is not a finite non-negative number", cutoff);
    return contact_maps_impl(frames, F, N, OpenPair{cutoff}, maps, stream);
}

extern "C" int mdno_contact_maps_pbc(const float* frames, int64_t F, int N, double cutoff, const double* box, uint8_t* maps,
                                     void* stream) {
    MDNO_REQUIRE(F >= 0 && N >= 0, MDNO_EINVAL, "contact_maps_pbc: F=%lld N=%d", (long long)F, N);
    PbcPair pair{cutoff, {}};
    MDNO_TRY(pbc_box_from(box, cutoff, &pair.box, "mdno_contact_maps_pbc"));
    return contact_maps_impl(frames, F, N, pair, maps, stream);
}
