// Internal coordinates on the device (include/mdno_internal.h states the rule and its evaluation order):
// pair distances, angle cosines and dihedral (cos, sin) of every frame as the rows of a feature matrix, and a per-column
// histogram of such a matrix (forecast.py: Featurizer, internal_coordinates, feature_histograms).
//
//   ic_features_kernel<lds>  grid (frame groups, item chunks).  An ITEM is one index tuple: a pair or a triple (one column)
//                            or a quad (two columns, one in radians).  A workgroup owns G = MDNO_IC_FRAMES_PER_GROUP(N)
//                            consecutive frames x kChunk items and its threads walk (frame, item) in strides of the
//                            workgroup, the item fastest: consecutive lanes read consecutive tuples and store consecutive
//                            columns.  lds: the G frames are first copied into LDS as they lie in memory (one contiguous
//                            run of G N 3 floats, dword for dword: coalesced loads, conflict-free stores) and the
//                            coordinates are gathered from there with ds_read_b32; otherwise they are gathered from
//                            global memory.  Both call ic_item, THE arithmetic: the bits cannot differ.
//   ic_hist_kernel           grid (row blocks, column tiles, column groups): integer atomics into a private table in LDS,
//                            flushed with 64-bit integer atomics.  The ranges travel by value (kHistCols columns per launch,
//                            shared by every group: the members of a feature tensor [S, M, D] are M groups of one launch).
// LDS IMAGE.  Atoms stay 12 bytes apart (array of structures).  ds_read_b32 banks are (dword address) mod 32 and a wave
// is served in two groups of 32 lanes: along a chain lane t reads atom a0 + t, dword 3 (a0 + t) + c, and 3 is odd, so the
// 32 lanes of a group fall on 32 distinct banks — the same as a structure-of-arrays image would give (stride 1).  Strided
// atom sets (stride s) conflict gcd(3 s, 32) = gcd(s, 32)-way in either image, and an arbitrary index list conflicts at
// random in any: no padding helps a gather whose addresses the caller chooses.  So the image is the one that costs
// nothing to build.  24 KiB per workgroup at most: six workgroups fit a CU's 160 KiB beside their registers.
#include "common.h"
#include "internal_rule.h"
#include "pbc.h"
#include "../../include/mdno_internal.h"

#include <cmath>

namespace mdno {
namespace {

constexpr int kThreads = MDNO_IC_WORKGROUP;
constexpr int kLdsAtoms = MDNO_IC_LDS_ATOMS;
constexpr int kChunk = MDNO_IC_FEATURE_CHUNK;
constexpr int kHistRows = MDNO_IC_HIST_ROWS, kHistTable = MDNO_IC_HIST_TABLE, kHistCols = MDNO_IC_HIST_COLUMNS;
constexpr int kHistTile = 64;                              // the most columns of one workgroup's table
static_assert(kThreads == 256, "four waves per workgroup");
static_assert(MDNO_IC_MAX_GROUP_FRAMES * (long long)kChunk < (1ll << 31), "the (frame, item) walk of a workgroup is an int");
static_assert(MDNO_IC_MAX_BINS + 2 <= kHistTable, "one column of the widest histogram fits the LDS table");
static_assert(kHistCols % kHistTile == 0 && 3 * kHistCols * sizeof(double) <= 3072, "the ranges of a launch fit the kernel arguments");

typedef unsigned long long u64;

__device__ __forceinline__ double nan_d() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double clamp1(double c) { return c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c); }
// (dot3, cross3, bond and inside are internal_rule.h's: the backward kernel forms the same vectors from them)

// One item of one frame: r[0] (and r[1] for a dihedral outside radians mode).  `it` counts pairs, then triples, then quads.
__device__ __forceinline__ void ic_item(const float* x, int N, int it, const int* __restrict__ pairs, int P,
                                        const int* __restrict__ triples, int A, const int* __restrict__ quads,
                                        const PbcBox& box, bool radians, double r[2]) {
    r[0] = r[1] = nan_d();
    if (it < P) {
        const int i = pairs[2 * it], j = pairs[2 * it + 1];
        if (!(inside(i, N) && inside(j, N))) return;
        double v[3];
        bond(x, i, j, box, v);
        r[0] = sqrt(dot3(v, v));
    } else if (it < P + A) {
        const int t = it - P;
        const int i = triples[3 * t], j = triples[3 * t + 1], k = triples[3 * t + 2];
        if (!(inside(i, N) && inside(j, N) && inside(k, N))) return;
        double u[3], w[3];
        bond(x, j, i, box, u);
        bond(x, j, k, box, w);
        const double c = clamp1(dot3(u, w) / (sqrt(dot3(u, u)) * sqrt(dot3(w, w))));
        r[0] = radians ? acos(c) : c;
    } else {
        const int t = it - P - A;
        const int i = quads[4 * t], j = quads[4 * t + 1], k = quads[4 * t + 2], l = quads[4 * t + 3];
        if (!(inside(i, N) && inside(j, N) && inside(k, N) && inside(l, N))) return;
        double b1[3], b2[3], b3[3], n1[3], n2[3];
        bond(x, i, j, box, b1);
        bond(x, j, k, box, b2);
        bond(x, k, l, box, b3);
        cross3(b1, b2, n1);
        cross3(b2, b3, n2);
        const double xx = dot3(n1, n2);
        const double yy = sqrt(dot3(b2, b2)) * dot3(b1, n2);
        const double h = sqrt(xx * xx + yy * yy);
        if (radians) {
            if (h > 0.0) r[0] = atan2(yy, xx);
        } else {
            r[0] = clamp1(xx / h);
            r[1] = clamp1(yy / h);
        }
    }
}

// grid (ceil(F / G), ceil(items / kChunk))
template <bool kLds, class T>
__global__ __launch_bounds__(kThreads) void ic_features_kernel(const float* __restrict__ frames, long long F, int N,
                                                               const int* __restrict__ pairs, int P,
                                                               const int* __restrict__ triples, int A,
                                                               const int* __restrict__ quads, int Tq, PbcBox box, int radians,
                                                               int G, T* __restrict__ out) {
    __shared__ float stage[kLds ? 3 * kLdsAtoms : 1];
    const int tid = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * G;
    const int nf = (int)(F - f0 < (long long)G ? F - f0 : (long long)G);
    const int items = P + A + Tq, it0 = blockIdx.y * kChunk;
    const int ni = items - it0 < kChunk ? items - it0 : kChunk;
    const int per_quad = radians ? 1 : 2;
    const long long D = (long long)P + A + (long long)per_quad * Tq;
    const float* src = frames + (size_t)f0 * N * 3;
    if (kLds) {
        const int n = nf * N * 3;                                    // <= 3 kLdsAtoms: G N <= kLdsAtoms
        for (int e = tid; e < n; e += kThreads) stage[e] = src[e];
        __syncthreads();
    }
    const int total = nf * ni;
    for (int e = tid; e < total; e += kThreads) {
        const int fl = e / ni, it = it0 + (e - fl * ni);
        const float* x = kLds ? stage + fl * N * 3 : src + (size_t)fl * N * 3;
        double r[2];
        ic_item(x, N, it, pairs, P, triples, A, quads, box, radians != 0, r);
        T* o = out + (size_t)(f0 + fl) * (size_t)D;
        if (it < P + A) {
            o[it] = (T)r[0];
        } else {
            o += (size_t)(P + A) + (size_t)(it - P - A) * per_quad;
            o[0] = (T)r[0];
            if (!radians) o[1] = (T)r[1];
        }
    }
}

struct HistRange {
    double lo[kHistCols], hi[kHistCols], inv_w[kHistCols];
};

// grid (row blocks of kHistRows, column tiles of `tile` columns, groups); columns c_base .. c_base + ncols - 1 of every group
// of x [R, groups D], whose ranges are rg.*[0 .. ncols - 1]
template <class T>
__global__ __launch_bounds__(kThreads) void ic_hist_kernel(const T* __restrict__ x, long long R, int D, int c_base, int ncols,
                                                           int tile, int n_bins, HistRange rg, u64* __restrict__ counts,
                                                           u64* __restrict__ n_nan) {
    __shared__ unsigned tab[kHistTable];
    __shared__ unsigned nan_s[kHistTile];
    __shared__ double lo_s[kHistTile], hi_s[kHistTile], inv_s[kHistTile];
    const int tid = threadIdx.x;
    const int c_lo = blockIdx.y * tile;
    const int nc = ncols - c_lo < tile ? ncols - c_lo : tile;
    const int width = n_bins + 2;
    const long long r0 = (long long)blockIdx.x * kHistRows;
    const int nr = (int)(R - r0 < (long long)kHistRows ? R - r0 : (long long)kHistRows);
    for (int e = tid; e < nc * width; e += kThreads) tab[e] = 0;
    if (tid < nc) {
        nan_s[tid] = 0;
        lo_s[tid] = rg.lo[c_lo + tid];
        hi_s[tid] = rg.hi[c_lo + tid];
        inv_s[tid] = rg.inv_w[c_lo + tid];
    }
    __syncthreads();
    const size_t ld = (size_t)gridDim.z * D;                         // a row of x holds every group's D columns
    const size_t col0 = (size_t)blockIdx.z * D + (size_t)(c_base + c_lo);
    const T* xs = x + (size_t)r0 * ld + col0;
    const int total = nr * nc;                                       // <= kHistRows kHistTile
    for (int e = tid; e < total; e += kThreads) {
        const int r = e / nc, c = e - r * nc;
        const double v = (double)xs[(size_t)r * ld + c];
        if (v != v) {
            atomicAdd(&nan_s[c], 1u);
            continue;
        }
        int b;
        if (v < lo_s[c]) {
            b = 0;
        } else if (v >= hi_s[c]) {
            b = n_bins + 1;
        } else {
            long long q = (long long)((v - lo_s[c]) * inv_s[c]);
            if (q >= n_bins) q = n_bins - 1;
            b = (int)q + 1;
        }
        atomicAdd(&tab[c * width + b], 1u);
    }
    __syncthreads();
    for (int e = tid; e < nc * width; e += kThreads)
        if (tab[e]) atomicAdd(&counts[col0 * width + e], (u64)tab[e]);
    if (tid < nc && nan_s[tid]) atomicAdd(&n_nan[col0 + tid], (u64)nan_s[tid]);
}

template <bool kLds, class T>
void launch_features(dim3 grid, hipStream_t st, const float* frames, long long F, int N, const int* pairs, int P,
                     const int* triples, int A, const int* quads, int Tq, const PbcBox& box, int radians, int G, void* out) {
    hipLaunchKernelGGL((ic_features_kernel<kLds, T>), grid, dim3(kThreads), 0, st, frames, F, N, pairs, P, triples, A, quads, Tq,
                       box, radians, G, static_cast<T*>(out));
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" int mdnoic_features(const float* frames, int64_t F, int N, const int32_t* pairs, int P, const int32_t* triples, int A,
                               const int32_t* quads, int T, const double* box, int flags, int out_dtype, void* out, int form,
                               void* stream) {
    const char* who = "ic_features";
    MDNO_REQUIRE(F >= 0 && N >= 0 && P >= 0 && A >= 0 && T >= 0, MDNO_EINVAL, "%s: F=%lld N=%d P=%d A=%d T=%d", who, (long long)F, N,
                 P, A, T);
    MDNO_REQUIRE(out_dtype == MDNO_IC_F32 || out_dtype == MDNO_IC_F64, MDNO_EINVAL, "%s: out_dtype=%d is neither f32 (0) nor f64 (1)",
                 who, out_dtype);
    MDNO_REQUIRE(form == MDNO_IC_FORM_AUTO || form == MDNO_IC_FORM_LDS || form == MDNO_IC_FORM_GLOBAL, MDNO_EINVAL,
                 "%s: form=%d (0 auto, 1 lds, 2 global)", who, form);
    MDNO_REQUIRE((flags & ~MDNO_IC_RADIANS) == 0, MDNO_EINVAL, "%s: flags=%d holds an unknown bit", who, flags);
    MDNO_REQUIRE(form != MDNO_IC_FORM_LDS || N <= MDNO_IC_LDS_ATOMS, MDNO_EINVAL, "%s: the lds form holds N <= %d atoms, N=%d", who,
                 MDNO_IC_LDS_ATOMS, N);
    PbcBox b = {};
    if (box) MDNO_TRY(pbc_box_from(box, 0.0, &b, who));
    const int radians = (flags & MDNO_IC_RADIANS) ? 1 : 0;
    const long long D = (long long)P + A + (radians ? 1ll : 2ll) * T;
    const long long items = (long long)P + A + T;
    MDNO_REQUIRE(D <= 0x7fffffffll, MDNO_EINVAL, "%s: D=%lld columns exceed 2^31 - 1", who, D);
    if (F == 0 || D == 0) return MDNO_OK;
    MDNO_REQUIRE((pairs || P == 0) && (triples || A == 0) && (quads || T == 0), MDNO_EINVAL, "%s: null pointer (an index array)", who);
    MDNO_REQUIRE(frames || N == 0, MDNO_EINVAL, "%s: null pointer (frames)", who);
    MDNO_REQUIRE(out != nullptr, MDNO_EINVAL, "%s: null pointer (out)", who);
    const int G = MDNO_IC_FRAMES_PER_GROUP(N);
    const long long groups = ((long long)F + G - 1) / G;
    MDNO_REQUIRE(groups < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "%s: F=%lld frames exceed the launch grid", who, (long long)F);
    const long long chunks = (items + kChunk - 1) / kChunk;          // <= 2^31 / 8192: fits grid.y
    const dim3 grid((unsigned)groups, (unsigned)chunks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool lds = form == MDNO_IC_FORM_LDS || (form == MDNO_IC_FORM_AUTO && N <= MDNO_IC_LDS_ATOMS);
    const bool f64 = out_dtype == MDNO_IC_F64;
    if (lds && f64) launch_features<true, double>(grid, st, frames, (long long)F, N, pairs, P, triples, A, quads, T, b, radians, G, out);
    else if (lds) launch_features<true, float>(grid, st, frames, (long long)F, N, pairs, P, triples, A, quads, T, b, radians, G, out);
    else if (f64) launch_features<false, double>(grid, st, frames, (long long)F, N, pairs, P, triples, A, quads, T, b, radians, G, out);
    else launch_features<false, float>(grid, st, frames, (long long)F, N, pairs, P, triples, A, quads, T, b, radians, G, out);
    return check_launch(who);
}

extern "C" int mdnoic_column_histogram(const void* x, int64_t R, int D, int groups, int dtype, const double* lo,
                                       const double* hi, int shared_range, int n_bins, int64_t* counts, int64_t* n_nan,
                                       void* stream) {
    const char* who = "ic_column_histogram";
    MDNO_REQUIRE(R >= 0 && D >= 0 && groups >= 0, MDNO_EINVAL, "%s: R=%lld D=%d groups=%d", who, (long long)R, D, groups);
    MDNO_REQUIRE((long long)D * groups <= 0x7fffffffll, MDNO_EINVAL, "%s: %d groups of D=%d columns exceed 2^31 - 1", who, groups, D);
    MDNO_REQUIRE(dtype == MDNO_IC_F32 || dtype == MDNO_IC_F64, MDNO_EINVAL, "%s: dtype=%d is neither f32 (0) nor f64 (1)", who, dtype);
    MDNO_REQUIRE(n_bins >= 1 && n_bins <= MDNO_IC_MAX_BINS, MDNO_EINVAL, "%s: n_bins=%d outside 1 .. %d", who, n_bins, MDNO_IC_MAX_BINS);
    if (D == 0 || groups == 0) return MDNO_OK;
    MDNO_REQUIRE(lo && hi, MDNO_EINVAL, "%s: null pointer (lo or hi)", who);
    const int n_ranges = shared_range ? 1 : D;
    for (int a = 0; a < n_ranges; ++a)
        MDNO_REQUIRE(std::isfinite(lo[a]) && std::isfinite(hi[a]) && hi[a] > lo[a] && std::isfinite(hi[a] - lo[a]) &&
                         std::isfinite((double)n_bins / (hi[a] - lo[a])),
                     MDNO_EINVAL, "%s: range [%g, %g) of column %d is not finite or is empty", who, lo[a], hi[a], a);
    MDNO_REQUIRE(counts && n_nan, MDNO_EINVAL, "%s: null pointer (counts or n_nan)", who);
    MDNO_REQUIRE(x || R == 0, MDNO_EINVAL, "%s: null pointer (x)", who);
    const long long blocks = ((long long)R + kHistRows - 1) / kHistRows;
    MDNO_REQUIRE(blocks < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "%s: R=%lld rows exceed the launch grid", who, (long long)R);
    MDNO_REQUIRE(groups <= 65535, MDNO_EUNSUPPORTED, "%s: groups=%d exceed the launch grid", who, groups);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int width = n_bins + 2;
    MDNO_HIP(hipMemsetAsync(counts, 0, (size_t)groups * D * width * sizeof(int64_t), st));
    MDNO_HIP(hipMemsetAsync(n_nan, 0, (size_t)groups * D * sizeof(int64_t), st));
    if (R == 0) return MDNO_OK;
    int tile = kHistTable / width;
    tile = tile < 1 ? 1 : (tile > kHistTile ? kHistTile : tile);
    for (int c_base = 0; c_base < D; c_base += kHistCols) {
        const int ncols = D - c_base < kHistCols ? D - c_base : kHistCols;
        HistRange rg;
        for (int c = 0; c < kHistCols; ++c) {
            const int a = shared_range ? 0 : (c < ncols ? c_base + c : c_base);
            rg.lo[c] = lo[a];
            rg.hi[c] = hi[a];
            rg.inv_w[c] = (double)n_bins / (hi[a] - lo[a]);
        }
        const dim3 grid((unsigned)blocks, (unsigned)((ncols + tile - 1) / tile), (unsigned)groups);
        if (dtype == MDNO_IC_F32)
            hipLaunchKernelGGL(ic_hist_kernel<float>, grid, dim3(kThreads), 0, st, static_cast<const float*>(x), (long long)R, D, c_base,
                               ncols, tile, n_bins, rg, reinterpret_cast<u64*>(counts), reinterpret_cast<u64*>(n_nan));
        else
            hipLaunchKernelGGL(ic_hist_kernel<double>, grid, dim3(kThreads), 0, st, static_cast<const double*>(x), (long long)R, D, c_base,
                               ncols, tile, n_bins, rg, reinterpret_cast<u64*>(counts), reinterpret_cast<u64*>(n_nan));
        MDNO_TRY(check_launch(who));
    }
    return MDNO_OK;
}
