// Contact statistics of a trajectory that lies in device memory (include/mdno_contacts.h states THE RULE):
// the reduction over TIME that the per-frame kernels (forecast.hip: contact maps; observe.hip: pair histograms) leave to the
// caller.  The pair arithmetic is pbc.h's dist2 of OpenPair / PbcPair, the one those kernels take the root of.
//
//   pair_stats_kernel     grid (tile pairs bi <= bj, members, blocks).  256 threads own a 64 x 64 tile of pairs: wave w
//                         holds the rows i0 + 16 w .. + 15, lane l the column j0 + l, so a thread carries 16 pairs of ONE
//                         column — count, sum r and sum s in registers — and a store instruction of a wave covers 64
//                         consecutive elements of one row.  The block's frames are walked in step order (one chain per
//                         pair: the bits do not depend on the grid); the 2 x 64 atoms of a frame lie in LDS, double
//                         buffered: frame f + 1 is loaded into registers before frame f is worked on and written to the
//                         other buffer after it, one barrier per frame.  x_j is read once per frame and thread (lanes 3
//                         dwords apart: no bank conflict), x_i is a broadcast.  The mirror tile goes through a padded
//                         LDS tile so that its stores run along rows too.  Steps are never split across workgroups.
//                         Without sum_r the root is not taken: s < s* (the header says why that is the same set).
//   contact_bits_kernel   grid (pair chunks, words, members).  A wave takes one pair at a time, lane l step 64 w + l, and
//                         __ballot gives the word; the workgroup's per-step counts are added up in LDS and go to
//                         per_frame with one integer atomic per step.  The 64 frames of a word are shared by every pair of
//                         every chunk: after the first touch the gathers are L2 hits.
//   contact_corr_kernel   one thread per (member, pair, lag), the lag fastest: the threads of a row read the same words
//                         (a broadcast), shift, AND and count.  The lags travel by value, kLagChunk per launch.
#include "common.h"
#include "pbc.h"
#include "../../include/mdno_contacts.h"

#include <cmath>

namespace mdno {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = MDNOCM_TILE;
constexpr int kRows = kTile / kWaves;              // rows of the tile one thread carries
constexpr int kPad = kTile + 1;                    // leading dimension of the mirror tile in LDS
constexpr int kPairChunk = MDNOCM_PAIR_CHUNK;
constexpr int kLagChunk = 256;
static_assert(kTile == 64 && kRows == 16, "a lane is a column of the tile, a wave 16 of its rows");

typedef unsigned long long u64;

// out[i0 + r, j0 + lane] for the thread's rows, then (off the diagonal) the mirror through `tile`
template <class T>
__device__ __forceinline__ void store_tile(const T (&v)[kRows], T* __restrict__ out, int N, int i0, int j0, bool mirror,
                                           T* tile) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = j0 + lane;
#pragma unroll
    for (int a = 0; a < kRows; ++a) {
        const int i = i0 + wave * kRows + a;
        if (i < N && j < N) out[(size_t)i * N + j] = v[a];
    }
    if (!mirror) return;
    __syncthreads();                               // (the tile may still be read by the previous output's mirror)
#pragma unroll
    for (int a = 0; a < kRows; ++a) tile[(wave * kRows + a) * kPad + lane] = v[a];
    __syncthreads();
    const int i = i0 + lane;
#pragma unroll
    for (int a = 0; a < kRows; ++a) {
        const int jl = wave * kRows + a;
        if (i < N && j0 + jl < N) out[(size_t)(j0 + jl) * N + i] = tile[lane * kPad + jl];
    }
}

// kR: sum_r is formed (and the root taken); kR2: sum_r2 is formed.  s_star: the smallest double whose root is >= threshold.
template <class Pair, bool kR, bool kR2>
__global__ __launch_bounds__(kThreads) void pair_stats_kernel(const float* __restrict__ frames, int S, int M, int N,
                                                              const Pair pair, double s_star, int block_len, int nt,
                                                              int* __restrict__ count, double* __restrict__ sum_r,
                                                              double* __restrict__ sum_r2) {
    __shared__ float stage[2][2 * kTile * 3];      // [buffer][tile i then tile j][atom][component]
    __shared__ double tile[kTile * kPad];
    int bi = 0, rest = blockIdx.x;                 // the bi-th row of the upper triangle holds nt - bi tiles
    while (rest >= nt - bi) {
        rest -= nt - bi;
        ++bi;
    }
    const int bj = bi + rest;
    const int m = blockIdx.y, blk = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = bi * kTile, j0 = bj * kTile;
    const int s0 = blk * block_len;
    const int nf = min(block_len, S - s0);
    // thread tid < 192 stages dword tid of tile i and of tile j; an atom past N is staged as zeros and never stored
    const bool stager = tid < kTile * 3;
    const int ai = i0 + tid / 3, aj = j0 + tid / 3;
    const bool li = stager && ai < N, lj = stager && aj < N;
    const size_t step = (size_t)M * N * 3;
    const float* base = frames + ((size_t)s0 * M + m) * (size_t)N * 3;
    float ri = 0.f, rj = 0.f;
    if (li) ri = base[(size_t)i0 * 3 + tid];
    if (lj) rj = base[(size_t)j0 * 3 + tid];
    if (stager) {
        stage[0][tid] = ri;
        stage[0][kTile * 3 + tid] = rj;
    }
    __syncthreads();
    int cnt[kRows];
    double ar[kRows], as[kRows];
#pragma unroll
    for (int a = 0; a < kRows; ++a) {
        cnt[a] = 0;
        ar[a] = 0.0;
        as[a] = 0.0;
    }
    for (int f = 0; f < nf; ++f) {
        const bool more = f + 1 < nf;
        if (more) {
            const float* nx = base + (size_t)(f + 1) * step;
            if (li) ri = nx[(size_t)i0 * 3 + tid];
            if (lj) rj = nx[(size_t)j0 * 3 + tid];
        }
        const float* xi = stage[f & 1] + (wave * kRows) * 3;
        const float* xj = stage[f & 1] + kTile * 3 + lane * 3;
        const float pj[3] = {xj[0], xj[1], xj[2]};
#pragma unroll
        for (int a = 0; a < kRows; ++a) {
            const double s = pair.dist2((double)xi[3 * a], (double)xi[3 * a + 1], (double)xi[3 * a + 2], pj);
            if (kR) {
                const double r = sqrt(s);
                cnt[a] += r < pair.cutoff ? 1 : 0;
                ar[a] = ar[a] + r;
            } else {
                cnt[a] += s < s_star ? 1 : 0;
            }
            if (kR2) as[a] = as[a] + s;
        }
        if (more && stager) {
            stage[(f + 1) & 1][tid] = ri;
            stage[(f + 1) & 1][kTile * 3 + tid] = rj;
        }
        __syncthreads();
    }
    const size_t map = ((size_t)blk * M + m) * (size_t)N * (size_t)N;
    const bool mirror = bi != bj;
    store_tile(cnt, count + map, N, i0, j0, mirror, reinterpret_cast<int*>(tile));
    if (kR) store_tile(ar, sum_r + map, N, i0, j0, mirror, tile);
    if (kR2) store_tile(as, sum_r2 + map, N, i0, j0, mirror, tile);
}

template <class Pair>
__global__ __launch_bounds__(kThreads) void contact_bits_kernel(const float* __restrict__ frames, int S, int M, int N,
                                                                const int* __restrict__ pairs,
                                                                const double* __restrict__ cut, int P, const Pair pair,
                                                                u64* __restrict__ bits, int* __restrict__ per_frame) {
    __shared__ int total[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = blockIdx.y, m = blockIdx.z;
    const int Wd = (S + 63) / 64;
    const int s = w * 64 + lane;
    const bool live = s < S;
    const float* x = frames + ((size_t)(live ? s : 0) * M + m) * (size_t)N * 3;
    const int p0 = blockIdx.x * kPairChunk;
    const int np = min(kPairChunk, P - p0);
    if (tid < 64) total[tid] = 0;
    __syncthreads();
    int mine = 0;
    for (int q = wave; q < np; q += kWaves) {
        const int p = p0 + q;
        const int i = pairs[2 * p], j = pairs[2 * p + 1];
        const double c = cut[p];
        bool in = false;
        if (live && (unsigned)i < (unsigned)N && (unsigned)j < (unsigned)N) {
            const float* pi = x + (size_t)i * 3;
            const double r = sqrt(pair.dist2((double)pi[0], (double)pi[1], (double)pi[2], x + (size_t)j * 3));
            in = r < c && r < pair.cutoff;
        }
        const u64 word = __ballot(in);
        mine += in ? 1 : 0;
        if (lane == 0) bits[((size_t)m * P + p) * Wd + w] = word;
    }
    if (per_frame == nullptr) return;
    if (mine) atomicAdd(&total[lane], mine);
    __syncthreads();
    if (tid < 64 && live && total[tid]) atomicAdd(&per_frame[(size_t)s * M + m], total[tid]);
}

struct LagChunk {
    int lag[kLagChunk];
};

__device__ __forceinline__ u64 low_bits(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }    // 0 <= n

// items = M P rows x nl lags of this launch; lags l_base .. l_base + nl - 1 of L
__global__ __launch_bounds__(kThreads) void contact_corr_kernel(const u64* __restrict__ bits, int S, long long rows, int L,
                                                                int l_base, int nl, LagChunk lags,
                                                                int* __restrict__ origins, int* __restrict__ both) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= rows * nl) return;
    const long long row = e / nl;
    const int l = (int)(e - row * nl);
    const int lag = lags.lag[l];
    const int Wd = (S + 63) / 64;
    const u64* wd = bits + (size_t)row * Wd;
    const int span = S - lag;                      // origins t = 0 .. span - 1, span >= 1
    const int q = lag >> 6, r = lag & 63;
    int n_or = 0, n_both = 0;
    const int kw = (span + 63) / 64;
    for (int k = 0; k < kw; ++k) {
        const u64 c = wd[k] & low_bits(span - 64 * k);
        const u64 lo = k + q < Wd ? wd[k + q] : 0ull;
        const u64 hi = (r != 0 && k + q + 1 < Wd) ? wd[k + q + 1] : 0ull;
        const u64 shifted = r == 0 ? lo : (lo >> r) | (hi << (64 - r));
        n_or += __popcll(c);
        n_both += __popcll(c & shifted);
    }
    const size_t o = (size_t)row * L + (size_t)(l_base + l);
    origins[o] = n_or;
    both[o] = n_both;
}

// the smallest double whose (correctly rounded) root is >= cut: sqrt(s) < cut  <=>  s < s_star, for every s (NaN: false)
double root_threshold(double cut) {
    double s = cut * cut;
    if (!std::isfinite(s)) return INFINITY;        // cut^2 overflows: the root of every finite s lies below cut, and Inf < Inf is false
    while (s > 0.0 && std::sqrt(s) >= cut) s = std::nextafter(s, 0.0);
    while (std::sqrt(s) < cut) s = std::nextafter(s, INFINITY);
    return s;
}

template <class Pair>
int launch_stats(const float* frames, int S, int M, int N, const Pair& pair, double s_star, int block_len, int nt, dim3 grid,
                 int32_t* count, double* sum_r, double* sum_r2, hipStream_t st) {
#define MDNOCM_STATS(R, R2)                                                                                              \
    hipLaunchKernelGGL((pair_stats_kernel<Pair, R, R2>), grid, dim3(kThreads), 0, st, frames, S, M, N, pair, s_star, block_len, \
                       nt, count, sum_r, sum_r2)
    if (sum_r && sum_r2) MDNOCM_STATS(true, true);
    else if (sum_r) MDNOCM_STATS(true, false);
    else if (sum_r2) MDNOCM_STATS(false, true);
    else MDNOCM_STATS(false, false);
#undef MDNOCM_STATS
    return check_launch("mdnocm_pair_statistics");
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" int mdnocm_pair_statistics(const float* frames, int S, int M, int N, double threshold, const double* box,
                                      int block_len, int32_t* count, double* sum_r, double* sum_r2, void* stream) {
    const char* who = "mdnocm_pair_statistics";
    MDNO_REQUIRE(S >= 0 && M >= 0 && N >= 0, MDNO_EINVAL, "%s: S=%d M=%d N=%d", who, S, M, N);
    MDNO_REQUIRE(block_len >= 1, MDNO_EINVAL, "%s: block_len=%d, expected >= 1", who, block_len);
    MDNO_REQUIRE(std::isfinite(threshold) && threshold > 0.0, MDNO_EINVAL, "%s: threshold %g is not a finite positive number", who,
                 threshold);
    const double s_star = root_threshold(threshold);
    PbcBox b{};
    if (box != nullptr) MDNO_TRY(pbc_box_from(box, threshold, &b, who));
    if (S == 0 || M == 0 || N == 0) return MDNO_OK;
    MDNO_REQUIRE(frames && count, MDNO_EINVAL, "%s: null pointer (frames or count)", who);
    const long long nt = ((long long)N + kTile - 1) / kTile;
    const long long tile_pairs = nt * (nt + 1) / 2;
    const int Bk = (int)(((long long)S + block_len - 1) / block_len);
    MDNO_REQUIRE(tile_pairs < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "%s: N=%d gives %lld pair tiles, the launch grid holds 2^31 - 1", who, N,
                 tile_pairs);
    MDNO_REQUIRE(M <= 65535 && Bk <= 65535, MDNO_EUNSUPPORTED, "%s: M=%d members or %d blocks exceed the launch grid (65535)", who, M, Bk);
    const dim3 grid((unsigned)tile_pairs, (unsigned)M, (unsigned)Bk);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (b.any()) return launch_stats(frames, S, M, N, PbcPair{threshold, b}, s_star, block_len, (int)nt, grid, count, sum_r, sum_r2, st);
    return launch_stats(frames, S, M, N, OpenPair{threshold}, s_star, block_len, (int)nt, grid, count, sum_r, sum_r2, st);
}

extern "C" int mdnocm_contact_bits(const float* frames, int S, int M, int N, const int32_t* pairs, const double* cut, int P,
                                   double cut_max, const double* box, uint64_t* bits, int32_t* per_frame, void* stream) {
    const char* who = "mdnocm_contact_bits";
    MDNO_REQUIRE(S >= 0 && M >= 0 && N >= 0 && P >= 0, MDNO_EINVAL, "%s: S=%d M=%d N=%d P=%d", who, S, M, N, P);
    MDNO_REQUIRE(std::isfinite(cut_max) && cut_max > 0.0, MDNO_EINVAL, "%s: cut_max %g is not a finite positive number", who, cut_max);
    PbcBox b{};
    if (box != nullptr) MDNO_TRY(pbc_box_from(box, cut_max, &b, who));
    if (S == 0 || M == 0 || P == 0) return MDNO_OK;
    MDNO_REQUIRE(pairs && cut && bits && (frames || N == 0), MDNO_EINVAL, "%s: null pointer", who);
    const int Wd = (S + 63) / 64;
    MDNO_REQUIRE(M <= 65535 && Wd <= 65535, MDNO_EUNSUPPORTED, "%s: M=%d members or %d words exceed the launch grid (65535)", who, M, Wd);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (per_frame) MDNO_HIP(hipMemsetAsync(per_frame, 0, (size_t)S * M * sizeof(int32_t), st));
    const dim3 grid((unsigned)((P + kPairChunk - 1) / kPairChunk), (unsigned)Wd, (unsigned)M);
    u64* out = reinterpret_cast<u64*>(bits);
    if (b.any())
        hipLaunchKernelGGL(contact_bits_kernel<PbcPair>, grid, dim3(kThreads), 0, st, frames, S, M, N, pairs, cut, P,
                           PbcPair{cut_max, b}, out, per_frame);
    else
        hipLaunchKernelGGL(contact_bits_kernel<OpenPair>, grid, dim3(kThreads), 0, st, frames, S, M, N, pairs, cut, P,
                           OpenPair{cut_max}, out, per_frame);
    return check_launch(who);
}

extern "C" int mdnocm_contact_correlation(const uint64_t* bits, int S, int M, int P, const int32_t* lags, int L,
                                          int32_t* origins, int32_t* both, void* stream) {
    const char* who = "mdnocm_contact_correlation";
    MDNO_REQUIRE(S >= 0 && M >= 0 && P >= 0 && L >= 0, MDNO_EINVAL, "%s: S=%d M=%d P=%d L=%d", who, S, M, P, L);
    MDNO_REQUIRE(L <= MDNOCM_MAX_LAGS, MDNO_EINVAL, "%s: %d lags, expected at most %d", who, L, MDNOCM_MAX_LAGS);
    MDNO_REQUIRE(lags || L == 0, MDNO_EINVAL, "%s: null pointer (lags)", who);
    if (S == 0 || M == 0 || P == 0 || L == 0) return MDNO_OK;
    for (int l = 0; l < L; ++l)
        MDNO_REQUIRE(lags[l] >= 0 && lags[l] < S, MDNO_EINVAL, "%s: lag %d is outside 0 .. %d (S=%d)", who, lags[l], S - 1, S);
    MDNO_REQUIRE(bits && origins && both, MDNO_EINVAL, "%s: null pointer", who);
    const long long rows = (long long)M * P;
    const long long groups = (rows * kLagChunk + kThreads - 1) / kThreads;
    MDNO_REQUIRE(groups < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "%s: M=%d x P=%d rows exceed the launch grid", who, M, P);
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int l_base = 0; l_base < L; l_base += kLagChunk) {
        const int nl = L - l_base < kLagChunk ? L - l_base : kLagChunk;
        LagChunk lc;
        for (int l = 0; l < kLagChunk; ++l) lc.lag[l] = l < nl ? lags[l_base + l] : 0;
        const long long items = rows * nl;
        hipLaunchKernelGGL(contact_corr_kernel, dim3((unsigned)((items + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                           reinterpret_cast<const u64*>(bits), S, rows, L, l_base, nl, lc, origins, both);
        MDNO_TRY(check_launch(who));
    }
    return MDNO_OK;
}
