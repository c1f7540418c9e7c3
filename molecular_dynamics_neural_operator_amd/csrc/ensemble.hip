// Verification of an ensemble forecast against the truth on the device (include/mdno_ensemble.h states THE RULE and the
// order of the sums): per step the sums behind the error of the ensemble mean, the spread and the CRPS,
// and the rank histogram (forecast.py: EnsembleScore).
//
// A sample is one (step, atom, component); the members' values of a sample lie M floats apart at stride 3 N in the
// trajectory layout, the samples of one member contiguously: every member's row of a tile is a coalesced read.  A workgroup
// owns MDNO_ENS_SAMPLE_TILE = 256 consecutive samples of one step and thread k contributes sample k's four terms to
// block_reduce_add, so both forms add the same values in the same order:
//   registers (M <= 64)   thread k loads the M values of sample k into VGPRs, sorts them with an unrolled network and
//                         walks the sorted values.
//   LDS (M <= 1024)       the workgroup stages [M, T] values (T columns, a power of two with M * T * 4 <= 64 KiB), its
//                         256 / T threads per column share each column's network, the column's first thread walks the sorted
//                         values and leaves the four terms in LDS at the sample's place in the tile; 256 / T such passes.
// THE NETWORK is the bitonic sorter written with every comparator pointing the same way (lower index <- smaller value): a
// "flip" (i against i ^ (k - 1)) and half-cleaners (i against i + d, d = k / 4 .. 1) per block size k = 2 .. P, P the power
// of two >= M.  Padding is by COUNT, not by value: the P - M absent wires are thought of as +infinity above the real ones,
// such a wire never moves under same-way comparators, so every comparator that touches a wire >= M is simply skipped —
// no sentinel enters the data (3e38 is a legal coordinate).
// The integer outputs: a u32 histogram of the ranks in LDS per workgroup, its non-zero bins added to the zeroed row with
// integer atomics (as dynamics.hip's), the two counters reduced over the workgroup and added likewise.
#include "common.h"
#include "reduce.h"
#include "../../include/mdno_ensemble.h"

#include <atomic>

namespace mdno {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = MDNO_ENS_SAMPLE_TILE;
constexpr int kMaxMembers = MDNO_ENS_MAX_MEMBERS;
constexpr int kRegMembers = MDNO_ENS_MAX_REGISTER_MEMBERS;
constexpr int kStageBytes = 64 * 1024;     // the LDS form's [M, T] tile: with the terms and the histogram < 80 KiB, two workgroups per CU
static_assert(kTile == kThreads, "thread k of a workgroup holds sample k of its tile");

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// lower <- the smaller (fp32 compare: equal values, -0 and +0 among them, stay where they are)
__device__ __forceinline__ void compare_exchange(float& lo, float& hi) {
    const bool swap = hi < lo;
    const float a = swap ? hi : lo, b = swap ? lo : hi;
    lo = a;
    hi = b;
}

// The walk over the sorted values x_(0) .. x_(M-1) of one sample, in ascending j: first() for every j, then mean(), then
// second() for every j, then finish().
struct Sample {
    double y, m_count;
    float yf;
    int M;
    double sum = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0, mu = 0.0;
    int r = 0;
    bool tie = false, ok;
    __device__ __forceinline__ Sample(float y_, int M_) : y((double)y_), m_count((double)M_), yf(y_), M(M_), ok(finite_f(y_)) {}
    __device__ __forceinline__ void first(int j, float x) {
        ok = ok && finite_f(x);
        const double d = (double)x - y;
        sum += d;
        q2 += fabs(d);
        q3 += (double)(2 * j - M + 1) * d;
        r += x < yf ? 1 : 0;
        tie = tie || x == yf;
    }
    __device__ __forceinline__ void mean() { mu = sum / m_count; }
    __device__ __forceinline__ void second(float x) {
        const double c = ((double)x - y) - mu;
        q1 += c * c;
    }
    // the four terms of the sample (NaN each where it is invalid); cnt += (invalid, tie); the rank into the LDS histogram
    __device__ __forceinline__ void finish(double (&q)[4], int (&cnt)[2], unsigned int* hist) const {
        if (ok) {
            q[0] = mu * mu;
            q[1] = M >= 2 ? q1 / (double)(M - 1) : 0.0;
            q[2] = q2;
            q[3] = q3;
            cnt[1] += tie ? 1 : 0;
            atomicAdd(hist + r, 1u);
        } else {
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            q[0] = q[1] = q[2] = q[3] = nan;
            cnt[0] += 1;
        }
    }
};

// what both forms end with: the threads' terms added in the fixed order, one partial per sum; the counters and the
// histogram's non-zero bins added to the step's zeroed rows
__device__ __forceinline__ void tile_epilogue(double (&q)[4], int (&cnt)[2], const unsigned int* hist, int M, int s, double* slots,
                                              int* islots, double* __restrict__ part, unsigned long long* __restrict__ rank_hist,
                                              unsigned long long* __restrict__ n_invalid, unsigned long long* __restrict__ n_ties) {
    block_reduce_add<kWaves>(q, slots);        // (starts and ends with a barrier: the histogram is complete after it)
    block_reduce_add<kWaves>(cnt, islots);
    const int tid = threadIdx.x;
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) part[(size_t)blockIdx.x * 4 + k] = q[k];
        if (cnt[0]) atomicAdd(n_invalid + s, (unsigned long long)cnt[0]);
        if (cnt[1]) atomicAdd(n_ties + s, (unsigned long long)cnt[1]);
    }
    unsigned long long* row = rank_hist + (size_t)s * (M + 1);
    for (int b = tid; b <= M; b += kThreads) {
        if (hist[b]) atomicAdd(row + b, (unsigned long long)hist[b]);
    }
}

// ---------------------------------------------------------------------------------------------- registers
// grid S * tiles; dynamic LDS: the histogram u32 [M + 1].  P: the power of two >= M (M <= P <= 64).
template <int P>
__global__ __launch_bounds__(kThreads) void ensemble_registers_kernel(const float* __restrict__ frames, const float* __restrict__ truth,
                                                                      int M, long long n, int tiles, double* __restrict__ part,
                                                                      unsigned long long* __restrict__ rank_hist,
                                                                      unsigned long long* __restrict__ n_invalid,
                                                                      unsigned long long* __restrict__ n_ties) {
    extern __shared__ unsigned int hist[];
    __shared__ double slots[kWaves * 4];
    __shared__ int islots[kWaves * 2];
    const int tid = threadIdx.x;
    const int s = blockIdx.x / tiles, tile = blockIdx.x - s * tiles;
    for (int b = tid; b <= M; b += kThreads) hist[b] = 0u;
    __syncthreads();
    const long long e = (long long)tile * kTile + tid;
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    int cnt[2] = {0, 0};
    if (e < n) {
        const float* col = frames + (size_t)s * M * n + e;
        float v[P];
#pragma unroll
        for (int m = 0; m < P; ++m) v[m] = m < M ? col[(size_t)m * n] : 0.f;
        Sample sm(truth[(size_t)s * n + e], M);
#pragma unroll
        for (int k = 2; k <= P; k <<= 1) {
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int j = i ^ (k - 1);
                if (i < j && j < M) compare_exchange(v[i], v[j]);
            }
#pragma unroll
            for (int d = k >> 2; d >= 1; d >>= 1) {
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    const int j = i ^ d;
                    if (i < j && j < M) compare_exchange(v[i], v[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < P; ++j) {
            if (j < M) sm.first(j, v[j]);
        }
        sm.mean();
#pragma unroll
        for (int j = 0; j < P; ++j) {
            if (j < M) sm.second(v[j]);
        }
        sm.finish(q, cnt, hist);
    }
    tile_epilogue(q, cnt, hist, M, s, slots, islots, part, rank_hist, n_invalid, n_ties);
}

// ---------------------------------------------------------------------------------------------- LDS
// grid S * tiles; dynamic LDS: the staged values f32 [M, T], then the histogram u32 [M + 1].  P = 1 << log_p >= M,
// T = 1 << log_t columns per pass.
__global__ __launch_bounds__(kThreads) void ensemble_lds_kernel(const float* __restrict__ frames, const float* __restrict__ truth, int M,
                                                                int log_p, int log_t, long long n, int tiles,
                                                                double* __restrict__ part, unsigned long long* __restrict__ rank_hist,
                                                                unsigned long long* __restrict__ n_invalid,
                                                                unsigned long long* __restrict__ n_ties) {
    extern __shared__ float staged[];
    __shared__ double terms[4 * kTile];
    __shared__ double slots[kWaves * 4];
    __shared__ int islots[kWaves * 2];
    const int T = 1 << log_t, P = 1 << log_p;
    unsigned int* hist = reinterpret_cast<unsigned int*>(staged + (size_t)M * T);
    const int tid = threadIdx.x;
    const int s = blockIdx.x / tiles, tile = blockIdx.x - s * tiles;
    for (int b = tid; b <= M; b += kThreads) hist[b] = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) terms[k * kTile + tid] = 0.0;
    const int col = tid & (T - 1), g = tid >> log_t, G = kThreads >> log_t;      // G threads share a column's comparators
    const float* F = frames + (size_t)s * M * n;
    int cnt[2] = {0, 0};
    for (int pass = 0; pass < (kTile >> log_t); ++pass) {
        const long long e0 = (long long)tile * kTile + (long long)pass * T;
        if (e0 >= n) break;                    // (the same for every thread)
        __syncthreads();                       // the last pass's walk is over; the first pass: the zeroing above
        for (int idx = tid; idx < M * T; idx += kThreads) {
            const int m = idx >> log_t, c = idx & (T - 1);
            staged[idx] = e0 + c < n ? F[(size_t)m * n + e0 + c] : 0.f;
        }
        __syncthreads();
        for (int lk = 1; lk <= log_p; ++lk) {
            const int k = 1 << lk, half = k >> 1;
            for (int c = g; c < (P >> 1); c += G) {
                const int i = ((c >> (lk - 1)) << lk) + (c & (half - 1)), j = i ^ (k - 1);
                if (j < M) compare_exchange(staged[i * T + col], staged[j * T + col]);
            }
            __syncthreads();
            for (int ld = lk - 2; ld >= 0; --ld) {
                const int d = 1 << ld;
                for (int c = g; c < (P >> 1); c += G) {
                    const int i = ((c >> ld) << (ld + 1)) + (c & (d - 1)), j = i + d;
                    if (j < M) compare_exchange(staged[i * T + col], staged[j * T + col]);
                }
                __syncthreads();
            }
        }
        if (g == 0 && e0 + col < n) {
            Sample sm(truth[(size_t)s * n + e0 + col], M);
            for (int j = 0; j < M; ++j) sm.first(j, staged[j * T + col]);
            sm.mean();
            for (int j = 0; j < M; ++j) sm.second(staged[j * T + col]);
            double q[4];
            sm.finish(q, cnt, hist);
#pragma unroll
            for (int k = 0; k < 4; ++k) terms[k * kTile + pass * T + col] = q[k];
        }
    }
    __syncthreads();
    double q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = terms[k * kTile + tid];
    tile_epilogue(q, cnt, hist, M, s, slots, islots, part, rank_hist, n_invalid, n_ties);
}

// one thread per (s, c): sums[s, c] = the step's partials added in ascending tile order
__global__ __launch_bounds__(kThreads) void ensemble_finish_kernel(const double* __restrict__ part, long long count, int tiles,
                                                                   double* __restrict__ sums) {
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= count) return;
    const long long s = id >> 2;
    const int c = (int)(id & 3);
    const double* p = part + (size_t)s * tiles * 4 + c;
    double acc = 0.0;
    for (int t = 0; t < tiles; ++t) acc += p[(size_t)t * 4];
    sums[id] = acc;
}

long long tiles_of(int N) { return (3ll * N + kTile - 1) / kTile; }

int log2_ceil(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// columns per pass of the LDS form: the largest power of two <= the tile with M * T * 4 <= kStageBytes (M = 1024: 16)
int log_columns(int M) {
    int l = log2_ceil(kTile);
    while (((size_t)M << l) * sizeof(float) > (size_t)kStageBytes) --l;
    return l;
}

template <int P>
void launch_registers(const float* frames, const float* truth, int M, long long n, int tiles, unsigned blocks, double* part,
                      unsigned long long* rank_hist, unsigned long long* n_invalid, unsigned long long* n_ties, hipStream_t st) {
    hipLaunchKernelGGL(ensemble_registers_kernel<P>, dim3(blocks), dim3(kThreads), (size_t)(M + 1) * 4, st, frames, truth, M, n, tiles,
                       part, rank_hist, n_invalid, n_ties);
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" size_t mdnoens_score_workspace_bytes(int S, int M, int N) {
    if (S <= 0 || M < 0 || N < 0) return 0;
    const long long tiles = tiles_of(N);
    Carver c(nullptr);
    c.take<double>((size_t)S * (size_t)(tiles > 0 ? tiles : 1) * 4);
    return c.used();
}

extern "C" int mdnoens_score(const float* frames, const float* truth, int S, int M, int N, double* sums, int64_t* rank_hist,
                             int64_t* n_invalid, int64_t* n_ties, int form, void* workspace, size_t workspace_bytes,
                             void* stream) {
    const char* who = "ensemble_score";
    MDNO_REQUIRE(S >= 0 && M >= 0 && N >= 0, MDNO_EINVAL, "%s: S=%d M=%d N=%d", who, S, M, N);
    MDNO_REQUIRE(form >= 0 && form <= 2, MDNO_EINVAL, "%s: form=%d is outside 0 .. 2", who, form);
    if (S == 0) return MDNO_OK;
    MDNO_REQUIRE(N == 0 || (M >= 1 && M <= kMaxMembers), MDNO_EINVAL, "%s: M=%d is outside 1 .. %d", who, M, kMaxMembers);
    MDNO_REQUIRE((frames && truth) || N == 0, MDNO_EINVAL, "%s: null pointer (frames or truth)", who);
    MDNO_REQUIRE(sums && rank_hist && n_invalid && n_ties, MDNO_EINVAL, "%s: null pointer (sums, rank_hist, n_invalid or n_ties)",
                 who);
    MDNO_REQUIRE(form != 1 || M <= kRegMembers, MDNO_EUNSUPPORTED, "%s: the register form holds at most %d members, M=%d", who,
                 kRegMembers, M);
    const long long tiles = tiles_of(N);
    MDNO_REQUIRE((long long)S * (tiles > 0 ? tiles : 1) < (1ll << 31) - 1, MDNO_EUNSUPPORTED,
                 "%s: S=%d steps of %lld tiles exceed the launch grid", who, S, tiles);
    const size_t need = mdnoens_score_workspace_bytes(S, M, N);
    MDNO_REQUIRE(workspace && workspace_bytes >= need, MDNO_EINVAL, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    MDNO_HIP(hipMemsetAsync(rank_hist, 0, (size_t)S * ((size_t)M + 1) * sizeof(int64_t), st));
    MDNO_HIP(hipMemsetAsync(n_invalid, 0, (size_t)S * sizeof(int64_t), st));
    MDNO_HIP(hipMemsetAsync(n_ties, 0, (size_t)S * sizeof(int64_t), st));
    Carver c(workspace);
    double* part = c.take<double>((size_t)S * (size_t)(tiles > 0 ? tiles : 1) * 4);
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(rank_hist);
    unsigned long long* inv = reinterpret_cast<unsigned long long*>(n_invalid);
    unsigned long long* ties = reinterpret_cast<unsigned long long*>(n_ties);
    if (N > 0) {
        const long long n = 3ll * N;
        const unsigned blocks = (unsigned)((long long)S * tiles);
        const int log_p = log2_ceil(M);
        if (form == 1 || (form == 0 && M <= kRegMembers)) {
            switch (log_p) {
                case 0: launch_registers<1>(frames, truth, M, n, (int)tiles, blocks, part, hist, inv, ties, st); break;
                case 1: launch_registers<2>(frames, truth, M, n, (int)tiles, blocks, part, hist, inv, ties, st); break;
                case 2: launch_registers<4>(frames, truth, M, n, (int)tiles, blocks, part, hist, inv, ties, st); break;
                case 3: launch_registers<8>(frames, truth, M, n, (int)tiles, blocks, part, hist, inv, ties, st); break;
                case 4: launch_registers<16>(frames, truth, M, n, (int)tiles, blocks, part, hist, inv, ties, st); break;
                case 5: launch_registers<32>(frames, truth, M, n, (int)tiles, blocks, part, hist, inv, ties, st); break;
                default: launch_registers<64>(frames, truth, M, n, (int)tiles, blocks, part, hist, inv, ties, st); break;
            }
        } else {
            static std::atomic<unsigned long long> raised{0};
            MDNO_TRY(raise_dynamic_lds(reinterpret_cast<const void*>(ensemble_lds_kernel), kStageBytes + (kMaxMembers + 1) * 4, raised));
            const int log_t = log_columns(M);
            const size_t lds = ((size_t)M << log_t) * sizeof(float) + (size_t)(M + 1) * 4;
            hipLaunchKernelGGL(ensemble_lds_kernel, dim3(blocks), dim3(kThreads), lds, st, frames, truth, M, log_p, log_t, n, (int)tiles,
                               part, hist, inv, ties);
        }
        MDNO_TRY(check_launch(who));
    }
    const long long count = (long long)S * 4;
    hipLaunchKernelGGL(ensemble_finish_kernel, dim3((unsigned)((count + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part, count,
                       (int)tiles, sums);
    return check_launch(who);
}
