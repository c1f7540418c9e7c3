// The solvent-accessible surface of frames that lie in device memory (include/mdno_surface.h states THE RULE; DESIGN.md
// §4.24): per atom the points of a sphere table that no neighbour's expanded sphere covers.  The pair arithmetic is pbc.h's
// (the differences and the shift of dist2_open / dist2_pbc, the summation order and the root of the radius graph's test).
//
// ONE WAVE PER ATOM, in both forms.  The lanes stride over j; the neighbours of a 64-atom step are compacted by the
// wave-wide ballot into the wave's LDS chunk (d and R_j^2, kChunk entries); when the next step would not fit, the wave tests
// its points against the chunk and empties it, so the number of neighbours has no cap.  Lane l owns the points l, l + 64,
// .. (at most 16) with one buried bit each in a register: the test walks the owned points outermost, with q = R_i U[p] in
// registers, and the chunk innermost, every entry a broadcast read.  A buried point is skipped, a step of points whose
// lanes are all buried ends early, and a wave whose points are all buried skips the rest of its pairs.  "Buried" is an OR,
// so none of this changes a count.  The count is a population count and a wave sum (reduce.h); lane 0 stores it.
//
//   exposed_staged_kernel   grid (frames, slices).  The frame and R lie in LDS as fp64 (32 N bytes, N <= 2,048) beside the
//                           point table (24 P bytes) and the four chunks; after ONE barrier the waves run independently,
//                           wave w of slice y taking the atoms 4 y + w, + 4 slices, ..
//   exposed_tiled_kernel    grid (frames, slices), any N.  The four waves of a workgroup take four atoms at a time and walk
//                           the frame in 256-atom tiles staged in LDS (two barriers per tile, uniform trip counts: a wave
//                           without an atom, or done, still arrives).
// `slices` is the host's choice (enough workgroups for few frames); no count depends on it.
#include "pbc.h"
#include "reduce.h"
#include "../../include/mdno_surface.h"

#include <atomic>
#include <cmath>

namespace mdno {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kStagedAtoms = MDNOSA_STAGED_ATOMS;
constexpr int kTile = MDNOSA_TILE;
constexpr int kChunk = MDNOSA_CHUNK;
constexpr int kMaxPoints = MDNOSA_MAX_POINTS;
constexpr int kOwned = kMaxPoints / 64;            // points per lane at most
constexpr int kTargetGroups = 2048;                // workgroups the host aims for when it splits a frame into slices
static_assert(kChunk == 64, "one 64-atom step always fits into an empty chunk");
static_assert(kTile == kThreads, "thread t stages atom t of a tile");
static_assert(kOwned <= 32, "the buried bits of a lane are one unsigned");

typedef unsigned long long u64;

// d_a of the rule: the difference dist2_open / dist2_pbc square
struct OpenDiff {
    __device__ __forceinline__ double operator()(double xi, double xj, int) const { return xj - xi; }
};
struct PbcDiff {
    PbcBox box;
    __device__ __forceinline__ double operator()(double xi, double xj, int a) const {
        return (xj - xi) - pbc_shift(xi, xj, box.L[a], box.inv[a]);
    }
};

// A wave's atom.  Everything is wave-uniform except `buried` and `own`.
struct Atom {
    double x, y, z, R;
    int index;              // the atom, or -1: no pair is looked at (no atom, or a non-finite one)
    int fill;               // neighbours waiting in the chunk
    bool done;              // every point is buried
    unsigned own;           // bit k: the lane owns point lane + 64 k (it is < P)
    unsigned buried;        // bit k: that point is buried
};

__device__ __forceinline__ unsigned owned_points(int lane, int P) {
    const int n = lane < P ? (P - lane + 63) / 64 : 0;          // 0 .. 16
    return n >= 32 ? ~0u : ((1u << n) - 1u);
}

__device__ __forceinline__ Atom begin_atom(int index, bool finite, double x, double y, double z, double R, int lane, int P) {
    Atom a;
    a.x = x, a.y = y, a.z = z, a.R = R;
    a.index = finite ? index : -1;
    a.fill = 0;
    a.done = !finite;
    a.own = owned_points(lane, P);
    a.buried = 0u;
    return a;
}

// tests the wave's points against the a.fill entries of its chunk ([dx, dy, dz, R_j^2] each) and empties it
__device__ __forceinline__ void bury(Atom& a, const double* chunk, const double* U, int P, int lane) {
    __builtin_amdgcn_wave_barrier();               // the entries were written by other lanes of this wave
    const int n = a.fill;
    a.fill = 0;
    if (n == 0 || a.done) return;
    for (int k = 0; k < kOwned && 64 * k < P; ++k) {
        const int p = lane + 64 * k;
        bool open = ((a.own & ~a.buried) >> k) & 1u;
        if (!__any(open)) continue;
        const int pr = open ? p : 0;               // (a lane without the point computes on row 0 and drops the result)
        const double qx = a.R * U[3 * pr], qy = a.R * U[3 * pr + 1], qz = a.R * U[3 * pr + 2];
        for (int e = 0; e < n; ++e) {
            const double* c = static_cast<const double*>(__builtin_assume_aligned(chunk + 4 * e, 16));
            const double ex = qx - c[0], ey = qy - c[1], ez = qz - c[2];
            const double t = (ex * ex + ey * ey) + ez * ez;
            if (open && t < c[3]) {
                open = false;
                a.buried |= 1u << k;
            }
            if (!__any(open)) break;
        }
    }
    a.done = !__any((a.own & ~a.buried) != 0u);
    __builtin_amdgcn_wave_barrier();               // the chunk is rewritten next
}

// atoms j_base .. j_base + count - 1, whose coordinates xs [count, 3] and radii Rs [count] lie in LDS as fp64
template <class Diff>
__device__ __forceinline__ void scan(Atom& a, const Diff& diff, const double* xs, const double* Rs, int j_base, int count,
                                     double* chunk, const double* U, int P, int lane) {
    for (int j0 = 0; j0 < count; j0 += 64) {
        if (a.done) return;
        const int j = j0 + lane;
        bool nb = false;
        double dx = 0.0, dy = 0.0, dz = 0.0, rj = 0.0;
        if (j < count && j_base + j != a.index) {
            dx = diff(a.x, xs[3 * j], 0);
            dy = diff(a.y, xs[3 * j + 1], 1);
            dz = diff(a.z, xs[3 * j + 2], 2);
            rj = Rs[j];
            const double s = (dx * dx + dy * dy) + dz * dz;
            nb = sqrt(s) < a.R + rj;               // false for a NaN or an Inf
        }
        const u64 mask = __ballot(nb);
        const int n = __popcll(mask);
        if (n == 0) continue;
        if (a.fill + n > kChunk) {
            bury(a, chunk, U, P, lane);
            if (a.done) return;
        }
        if (nb) {
            double* c = chunk + 4 * (a.fill + __popcll(mask & ((1ull << lane) - 1ull)));      // slot < kChunk
            c[0] = dx, c[1] = dy, c[2] = dz, c[3] = rj * rj;
        }
        a.fill += n;
    }
}

// the rest of the chunk, then the count; `live`: the wave has an atom (finite or not)
__device__ __forceinline__ void finish_atom(Atom& a, bool live, bool finite, const double* chunk, const double* U, int P, int lane,
                                            int* __restrict__ out) {
    if (!live) return;
    if (finite) bury(a, chunk, U, P, lane);
    const int n = wave_reduce_add((int)__popc(a.own & ~a.buried));
    if (lane == 0) *out = finite ? n : -1;
}

__device__ __forceinline__ bool finite3(double x, double y, double z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

// dynamic LDS (fp64): chunks [kWaves, kChunk, 4] | U [P, 3] | x [N, 3] | R [N]
template <class Diff>
__global__ __launch_bounds__(kThreads) void exposed_staged_kernel(const float* __restrict__ frames, int N,
                                                                  const double* __restrict__ R, const double* __restrict__ U,
                                                                  int P, const Diff diff, int* __restrict__ counts) {
    extern __shared__ __align__(16) double lds[];
    double* chunk = lds;                           // (first: 16-byte aligned entries, read as two 16-byte words)
    double* Us = chunk + kWaves * kChunk * 4;
    double* xs = Us + 3 * P;
    double* Rs = xs + 3 * (size_t)N;
    const long long f = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* X = frames + (size_t)f * N * 3;
    for (int k = tid; k < 3 * P; k += kThreads) Us[k] = U[k];
    for (int k = tid; k < 3 * N; k += kThreads) xs[k] = (double)X[k];
    for (int k = tid; k < N; k += kThreads) Rs[k] = R[k];
    __syncthreads();
    chunk += wave * kChunk * 4;
    for (int i = blockIdx.y * kWaves + wave; i < N; i += gridDim.y * kWaves) {
        const double x = xs[3 * i], y = xs[3 * i + 1], z = xs[3 * i + 2];
        const bool finite = finite3(x, y, z);
        Atom a = begin_atom(i, finite, x, y, z, Rs[i], lane, P);
        scan(a, diff, xs, Rs, 0, N, chunk, Us, P, lane);
        finish_atom(a, true, finite, chunk, Us, P, lane, counts + (size_t)f * N + i);
    }
}

// dynamic LDS (fp64): chunks [kWaves, kChunk, 4] | U [P, 3] | x [kTile, 3] | R [kTile]
template <class Diff>
__global__ __launch_bounds__(kThreads) void exposed_tiled_kernel(const float* __restrict__ frames, int N,
                                                                 const double* __restrict__ R, const double* __restrict__ U,
                                                                 int P, const Diff diff, int* __restrict__ counts) {
    extern __shared__ __align__(16) double lds[];
    double* chunk = lds;
    double* Us = chunk + kWaves * kChunk * 4;
    double* xs = Us + 3 * P;
    double* Rs = xs + 3 * kTile;
    const long long f = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* X = frames + (size_t)f * N * 3;
    for (int k = tid; k < 3 * P; k += kThreads) Us[k] = U[k];
    chunk += wave * kChunk * 4;
    for (int g = blockIdx.y * kWaves; g < N; g += gridDim.y * kWaves) {          // the same trips for every wave
        const int i = g + wave;
        const bool live = i < N;
        double x = 0.0, y = 0.0, z = 0.0, Ri = 0.0;
        if (live) x = X[3 * (size_t)i], y = X[3 * (size_t)i + 1], z = X[3 * (size_t)i + 2], Ri = R[i];
        const bool finite = live && finite3(x, y, z);
        Atom a = begin_atom(i, finite, x, y, z, Ri, lane, P);
        for (int j0 = 0; j0 < N; j0 += kTile) {
            const int nj = min(kTile, N - j0);
            __syncthreads();                       // the previous tile was read by every wave (first: nothing to wait for)
            if (tid < nj) {
                const float* pj = X + 3 * (size_t)(j0 + tid);
                xs[3 * tid] = (double)pj[0], xs[3 * tid + 1] = (double)pj[1], xs[3 * tid + 2] = (double)pj[2];
                Rs[tid] = R[j0 + tid];
            }
            __syncthreads();                       // (the first one also publishes U)
            scan(a, diff, xs, Rs, j0, nj, chunk, Us, P, lane);
        }
        finish_atom(a, live, finite, chunk, Us, P, lane, counts + (size_t)f * N + (live ? i : 0));
    }
}

bool form_ok(int form) { return form >= MDNO_FORECAST_AUTO && form <= MDNO_FORECAST_TILED; }

bool use_staged_form(int N, int form) { return form == MDNO_FORECAST_LDS || (form == MDNO_FORECAST_AUTO && N <= kStagedAtoms); }

size_t lds_bytes(int atoms, int P) { return ((size_t)3 * P + (size_t)kWaves * kChunk * 4 + (size_t)4 * atoms) * sizeof(double); }

constexpr int kMaxLdsBytes = (3 * kMaxPoints + kWaves * kChunk * 4 + 4 * kStagedAtoms) * (int)sizeof(double);      // 96 KiB
static_assert(kMaxLdsBytes <= 160 * 1024, "a workgroup's LDS");

template <class Diff>
int exposed_impl(const float* frames, int64_t F, int N, const double* R, const double* U, int P, const Diff& diff, int32_t* counts,
                 bool staged, hipStream_t st) {
    // enough workgroups for few frames: a frame is split into slices of its atoms (four atoms, one per wave, at least)
    const long long groups_of_four = ((long long)N + kWaves - 1) / kWaves;
    long long slices = (kTargetGroups + F - 1) / F;
    slices = slices < 1 ? 1 : (slices > groups_of_four ? groups_of_four : slices);
    slices = slices > 65535 ? 65535 : slices;
    const dim3 grid((unsigned)F, (unsigned)slices);
    if (staged) {
        // (a frame above 64 KiB of LDS needs the kernel's dynamic-LDS bound raised: once per device)
        static std::atomic<unsigned long long> raised{0};
        MDNO_TRY(raise_dynamic_lds(reinterpret_cast<const void*>(&exposed_staged_kernel<Diff>), kMaxLdsBytes, raised));
        hipLaunchKernelGGL(exposed_staged_kernel<Diff>, grid, dim3(kThreads), lds_bytes(N, P), st, frames, N, R, U, P, diff, counts);
    } else {
        hipLaunchKernelGGL(exposed_tiled_kernel<Diff>, grid, dim3(kThreads), lds_bytes(kTile, P), st, frames, N, R, U, P, diff, counts);
    }
    return check_launch("mdnosa_exposed_points");
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" size_t mdnosa_workspace_bytes(int64_t F, int N, int P, int form) {
    (void)F, (void)N, (void)P, (void)form;
    return 0;      // every count is stored once by the wave that owns its atom
}

extern "C" int mdnosa_exposed_points(const float* frames, int64_t F, int N, const double* R, const double* U, int P,
                                     const double* box, double reach, int32_t* counts, int form, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    const char* who = "mdnosa_exposed_points";
    MDNO_REQUIRE(F >= 0 && N >= 0, MDNO_EINVAL, "%s: F=%lld N=%d", who, (long long)F, N);
    MDNO_REQUIRE(form_ok(form), MDNO_EINVAL, "%s: form=%d", who, form);
    MDNO_REQUIRE(P >= 1 && P <= kMaxPoints, MDNO_EINVAL, "%s: P=%d points is outside 1 .. %d", who, P, kMaxPoints);
    MDNO_REQUIRE(std::isfinite(reach) && reach > 0.0, MDNO_EINVAL, "%s: reach %g is not a finite positive number", who, reach);
    PbcBox b{};
    if (box != nullptr) MDNO_TRY(pbc_box_from(box, reach, &b, who));
    const size_t need = mdnosa_workspace_bytes(F, N, P, form);
    MDNO_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), MDNO_EINVAL, "%s: workspace %zu < %zu", who, workspace_bytes,
                 need);
    if (F == 0) return MDNO_OK;
    MDNO_REQUIRE(N == 0 || (frames && R && counts), MDNO_EINVAL, "%s: null pointer (frames, R or counts)", who);
    MDNO_REQUIRE(U, MDNO_EINVAL, "%s: null pointer (U)", who);
    const bool staged = use_staged_form(N, form);
    MDNO_REQUIRE(!staged || N <= kStagedAtoms, MDNO_EUNSUPPORTED, "%s: the staged form holds at most %d atoms (N=%d)", who,
                 kStagedAtoms, N);
    MDNO_REQUIRE(F < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "%s: F = %lld exceeds the launch grid", who, (long long)F);
    if (N == 0) return MDNO_OK;        // no atom, no count
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (b.any()) return exposed_impl(frames, F, N, R, U, P, PbcDiff{b}, counts, staged, st);
    return exposed_impl(frames, F, N, R, U, P, OpenDiff{}, counts, staged, st);
}
