// The adjoint of the internal coordinates (include/mdno_internal_grad.h states the rule, its evaluation order and the
// incidence table): g [F, D] with respect to the features -> grad [F, N, 3] with respect to the positions
// (forecast.py: internal_coordinates under autograd; training.py: StructureLoss).
//
//   icg_bwd_kernel<lds>  grid (frame groups, atom chunks).  A workgroup owns G = MDNO_IC_FRAMES_PER_GROUP(N) consecutive
//                        frames x C consecutive atoms and its threads walk (frame, atom) in strides of the workgroup, the
//                        atom fastest.  ONE thread owns one (frame, atom): it walks the atom's incidences (item, slot) in
//                        the table's order and adds each contribution to three fp64 accumulators — a gather: nothing is
//                        summed across threads, no atomics, the chain is the header's.  lds: the G frames are first copied
//                        into LDS as they lie in memory (the forward's image: consecutive lanes own consecutive atoms,
//                        12 bytes apart, 3 is odd: 32 distinct banks per lane group for the atom's own coordinates; the
//                        partners' are a gather whose addresses the caller chooses); otherwise the coordinates are gathered
//                        from global memory.  Both call icg_contribution, THE arithmetic: the bits cannot differ.
// fp64 RATE.  An incidence costs ~40 (pair) to ~150 (quad) fp64 operations, among them 2 to 9 divisions and square roots,
// against 6 to 12 LDS dwords and one table entry: the kernel is bound by the fp64 pipe and by the longest chain of a wave
// (the lanes of a wave own different atoms; a hub atom holds its wave), not by LDS or memory.  The chain is the contract:
// it is not split across lanes here (scripts/bench_internal_grad.py measures what the uneven chains cost).
#include "common.h"
#include "internal_rule.h"
#include "pbc.h"
#include "../../include/mdno_internal_grad.h"

namespace mdno {
namespace {

constexpr int kThreads = MDNO_IC_WORKGROUP;
constexpr int kLdsAtoms = MDNO_IC_LDS_ATOMS;
static_assert(kThreads == 256, "four waves per workgroup");
static_assert(MDNO_IC_MAX_GROUP_FRAMES * (long long)MDNO_IC_LDS_ATOMS < (1ll << 31), "the (frame, atom) walk of a workgroup is an int");
static_assert(4ll * MDNO_ICG_MAX_ITEMS == (1ll << 31), "an incidence item * 4 + slot is a non-negative int32");

// The contribution of item `it`, seen from position `slot` of its tuple, to atom `a` of the frame x: r[0 .. 2], or false
// where the entry is skipped (the tuple's slot does not name a, an index outside 0 .. N - 1, a zero incoming gradient,
// r == 0 of a distance).  grow = row g[f, :] of the frame; `it` < P + A + T and slot < 4 are the caller's.
template <class Tg>
__device__ __forceinline__ bool icg_contribution(const float* x, int N, int a, int it, int slot, const int* __restrict__ pairs, int P,
                                                 const int* __restrict__ triples, int A, const int* __restrict__ quads,
                                                 const PbcBox& box, const Tg* __restrict__ grow, double r[3]) {
    if (it < P) {
        if (slot >= 2) return false;
        const int i = pairs[2 * it], j = pairs[2 * it + 1];
        if ((slot == 0 ? i : j) != a) return false;
        if (!(inside(i, N) && inside(j, N))) return false;
        const double g = (double)grow[it];
        if (g == 0.0) return false;
        double v[3];
        bond(x, i, j, box, v);
        const double len = sqrt(dot3(v, v));
        if (len == 0.0) return false;
        const double s = g / len;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double t = s * v[c];
            r[c] = slot == 1 ? t : -t;
        }
        return true;
    }
    if (it < P + A) {
        if (slot >= 3) return false;
        const int t = it - P;
        const int i = triples[3 * t], j = triples[3 * t + 1], k = triples[3 * t + 2];
        if ((slot == 0 ? i : (slot == 1 ? j : k)) != a) return false;
        if (!(inside(i, N) && inside(j, N) && inside(k, N))) return false;
        const double g = (double)grow[it];
        if (g == 0.0) return false;
        double u[3], w[3];
        bond(x, j, i, box, u);
        bond(x, j, k, box, w);
        const double uu = dot3(u, u), ww = dot3(w, w);
        const double den = sqrt(uu) * sqrt(ww);
        const double cs = dot3(u, w) / den;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double di = (w[c] / den) - ((cs * u[c]) / uu);
            const double dk = (u[c] / den) - ((cs * w[c]) / ww);
            r[c] = slot == 0 ? g * di : (slot == 2 ? g * dk : -(g * (di + dk)));
        }
        return true;
    }
    const int t = it - P - A;
    const int i = quads[4 * t], j = quads[4 * t + 1], k = quads[4 * t + 2], l = quads[4 * t + 3];
    if ((slot == 0 ? i : (slot == 1 ? j : (slot == 2 ? k : l))) != a) return false;
    if (!(inside(i, N) && inside(j, N) && inside(k, N) && inside(l, N))) return false;
    const size_t col = (size_t)(P + A) + 2 * (size_t)t;
    const double gc = (double)grow[col], gs = (double)grow[col + 1];
    if (gc == 0.0 && gs == 0.0) return false;
    double b1[3], b2[3], b3[3], n1[3], n2[3];
    bond(x, i, j, box, b1);
    bond(x, j, k, box, b2);
    bond(x, k, l, box, b3);
    cross3(b1, b2, n1);
    cross3(b2, b3, n2);
    const double bb = dot3(b2, b2), lb = sqrt(bb);
    const double xx = dot3(n1, n2);
    const double yy = lb * dot3(b1, n2);
    const double h = sqrt(xx * xx + yy * yy);
    const double gphi = gs * (xx / h) - gc * (yy / h);
    const double ki = lb / dot3(n1, n1), kl = lb / dot3(n2, n2);
    const double p = dot3(b1, b2) / bb, q = dot3(b3, b2) / bb;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double fi = -(ki * n1[c]);
        const double fl = kl * n2[c];
        double f;
        if (slot == 0) f = fi;
        else if (slot == 3) f = fl;
        else if (slot == 1) f = (-fi - p * fi) + q * fl;
        else f = (-fl + p * fi) - q * fl;
        r[c] = gphi * f;
    }
    return true;
}

// grid (ceil(F / G), ceil(N / C))
template <bool kLds, class Tg, class To>
__global__ __launch_bounds__(kThreads) void icg_bwd_kernel(const float* __restrict__ frames, long long F, int N,
                                                           const int* __restrict__ pairs, int P, const int* __restrict__ triples,
                                                           int A, const int* __restrict__ quads, int Tq,
                                                           const int* __restrict__ atom_ptr, const int* __restrict__ inc,
                                                           long long n_inc, PbcBox box, int G, int C, const Tg* __restrict__ g,
                                                           To* __restrict__ grad) {
    __shared__ float stage[kLds ? 3 * kLdsAtoms : 1];
    const int tid = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * G;
    const int nf = (int)(F - f0 < (long long)G ? F - f0 : (long long)G);
    const long long a0 = (long long)blockIdx.y * C;
    const int na = (int)((long long)N - a0 < (long long)C ? (long long)N - a0 : (long long)C);
    const int items = P + A + Tq;
    const size_t D = (size_t)P + (size_t)A + 2 * (size_t)Tq;
    const float* src = frames + (size_t)f0 * N * 3;
    if (kLds) {
        const int n = nf * N * 3;                                    // <= 3 kLdsAtoms: G N <= kLdsAtoms
        for (int e = tid; e < n; e += kThreads) stage[e] = src[e];
        __syncthreads();
    }
    const int total = nf * na;                                       // nf == 1 wherever N > kLdsAtoms
    for (int e = tid; e < total; e += kThreads) {
        const int fl = e / na, a = (int)a0 + (e - fl * na);
        const float* x = kLds ? stage + fl * N * 3 : src + (size_t)fl * N * 3;
        const Tg* grow = g + (size_t)(f0 + fl) * D;
        long long lo = atom_ptr[a], hi = atom_ptr[a + 1];            // clamped: a wrong table reads inside inc or nothing
        lo = lo < 0 ? 0 : (lo > n_inc ? n_inc : lo);
        hi = hi < 0 ? 0 : (hi > n_inc ? n_inc : hi);
        double acc[3] = {0.0, 0.0, 0.0};
        for (long long q = lo; q < hi; ++q) {
            const unsigned code = (unsigned)inc[q];
            const unsigned it = code >> 2;
            if (it >= (unsigned)items) continue;
            double r[3];
            if (!icg_contribution<Tg>(x, N, a, (int)it, (int)(code & 3u), pairs, P, triples, A, quads, box, grow, r)) continue;
            acc[0] = acc[0] + r[0];
            acc[1] = acc[1] + r[1];
            acc[2] = acc[2] + r[2];
        }
        To* o = grad + ((size_t)(f0 + fl) * N + (size_t)a) * 3;
        o[0] = (To)acc[0];
        o[1] = (To)acc[1];
        o[2] = (To)acc[2];
    }
}

template <bool kLds, class Tg, class To>
void launch_bwd(dim3 grid, hipStream_t st, const float* frames, long long F, int N, const int* pairs, int P, const int* triples,
                int A, const int* quads, int Tq, const int* atom_ptr, const int* inc, long long n_inc, const PbcBox& box, int G,
                int C, const void* g, void* grad) {
    hipLaunchKernelGGL((icg_bwd_kernel<kLds, Tg, To>), grid, dim3(kThreads), 0, st, frames, F, N, pairs, P, triples, A, quads, Tq,
                       atom_ptr, inc, n_inc, box, G, C, static_cast<const Tg*>(g), static_cast<To*>(grad));
}

template <bool kLds, class Tg, class... Rest>
void launch_bwd_out(bool out64, Rest... rest) {
    if (out64) launch_bwd<kLds, Tg, double>(rest...);
    else launch_bwd<kLds, Tg, float>(rest...);
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" int mdnoicg_features_bwd(const float* frames, int64_t F, int N, const int32_t* pairs, int P, const int32_t* triples,
                                    int A, const int32_t* quads, int T, const int32_t* atom_ptr, const int32_t* inc, int64_t n_inc,
                                    const double* box, int flags, const void* g, int g_dtype, void* grad, int grad_dtype, int form,
                                    void* stream) {
    const char* who = "ic_features_bwd";
    MDNO_REQUIRE(F >= 0 && N >= 0 && P >= 0 && A >= 0 && T >= 0 && n_inc >= 0, MDNO_EINVAL, "%s: F=%lld N=%d P=%d A=%d T=%d n_inc=%lld",
                 who, (long long)F, N, P, A, T, (long long)n_inc);
    MDNO_REQUIRE(g_dtype == MDNO_IC_F32 || g_dtype == MDNO_IC_F64, MDNO_EINVAL, "%s: g_dtype=%d is neither f32 (0) nor f64 (1)", who,
                 g_dtype);
    MDNO_REQUIRE(grad_dtype == MDNO_IC_F32 || grad_dtype == MDNO_IC_F64, MDNO_EINVAL, "%s: grad_dtype=%d is neither f32 (0) nor f64 (1)",
                 who, grad_dtype);
    MDNO_REQUIRE(form == MDNO_IC_FORM_AUTO || form == MDNO_IC_FORM_LDS || form == MDNO_IC_FORM_GLOBAL, MDNO_EINVAL,
                 "%s: form=%d (0 auto, 1 lds, 2 global)", who, form);
    MDNO_REQUIRE(!(flags & MDNO_IC_RADIANS), MDNO_EINVAL, "%s: flags=%d asks for radians, which are not differentiable here", who, flags);
    MDNO_REQUIRE(flags == 0, MDNO_EINVAL, "%s: flags=%d holds an unknown bit", who, flags);
    MDNO_REQUIRE(form != MDNO_IC_FORM_LDS || N <= MDNO_IC_LDS_ATOMS, MDNO_EINVAL, "%s: the lds form holds N <= %d atoms, N=%d", who,
                 MDNO_IC_LDS_ATOMS, N);
    const long long items = (long long)P + A + T;
    MDNO_REQUIRE(items < (long long)MDNO_ICG_MAX_ITEMS, MDNO_EINVAL, "%s: P + A + T = %lld items, the table holds fewer than 2^29", who,
                 items);
    PbcBox b = {};
    if (box) MDNO_TRY(pbc_box_from(box, 0.0, &b, who));
    if (F == 0 || N == 0) return MDNO_OK;
    MDNO_REQUIRE((pairs || P == 0) && (triples || A == 0) && (quads || T == 0), MDNO_EINVAL, "%s: null pointer (an index array)", who);
    MDNO_REQUIRE(atom_ptr && (inc || n_inc == 0), MDNO_EINVAL, "%s: null pointer (atom_ptr or inc)", who);
    MDNO_REQUIRE(frames && grad && (g || items == 0), MDNO_EINVAL, "%s: null pointer (frames, g or grad)", who);
    const int G = MDNO_IC_FRAMES_PER_GROUP(N);
    const long long groups = ((long long)F + G - 1) / G;
    MDNO_REQUIRE(groups < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "%s: F=%lld frames exceed the launch grid", who, (long long)F);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool out64 = grad_dtype == MDNO_IC_F64;
    if (items == 0) {
        MDNO_HIP(hipMemsetAsync(grad, 0, (size_t)F * N * 3 * (out64 ? sizeof(double) : sizeof(float)), st));
        return MDNO_OK;
    }
    // the atom chunk of the header: halved while the grid is small and a workgroup still has more than a wave of work
    long long C = N;
    while (groups * ((N + C - 1) / C) < MDNO_ICG_TARGET_GROUPS && (long long)G * C > MDNO_ICG_MIN_THREADS) C = (C + 1) / 2;
    const long long chunks = (N + C - 1) / C;                       // < 2 MDNO_ICG_TARGET_GROUPS: fits grid.y
    const dim3 grid((unsigned)groups, (unsigned)chunks);
    const bool lds = form == MDNO_IC_FORM_LDS || (form == MDNO_IC_FORM_AUTO && N <= MDNO_IC_LDS_ATOMS);
    const bool g64 = g_dtype == MDNO_IC_F64;
    if (lds && g64) launch_bwd_out<true, double>(out64, grid, st, frames, (long long)F, N, pairs, P, triples, A, quads, T, atom_ptr, inc, (long long)n_inc, b, G, (int)C, g, grad);
    else if (lds) launch_bwd_out<true, float>(out64, grid, st, frames, (long long)F, N, pairs, P, triples, A, quads, T, atom_ptr, inc, (long long)n_inc, b, G, (int)C, g, grad);
    else if (g64) launch_bwd_out<false, double>(out64, grid, st, frames, (long long)F, N, pairs, P, triples, A, quads, T, atom_ptr, inc, (long long)n_inc, b, G, (int)C, g, grad);
    else launch_bwd_out<false, float>(out64, grid, st, frames, (long long)F, N, pairs, P, triples, A, quads, T, atom_ptr, inc, (long long)n_inc, b, G, (int)C, g, grad);
    return check_launch(who);
}
