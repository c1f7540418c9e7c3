// Distance-constraint projection on the device (include/mdno_constrain.h states the rule, the order and the form;
// DESIGN.md §4.21): mdnocst_project on any stack of frames, and constrain_step, the launch a rollout step ends with when its
// plan was given constraints (engine.hip: mdnocst_rollout_plan_set_constraints).
//
//   cst_project_kernel   grid (frame groups).  A workgroup owns G = MDNOCST_FRAMES_PER_GROUP(N) consecutive frames for all
//                        sweeps: it widens them into LDS (fp64, 24 B per atom, as they lie in memory), measures, and then
//                        repeats { every colour in ascending order, a barrier after each; measure } while one of its frames
//                        is still outside its bands, and rounds the state to fp32 once.  Its threads walk (frame, constraint
//                        of the colour) in strides of the workgroup, the constraint fastest.  Both the sweep and the measure
//                        call cst_eval, THE arithmetic.
// The violation of a frame is a maximum of non-negative doubles, whose bit patterns order as unsigned integers: it is taken
// with an integer atomic max in LDS, which is exact and does not depend on the order.  Nothing else is accumulated across
// threads.  The two violation rows alternate (this sweep's decision reads one, the measure after it fills the other), so the
// only barriers of a sweep are those after its colours and the one after its measure.
// The table (pairs, bands, weights) is read from global memory in every colour: it is shared by every workgroup and stays
// in L2; LDS is kept for the state, which is what sets the largest N.
#include "kernels.h"
#include "pbc.h"
#include "../../include/mdno_constrain.h"

#include <atomic>
#include <cmath>

namespace mdno {
namespace {

constexpr int kThreads = MDNOCST_WORKGROUP;
constexpr int kMaxGroup = MDNOCST_MAX_GROUP_FRAMES;
constexpr int kStateAtoms = MDNOCST_MAX_ATOMS > MDNOCST_GROUP_ATOMS ? MDNOCST_MAX_ATOMS : MDNOCST_GROUP_ATOMS;
constexpr int kMaxLdsBytes = kStateAtoms * 24 + 2 * kMaxGroup * 8;
static_assert(kMaxLdsBytes <= 160 * 1024, "the state of the largest frame and the violation rows fit the LDS of a compute unit");
static_assert(MDNOCST_MAX_ATOMS >= 4096, "the form holds at least 4,096 atoms");
static_assert(2 * kMaxGroup <= kThreads, "one thread per violation word");
static_assert((long long)kMaxGroup * MDNOCST_MAX_CONSTRAINTS < (1ll << 31), "the (frame, constraint) walk of a workgroup is an int");

typedef unsigned long long u64;

struct CstTable {
    const int* pairs;          // [C, 2]
    const double* lo;          // [C]
    const double* hi;          // [C]
    const int* colour_ptr;     // [n_colours + 1]
    const float* weights;      // [N] or NULL
    int C, n_colours;
};

__device__ __forceinline__ double as_double(u64 b) { return __longlong_as_double((long long)b); }

// One constraint on the fp64 state x of one frame (the rule of the header): false = skipped.  r = the bond vector, len its
// length, t the length the band asks for, wi / wj the weights of the two atoms.
__device__ __forceinline__ bool cst_eval(const double* x, int N, const CstTable& tb, const PbcBox& box, int k, int& i, int& j,
                                         double r[3], double& len, double& t, double& wi, double& wj) {
    i = tb.pairs[2 * k];
    j = tb.pairs[2 * k + 1];
    if (!((unsigned)i < (unsigned)N && (unsigned)j < (unsigned)N)) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double d = x[3 * i + a] - x[3 * j + a];
        if (box.L[a] > 0.0) d = d - rint(d * box.inv[a]) * box.L[a];
        r[a] = d;
    }
    len = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    const double lo = tb.lo[k], hi = tb.hi[k];
    t = len < lo ? lo : (len > hi ? hi : len);
    wi = tb.weights ? (double)tb.weights[i] : 1.0;
    wj = tb.weights ? (double)tb.weights[j] : 1.0;
    if (!std::isfinite(len) || len == 0.0 || t == len || wi + wj == 0.0) return false;
    return true;
}

// max over the non-skipped constraints of |len - t| for the frames of the workgroup whose word in `gate` exceeds tol (all of
// them when gate is NULL), into row[frame] (zeroed by the caller)
__device__ __forceinline__ void cst_measure(const double* x, int N, int nf, const CstTable& tb, const PbcBox& box, const u64* gate,
                                            double tol, u64* row) {
    const int total = nf * tb.C;
    for (int e = threadIdx.x; e < total; e += kThreads) {
        const int fl = e / tb.C, k = e - fl * tb.C;
        if (gate && !(as_double(gate[fl]) > tol)) continue;
        int i, j;
        double r[3], len, t, wi, wj;
        if (!cst_eval(x + (size_t)fl * N * 3, N, tb, box, k, i, j, r, len, t, wi, wj)) continue;
        atomicMax(&row[fl], (u64)__double_as_longlong(fabs(len - t)));
    }
}

// grid (ceil(F / G)); dynamic LDS: G N 3 doubles, then 2 G violation words.  t_dev: the rollout's device-side step counter
// (the frames are those of step *t_dev - 1 of a trajectory [frame0 + max_steps, F, N, 3], the reports row `step` of
// [max_steps, F]), or NULL (frames [F, N, 3] as given)
__global__ __launch_bounds__(kThreads) void cst_project_kernel(const float* in, float* out, long long F, int N, CstTable tb,
                                                               PbcBox box, int iterations, double tol, int G,
                                                               const int* __restrict__ t_dev, int frame0, int max_steps,
                                                               int* __restrict__ sweeps, double* __restrict__ viol_in,
                                                               double* __restrict__ viol_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cst_lds[];
    double* x = reinterpret_cast<double*>(cst_lds);
    u64* viol = reinterpret_cast<u64*>(x + (size_t)G * N * 3);          // [2][G]
    const int tid = threadIdx.x;
    long long frame_base = 0, report_base = 0;
    if (t_dev) {
        const int step = *t_dev - 1;                                    // (the same for every thread: no barrier is skipped by some)
        if (step < 0 || step >= max_steps) return;
        frame_base = (long long)(frame0 + step) * F;
        report_base = (long long)step * F;
    }
    const long long f0 = (long long)blockIdx.x * G;
    const int nf = (int)(F - f0 < (long long)G ? F - f0 : (long long)G);
    const size_t off = (size_t)(frame_base + f0) * N * 3;
    const int n = nf * N * 3;                                           // <= 3 kStateAtoms
    for (int e = tid; e < n; e += kThreads) x[e] = (double)in[off + e];
    if (tid < 2 * G) viol[tid] = 0;
    __syncthreads();
    cst_measure(x, N, nf, tb, box, nullptr, tol, viol);
    __syncthreads();
    int cur = 0, my_sweeps = 0;
    const double my_in = tid < nf ? as_double(viol[tid]) : 0.0;
    for (int s = 0; s < iterations; ++s) {
        const u64* gate = viol + cur * G;
        bool any = false;
        for (int f = 0; f < nf; ++f) any = any || as_double(gate[f]) > tol;
        if (!any) break;                                                // (LDS words every thread reads alike: uniform)
        u64* next = viol + (cur ^ 1) * G;
        if (tid < nf) {                                                 // a frame that is done keeps its violation
            const bool act = as_double(gate[tid]) > tol;
            next[tid] = act ? 0 : gate[tid];
            my_sweeps += act ? 1 : 0;
        }
        for (int c = 0; c < tb.n_colours; ++c) {
            int b = tb.colour_ptr[c], e1 = tb.colour_ptr[c + 1];
            b = b < 0 ? 0 : (b > tb.C ? tb.C : b);
            e1 = e1 < b ? b : (e1 > tb.C ? tb.C : e1);
            const int nc = e1 - b, total = nf * nc;
            for (int e = tid; e < total; e += kThreads) {
                const int fl = e / nc, k = b + (e - fl * nc);
                if (!(as_double(gate[fl]) > tol)) continue;
                double* xf = x + (size_t)fl * N * 3;
                int i, j;
                double r[3], len, t, wi, wj;
                if (!cst_eval(xf, N, tb, box, k, i, j, r, len, t, wi, wj)) continue;
                const double g = ((len - t) / len) / (wi + wj);
                const double gi = wi * g, gj = wj * g;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    xf[3 * i + a] = xf[3 * i + a] - gi * r[a];
                    xf[3 * j + a] = xf[3 * j + a] + gj * r[a];
                }
            }
            __syncthreads();
        }
        cst_measure(x, N, nf, tb, box, gate, tol, next);
        __syncthreads();
        cur ^= 1;
    }
    for (int e = tid; e < n; e += kThreads) out[off + e] = (float)x[e];
    if (tid < nf) {
        const size_t at = (size_t)(report_base + f0 + tid);
        if (sweeps) sweeps[at] = my_sweeps;
        if (viol_in) viol_in[at] = my_in;
        if (viol_out) viol_out[at] = as_double(viol[cur * G + tid]);
    }
}

int cst_check_table(const char* who, int N, const int* pairs, const double* lo, const double* hi, long long C, const int* colour_ptr,
                    int n_colours, int iterations, double tol) {
    MDNO_REQUIRE(N >= 0 && C >= 0 && n_colours >= 0 && iterations >= 0, MDNO_EINVAL, "%s: N=%d C=%lld n_colours=%d iterations=%d", who, N,
                 C, n_colours, iterations);
    MDNO_REQUIRE(N <= MDNOCST_MAX_ATOMS, MDNO_EINVAL, "%s: N=%d, the LDS form holds frames of at most %d atoms", who, N, MDNOCST_MAX_ATOMS);
    MDNO_REQUIRE(C <= MDNOCST_MAX_CONSTRAINTS, MDNO_EINVAL, "%s: C=%lld constraints exceed %d", who, C, MDNOCST_MAX_CONSTRAINTS);
    MDNO_REQUIRE(tol >= 0.0, MDNO_EINVAL, "%s: tol=%g must be >= 0", who, tol);
    MDNO_REQUIRE(C == 0 || (pairs && lo && hi && colour_ptr), MDNO_EINVAL, "%s: null pointer (pairs, lo, hi or colour_ptr)", who);
    MDNO_REQUIRE(C == 0 || n_colours >= 1, MDNO_EINVAL, "%s: C=%lld constraints in no colour", who, C);
    return MDNO_OK;
}

// (a frame above 64 KiB of state needs the kernel's dynamic-LDS bound raised: once per device, outside any capture)
int cst_raise_lds() {
    static std::atomic<unsigned long long> raised{0};
    return raise_dynamic_lds(reinterpret_cast<const void*>(&cst_project_kernel), kMaxLdsBytes, raised);
}

int cst_launch(const char* who,const float* in, float* out, long long F, int N, const CstTable& tb, const PbcBox& box, int iterations,
               double tol, const int* t_dev, int frame0, int max_steps, int* sweeps, double* viol_in, double* viol_out, hipStream_t s) {
    MDNO_TRY(cst_raise_lds());
    const int G = MDNOCST_FRAMES_PER_GROUP(N);
    const long long groups = (F + G - 1) / G;
    MDNO_REQUIRE(groups < (1ll << 31) - 1, MDNO_EUNSUPPORTED, "%s: F=%lld frames exceed the launch grid", who, F);
    const size_t lds = (size_t)G * N * 24 + 2 * (size_t)G * 8;          // <= kMaxLdsBytes: G N <= kStateAtoms, G <= kMaxGroup
    hipLaunchKernelGGL(cst_project_kernel, dim3((unsigned)groups), dim3(kThreads), lds, s, in, out, F, N, tb, box, iterations, tol, G,
                       t_dev, frame0, max_steps, sweeps, viol_in, viol_out);
    return check_launch(who);
}

}  // namespace

int constrain_prepare() { return cst_raise_lds(); }

int constrain_check(const char* who, int N, const int* pairs, const double* lo, const double* hi, long long C, const int* colour_ptr,
                    int n_colours, int iterations, double tol) {
    return cst_check_table(who, N, pairs, lo, hi, C, colour_ptr, n_colours, iterations, tol);
}

int constrain_step(float* traj, int W, const int* t_dev, int M, int N, int max_steps, const int* pairs, const double* lo,
                   const double* hi, long long C, const int* colour_ptr, int n_colours, const float* weights, const PbcBox* box,
                   int iterations, double tol, int* sweeps, double* viol_in, double* viol_out, hipStream_t s) {
    const char* who = "constrain_step";
    MDNO_REQUIRE(traj && t_dev && M > 0 && N > 0 && W > 0 && max_steps > 0 && C > 0, MDNO_EINVAL, "%s: M=%d N=%d C=%lld", who, M, N, C);
    MDNO_TRY(cst_check_table(who, N, pairs, lo, hi, C, colour_ptr, n_colours, iterations, tol));
    const CstTable tb{pairs, lo, hi, colour_ptr, weights, (int)C, n_colours};
    const PbcBox none{};
    // the step's last kernel has moved the counter on: the frame just written (and perturbed) is that of step *t_dev - 1
    return cst_launch(who, traj, traj, (long long)M, N, tb, box ? *box : none, iterations, tol, t_dev, W, max_steps, sweeps, viol_in,
                      viol_out, s);
}

}  // namespace mdno

using namespace mdno;

extern "C" int mdnocst_project(const float* in, float* out, int64_t F, int N, const int32_t* pairs, const double* lo,
                               const double* hi, int64_t C, const int32_t* colour_ptr, int n_colours, const float* weights,
                               const double* box, int iterations, double tol, int32_t* sweeps, double* viol_in,
                               double* viol_out, void* stream) {
    const char* who = "mdnocst_project";
    MDNO_REQUIRE(F >= 0, MDNO_EINVAL, "%s: F=%lld", who, (long long)F);
    MDNO_TRY(cst_check_table(who, N, pairs, lo, hi, (long long)C, colour_ptr, n_colours, iterations, tol));
    PbcBox b{};
    if (box) MDNO_TRY(pbc_box_from(box, 0.0, &b, who));
    if (F == 0) return MDNO_OK;
    MDNO_REQUIRE((in && out) || N == 0, MDNO_EINVAL, "%s: null pointer (in or out)", who);
    const CstTable tb{pairs, lo, hi, colour_ptr, weights, (int)C, n_colours};
    return cst_launch(who, in, out, (long long)F, N, tb, b, iterations, tol, nullptr, 0, 0, sweeps, viol_in, viol_out,
                      static_cast<hipStream_t>(stream));
}
