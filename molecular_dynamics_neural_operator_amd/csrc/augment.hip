// Random rigid motions of training samples on the device (include/mdno_augment.h; the rule and its operation order:
// rigid_rule.h, which this file only runs).
//
//   motions_kernel    one wave per sample: the centroid of its first window frame in the rule's fixed order (a partial
//                     sum per lane, folded with shuffles), then lane 0 draws the translation and runs the bounded
//                     rejection loop and writes q, c, t and the two accepted elements
//   apply_kernel      one thread per row of one sample over all F frames (rows of a sample are consecutive: a wave
//                     reads and writes 768 consecutive bytes); thread 0 forms R, c and c + t from q once per workgroup
//   edge_attr_kernel  one thread per edge: the two end rows of x0, written as three 8-byte stores
//
// Streaming kernels: nothing is accumulated across threads, no atomics, vector stores only.
#include "kernels.h"
#include "rigid_rule.h"
#include "../../include/mdno_augment.h"

namespace mdno {
namespace {

__global__ __launch_bounds__(64) void motions_kernel(unsigned long long seed, const int* __restrict__ sample_ids,
                                                     long long epoch, int rotate, double translate, int last_element,
                                                     const float* __restrict__ frames, int N, double* __restrict__ q_out,
                                                     double* __restrict__ c_out, double* __restrict__ t_out,
                                                     int* __restrict__ attempts_out) {
    const int b = blockIdx.x, l = threadIdx.x;
    double c[3] = {0.0, 0.0, 0.0};
    if (frames) {
        const float* x = frames + (size_t)b * N * 3;
        for (int r = l; r < N; r += kRigidCentroidLanes) {
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = c[k] + (double)x[3 * (size_t)r + k];
        }
        for (int off = kRigidCentroidLanes / 2; off > 0; off >>= 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = c[k] + __shfl_down(c[k], off, kRigidCentroidLanes);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = c[k] / (double)N;
    }
    if (l != 0) return;
    const uint32_t sid = (uint32_t)sample_ids[b];
    double t[3], q[4] = {1.0, 0.0, 0.0, 0.0};
    int attempts[2] = {-1, -1};
    rigid_shift(seed, sid, epoch, translate, t);
    if (rotate) rigid_quaternion(seed, sid, epoch, last_element, q, attempts);
#pragma unroll
    for (int k = 0; k < 4; ++k) q_out[4 * (size_t)b + k] = q[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c_out[3 * (size_t)b + k] = c[k];
        t_out[3 * (size_t)b + k] = t[k];
    }
    attempts_out[2 * (size_t)b] = attempts[0];
    attempts_out[2 * (size_t)b + 1] = attempts[1];
}

__global__ __launch_bounds__(256) void apply_kernel(const double* __restrict__ quaternion, const double* __restrict__ pivot,
                                                    const double* __restrict__ shift, int B, int N, int F, int inverse,
                                                    const float* x_in, float* x_out) {      // (may alias)
    __shared__ double sR[9], sC[3], sCT[3];
    const int b = blockIdx.y;
    if (threadIdx.x == 0) {
        double q[4], c[3], t[3], ct[3], R[9];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = quaternion[4 * (size_t)b + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c[k] = pivot[3 * (size_t)b + k];
            t[k] = shift[3 * (size_t)b + k];
        }
        rigid_matrix(q, R);
        rigid_pivot_shift(c, t, ct);
#pragma unroll
        for (int k = 0; k < 9; ++k) sR[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            sC[k] = c[k];
            sCT[k] = ct[k];
        }
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;      // row i of the sample's F * N
    if (i >= (long long)F * N) return;
    const long long f = i / N, r = i - f * N;
    const size_t at = ((size_t)f * B * N + (size_t)b * N + (size_t)r) * 3;
    double R[9], c[3], ct[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = sR[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c[k] = sC[k];
        ct[k] = sCT[k];
    }
    const float p[3] = {x_in[at], x_in[at + 1], x_in[at + 2]};
    float o[3];
    if (inverse) rigid_invert_row(R, c, ct, p, o);
    else rigid_apply_row(R, c, ct, p, o);
    x_out[at] = o[0];
    x_out[at + 1] = o[1];
    x_out[at + 2] = o[2];
}

__global__ __launch_bounds__(256) void edge_attr_kernel(const float* __restrict__ x0, const long long* __restrict__ edge_index,
                                                        long long E, long long R, float* __restrict__ attr_out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const long long s = edge_index[e], d = edge_index[E + e];
    const float nan = __builtin_nanf("");
    float v[6] = {nan, nan, nan, nan, nan, nan};
    if (s >= 0 && s < R && d >= 0 && d < R) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = x0[3 * (size_t)s + k];
            v[3 + k] = x0[3 * (size_t)d + k];
        }
    }
    float2* out = reinterpret_cast<float2*>(attr_out + 6 * (size_t)e);      // (rows of 24 bytes: 8-byte aligned)
    out[0] = make_float2(v[0], v[1]);
    out[1] = make_float2(v[2], v[3]);
    out[2] = make_float2(v[4], v[5]);
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" int mdnoaug_motions(uint64_t seed, const int32_t* sample_ids, int B, int64_t epoch, int rotate, double translate,
                               int last_element, const float* pivot_frames, int N, double* quaternion, double* pivot,
                               double* shift, int32_t* attempts, void* stream) {
    MDNO_REQUIRE(B >= 0 && B <= 65535 && (rotate == 0 || rotate == 1), MDNO_EINVAL, "mdnoaug_motions: B=%d (0 <= B <= 65535) rotate=%d (0 or 1)",
                 B, rotate);
    MDNO_REQUIRE(epoch >= 0 && epoch < kNoiseMaxIndex, MDNO_EINVAL, "mdnoaug_motions: epoch=%lld (0 <= epoch < 2^48)",
                 (long long)epoch);
    MDNO_REQUIRE(translate >= 0.0 && translate <= 1.79769313486231570815e308, MDNO_EINVAL,
                 "mdnoaug_motions: translate=%g (finite and >= 0)", translate);
    MDNO_REQUIRE(last_element >= kRigidFirstElement && last_element <= kRigidLastElement, MDNO_EINVAL,
                 "mdnoaug_motions: last_element=%d (%d <= last_element <= %d)", last_element, kRigidFirstElement, kRigidLastElement);
    MDNO_REQUIRE(!pivot_frames || N >= 1, MDNO_EINVAL, "mdnoaug_motions: N=%d (>= 1 with pivot_frames)", N);
    if (B == 0) return MDNO_OK;
    MDNO_REQUIRE(sample_ids && quaternion && pivot && shift && attempts, MDNO_EINVAL, "mdnoaug_motions: null pointer");
    hipLaunchKernelGGL(motions_kernel, dim3(B), dim3(kRigidCentroidLanes), 0, static_cast<hipStream_t>(stream),
                       (unsigned long long)seed, sample_ids, (long long)epoch, rotate, translate, last_element, pivot_frames, N,
                       quaternion, pivot, shift, attempts);
    return check_launch("mdnoaug_motions");
}

extern "C" int mdnoaug_apply(const double* quaternion, const double* pivot, const double* shift, int B, int N, int F,
                             int inverse, const float* x_in, float* x_out, void* stream) {
    MDNO_REQUIRE(B >= 0 && B <= 65535 && N >= 0 && F >= 0 && (long long)F * N < (1ll << 31), MDNO_EINVAL,
                 "mdnoaug_apply: B=%d N=%d F=%d (0 <= B <= 65535, F * N < 2^31)", B, N, F);
    if (B == 0 || N == 0 || F == 0) return MDNO_OK;
    MDNO_REQUIRE(quaternion && pivot && shift && x_in && x_out, MDNO_EINVAL, "mdnoaug_apply: null pointer");
    const unsigned blocks = (unsigned)(((long long)F * N + 255) / 256);
    hipLaunchKernelGGL(apply_kernel, dim3(blocks, B), dim3(256), 0, static_cast<hipStream_t>(stream), quaternion, pivot,
                       shift, B, N, F, inverse != 0, x_in, x_out);
    return check_launch("mdnoaug_apply");
}

extern "C" int mdnoaug_edge_attr(const float* x0, const int64_t* edge_index, int64_t E, int64_t R, float* attr_out,
                                 void* stream) {
    MDNO_REQUIRE(E >= 0 && E < (1ll << 39) && R >= 0 && R <= (1ll << 40), MDNO_EINVAL,
                 "mdnoaug_edge_attr: E=%lld R=%lld (0 <= E < 2^39, 0 <= R <= 2^40)", (long long)E, (long long)R);
    if (E == 0) return MDNO_OK;
    MDNO_REQUIRE(edge_index && attr_out && (x0 || R == 0), MDNO_EINVAL, "mdnoaug_edge_attr: null pointer");
    MDNO_REQUIRE(reinterpret_cast<uintptr_t>(attr_out) % 8 == 0, MDNO_EINVAL, "mdnoaug_edge_attr: attr_out must be 8-byte aligned");
    hipLaunchKernelGGL(edge_attr_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x0,
                       reinterpret_cast<const long long*>(edge_index), (long long)E, (long long)R, attr_out);
    return check_launch("mdnoaug_edge_attr");
}
