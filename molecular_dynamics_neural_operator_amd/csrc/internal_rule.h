// The bond vector, dot product and cross product of include/mdno_internal.h, shared by internal.hip (the features) and
// internal_grad.hip (their adjoint, include/mdno_internal_grad.h): ONE definition, so the backward forms the forward's
// vectors bit for bit.  fp64 on the fp32 coordinates, + - x rint only, each rounded once (the library is built with
// -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include "pbc.h"

namespace mdno {

__device__ __forceinline__ double dot3(const double p[3], const double q[3]) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }
__device__ __forceinline__ void cross3(const double p[3], const double q[3], double r[3]) {
    r[0] = p[1] * q[2] - p[2] * q[1];
    r[1] = p[2] * q[0] - p[0] * q[2];
    r[2] = p[0] * q[1] - p[1] * q[0];
}
// v(a->b) under the box; x = the frame's coordinates (LDS or global), a and b inside 0 .. N - 1
__device__ __forceinline__ void bond(const float* x, int a, int b, const PbcBox& box, double v[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double d = (double)x[3 * b + c] - (double)x[3 * a + c];
        if (box.L[c] > 0.0) d = d - rint(d * box.inv[c]) * box.L[c];
        v[c] = d;
    }
}
__device__ __forceinline__ bool inside(int a, int N) { return (unsigned)a < (unsigned)N; }

}  // namespace mdno
