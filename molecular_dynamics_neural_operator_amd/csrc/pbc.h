// Orthorhombic periodic boundary conditions: THE minimum-image rule (include/mdno_pbc.h), used by the
// radius graph under a box (graph.hip: radius_graph, which a periodic rollout step calls) and by the periodic scoring
// kernels (forecast.hip).  One definition: every kernel that tests a pair under a box calls within_pbc below.
#pragma once
#include "graph_small.h"

namespace mdno {

// box lengths and their reciprocals (1.0 / L, formed once on the host); L == 0: the axis is open (inv == 0 as well)
struct PbcBox {
    double L[3];
    double inv[3];
    bool any() const { return L[0] > 0.0 || L[1] > 0.0 || L[2] > 0.0; }
};

// Validates `box` (f64 [3]: every entry finite and >= 0; 0 = open axis; a periodic axis needs L >= 2 * cutoff so that a
// pair has at most one image inside the strict cutoff) and fills `out`.  MDNO_EINVAL with a message otherwise.
int pbc_box_from(const double* box, double cutoff, PbcBox* out, const char* who);

// k * L for the image of source coordinate xj next to destination coordinate xi on one axis: all in fp64 on the fp32
// coordinates, k = rint(d / L) round-half-even (rint is odd: the rule is symmetric in i and j), k = 0 on an open axis
__device__ __forceinline__ double pbc_shift(double xi, double xj, double L, double inv) {
    const double k = L > 0.0 ? rint((xj - xi) * inv) : 0.0;
    return k * L;
}

// the pair test of within() (graph_small.h: same differences, same summation order, strict <) on the minimum image;
// sh[a] = the shift that was tested, so that the caller can form the source's image (float)(x_j - sh)
__device__ __forceinline__ bool within_pbc(double xi, double yi, double zi, const float* __restrict__ pj, double cutoff,
                                           const PbcBox& b, double sh[3]) {
    const double xj = pj[0], yj = pj[1], zj = pj[2];
    sh[0] = pbc_shift(xi, xj, b.L[0], b.inv[0]);
    sh[1] = pbc_shift(yi, yj, b.L[1], b.inv[1]);
    sh[2] = pbc_shift(zi, zj, b.L[2], b.inv[2]);
    const double dx = (xj - xi) - sh[0], dy = (yj - yi) - sh[1], dz = (zj - zi) - sh[2];
    const double s = (dx * dx + dy * dy) + dz * dz;
    return sqrt(s) < cutoff;
}

// the squared distance that within() / within_pbc test, for kernels that need the distance itself (observe.hip): the
// same differences, the same shifts and the same summation order, so sqrt(dist2) < cutoff IS the pair test
__device__ __forceinline__ double dist2_open(double xi, double yi, double zi, const float* __restrict__ pj) {
    const double dx = (double)pj[0] - xi, dy = (double)pj[1] - yi, dz = (double)pj[2] - zi;
    return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ double dist2_pbc(double xi, double yi, double zi, const float* __restrict__ pj, const PbcBox& b) {
    const double xj = pj[0], yj = pj[1], zj = pj[2];
    const double dx = (xj - xi) - pbc_shift(xi, xj, b.L[0], b.inv[0]);
    const double dy = (yj - yi) - pbc_shift(yi, yj, b.L[1], b.inv[1]);
    const double dz = (zj - zi) - pbc_shift(zi, zj, b.L[2], b.inv[2]);
    return (dx * dx + dy * dy) + dz * dz;
}

// Pair tests as kernel arguments (graph.hip's brute-force form and forecast.hip are templated on one of them): the open
// test is within() itself.  The second call operator also yields sh[a] = the shift that was tested (zeros for the open
// rule); has_image says whether a source can have an image other than itself; dist2 is the squared distance the test takes
// the root of.
struct OpenPair {
    static constexpr bool has_image = false;
    double cutoff;
    __device__ __forceinline__ bool operator()(double xi, double yi, double zi, const float* __restrict__ pj) const {
        return within(xi, yi, zi, pj, cutoff);
    }
    __device__ __forceinline__ bool operator()(double xi, double yi, double zi, const float* __restrict__ pj,
                                               double sh[3]) const {
        sh[0] = sh[1] = sh[2] = 0.0;
        return within(xi, yi, zi, pj, cutoff);
    }
    __device__ __forceinline__ double dist2(double xi, double yi, double zi, const float* __restrict__ pj) const {
        return dist2_open(xi, yi, zi, pj);
    }
};
struct PbcPair {
    static constexpr bool has_image = true;
    double cutoff;
    PbcBox box;
    __device__ __forceinline__ bool operator()(double xi, double yi, double zi, const float* __restrict__ pj) const {
        double sh[3];
        return within_pbc(xi, yi, zi, pj, cutoff, box, sh);
    }
    __device__ __forceinline__ bool operator()(double xi, double yi, double zi, const float* __restrict__ pj,
                                               double sh[3]) const {
        return within_pbc(xi, yi, zi, pj, cutoff, box, sh);
    }
    __device__ __forceinline__ double dist2(double xi, double yi, double zi, const float* __restrict__ pj) const {
        return dist2_pbc(xi, yi, zi, pj, box);
    }
};

}  // namespace mdno
