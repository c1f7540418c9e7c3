// The eigen-solve of the optimal rigid superposition, shared by forecast.hip (one frame against its same-step truth) and
// conformations.hip (every frame against every reference frame): ONE definition, so both give the same bits for the same
// moments.
#pragma once
#include <hip/hip_runtime.h>

namespace mdno {

constexpr int kJacobiSweeps = 12;      // a 4 x 4 symmetric matrix is diagonal to fp64 after 5-6 (quadratic convergence)

// rmsd^2 from the cross-covariance s[3*r+c] = sum a_r b_c of two centred frames and G = sum |a|^2 + sum |b|^2; n = N as a
// double.  lambda, the largest eigenvalue of Horn's 4 x 4 quaternion matrix of s, by cyclic Jacobi sweeps (a fixed number of
// them; exact zeros are skipped, so identical, planar, collinear and one- or two-atom frames need no special case):
// rmsd^2 = max(0, G - 2 lambda) / n.
__device__ inline double rmsd2_from_moments(const double* s, double G, double n) {
    double a[4][4];
    a[0][0] = (s[0] + s[4]) + s[8];
    a[1][1] = (s[0] - s[4]) - s[8];
    a[2][2] = (s[4] - s[0]) - s[8];
    a[3][3] = (s[8] - s[0]) - s[4];
    a[0][1] = a[1][0] = s[5] - s[7];
    a[0][2] = a[2][0] = s[6] - s[2];
    a[0][3] = a[3][0] = s[1] - s[3];
    a[1][2] = a[2][1] = s[1] + s[3];
    a[1][3] = a[3][1] = s[6] + s[2];
    a[2][3] = a[3][2] = s[5] + s[7];
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                a[p][p] -= t * apq;
                a[q][q] += t * apq;
                a[p][q] = a[q][p] = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (r == p || r == q) continue;
                    const double arp = a[r][p], arq = a[r][q];
                    a[r][p] = a[p][r] = c * arp - sn * arq;
                    a[r][q] = a[q][r] = sn * arp + c * arq;
                }
            }
        }
    }
    double lam = a[0][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) lam = a[k][k] > lam ? a[k][k] : lam;
    const double trace = (a[0][0] + a[1][1]) + (a[2][2] + a[3][3]);
    if (trace != trace) lam = trace;      // a non-finite truth frame: NaN, whatever the comparisons above made of it
    const double r2 = (G - 2.0 * lam) / n;
    return r2 < 0.0 ? 0.0 : r2;           // rounding only (a NaN stays a NaN)
}

// The same solve with the rotations accumulated (include/mdno_essential.h): rot[3*i+j] is the proper rotation that takes
// the centred frame a onto the centred frame b, R a_k ~ b_k, from the eigenvector of the largest eigenvalue of Horn's matrix
// (among equal diagonal entries the lowest index) taken as a quaternion and normalised; the return value is that
// eigenvalue, NaN where the moments are not finite (rot is then NaN too).  A quaternion gives a proper rotation whatever
// it is, so a degenerate eigenvalue yields one of the optimal rotations and never a reflection.  Host-callable, so that
// the convention can be checked without a device.
__host__ __device__ inline double rotation_from_moments(const double* s, double* rot) {
    double a[4][4], v[4][4];
    a[0][0] = (s[0] + s[4]) + s[8];
    a[1][1] = (s[0] - s[4]) - s[8];
    a[2][2] = (s[4] - s[0]) - s[8];
    a[3][3] = (s[8] - s[0]) - s[4];
    a[0][1] = a[1][0] = s[5] - s[7];
    a[0][2] = a[2][0] = s[6] - s[2];
    a[0][3] = a[3][0] = s[1] - s[3];
    a[1][2] = a[2][1] = s[1] + s[3];
    a[1][3] = a[3][1] = s[6] + s[2];
    a[2][3] = a[3][2] = s[5] + s[7];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                a[p][p] -= t * apq;
                a[q][q] += t * apq;
                a[p][q] = a[q][p] = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double vrp = v[r][p], vrq = v[r][q];
                    v[r][p] = c * vrp - sn * vrq;
                    v[r][q] = sn * vrp + c * vrq;
                    if (r == p || r == q) continue;
                    const double arp = a[r][p], arq = a[r][q];
                    a[r][p] = a[p][r] = c * arp - sn * arq;
                    a[r][q] = a[q][r] = sn * arp + c * arq;
                }
            }
        }
    }
    double lam = a[0][0];
    double q0 = v[0][0], q1 = v[1][0], q2 = v[2][0], q3 = v[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        if (a[k][k] > lam) lam = a[k][k], q0 = v[0][k], q1 = v[1][k], q2 = v[2][k], q3 = v[3][k];
    }
    const double trace = (a[0][0] + a[1][1]) + (a[2][2] + a[3][3]);
    if (trace != trace) lam = trace, q0 = trace;
    const double n2 = (q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3);
    rot[0] = (((q0 * q0 + q1 * q1) - q2 * q2) - q3 * q3) / n2;
    rot[1] = 2.0 * (q1 * q2 - q0 * q3) / n2;
    rot[2] = 2.0 * (q1 * q3 + q0 * q2) / n2;
    rot[3] = 2.0 * (q1 * q2 + q0 * q3) / n2;
    rot[4] = (((q0 * q0 - q1 * q1) + q2 * q2) - q3 * q3) / n2;
    rot[5] = 2.0 * (q2 * q3 - q0 * q1) / n2;
    rot[6] = 2.0 * (q1 * q3 - q0 * q2) / n2;
    rot[7] = 2.0 * (q2 * q3 + q0 * q1) / n2;
    rot[8] = (((q0 * q0 - q1 * q1) - q2 * q2) + q3 * q3) / n2;
    return lam;
}

}  // namespace mdno
