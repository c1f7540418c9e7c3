// Periodic radius graph: minimum-image pair test under an orthorhombic box -> destination-sorted CSR plus the edge
// attribute rows [image of the source next to the destination, destination] (include/mdno_pbc.h, pbc.h).
//
// The count / scan / fill structure of graph.hip's brute-force form, one wave per destination row: lane l tests atoms
// j = l, l + 64, ... of the row's own member, ballot + prefix popcount keeps a row's sources ascending.  The scan is
// graph.hip's scan_rows_kernel itself.  The box travels BY VALUE in the kernel arguments, so a captured rollout step
// holds it.  The fill pass writes the attribute row beside src[p]: the shift k * L that the test used is the shift the
// attribute is formed with, so the edge-MLP sees exactly the image that was inside the cutoff.
#include "pbc.h"
#include "../../include/mdno_pbc.h"

#include <cmath>

namespace mdno {

namespace {

constexpr int kRowsPerBlock = 4;  // one wave per destination row

// FILL = false: in-degree of every row -> deg[r].  FILL = true: the row's sources (and destinations, attributes).
template <bool FILL>
__global__ __launch_bounds__(256) void radius_pbc_kernel(const float* __restrict__ frames, int frame,
                                                         const int* __restrict__ t_dev, int N, int R, double cutoff,
                                                         const PbcBox box, int* __restrict__ deg,
                                                         const int* __restrict__ row_ptr, long long cap,
                                                         int* __restrict__ src, int* __restrict__ dst,
                                                         float* __restrict__ attr) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (r >= R) return;
    const float* pos = frames + (size_t)(frame + (t_dev ? *t_dev : 0)) * R * 3;
    const int m = r / N;
    const float* pm = pos + (size_t)m * N * 3;
    const float* pi = pos + (size_t)r * 3;
    const float fxi = pi[0], fyi = pi[1], fzi = pi[2];
    const double xi = fxi, yi = fyi, zi = fzi;
    long long base = FILL ? row_ptr[r] : 0;
    int cnt = 0;
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int j0 = 0; j0 < N; j0 += 64) {
        const int j = j0 + lane;
        double sh[3] = {0.0, 0.0, 0.0};
        const float* pj = pm + (size_t)(j < N ? j : 0) * 3;
        const bool in = (j < N) && within_pbc(xi, yi, zi, pj, cutoff, box, sh);
        const unsigned long long mask = __ballot(in);
        if (!FILL) {
            cnt += __popcll(mask);
        } else {
            if (in) {
                const long long p = base + __popcll(mask & lt);
                if (p < cap) {
                    src[p] = m * N + j;
                    if (dst) dst[p] = r;
                    if (attr) {
                        float2* a = reinterpret_cast<float2*>(attr + (size_t)p * 6);      // rows of 24 B: 8-B aligned
                        a[0] = make_float2((float)((double)pj[0] - sh[0]), (float)((double)pj[1] - sh[1]));
                        a[1] = make_float2((float)((double)pj[2] - sh[2]), fxi);
                        a[2] = make_float2(fyi, fzi);
                    }
                }
            }
            base += __popcll(mask);
        }
    }
    if (!FILL && lane == 0) deg[r] = cnt;
}

}  // namespace

int pbc_box_from(const double* box, double cutoff, PbcBox* out, const char* who) {
    MDNO_REQUIRE(box != nullptr, MDNO_EINVAL, "%s: null box", who);
    MDNO_REQUIRE(std::isfinite(cutoff) && cutoff >= 0.0, MDNO_EINVAL, "%s: cutoff %g is not a finite non-negative number",
                 who, cutoff);
    for (int a = 0; a < 3; ++a) {
        const double L = box[a];
        MDNO_REQUIRE(std::isfinite(L) && L >= 0.0, MDNO_EINVAL, "%s: box[%d] = %g (a finite length, or 0 for an open axis)",
                     who, a, L);
        MDNO_REQUIRE(L == 0.0 || L >= 2.0 * cutoff, MDNO_EINVAL,
                     "%s: box[%d] = %g < 2 * cutoff = %g (a pair would have more than one image inside the cutoff)", who, a,
                     L, 2.0 * cutoff);
        out->L[a] = L;
        out->inv[a] = L > 0.0 ? 1.0 / L : 0.0;
    }
    return MDNO_OK;
}

int radius_graph_pbc(const float* frames, int frame, const int* t_dev, int M, int N, double cutoff, const PbcBox& box,
                     int* row_ptr, int* src, int* dst, float* edge_attr, long long edge_cap, int* num_edges, int* status,
                     hipStream_t s, int* zero_words, int n_zero) {
    MDNO_REQUIRE(frames && row_ptr && src && num_edges, MDNO_EINVAL, "radius_graph_pbc: null pointer");
    MDNO_REQUIRE(M > 0 && N > 0 && edge_cap > 0 && frame >= 0, MDNO_EINVAL, "radius_graph_pbc: M=%d N=%d cap=%lld", M, N,
                 edge_cap);
    MDNO_REQUIRE((long long)M * N < (1ll << 31) - 1 && edge_cap < (1ll << 31) - 1, MDNO_EUNSUPPORTED,
                 "radius_graph_pbc: row or edge count exceeds int32 indexing");
    const int R = M * N;
    // The in-degrees are staged in src[0..R) (needs edge_cap >= R); the fill pass overwrites them.
    MDNO_REQUIRE(edge_cap >= R, MDNO_EINVAL, "radius_graph_pbc: edge_cap (%lld) < rows (%d)", edge_cap, R);
    MDNO_REQUIRE(n_zero >= 0 && n_zero <= 64 && (n_zero == 0 || zero_words), MDNO_EINVAL, "radius_graph_pbc: n_zero=%d", n_zero);
    MDNO_REQUIRE(!edge_attr || (reinterpret_cast<uintptr_t>(edge_attr) & 7) == 0, MDNO_EINVAL,
                 "radius_graph_pbc: edge_attr not 8-B aligned");
    const int blocks = (R + kRowsPerBlock - 1) / kRowsPerBlock;
    TimedSection ts(KID_GRAPH, s);
    hipLaunchKernelGGL(radius_pbc_kernel<false>, dim3(blocks), dim3(256), 0, s, frames, frame, t_dev, N, R, cutoff, box, src,
                       (const int*)nullptr, edge_cap, (int*)nullptr, (int*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(scan_rows_kernel, dim3(1), dim3(1024), 0, s, (const int*)src, R, edge_cap, row_ptr, num_edges,
                       status, zero_words, n_zero);
    hipLaunchKernelGGL(radius_pbc_kernel<true>, dim3(blocks), dim3(256), 0, s, frames, frame, t_dev, N, R, cutoff, box,
                       (int*)nullptr, (const int*)row_ptr, edge_cap, src, dst, edge_attr);
    return check_launch("radius_graph_pbc");
}

}  // namespace mdno

using namespace mdno;

extern "C" int mdno_radius_graph_pbc(const float* pos, int M, int N, double cutoff, const double* box, int32_t* row_ptr,
                                     int32_t* src, int32_t* dst, float* edge_attr, int64_t edge_cap, int32_t* num_edges,
                                     int32_t* status, void* stream) {
    PbcBox b{};
    MDNO_TRY(pbc_box_from(box, cutoff, &b, "mdno_radius_graph_pbc"));
    return radius_graph_pbc(pos, 0, nullptr, M, N, cutoff, b, row_ptr, src, dst, edge_attr, (long long)edge_cap, num_edges,
                            status, static_cast<hipStream_t>(stream));
}
