// Training under a periodic box (include/mdno_pbc_train.h): the one kernel the feature adds — the
// edge attributes of an edge list as a function of the positions, with the source moved to its minimum image next to
// the destination.  The rule is pbc.h's pbc_shift, the one the periodic radius graph tests and writes with
// (graph.hip radius_row_kernel<PbcPair>): the same operands in the same operations, so on that graph's own list the
// rows are its attribute rows bit for bit.  Its adjoint is input_grad.hip's edge_attr_pos_bwd_kernel as it is: the
// shift is a constant of the edge.
//
// One thread per edge: two scalar index loads, two 12-byte gathers (pos is small and stays in L2), six fp64
// operations per axis, and the 24-byte row as three 8-byte vector stores — a wave writes 1,536 contiguous bytes.
// The box travels by value in the kernel arguments.  No LDS, no scratch, no atomics.
#include "pbc.h"
#include "../../include/mdno_pbc_train.h"

namespace mdno {
namespace {

__global__ __launch_bounds__(256) void pbc_edge_attr_from_pos_kernel(const float* __restrict__ pos, const int* __restrict__ src,
                                                                     const int* __restrict__ dst,
                                                                     const int* __restrict__ num_edges, long long edge_cap,
                                                                     int R, const PbcBox box, float* __restrict__ ea) {
    long long E = *num_edges;
    E = E > edge_cap ? edge_cap : E;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < E; p += (long long)gridDim.x * 256) {
        int s = src[p], d = dst[p];
        s = s < 0 ? 0 : (s >= R ? R - 1 : s);
        d = d < 0 ? 0 : (d >= R ? R - 1 : d);
        const float* ps = pos + (size_t)s * 3;
        const float* pd = pos + (size_t)d * 3;
        const float fxs = ps[0], fys = ps[1], fzs = ps[2];
        const float fxd = pd[0], fyd = pd[1], fzd = pd[2];
        const double xs = fxs, ys = fys, zs = fzs;
        const double sx = pbc_shift((double)fxd, xs, box.L[0], box.inv[0]);
        const double sy = pbc_shift((double)fyd, ys, box.L[1], box.inv[1]);
        const double sz = pbc_shift((double)fzd, zs, box.L[2], box.inv[2]);
        float2* a = reinterpret_cast<float2*>(ea + (size_t)p * 6);          // rows of 24 B: 8-B aligned
        a[0] = make_float2((float)(xs - sx), (float)(ys - sy));
        a[1] = make_float2((float)(zs - sz), fxd);
        a[2] = make_float2(fyd, fzd);
    }
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" int mdnopbt_edge_attr_from_pos(const float* pos, const int32_t* src, const int32_t* dst, const int32_t* num_edges,
                                          int64_t edge_cap, int num_rows, double cutoff, const double* box, float* edge_attr,
                                          void* stream) {
    PbcBox b{};
    MDNO_TRY(pbc_box_from(box, cutoff, &b, "mdnopbt_edge_attr_from_pos"));
    MDNO_REQUIRE(edge_cap >= 0 && edge_cap <= (1ll << 36) && num_rows > 0, MDNO_EINVAL,
                 "mdnopbt_edge_attr_from_pos: edge_cap=%lld num_rows=%d", (long long)edge_cap, num_rows);
    if (edge_cap == 0) return MDNO_OK;
    MDNO_REQUIRE(pos && src && dst && num_edges && edge_attr, MDNO_EINVAL, "mdnopbt_edge_attr_from_pos: null pointer");
    MDNO_REQUIRE((reinterpret_cast<uintptr_t>(edge_attr) & 7) == 0, MDNO_EINVAL,
                 "mdnopbt_edge_attr_from_pos: edge_attr is not 8-byte aligned");
    const long long blocks = (edge_cap + 255) / 256;
    hipLaunchKernelGGL(pbc_edge_attr_from_pos_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), pos, src, dst, num_edges, (long long)edge_cap, num_rows, b, edge_attr);
    return check_launch("mdnopbt_edge_attr_from_pos");
}
