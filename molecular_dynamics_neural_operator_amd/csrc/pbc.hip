// Periodic boxes on the host side: validation of a box (pbc.h: pbc_box_from) and the C entry of the periodic radius
// graph (include/mdno_pbc.h).  The graph itself is graph.hip's brute-force form under the minimum-image
// rule (radius_graph with a box): the box travels BY VALUE in the kernel arguments, so a captured rollout step holds it.
#include "pbc.h"
#include "../../include/mdno_pbc.h"

#include <cmath>

namespace mdno {

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

}  // namespace mdno

using namespace mdno;

extern "C" int mdno_radius_graph_pbc(const float* pos, int M, int N, double cutoff, const double* box, int32_t* row_ptr,
                                     int32_t* src, int32_t* dst, float* edge_attr, int64_t edge_cap, int32_t* num_edges,
                                     int32_t* status, void* stream) {
    PbcBox b{};
    MDNO_TRY(pbc_box_from(box, cutoff, &b, "mdno_radius_graph_pbc"));
    return radius_graph(pos, 0, nullptr, M, N, cutoff, &b, edge_attr, row_ptr, src, dst, (long long)edge_cap, num_edges,
                        status, static_cast<hipStream_t>(stream));
}
