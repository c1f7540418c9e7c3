// Gradients with respect to the model's inputs, and the targets of an unrolled training step (include/mdno_unroll.h;
// DESIGN.md §4.11).  The window frames' gradient is the prologue backward's (train_nodes.hip); here:
//
//   edge_mlp_input_bwd_kernel  d_edge_attr [E, ker_in] = gz1 [E, k] . W0 [k, ker_in]: the one kernel of the feature that
//                              moves real bytes (E k 4 in, E ker_in 4 out).  One pass over gz1: a wave owns 4 edge rows
//                              at a time, lane l reads 16 bytes of each (columns 4 l .. 4 l + 3 of every 256: four 1 KiB
//                              loads in flight per wave), W0 sits in LDS transposed [8][1024] (one conflict-free 16-byte
//                              read per (j, column quad), shared by the 4 rows) and the wave's 4 x 8 per-lane sums meet
//                              in a transposing butterfly: 16 + 8 + 4 + 2 + 1 + 1 exchanges instead of 32 x 6.
//   edge_attr_from_pos_kernel  edge_attr[p] = [pos[src p], pos[dst p]]
//   edge_attr_pos_bwd_kernel   its adjoint, gathered per atom from the by-source list and the destination CSR
//   collate_targets_kernel     y [K, B N, 3] from the resident trajectory
//
// Nothing is accumulated across workgroups: no atomics, every sum in a fixed order.
#include "kernels.h"
#include "../../include/mdno_unroll.h"

namespace mdno {
namespace {

constexpr int KC = 1024;          // columns of W0 resident in LDS at a time (all of them up to ker_width 1024)
constexpr int JP = 8;             // ker_in padded: the largest the edge-MLP's first layer reads
constexpr int WROWS = 4;          // edge rows a wave carries at once
constexpr int GROUP = 4 * WROWS;  // rows per workgroup step (4 waves)

// W0[c0 .. c0 + kc) -> w_s[j][c] (zero for j >= ker_in and c >= kc)
__device__ __forceinline__ void stage_w0(const float* __restrict__ w0, int c0, int kc, int ker_in, float (*w_s)[KC]) {
#pragma unroll 4
    for (int i = threadIdx.x; i < JP * KC; i += 256) {
        const int j = i / KC, c = i - j * KC;
        w_s[j][c] = (j < ker_in && c < kc) ? w0[(size_t)(c0 + c) * ker_in + j] : 0.f;
    }
}

template <bool VEC>      // VEC: ker_width % 4 == 0 and 16-byte aligned rows — float4 loads along k
__global__ __launch_bounds__(256, 4) void edge_mlp_input_bwd_kernel(const float* __restrict__ gz1, const float* __restrict__ w0,
                                                                 const int* __restrict__ num_edges, long long edge_cap, int k,
                                                                 int ker_in, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float w_s[JP][KC];
    long long E = *num_edges;
    E = E < 0 ? 0 : (E > edge_cap ? edge_cap : E);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool single = k <= KC;
    if (single) {
        stage_w0(w0, 0, k, ker_in, w_s);
        __syncthreads();
    }
    const long long groups = (E + GROUP - 1) / GROUP;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {       // (the same trip count in every wave of the block)
        const long long e0 = g * GROUP + wave * WROWS;
        const float* row[WROWS];
#pragma unroll
        for (int r = 0; r < WROWS; ++r) {
            const long long e = e0 + r < E ? e0 + r : E - 1;           // a row past the count reads the last one, stores nothing
            row[r] = gz1 + (size_t)e * k;
        }
        float acc[WROWS * JP];
#pragma unroll
        for (int i = 0; i < WROWS * JP; ++i) acc[i] = 0.f;
        for (int c0 = 0; c0 < k; c0 += KC) {
            const int kc = k - c0 < KC ? k - c0 : KC;
            if (!single) {
                __syncthreads();
                stage_w0(w0, c0, kc, ker_in, w_s);
                __syncthreads();
            }
            if (VEC) {
#pragma unroll 1
                for (int c = 4 * lane; c < kc; c += 256) {
                    float4 v[WROWS];
#pragma unroll
                    for (int r = 0; r < WROWS; ++r) v[r] = *reinterpret_cast<const float4*>(row[r] + c0 + c);
#pragma unroll
                    for (int j = 0; j < JP; ++j) {
                        const float4 w = *reinterpret_cast<const float4*>(&w_s[j][c]);
#pragma unroll
                        for (int r = 0; r < WROWS; ++r) {
                            float s = acc[r * JP + j];
                            s = fmaf(v[r].x, w.x, s);
                            s = fmaf(v[r].y, w.y, s);
                            s = fmaf(v[r].z, w.z, s);
                            s = fmaf(v[r].w, w.w, s);
                            acc[r * JP + j] = s;
                        }
                    }
                }
            } else {
#pragma unroll 1
                for (int c = lane; c < kc; c += 64) {
                    float v[WROWS];
#pragma unroll
                    for (int r = 0; r < WROWS; ++r) v[r] = row[r][c0 + c];
#pragma unroll
                    for (int j = 0; j < JP; ++j) {
                        const float w = w_s[j][c];
#pragma unroll
                        for (int r = 0; r < WROWS; ++r) acc[r * JP + j] = fmaf(v[r], w, acc[r * JP + j]);
                    }
                }
            }
        }
        // transposing butterfly over the wave: at offset 32 >> s a lane keeps one half of its values and hands the
        // other half to its partner; after offsets 32 .. 2 lane l holds value l >> 1 summed over 32 lanes, the last
        // exchange adds the two halves.  Value i = row i / 8, attribute i % 8.
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const int half = (WROWS * JP / 2) >> s, off = 32 >> s;
            const bool up = (lane & off) != 0;
#pragma unroll
            for (int i = 0; i < half; ++i) {
                float lo = acc[i], hi = acc[i + half];
                // (opaque to the optimiser: a select between two array elements would otherwise be turned into one
                // element at a run-time index, and the array into scratch)
                asm volatile("" : "+v"(lo), "+v"(hi));
                acc[i] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, off);
            }
        }
        const float total = acc[0] + __shfl_xor(acc[0], 1);
        const int i = lane >> 1, r = i / JP, j = i - r * JP;
        if ((lane & 1) == 0 && e0 + r < E && j < ker_in) out[(size_t)(e0 + r) * ker_in + j] = total;
    }
}

__global__ __launch_bounds__(256) void edge_attr_from_pos_kernel(const float* __restrict__ pos, const int* __restrict__ src,
                                                                 const int* __restrict__ dst, const int* __restrict__ num_edges,
                                                                 long long edge_cap, int R, float* __restrict__ ea) {
    long long E = *num_edges;
    E = E > edge_cap ? edge_cap : E;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < E; p += (long long)gridDim.x * 256) {
        int s = src[p], d = dst[p];
        s = s < 0 ? 0 : (s >= R ? R - 1 : s);
        d = d < 0 ? 0 : (d >= R ? R - 1 : d);
        float* a = ea + p * 6;
        a[0] = pos[(size_t)s * 3]; a[1] = pos[(size_t)s * 3 + 1]; a[2] = pos[(size_t)s * 3 + 2];
        a[3] = pos[(size_t)d * 3]; a[4] = pos[(size_t)d * 3 + 1]; a[5] = pos[(size_t)d * 3 + 2];
    }
}

// one thread per (atom, component)
__global__ __launch_bounds__(256) void edge_attr_pos_bwd_kernel(const float* __restrict__ d_ea, const int* __restrict__ row_ptr,
                                                                const int* __restrict__ row_ptr_s, const int* __restrict__ eid_s,
                                                                int R, float* __restrict__ d_pos) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= 3ll * R) return;
    const int a = (int)(id / 3), c = (int)(id - 3ll * a);
    const long long E = row_ptr[R];
    float out_sum = 0.f, in_sum = 0.f;
    long long q0 = row_ptr_s[a], q1 = row_ptr_s[a + 1];
    q0 = q0 < 0 ? 0 : q0;
    q1 = q1 > E ? E : q1;
    for (long long q = q0; q < q1; ++q) {
        const long long p = eid_s[q];
        if (p >= 0 && p < E) out_sum += d_ea[p * 6 + c];
    }
    long long p0 = row_ptr[a], p1 = row_ptr[a + 1];
    p0 = p0 < 0 ? 0 : p0;
    p1 = p1 > E ? E : p1;
    for (long long p = p0; p < p1; ++p) in_sum += d_ea[p * 6 + 3 + c];
    d_pos[id] = out_sum + in_sum;
}

__global__ __launch_bounds__(256) void collate_targets_kernel(const float* __restrict__ pos, long long T,
                                                              const long long* __restrict__ meta, int B, int N, int first,
                                                              int K, float* __restrict__ y) {
    const long long per_step = (long long)B * N * 3;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= per_step * K) return;
    const int k = (int)(id / per_step);
    const long long r = id - (long long)k * per_step;
    const int b = (int)(r / (N * 3));
    const int nd = (int)(r - (long long)b * N * 3);
    const long long frame = meta[b] + first + k;
    if (frame < 0 || frame >= T) return;
    y[id] = pos[frame * N * 3 + nd];
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" int mdno_edge_mlp_input_bwd(const float* gz1, const float* w0, const int32_t* num_edges, int64_t edge_cap,
                                       int ker_width, int ker_in, float* d_edge_attr, void* stream) {
    MDNO_REQUIRE(ker_in >= 1 && ker_in <= JP && ker_width >= 1 && edge_cap >= 0, MDNO_EINVAL,
                 "mdno_edge_mlp_input_bwd: ker_in=%d (1..%d) ker_width=%d (>= 1) edge_cap=%lld (>= 0)", ker_in, JP, ker_width,
                 (long long)edge_cap);
    MDNO_REQUIRE(edge_cap <= (1ll << 40) / ker_width, MDNO_EINVAL, "mdno_edge_mlp_input_bwd: edge_cap=%lld x ker_width=%d too large",
                 (long long)edge_cap, ker_width);
    if (edge_cap == 0) return MDNO_OK;
    MDNO_REQUIRE(gz1 && w0 && num_edges && d_edge_attr, MDNO_EINVAL, "mdno_edge_mlp_input_bwd: null pointer");
    const long long groups = (edge_cap + GROUP - 1) / GROUP;
    // memory-bound: at most 5 workgroups (32 KiB of LDS each) per CU x 256 CUs, the rest by the grid stride
    const unsigned grid = (unsigned)(groups < 1280 ? groups : 1280);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool vec = ker_width % 4 == 0 && (reinterpret_cast<uintptr_t>(gz1) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(edge_mlp_input_bwd_kernel<true>, dim3(grid), dim3(256), 0, s, gz1, w0, num_edges,
                           (long long)edge_cap, ker_width, ker_in, d_edge_attr);
    else
        hipLaunchKernelGGL(edge_mlp_input_bwd_kernel<false>, dim3(grid), dim3(256), 0, s, gz1, w0, num_edges,
                           (long long)edge_cap, ker_width, ker_in, d_edge_attr);
    return check_launch("mdno_edge_mlp_input_bwd");
}

extern "C" int mdno_edge_attr_from_pos(const float* pos, const int32_t* src, const int32_t* dst, const int32_t* num_edges,
                                       int64_t edge_cap, int num_rows, float* edge_attr, void* stream) {
    MDNO_REQUIRE(edge_cap >= 0 && edge_cap <= (1ll << 36) && num_rows > 0, MDNO_EINVAL,
                 "mdno_edge_attr_from_pos: edge_cap=%lld num_rows=%d", (long long)edge_cap, num_rows);
    if (edge_cap == 0) return MDNO_OK;
    MDNO_REQUIRE(pos && src && dst && num_edges && edge_attr, MDNO_EINVAL, "mdno_edge_attr_from_pos: null pointer");
    const long long blocks = (edge_cap + 255) / 256;
    hipLaunchKernelGGL(edge_attr_from_pos_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), pos, src, dst, num_edges, (long long)edge_cap, num_rows, edge_attr);
    return check_launch("mdno_edge_attr_from_pos");
}

extern "C" int mdno_edge_attr_pos_bwd(const float* d_edge_attr, const int32_t* row_ptr, const int32_t* row_ptr_s,
                                      const int32_t* eid_s, int num_rows, float* d_pos, void* stream) {
    MDNO_REQUIRE(num_rows > 0, MDNO_EINVAL, "mdno_edge_attr_pos_bwd: num_rows=%d", num_rows);
    MDNO_REQUIRE(d_edge_attr && row_ptr && row_ptr_s && eid_s && d_pos, MDNO_EINVAL, "mdno_edge_attr_pos_bwd: null pointer");
    const long long n = 3ll * num_rows;
    hipLaunchKernelGGL(edge_attr_pos_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_edge_attr, row_ptr, row_ptr_s, eid_s, num_rows, d_pos);
    return check_launch("mdno_edge_attr_pos_bwd");
}

extern "C" int mdno_collate_targets(const float* pos, int64_t num_frames, const int64_t* meta, int B, int N, int W,
                                    int horizon, int K, float* y, void* stream) {
    MDNO_REQUIRE(B > 0 && N > 0 && W > 0 && horizon > 0 && K > 0 && num_frames > 0, MDNO_EINVAL,
                 "mdno_collate_targets: B=%d N=%d W=%d horizon=%d K=%d (all > 0) num_frames=%lld", B, N, W, horizon, K,
                 (long long)num_frames);
    MDNO_REQUIRE(pos && meta && y, MDNO_EINVAL, "mdno_collate_targets: null pointer");
    const long long n = (long long)B * N * 3 * K;
    MDNO_REQUIRE(n < (1ll << 40), MDNO_EINVAL, "mdno_collate_targets: %lld values", n);
    hipLaunchKernelGGL(collate_targets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), pos, (long long)num_frames, (const long long*)meta, B, N,
                       W + horizon - 1, K, y);
    return check_launch("mdno_collate_targets");
}
