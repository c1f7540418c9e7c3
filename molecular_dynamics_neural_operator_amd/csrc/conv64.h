// The 64x64 materialised conv's lane mapping and association — the one definition.  Every kernel that multiplies by an
// edge's 64x64 matrix W_e (forward: nnconv.hip, train_conv.hip; input gradient: train_conv.hip) includes this header, so
// that inference, fp32 training and bf16 training add the same terms in the same order: bitwise run-to-run equality,
// member-alone == member-in-batch and bf16w == fp32 on bf16-representable weights all rest on it.
//
// A wave holds one matrix at a time.  Lane l = (g, q), g = l >> 4, q = l & 15, owns input rows 16g..16g+15 x output
// columns 4q..4q+3: every wave-instruction is a 16-B (fp32) or 8-B (bf16) load per lane covering four whole rows of
// the matrix, fully coalesced, 16 such loads per matrix.  Device helpers only: nothing here launches.
#pragma once
#include <hip/hip_runtime.h>

#include "bf16.h"

namespace mdno {

// A row's edges are dealt to CHAINS = 16 summation chains (edge i of the row -> chain i % 16) whatever
// the launch shape: with 16 waves a wave owns one chain, with 4 waves it owns chains w, w+4, w+8, w+12
// (one accumulator each).  The chains are then added in chain order, so the 4- and the 16-wave launch
// give the same bits and a row's result does not depend on how many rows it is batched with.
constexpr int CHAINS = 16;

__device__ __forceinline__ void fma4(float4& a, float s, const float4& w) {
    a.x = fmaf(s, w.x, a.x);
    a.y = fmaf(s, w.y, a.y);
    a.z = fmaf(s, w.z, a.z);
    a.w = fmaf(s, w.w, a.w);
}

__device__ __forceinline__ float4 reduce_over_g(float4 a) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        a.x += __shfl_xor(a.x, o);
        a.y += __shfl_xor(a.y, o);
        a.z += __shfl_xor(a.z, o);
        a.w += __shfl_xor(a.w, o);
    }
    return a;
}

// 4 consecutive weights as a float4; WT = float (16-B load) or __bf16 (8-B load, widened exactly).
// STREAM: a non-temporal load (global_load ... nt) — an edge's W_e is read exactly once per conv application and is
// far larger than the caches, so it is streamed past them and leaves them to x.  The callers' policy: fp32 W_e is
// streamed unless all of it fits the L2s (nnconv.hip decides), bf16 W_e always, root (read by every row: cached) never.
template <class WT, bool STREAM>
__device__ __forceinline__ float4 ld_w4(const WT* p);
template <>
__device__ __forceinline__ float4 ld_w4<float, false>(const float* p) { return *reinterpret_cast<const float4*>(p); }
template <>
__device__ __forceinline__ float4 ld_w4<float, true>(const float* p) {
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    const f32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p));
    return make_float4(t.x, t.y, t.z, t.w);
}
template <>
__device__ __forceinline__ float4 ld_w4<__bf16, false>(const __bf16* p) { return ld4_bf16(p); }
template <>
__device__ __forceinline__ float4 ld_w4<__bf16, true>(const __bf16* p) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 u = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
    return unpack4_bf16(u.x, u.y);
}

// Forward, one edge: acc += x[16g..16g+15] . Wblk[16g..16g+15][4q..4q+3].  STREAM: W is read once per application and
// is far larger than the caches (nt loads leave them to x); !STREAM: all of W_e fits the L2s (a short chain: 330 edges
// = 5.4 MB over 8 x 4 MB), the 2 x depth applications of a forward re-read it, and a row's 12 x 16 KiB reach its ONE CU
// at the L2's 66-73 GB/s per CU instead of the Infinity Cache's 33 (MI355X_MICROARCH.md, gather rates): the
// application is bound by exactly that
template <class WT, bool STREAM>
__device__ __forceinline__ void edge_accumulate64(float4& acc, const float* __restrict__ xrow,
                                                  const WT* __restrict__ wmat, int g, int q) {
    // the matrix first: its address does not wait for src[p], which the x row's does
    const WT* wp = wmat + (16 * g) * 64 + 4 * q;
    float4 w[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) w[r] = ld_w4<WT, STREAM>(wp + r * 64);
    const float* xp = xrow + 16 * g;
    const float4 x0 = *reinterpret_cast<const float4*>(xp), x1 = *reinterpret_cast<const float4*>(xp + 4);
    const float4 x2 = *reinterpret_cast<const float4*>(xp + 8), x3 = *reinterpret_cast<const float4*>(xp + 12);
    // all twenty loads in flight before the first FMA waits for one (left alone, the scheduler waits for the
    // x row after nine of them and issues the rest behind that round trip) — a batch row has ~12 edges, one per
    // wave, so a workgroup's life is its chain of round trips
    __builtin_amdgcn_sched_barrier(0);
    fma4(acc, x0.x, w[0]);  fma4(acc, x0.y, w[1]);  fma4(acc, x0.z, w[2]);  fma4(acc, x0.w, w[3]);
    fma4(acc, x1.x, w[4]);  fma4(acc, x1.y, w[5]);  fma4(acc, x1.z, w[6]);  fma4(acc, x1.w, w[7]);
    fma4(acc, x2.x, w[8]);  fma4(acc, x2.y, w[9]);  fma4(acc, x2.z, w[10]); fma4(acc, x2.w, w[11]);
    fma4(acc, x3.x, w[12]); fma4(acc, x3.y, w[13]); fma4(acc, x3.z, w[14]); fma4(acc, x3.w, w[15]);
}

// Input gradient, one edge (the transposed product): acc[r] += W[16g + r][4q..4q+3] . gvec[4q..4q+3].  The per-lane
// partial dot products are summed over ALL of a row's edges first and reduced across the 16 q-lanes once per row.
template <class WT, bool STREAM>
__device__ __forceinline__ void wg_accumulate(float (&acc)[16], const WT* __restrict__ wmat,
                                              const float* __restrict__ gvec, int g, int q) {
    const float4 gq = *reinterpret_cast<const float4*>(gvec + 4 * q);
    const WT* wp = wmat + (16 * g) * 64 + 4 * q;
    float4 w[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) w[r] = ld_w4<WT, STREAM>(wp + r * 64);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        acc[r] = fmaf(w[r].x, gq.x, fmaf(w[r].y, gq.y, fmaf(w[r].z, gq.z, fmaf(w[r].w, gq.w, acc[r]))));
}

}  // namespace mdno
