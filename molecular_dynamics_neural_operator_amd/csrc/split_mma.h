// The common types of ALL matrix-pipe kernels (the vector and address-space typedefs: the fp32-MFMA kernels take
// f32x16 from here too, through mfma_f32.h) and the arithmetic every split-plane kernel shares, once: the plane products in their one order, the packed forms of split3 / split2h (split_layout.h), the C/D row map of the
// 32x32 MFMA and the XCD-aware tile range.  The bitwise promises (the choice of GEMM kernel never shows in a result;
// training forward == eval factored forward) rest on every kernel taking these from here.
#pragma once
#include <hip/hip_runtime.h>

#include "split_layout.h"

namespace mdno {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) unsigned char lds_u8;
typedef __attribute__((address_space(1))) const unsigned char glb_u8;

// ---- three bf16 planes: the six leading plane products of (a0 + a1 + a2)(b0 + b1 + b2), SMALLEST FIRST
// (a1 b1, a2 b0, a0 b2, then a1 b0, a0 b1, then a0 b0).  This order is part of every result's bits.
__device__ __forceinline__ void mma6_bf16(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
}

// ---- two fp16 planes: the three leading plane products of (a0 + a1)(b0 + b1), smallest first: the cross terms
// a1 b0, a0 b1 into accx, a0 b0 into acc.  Two forms, one order:
//   * two accumulators (ACC, ACCX; the split GEMMs, edge_mlp_split.hip): the lo plane is split2h's, scaled by 2^11, so the cross
//     terms carry a 2^-11 that the epilogue applies once, exactly (acc + accx * F16_LO_UNSCALE);
//   * one accumulator (mma3_f16, ACCX = ACC; the factored conv, moment.hip): the lo plane is split2_store4's, NOT scaled, so the three
//     products add up as they are — K1 has no registers for a second accumulator at three workgroups per CU.
// The definition is a macro because the two-accumulator GEMM kernels need it expanded in place (behind a function call
// the few-rows kernel's OUT_PLANES_F16 instances come out 13-16 instructions longer); everybody else calls mma3_f16.
#define MDNO_MMA3_F16(A, B, ACC, ACCX)                                                  \
    ACCX = __builtin_amdgcn_mfma_f32_32x32x16_f16((A)[1], (B)[0], ACCX, 0, 0, 0);       \
    ACCX = __builtin_amdgcn_mfma_f32_32x32x16_f16((A)[0], (B)[1], ACCX, 0, 0, 0);       \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_f16((A)[0], (B)[0], ACC, 0, 0, 0);
__device__ __forceinline__ void mma3_f16(const f16x8 (&a)[2], const f16x8 (&b)[2], f32x16& acc) { MDNO_MMA3_F16(a, b, acc, acc) }

// C/D map of the 32x32 MFMA: accumulator register e (0..15) of a lane in half-wave h = lane >> 5 holds row
// mfma32_row(e, h) of column lane & 31.  `base` (the tile's first row) is added FIRST, term by term: the sum then
// associates as the kernels always wrote it, and the compiler's address arithmetic stays what was measured.
template <class I = int>
__device__ __forceinline__ constexpr I mfma32_row(int e, int h, I base = 0) {
    return base + (e & 3) + 8 * (e >> 2) + 4 * h;
}

// XCD-aware tile order: workgroups b, b + 8, ... share an XCD (round-robin dispatch); XCD x owns a contiguous range of
// the nwg tiles — `count` of them from `first` — so that neighbouring tiles share an operand panel through that XCD's
// L2.  Workgroup `orig` takes tile first + (orig >> 3); bijective for any nwg.
template <class I>
__device__ __forceinline__ void xcd_tile_range(I orig, I nwg, I& first, I& count) {
    const I xcd = orig & 7, q = nwg >> 3, r8 = nwg & 7;
    first = xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q;
    count = q + (xcd < r8 ? 1 : 0);
}
__device__ __forceinline__ int xcd_tile(int orig, int nwg) {
    int first, count;
    xcd_tile_range(orig, nwg, first, count);
    return first + (orig >> 3);
}

// ---- the packed forms of split3 / split2h: the same planes, two values per conversion instruction
// (a, b) -> packed bf16 pair (one v_cvt_pk_bf16_f32) and the pair's values back in fp32
__device__ __forceinline__ unsigned pack_bf16(float a, float b, float& fa, float& fb) {
    const f32x2 v = {a, b};
    const bf16x2 p = __builtin_convertvector(v, bf16x2);
    const unsigned u = __builtin_bit_cast(unsigned, p);
    fa = __builtin_bit_cast(float, u << 16);
    fb = __builtin_bit_cast(float, u & 0xffff0000u);
    return u;
}

// four fp32 -> 3 x four bf16 (hi, mid, lo: split3's planes), 8 bytes per plane at dst + p * plane_bytes
__device__ __forceinline__ void split_store4(const float4 v, unsigned char* dst, int plane_bytes) {
    float h0, h1, h2, h3, m0, m1, m2, m3, t0, t1;
    uint2 hi, mid, lo;
    hi.x = pack_bf16(v.x, v.y, h0, h1);
    hi.y = pack_bf16(v.z, v.w, h2, h3);
    const float r0 = v.x - h0, r1 = v.y - h1, r2 = v.z - h2, r3 = v.w - h3;
    mid.x = pack_bf16(r0, r1, m0, m1);
    mid.y = pack_bf16(r2, r3, m2, m3);
    lo.x = pack_bf16(r0 - m0, r1 - m1, t0, t1);
    lo.y = pack_bf16(r2 - m2, r3 - m3, t0, t1);
    *reinterpret_cast<uint2*>(dst) = hi;
    *reinterpret_cast<uint2*>(dst + plane_bytes) = mid;
    *reinterpret_cast<uint2*>(dst + 2 * plane_bytes) = lo;
}

// (a, b) -> packed fp16 pair (one v_cvt_pk_f16_f32 on gfx950) and the pair's values back in fp32
__device__ __forceinline__ unsigned pack_f16(float a, float b, float& fa, float& fb) {
    const f32x2 v = {a, b};
    const f16x2 p = __builtin_convertvector(v, f16x2);
    fa = (float)p.x;
    fb = (float)p.y;
    return __builtin_bit_cast(unsigned, p);
}

// four fp32 (already scaled) -> 2 x four fp16 (hi, lo), 8 bytes per plane at dst + p * plane_bytes.  split2h's hi plane;
// the lo plane is NOT multiplied by F16_LO_SCALE (the one-accumulator form of mma3_f16; moment.hip says how the absolute
// floor this leaves is kept out of sight)
__device__ __forceinline__ void split2_store4(const float4 v, unsigned char* dst, int plane_bytes) {
    float h0, h1, h2, h3, t0, t1;
    uint2 hi, lo;
    hi.x = pack_f16(v.x, v.y, h0, h1);
    hi.y = pack_f16(v.z, v.w, h2, h3);
    lo.x = pack_f16(v.x - h0, v.y - h1, t0, t1);
    lo.y = pack_f16(v.z - h2, v.w - h3, t0, t1);
    *reinterpret_cast<uint2*>(dst) = hi;
    *reinterpret_cast<uint2*>(dst + plane_bytes) = lo;
}

}  // namespace mdno
