// Four bf16 at a time, as the kernels that store activations, W_e or dW_e in bf16 read and write them.
#pragma once
#include <hip/hip_runtime.h>

namespace mdno {

__device__ __forceinline__ float4 unpack4_bf16(unsigned lo, unsigned hi) {      // two words of two bf16 -> float4 (exact)
    return make_float4(__builtin_bit_cast(float, lo << 16), __builtin_bit_cast(float, lo & 0xffff0000u),
                       __builtin_bit_cast(float, hi << 16), __builtin_bit_cast(float, hi & 0xffff0000u));
}
__device__ __forceinline__ float4 ld4_bf16(const __bf16* p) {      // 4 consecutive bf16 -> float4 (8-B load)
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    return unpack4_bf16(u.x, u.y);
}
__device__ __forceinline__ uint2 pack4_bf16(float a, float b, float c, float d) {      // RNE, 8 B
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    const bf16x4 v = {(__bf16)a, (__bf16)b, (__bf16)c, (__bf16)d};
    return __builtin_bit_cast(uint2, v);
}

}  // namespace mdno
