// The layouts moment.hip's kernels share with the training backward (train_moment.hip): the k-tiled images and the
// chunking of the destinations.
//   H image   fp32 [E/128][k/32][128][32]            element (edge e, hidden unit c)
//   S image   fp32 [chunk rows/128][64k/32 + 2][128][32], kappa = i*k + c (and 64 k + i for s0_t[i])
//   W3R       fp32 [(64k + 64)/32][64 o][32]         W3R[kappa][o] = W3[(i*64 + o)*k + c], B3[i][o] at kappa = 64 k + i
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace mdno {

// k-tiles (32 kappa) of a destination's row of the S image: 64 k / 32 for S_t itself + 2 for s0_t (kappa = 64 k + i)
__host__ __device__ constexpr size_t moment_nkt(int K) { return (size_t)64 * K / 32 + 2; }

constexpr int MO_CQ = 256;                 // hidden units per K1 workgroup

constexpr int kMomentChunkRows = 512;      // destinations per S chunk: 512 x 64 k x 4 B = 128 MiB at k = 1024, written by K1
                                           // and read back by K2 while still in the 256 MiB Infinity Cache
inline int moment_chunk_rows(int num_rows) {
    const int padded = (num_rows + 127) / 128 * 128;
    return padded < kMomentChunkRows ? padded : kMomentChunkRows;
}

// offset of element (edge e, hidden unit c) in the H image
__host__ __device__ inline size_t h_image_offset(long long e, int c, int K) {
    return ((size_t)(e >> 7) * (size_t)(K >> 5) + (size_t)(c >> 5)) * 4096 + (size_t)(e & 127) * 32 + (size_t)(c & 31);
}

}  // namespace mdno
