// Seeded Gaussian noise on the device (include/mdno_noise.h; the generator and its counter layout: philox.h).
//
//   noise_frames_kernel  frame[m][a][c] += sigma * z(seed, member_ids[m], step, a * 3 + c): the frame a rollout step
//                        has just produced, step read from the plan's device-side counter (engine.hip)
//   noise_window_kernel  the same over the input windows of a collated training batch [W, R, 3], every row attributed
//                        to its sample through the batch's row offsets
//   noise_fill_kernel    the raw values (and the Philox words behind them) for tests and callers
//
// One thread makes the four values of one Philox block pair (elements 4g .. 4g+3 of a stream) and moves them with one
// 16-byte load / store where the four lie in a row at an aligned address, one by one otherwise (frames of 3 N floats
// are not 16-byte multiples; the tail of a stream).  Nothing is accumulated across threads: no atomics.
#include "kernels.h"
#include "philox.h"
#include "../../include/mdno_noise.h"

namespace mdno {
namespace {

// sigma * z of elements 4g .. 4g+3 of stream `sid`; w1 / w2: the words behind u1 / u2
__device__ __forceinline__ void noise_quad(unsigned long long seed, uint32_t sid, long long index, uint32_t g, int purpose,
                                           float sigma, float v[4], uint32_t w1[4], uint32_t w2[4]) {
    noise_block(seed, sid, index, g, purpose, 0, w1);
    noise_block(seed, sid, index, g, purpose, 1, w2);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = sigma * noise_normal(w1[j], w2[j]);
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// out[0..cnt) = in[0..cnt) + v[0..cnt), cnt <= 4 consecutive floats (in may be out)
__device__ __forceinline__ void add_run(const float* in, float* out, const float v[4], int cnt) {
    if (cnt == 4 && aligned16(in) && aligned16(out)) {
        float4 x = *reinterpret_cast<const float4*>(in);
        x.x += v[0]; x.y += v[1]; x.z += v[2]; x.w += v[3];
        *reinterpret_cast<float4*>(out) = x;
    } else {
        for (int j = 0; j < cnt; ++j) out[j] = in[j] + v[j];
    }
}

__global__ __launch_bounds__(256) void noise_frames_kernel(float* __restrict__ frames, int frame, const int* __restrict__ t_dev,
                                                           int step_offset, int M, int N, const int* __restrict__ member_ids,
                                                           unsigned long long seed, float sigma) {
    const int n = 3 * N, m = blockIdx.y;
    const long long e0 = 4ll * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (e0 >= n) return;
    const int step = (t_dev ? *t_dev : 0) + step_offset;
    if (step < 0) return;
    float v[4];
    uint32_t w1[4], w2[4];
    noise_quad(seed, (uint32_t)member_ids[m], step, (uint32_t)(e0 >> 2), NOISE_ROLLOUT, sigma, v, w1, w2);
    float* p = frames + ((size_t)(frame + step) * M + m) * n + e0;
    add_run(p, p, v, n - e0 < 4 ? (int)(n - e0) : 4);
}

__global__ __launch_bounds__(256) void noise_window_kernel(const float* x_in, float* x_out,      // (may alias)
                                                           const int* __restrict__ sample_ids,
                                                           const int* __restrict__ row_offsets, int W, long long R,
                                                           long long epoch, unsigned long long seed, float sigma) {
    const int b = blockIdx.y;
    const long long r0 = row_offsets[b], nb = row_offsets[b + 1] - r0;
    if (nb <= 0 || r0 < 0 || r0 + nb > R) return;      // (a malformed table writes nothing)
    const long long fe = nb * 3, total = fe * W;        // floats of the sample per frame, per window
    const long long e0 = 4ll * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (e0 >= total) return;
    float v[4];
    uint32_t w1[4], w2[4];
    noise_quad(seed, (uint32_t)sample_ids[b], epoch, (uint32_t)(e0 >> 2), NOISE_TRAIN_WINDOW, sigma, v, w1, w2);
    const int cnt = total - e0 < 4 ? (int)(total - e0) : 4;
    const long long w = e0 / fe, e = e0 - w * fe;
    if (e + cnt <= fe) {                                // the run lies in one frame
        const size_t at = (size_t)(w * R + r0) * 3 + e;
        add_run(x_in + at, x_out + at, v, cnt);
    } else {
        for (int j = 0; j < cnt; ++j) {
            const long long wj = (e0 + j) / fe, ej = e0 + j - wj * fe;
            const size_t at = (size_t)(wj * R + r0) * 3 + ej;
            x_out[at] = x_in[at] + v[j];
        }
    }
}

__global__ __launch_bounds__(256) void noise_fill_kernel(const int* __restrict__ stream_ids, long long index, int E,
                                                         int purpose, unsigned long long seed, float sigma,
                                                         float* __restrict__ z_out, uint32_t* __restrict__ words_out) {
    const int m = blockIdx.y;
    const long long e0 = 4ll * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (e0 >= E) return;
    float v[4];
    uint32_t w1[4], w2[4];
    noise_quad(seed, (uint32_t)stream_ids[m], index, (uint32_t)(e0 >> 2), purpose, sigma, v, w1, w2);
    const int cnt = E - e0 < 4 ? (int)(E - e0) : 4;
    float* z = z_out + (size_t)m * E + e0;
    if (cnt == 4 && aligned16(z)) {
        *reinterpret_cast<float4*>(z) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < cnt; ++j) z[j] = v[j];
    }
    if (words_out) {
        uint32_t* wo = words_out + ((size_t)m * E + e0) * 2;      // (4-byte stores: the header asks for no more alignment)
        for (int j = 0; j < cnt; ++j) {
            wo[2 * j] = w1[j];
            wo[2 * j + 1] = w2[j];
        }
    }
}

unsigned quad_blocks(long long elems) { return (unsigned)(((elems + 3) / 4 + 255) / 256); }

}  // namespace

int noise_step(float* traj, int W, const int* t_dev, int M, int N, const int* member_ids, unsigned long long seed,
               float sigma, hipStream_t s) {
    MDNO_REQUIRE(traj && t_dev && member_ids && M > 0 && M <= 65535 && N > 0, MDNO_EINVAL, "noise_step: M=%d N=%d", M, N);
    // the step's last kernel has moved the counter on: the frame just written is that of step *t_dev - 1
    hipLaunchKernelGGL(noise_frames_kernel, dim3(quad_blocks(3ll * N), M), dim3(256), 0, s, traj, W, t_dev, -1, M, N,
                       member_ids, seed, sigma);
    return check_launch("noise_frames");
}

}  // namespace mdno

using namespace mdno;

extern "C" int mdno_noise_fill(uint64_t seed, const int32_t* stream_ids, int M, int64_t index, int N, int per_stream_elems,
                               int purpose, float sigma, float* z_out, uint32_t* words_out, void* stream) {
    MDNO_REQUIRE(M >= 0 && M <= 65535 && N > 0 && per_stream_elems >= 0 && per_stream_elems % (3ll * N) == 0, MDNO_EINVAL,
                 "mdno_noise_fill: M=%d N=%d per_stream_elems=%d (a multiple of 3 N; M <= 65535)", M, N, per_stream_elems);
    MDNO_REQUIRE(index >= 0 && index < kNoiseMaxIndex && purpose >= 0 && purpose < 256, MDNO_EINVAL,
                 "mdno_noise_fill: index=%lld (0 <= index < 2^48) purpose=%d (0 <= purpose < 256)", (long long)index, purpose);
    if (M == 0 || per_stream_elems == 0) return MDNO_OK;
    MDNO_REQUIRE(stream_ids && z_out, MDNO_EINVAL, "mdno_noise_fill: null pointer");
    hipLaunchKernelGGL(noise_fill_kernel, dim3(quad_blocks(per_stream_elems), M), dim3(256), 0,
                       static_cast<hipStream_t>(stream), stream_ids, (long long)index, per_stream_elems, purpose,
                       (unsigned long long)seed, sigma, z_out, words_out);
    return check_launch("mdno_noise_fill");
}

extern "C" int mdno_noise_add_window(uint64_t seed, const int32_t* sample_ids, const int32_t* row_offsets, int B, int W,
                                     int64_t R, int max_rows_per_sample, int64_t epoch, float sigma, const float* x_in,
                                     float* x_out, void* stream) {
    MDNO_REQUIRE(B >= 0 && B <= 65535 && W > 0 && R >= 0 && R <= (1ll << 40) && max_rows_per_sample >= 0 &&
                     max_rows_per_sample <= R,
                 MDNO_EINVAL, "mdno_noise_add_window: B=%d W=%d R=%lld max_rows_per_sample=%d", B, W, (long long)R,
                 max_rows_per_sample);
    MDNO_REQUIRE(epoch >= 0 && epoch < kNoiseMaxIndex, MDNO_EINVAL, "mdno_noise_add_window: epoch=%lld (0 <= epoch < 2^48)",
                 (long long)epoch);
    const long long per_sample = 3ll * W * max_rows_per_sample;
    MDNO_REQUIRE(per_sample < (1ll << 34), MDNO_EINVAL, "mdno_noise_add_window: %lld values per sample (element >> 2 is a 32-bit word)",
                 per_sample);
    if (B == 0 || per_sample == 0) return MDNO_OK;
    MDNO_REQUIRE(sample_ids && row_offsets && x_in && x_out, MDNO_EINVAL, "mdno_noise_add_window: null pointer");
    hipLaunchKernelGGL(noise_window_kernel, dim3(quad_blocks(per_sample), B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x_in, x_out, sample_ids, row_offsets, W, (long long)R, (long long)epoch, (unsigned long long)seed, sigma);
    return check_launch("mdno_noise_add_window");
}
