// The gradient bucket of data-parallel training (data_parallel.py): a host-described list of fp32 tensors copied into
// (pack) or out of (unpack) ONE flat fp32 buffer in one launch, so that the ranks reduce one contiguous buffer with one
// all-reduce per step.  Laid out as adam_kernel (optim.hip): the tensors' addresses and slot offsets travel as a kernel
// argument (no device-side lists, nothing uploaded), every workgroup copies one 4,096-element chunk of one tensor with
// float4 loads and stores where both ends are 16-B aligned and scalar ones elsewhere.  Pack zero-fills the slot of an
// entry without data (a parameter without a gradient, a rank without samples in this batch): the reduction still
// receives its zeros.  Plain C++ loads and stores, nothing else.
#include <algorithm>
#include <climits>
#include <vector>

#include "kernels.h"

namespace mdno {
namespace {

constexpr int BK_MAX_TENSORS = 64;      // per launch (a model has 27); the table below stays well under the 4 KiB argument limit
constexpr int BK_CHUNK = 4096;          // elements per workgroup: 256 threads x 4 float4

struct BucketArgs {
    float* data[BK_MAX_TENSORS];        // nullptr in pack: zero-fill the slot
    long long n[BK_MAX_TENSORS];
    long long offset[BK_MAX_TENSORS];   // in elements of flat
    int chunk0[BK_MAX_TENSORS + 1];     // first workgroup of each tensor
    int count;
    float* flat;
};

template <bool PACK>
__global__ __launch_bounds__(256) void bucket_kernel(const BucketArgs a) {
    int t = 0;
    while (t + 1 < a.count && a.chunk0[t + 1] <= (int)blockIdx.x) ++t;
    const long long base = (long long)((int)blockIdx.x - a.chunk0[t]) * BK_CHUNK;
    const long long n = a.n[t];
    float* __restrict__ x = a.data[t];
    float* __restrict__ f = a.flat + a.offset[t];
    const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(f)) & 15) == 0;
#pragma unroll
    for (int u = 0; u < BK_CHUNK / 1024; ++u) {
        const long long i = base + u * 1024 + threadIdx.x * 4;
        if (i >= n) return;
        if (vec && i + 4 <= n) {
            if (PACK) {
                *reinterpret_cast<float4*>(f + i) = x ? *reinterpret_cast<const float4*>(x + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                *reinterpret_cast<float4*>(x + i) = *reinterpret_cast<const float4*>(f + i);
            }
        } else {
            for (long long j = i; j < n && j < i + 4; ++j) {
                if (PACK) f[j] = x ? x[j] : 0.f;
                else x[j] = f[j];
            }
        }
    }
}

// every check before any device work: null flat, negative sizes or offsets, a null source in unpack, slots that overlap
int validate(int count, const mdno_flat_tensor* tensors, const float* flat, bool pack, const char* what) {
    MDNO_REQUIRE(count >= 0 && (count == 0 || tensors != nullptr), MDNO_EINVAL, "%s: bad arguments (count=%d)", what, count);
    MDNO_REQUIRE(flat != nullptr, MDNO_EINVAL, "%s: flat is null", what);
    std::vector<int> order;
    order.reserve(count);
    for (int i = 0; i < count; ++i) {
        const mdno_flat_tensor& t = tensors[i];
        MDNO_REQUIRE(t.numel >= 0 && t.offset >= 0, MDNO_EINVAL, "%s: tensor %d has numel=%lld offset=%lld", what, i,
                     (long long)t.numel, (long long)t.offset);
        MDNO_REQUIRE(t.numel <= LLONG_MAX - t.offset, MDNO_EINVAL, "%s: tensor %d: offset + numel overflows", what, i);
        MDNO_REQUIRE(pack || t.numel == 0 || t.data != nullptr, MDNO_EINVAL, "%s: null destination in tensor %d", what, i);
        MDNO_REQUIRE((t.numel + BK_CHUNK - 1) / BK_CHUNK < INT_MAX / 2, MDNO_EINVAL, "%s: tensor %d is too large", what, i);
        if (t.numel > 0) order.push_back(i);
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return tensors[a].offset < tensors[b].offset; });
    for (size_t k = 1; k < order.size(); ++k) {
        const mdno_flat_tensor& p = tensors[order[k - 1]];
        MDNO_REQUIRE(p.offset + p.numel <= tensors[order[k]].offset, MDNO_EINVAL,
                     "%s: the slots of tensors %d and %d overlap", what, order[k - 1], order[k]);
    }
    return MDNO_OK;
}

template <bool PACK>
int run(int count, const mdno_flat_tensor* tensors, float* flat, void* stream, const char* what) {
    MDNO_TRY(validate(count, tensors, flat, PACK, what));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int i = 0;
    while (i < count) {
        BucketArgs a{};
        a.flat = flat;
        long long chunks = 0;
        for (; i < count && a.count < BK_MAX_TENSORS; ++i) {
            const mdno_flat_tensor& t = tensors[i];
            if (t.numel == 0) continue;
            const long long c = (t.numel + BK_CHUNK - 1) / BK_CHUNK;
            if (a.count > 0 && chunks + c > INT_MAX / 2) break;        // this tensor opens the next launch
            const int k = a.count++;
            a.data[k] = t.data; a.n[k] = t.numel; a.offset[k] = t.offset;
            a.chunk0[k] = (int)chunks;
            chunks += c;
        }
        if (a.count == 0) continue;
        a.chunk0[a.count] = (int)chunks;
        hipLaunchKernelGGL(bucket_kernel<PACK>, dim3((unsigned)chunks), dim3(256), 0, s, a);
        MDNO_TRY(check_launch(what));
    }
    return MDNO_OK;
}

}  // namespace
}  // namespace mdno

using namespace mdno;

extern "C" int mdno_pack_tensors(int count, const mdno_flat_tensor* tensors, float* flat, void* stream) {
    return run<true>(count, tensors, flat, stream, "mdno_pack_tensors");
}

extern "C" int mdno_unpack_tensors(int count, const mdno_flat_tensor* tensors, const float* flat, void* stream) {
    return run<false>(count, tensors, const_cast<float*>(flat), stream, "mdno_unpack_tensors");
}
