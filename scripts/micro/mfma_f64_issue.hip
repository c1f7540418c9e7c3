// Dev microbenchmark: what the chip reaches on v_mfma_f64_16x16x4_f64 when nothing but these MFMAs runs — the yardstick
// for csrc/conformations.hip (EXPERIMENTS.md), whose issue rate is in neither programming guide.  Every wave
// is a chain-free stream of MFMAs on register operands over ACCS independent accumulators (the kernel has nine), WAVES waves
// per SIMD, one workgroup per CU.  Prints time, executed fp64 TFLOP/s (2 * 16 * 16 * 4 flop per MFMA), and the cycles per
// MFMA and SIMD that the time implies at the NOMINAL 2.4 GHz (the clock under load is not read: the TFLOP/s is the figure
// to compare with).
// hipcc --offload-arch=gfx950 -O3 -o mfma_f64_issue mfma_f64_issue.hip
#include <hip/hip_runtime.h>
#include <cstdio>

typedef double f64x4 __attribute__((ext_vector_type(4)));

template <int ACCS>
__global__ __launch_bounds__(512) void issue_kernel(int iters, double* out) {
    const int lane = threadIdx.x & 63;
    const double a = 1e-3 * lane, b = 2e-3 * (lane - 7);
    f64x4 acc[ACCS];
#pragma unroll
    for (int j = 0; j < ACCS; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int j = 0; j < 36; ++j) acc[j % ACCS] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j % ACCS], 0, 0, 0);
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < ACCS; ++j) s += acc[j][0] + acc[j][3];
    if (s == 12345.678) out[0] = s;
}

template <int ACCS>
static void run(int cus, int waves_per_simd, double* out) {
    const int iters = 2000, threads = 256 * waves_per_simd;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    for (int i = 0; i < 2; ++i) issue_kernel<ACCS><<<cus, threads>>>(iters, out);
    hipDeviceSynchronize();
    for (int rep = 0; rep < 3; ++rep) {
        hipEventRecord(e0);
        issue_kernel<ACCS><<<cus, threads>>>(iters, out);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        const double per_simd = (double)waves_per_simd * iters * 36;
        const double flops = (double)cus * 4 * per_simd * 2048.0;
        printf("%d accumulators, %d wave(s)/SIMD: %8.1f us  %6.2f fp64 TFLOP/s  %.1f cycles per MFMA and SIMD at a nominal 2.4 GHz\n", ACCS,
               waves_per_simd, ms * 1e3, flops / ms / 1e9, ms * 1e-3 * 2.4e9 / per_simd);
    }
}

int main() {
    hipDeviceProp_t p;
    hipGetDeviceProperties(&p, 0);
    const int cus = p.multiProcessorCount;
    double* out;
    hipMalloc(&out, 64);
    printf("%s, %d CUs, one workgroup per CU\n", p.name, cus);
    run<1>(cus, 1, out);
    run<2>(cus, 1, out);
    run<4>(cus, 1, out);
    run<9>(cus, 1, out);
    run<9>(cus, 2, out);
    return 0;
}
