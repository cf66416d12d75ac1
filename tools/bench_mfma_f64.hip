// Issue rate of v_mfma_f64_16x16x4_f64 on one GPU: every wavefront runs independent accumulator chains (4 per wave,
// enough to cover the MFMA latency) for ITERS steps; TFLOP/s = 2 * 16 * 16 * 4 * MFMAs / time.  The yardstick of
// k_gram_f64 (icv_pca.hpp): the guides list no f64 MFMA rate.
//     hipcc --offload-arch=gfx950 -O3 -o bench_mfma_f64 tools/bench_mfma_f64.hip && ./bench_mfma_f64
#include <hip/hip_runtime.h>
#include <cstdio>

typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int ITERS = 4096, CHAINS = 4;

__global__ void __launch_bounds__(256) k_mfma_f64(double* out, double a, double b) {
    f64x4 acc[CHAINS];
    for (int c = 0; c < CHAINS; ++c) acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double x = a + threadIdx.x * 1e-9, y = b - threadIdx.x * 1e-9;
    for (int i = 0; i < ITERS; ++i)
#pragma unroll
        for (int c = 0; c < CHAINS; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc[c], 0, 0, 0);
    double s = 0.0;
    for (int c = 0; c < CHAINS; ++c) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

#define CK(e)                                                                           \
    do {                                                                                \
        hipError_t r_ = (e);                                                            \
        if (r_ != hipSuccess) {                                                         \
            std::printf("%s: %s\n", #e, hipGetErrorString(r_));                         \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

int main() {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cu = prop.multiProcessorCount;
    std::printf("device %s, %d CUs\n", prop.name, cu);
    for (int wg_per_cu : {1, 2, 4, 8}) {
        const int grid = cu * wg_per_cu;
        double* out;
        CK(hipMalloc(&out, (size_t)grid * 256 * sizeof(double)));
        hipLaunchKernelGGL(k_mfma_f64, dim3(grid), dim3(256), 0, 0, out, 1.0, 0.5);
        CK(hipDeviceSynchronize());
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0));
        CK(hipEventCreate(&e1));
        float best = 1e30f;
        for (int rep = 0; rep < 5; ++rep) {
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(k_mfma_f64, dim3(grid), dim3(256), 0, 0, out, 1.0, 0.5);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms = 0;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (ms < best) best = ms;
        }
        const double flops = 2.0 * 16 * 16 * 4 * (double)ITERS * CHAINS * (grid * 4.0);
        std::printf("workgroups/CU %d (waves/SIMD %d): best of 5 %.3f ms, %.1f TFLOP/s f64 MFMA\n", wg_per_cu, wg_per_cu,
                    best, flops / (best * 1e-3) / 1e12);
        CK(hipFree(out));
    }
    return 0;
}
