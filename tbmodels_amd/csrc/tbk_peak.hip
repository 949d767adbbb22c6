// tbk_peak.hip -- microbenchmark of the sustained v_mfma_f64_16x16x4_f64 rate.
//
// The local hardware guide lists no FP64 matrix peak; AMD's public figure for MI355X is
// 78.6 TFLOP/s.  bench.py reports both the spec and what this loop sustains on the device it runs
// on, so roofline fractions can be read against either.

#include "tbk_internal.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) mfma_f64_loop(double* out, int iters, double seed) {
    d4 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = (d4){0.0, 0.0, 0.0, 0.0};
    double a = seed == 0.0 ? 0.0 : seed + threadIdx.x * 1e-3;
    double b = seed == 0.0 ? 0.0 : seed - threadIdx.x * 1e-3;
    // The whole loop is ONE asm block with the eight accumulators in AGPRs: written with the builtin, hipcc moved all
    // 64 accumulator registers between VGPRs and AGPRs on every trip (128 v_accvgpr moves per 8 MFMAs), and with the
    // accumulators in VGPRs the loop reported 47 TFLOP/s while the H(k) kernel (AGPR accumulators) sustained 68.
    asm volatile(
        "s_mov_b32 s20, %10\n"
        "1:\n"
        "v_mfma_f64_16x16x4_f64 %0, %8, %9, %0\n"
        "v_mfma_f64_16x16x4_f64 %1, %8, %9, %1\n"
        "v_mfma_f64_16x16x4_f64 %2, %8, %9, %2\n"
        "v_mfma_f64_16x16x4_f64 %3, %8, %9, %3\n"
        "v_mfma_f64_16x16x4_f64 %4, %8, %9, %4\n"
        "v_mfma_f64_16x16x4_f64 %5, %8, %9, %5\n"
        "v_mfma_f64_16x16x4_f64 %6, %8, %9, %6\n"
        "v_mfma_f64_16x16x4_f64 %7, %8, %9, %7\n"
        "s_sub_u32 s20, s20, 1\n"
        "s_cmp_lg_u32 s20, 0\n"
        "s_cbranch_scc1 1b\n"
        : "+a"(acc[0]), "+a"(acc[1]), "+a"(acc[2]), "+a"(acc[3]), "+a"(acc[4]), "+a"(acc[5]), "+a"(acc[6]), "+a"(acc[7])
        : "v"(a), "v"(b), "s"(iters)
        : "s20", "scc");
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678) out[blockIdx.x * blockDim.x + threadIdx.x] = s;  // keep the loop alive
}

}  // namespace

int tbk_run_mfma_f64_peak(double* tflops) {
    hipDeviceProp_t prop;
    int dev = 0;
    TBK_HIP(hipGetDevice(&dev));
    TBK_HIP(hipGetDeviceProperties(&prop, dev));
    const int iters = 100000;  // ~20 ms per launch: long enough for the clock to settle
    DevPtr<double> d_out;
    TBK_HIP(hipMalloc(d_out.put(), (size_t)prop.multiProcessorCount * 4 * 256 * sizeof(double)));
    Event e0, e1;
    TBK_HIP(hipEventCreate(e0.put()));
    TBK_HIP(hipEventCreate(e1.put()));
    double best = 0.0;
    // waves per SIMD x {non-trivial operands, all-zero operands}: the chip clocks to its power budget, so
    // the sustained rate depends on both (MI355X_MICROARCH.md, DVFS give-back)
    for (int wps = 1; wps <= 4; wps *= 2) {
        const int grid = prop.multiProcessorCount * wps;
        for (int zero = 0; zero < 2; ++zero) {
            double best_cfg = 0.0;
            for (int rep = 0; rep < 3; ++rep) {
                TBK_HIP(hipEventRecord(e0, 0));
                hipLaunchKernelGGL(mfma_f64_loop, dim3(grid), dim3(256), 0, 0, d_out, iters,
                                   zero ? 0.0 : 1.0 + rep);
                TBK_HIP(hipEventRecord(e1, 0));
                TBK_HIP(hipEventSynchronize(e1));
                float ms = 0.f;
                TBK_HIP(hipEventElapsedTime(&ms, e0, e1));
                const double flops = (double)grid * 4 /*waves*/ * iters * 8.0 * (2.0 * 16 * 16 * 4);
                const double tf = flops / (ms * 1e-3) / 1e12;
                if (rep > 0 && tf > best_cfg) best_cfg = tf;
            }
            if (!zero && best_cfg > best) best = best_cfg;
        }
    }
    *tflops = best;
    return TBK_OK;
}
