// ulp_probe.hip -- the device's exp and expm1 (double) on a fixed set of non-positive arguments, written to a file for
// tools/ulp_probe.py to compare with NumPy's: the allowance of tol_chi comes from this run.
//   hipcc --offload-arch=gfx950 -O3 tools/ulp_probe.hip -o /tmp/ulp_probe && /tmp/ulp_probe /tmp/ulp.bin && python tools/ulp_probe.py /tmp/ulp.bin
// Arguments: N linear points of (-800, 0) (exp(-|E - mu| / T) down to its underflow) and N logarithmic points of -[1e-12, 1e4]
// (y = (lo - hi) / T).  Output: double [3][2 N]: x, exp(x), expm1(x).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

constexpr int N = 1 << 20;

__global__ void probe(const double* x, double* e, double* m, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    e[i] = exp(x[i]);
    m[i] = expm1(x[i]);
}

#define CHECK(expr)                                                         \
    do {                                                                    \
        hipError_t e_ = (expr);                                             \
        if (e_ != hipSuccess) {                                             \
            std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_)); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: ulp_probe OUTPUT\n");
        return 2;
    }
    std::vector<double> x(2 * N), out(3 * 2 * N);
    for (int i = 0; i < N; ++i) {
        x[i] = -(i + 0.5) * 800.0 / N;
        x[N + i] = -std::pow(10.0, -12.0 + 16.0 * (i + 0.5) / N);
    }
    double *d_x, *d_e, *d_m;
    const size_t bytes = 2 * N * sizeof(double);
    CHECK(hipMalloc(&d_x, bytes));
    CHECK(hipMalloc(&d_e, bytes));
    CHECK(hipMalloc(&d_m, bytes));
    CHECK(hipMemcpy(d_x, x.data(), bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(probe, dim3(2 * N / 256), dim3(256), 0, 0, d_x, d_e, d_m, 2 * N);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(out.data(), d_x, bytes, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(out.data() + 2 * N, d_e, bytes, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(out.data() + 4 * N, d_m, bytes, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_x));
    CHECK(hipFree(d_e));
    CHECK(hipFree(d_m));
    FILE* f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) {
        std::fprintf(stderr, "cannot write %s\n", argv[1]);
        return 1;
    }
    std::fclose(f);
    std::printf("wrote %zu doubles to %s\n", out.size(), argv[1]);
    return 0;
}
