// The accuracy of the five fp32 math functions that the chain's step kernels call (csrc/small_kernels.hip: normal4, step_kernel), measured
// on the device over the arguments those kernels can form. ROCm ships no accuracy table on the build hosts, so tests/step_op_cases.py takes
// its allowances (twice what is measured here) from this program's output; DESIGN.md 4b-i records both.
//
//   logf(u)            every u = ((k + 0.5) 2^-23), k = 0 .. 2^23 - 1: all values u01() can return
//   sqrtf(-2 logf(u))  the same u
//   sinf / cosf(ta)    ta = 6.2831855f * u, the same u
//   expf(0.5f * lv)    lv = every float of the file given as argv[1] (the posterior_log_variance_clipped tables the tests install), and
//                      2^22 evenly spaced values of [-46.1, 0] (the clipped range: log(1e-20) .. 0)
//
// Error unit: |fp32 result - float64 result| / ulp(float64 result), ulp(x) = 2^(floor(log2 |x|) - 23). The float64 side is the device's
// double function on the same fp32 argument (its own error is 2^-29 of this unit). Build with the library's flags:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/step_math_ulp.hip -o tools/step_math_ulp
// Prints one JSON line.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(e)                                                                          \
    do {                                                                                  \
        hipError_t err_ = (e);                                                            \
        if (err_ != hipSuccess) {                                                         \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(err_)); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

enum { F_LOG = 0, F_SQRT, F_SIN, F_COS, F_EXP_TABLE, F_EXP_GRID, F_COUNT };

__device__ __forceinline__ double ulps(float got, double ref) {
    const double a = fabs(ref);
    if (!(a > 0.0)) return got == 0.0f ? 0.0 : 1e30;
    return fabs((double)got - ref) / ldexp(1.0, ilogb(a) - 23);
}

__device__ __forceinline__ void keep(unsigned long long* worst, int f, double e) {
    // non-negative doubles order as their bit patterns
    atomicMax(worst + f, (unsigned long long)__double_as_longlong(e));
}

__device__ __forceinline__ float u01(uint32_t k) { return ((float)k + 0.5f) * (1.0f / 8388608.0f); }

__global__ __launch_bounds__(256) void lattice_kernel(unsigned long long* worst) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= (1u << 23)) return;
    const float u = u01(k);
    const float l = logf(u);
    keep(worst, F_LOG, ulps(l, log((double)u)));
    const float a = -2.0f * l;
    keep(worst, F_SQRT, ulps(sqrtf(a), sqrt((double)a)));
    const float ta = 6.28318530717958647692f * u;
    keep(worst, F_SIN, ulps(sinf(ta), sin((double)ta)));
    keep(worst, F_COS, ulps(cosf(ta), cos((double)ta)));
}

__global__ __launch_bounds__(256) void exp_kernel(const float* lv, int n, int grid_n, unsigned long long* worst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float a = 0.5f * lv[i];
        keep(worst, F_EXP_TABLE, ulps(expf(a), exp((double)a)));
    }
    if (i < grid_n) {
        const float a = 0.5f * (-46.1f * (float)i / (float)grid_n);
        keep(worst, F_EXP_GRID, ulps(expf(a), exp((double)a)));
    }
}

int main(int argc, char** argv) {
    std::vector<float> table;
    if (argc > 1) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
        float v;
        while (fread(&v, sizeof v, 1, f) == 1) table.push_back(v);
        fclose(f);
    }
    const int n = (int)table.size(), grid_n = 1 << 22;
    unsigned long long* worst = nullptr;
    float* lv = nullptr;
    CHECK(hipMalloc(&worst, F_COUNT * sizeof(unsigned long long)));
    CHECK(hipMemset(worst, 0, F_COUNT * sizeof(unsigned long long)));
    CHECK(hipMalloc(&lv, (size_t)(n > 0 ? n : 1) * sizeof(float)));
    if (n) CHECK(hipMemcpy(lv, table.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(lattice_kernel, dim3((1u << 23) / 256), dim3(256), 0, nullptr, worst);
    hipLaunchKernelGGL(exp_kernel, dim3(((n > grid_n ? n : grid_n) + 255) / 256), dim3(256), 0, nullptr, lv, n, grid_n, worst);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    unsigned long long bits[F_COUNT];
    CHECK(hipMemcpy(bits, worst, sizeof bits, hipMemcpyDeviceToHost));
    double e[F_COUNT];
    for (int i = 0; i < F_COUNT; ++i) memcpy(&e[i], &bits[i], sizeof(double));
    printf("{\"unit\": \"ulp of the float64 result\", \"logf\": %.4f, \"sqrtf\": %.4f, \"sinf\": %.4f, \"cosf\": %.4f, "
           "\"expf_tables\": %.4f, \"expf_tables_n\": %d, \"expf_grid\": %.4f}\n",
           e[F_LOG], e[F_SQRT], e[F_SIN], e[F_COS], e[F_EXP_TABLE], n, e[F_EXP_GRID]);
    CHECK(hipFree(worst));
    CHECK(hipFree(lv));
    return 0;
}
