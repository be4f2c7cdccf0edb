// log_f64_ulp.hip — how far is the device's double-precision log from the host's long-double logl on depth ratios?
// depth_eval.hip takes one log(d / g) per pixel; the gates of tests/test_gpu_eval_depth.py on the log sums carry the figure this
// probe prints.  The reference is the host libm in long double, not the code under test.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o log_f64_ulp log_f64_ulp.hip && ./log_f64_ulp
// Ratios: 4,096 spread evenly in log2 over [0.25, 4], 2,049 of the form 1 + k 2^-31 (|q - 1| <= 4.8e-7), 2,048 quotients of
// neighbouring fp32 values (what d / g is when a depth is one or two ulps off its ground truth), and the delta boundaries.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

__global__ void log_kernel(const double* __restrict__ q, double* __restrict__ l, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) l[i] = log(q[i]);
}

#define CHECK(x)                                                                 \
    do {                                                                         \
        hipError_t e__ = (x);                                                    \
        if (e__ != hipSuccess) {                                                 \
            std::printf("%s: %s\n", #x, hipGetErrorString(e__));                 \
            return 2;                                                            \
        }                                                                        \
    } while (0)

int main() {
    std::vector<double> q;
    for (int i = 0; i <= 4095; ++i) q.push_back(std::exp2(-2.0 + 4.0 * i / 4095.0));
    for (int k = -1024; k <= 1024; ++k) q.push_back(1.0 + k * std::ldexp(1.0, -31));
    for (int i = 0; i < 1024; ++i) {
        const float g = 0.5f + 7.5f * (float)i / 1023.f;
        q.push_back((double)std::nextafterf(g, 100.f) / (double)g);
        q.push_back((double)std::nextafterf(std::nextafterf(g, 0.f), 0.f) / (double)g);
    }
    const double edges[] = {1.25, 1.5625, 1.953125, 0.8, 0.64, 0.512, 0.25, 4.0};
    for (double e : edges) q.push_back(e);
    const int n = (int)q.size();
    double *dq = nullptr, *dl = nullptr;
    CHECK(hipMalloc(&dq, n * sizeof(double)));
    CHECK(hipMalloc(&dl, n * sizeof(double)));
    CHECK(hipMemcpy(dq, q.data(), n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(log_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dq, dl, n);
    CHECK(hipGetLastError());
    std::vector<double> l(n);
    CHECK(hipMemcpy(l.data(), dl, n * sizeof(double), hipMemcpyDeviceToHost));
    CHECK(hipFree(dq));
    CHECK(hipFree(dl));
    long double worst = 0, worst_near = 0, worst_host = 0;
    double at = 1.0;
    for (int i = 0; i < n; ++i) {
        const long double ref = logl((long double)q[i]);
        if (ref == 0) {
            if (l[i] != 0.0) { std::printf("log(1) = %a on the device\n", l[i]); return 1; }
            continue;
        }
        int ex;
        std::frexp((double)ref, &ex);                                   // |ref| in [2^(ex-1), 2^ex): one ulp of the result is 2^(ex-53)
        const long double ulp = std::ldexp(1.0L, ex - 53);
        const long double err = fabsl((long double)l[i] - ref) / ulp;
        const long double err_host = fabsl((long double)std::log(q[i]) - ref) / ulp;
        if (err > worst) { worst = err; at = q[i]; }
        if (std::fabs(q[i] - 1.0) <= 1e-6 && err > worst_near) worst_near = err;
        if (err_host > worst_host) worst_host = err_host;
    }
    std::printf("ratios %d  U_dev = %.4Lf ulp (at q = %.17g)  within 1e-6 of 1: %.4Lf ulp  host log: %.4Lf ulp\n", n, worst, at, worst_near,
                worst_host);
    return 0;
}
