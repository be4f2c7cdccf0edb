// optim.hip — the Adam update of the training loop (train_KVNet.py:228-232: optim.Adam(model_KVnet.parameters(), lr, betas=(.9, .999));
// train_utils/train_KVNet.py:153 optimizer_KV.step()) as ONE kernel type over all 459 parameter tensors.
//
// torch.optim.Adam's default path runs six _foreach_ launches per 30-odd-tensor slab of the parameter list (~50 kernel launches,
// 0.47 ms per iteration at config 4 — the 21 MB of state is a 30 us stream).  Here a launch takes up to 48 tensors BY VALUE in its
// kernel arguments (pointers of parameter / gradient / both moments / step counter, element counts, chunk prefix sums — 2.3 KB of
// kernarg), so nothing is uploaded and the launches can be captured into a hipGraph as they are; a workgroup walks 2,048-element
// chunks of the slab.  459 tensors = 10 launches.
// Arithmetic = torch.optim.adam._single_tensor_adam (non-capturable form), operation for operation in fp32:
//     g' = g (+ weight_decay * p);  m += (g' - m) * (1 - beta1);  v = v * beta2 + (1 - beta2) * g' * g'
//     p -= (lr / (1 - beta1^t)) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps))
// with the scalar factors formed in double on the device from the tensor's own step counter t (a device float, incremented by
// a second tiny launch: parameters that got no gradient in a step — the K-Net on a first frame — are simply not in the list
// and keep their count, as in torch).
//
// Global-norm gradient clipping (train_KVNet.py:143-145,180-181: torch.nn.utils.clip_grad_norm_(parameters, grad_clip_max) before the
// step; ATen: ~460 tensors through _foreach_norm / _foreach_mul_ slabs and a stack + norm) on the same tensor-list idiom:
//     sumsq_kernel     one fp32 partial per 2,048-element chunk, written to workspace[global chunk index] — fixed order inside a chunk
//                      (8 squares per thread added in index order, wave64 shuffle tree, 4 wave sums through LDS in wave order), so the
//                      partials depend neither on the grid nor on which workgroup took which chunk; no atomics
//     norm_finalize    one workgroup adds all partials in a fixed order in double and writes the record clip[4] =
//                      (total_norm, coef = min(1, max_norm / (total_norm + 1e-6)), non-finite flag, 0)
//     adam_clipped_kernel  the Adam update (adam_update<true>) with g * coef folded into the gradient read (one rounded multiply = torch.mul; the gradients in
//                      memory stay as they are); with skip_nonfinite and a non-finite norm nothing is written and no counter advances
//     scale_kernel     t *= coef in place (the free function optim.clip_grad_norm_ for any other optimizer)
// Nothing is allocated, uploaded or synchronised: a hipGraph captures the launches as they are, and the result is the same bits in
// every run.
#include "common.hpp"

namespace nrgbd {

constexpr int kAdamSlab = 48, kAdamChunk = 2048;

struct AdamSlab {
    float* p[kAdamSlab];
    const float* g[kAdamSlab];
    float* m[kAdamSlab];
    float* v[kAdamSlab];
    float* step[kAdamSlab];
    int first_chunk[kAdamSlab + 1];
    int n[kAdamSlab];
    int nt;
};

// The update of both kernels below.  CLIPPED = false is the plain one (nrgbd_adam_step: `clip` and `skip` are not read, and
// adam_kernel keeps the arguments it always had).  CLIPPED = true reads the record of norm_finalize once per workgroup: coef scales
// the gradient as it is read, and with `skip` a non-finite norm leaves p / m / v untouched.
template <bool CLIPPED>
__device__ __forceinline__ void adam_update(const AdamSlab& a, double lr, double beta1, double beta2, double eps, double wd, int maximize,
                                            const float* __restrict__ clip, int skip) {
    float coef = 1.f;
    if (CLIPPED) {
        if (skip && clip[2] != 0.f) return;
        coef = clip[1];
    }
    const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2), epsf = (float)eps, wdf = (float)wd;
    const int nchunks = a.first_chunk[a.nt];
    int ti = 0;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        while (c >= a.first_chunk[ti + 1]) ++ti;            // uniform; chunks of a workgroup come in increasing order
        const double t = (double)a.step[ti][0] + 1.0;
        const float step_size = (float)(lr / (1.0 - pow(beta1, t)));
        const float bc2_sqrt = (float)sqrt(1.0 - pow(beta2, t));
        float* __restrict__ p = a.p[ti];
        const float* __restrict__ g = a.g[ti];
        float* __restrict__ m = a.m[ti];
        float* __restrict__ v = a.v[ti];
        const int n = a.n[ti], base = (c - a.first_chunk[ti]) * kAdamChunk;
#pragma unroll
        for (int j = 0; j < kAdamChunk / 256; ++j) {
            const int i = base + j * 256 + (int)threadIdx.x;
            if (i < n) {
                float gi = g[i];
                if (CLIPPED) gi = gi * coef;             // torch.mul(g, coef): maximize / weight_decay see the scaled gradient
                gi = maximize ? -gi : gi;
                const float pi = p[i];
                if (wdf != 0.f) gi = gi + wdf * pi;
                const float mi = m[i] + (gi - m[i]) * w1;
                const float vi = v[i] * b2 + w2 * gi * gi;
                m[i] = mi; v[i] = vi;
                const float denom = sqrtf(vi) / bc2_sqrt + epsf;
                p[i] = pi - step_size * (mi / denom);
            }
        }
    }
}

__global__ __launch_bounds__(256) void adam_kernel(const AdamSlab a, double lr, double beta1, double beta2, double eps, double wd, int maximize) {
    adam_update<false>(a, lr, beta1, beta2, eps, wd, maximize, nullptr, 0);
}

__global__ __launch_bounds__(256) void adam_clipped_kernel(const AdamSlab a, double lr, double beta1, double beta2, double eps, double wd,
                                                           int maximize, const float* __restrict__ clip, int skip) {
    adam_update<true>(a, lr, beta1, beta2, eps, wd, maximize, clip, skip);
}

__global__ void adam_count_kernel(const AdamSlab a) {
    const int i = threadIdx.x;
    if (i < a.nt) a.step[i][0] += 1.f;
}

__global__ void adam_count_clipped_kernel(const AdamSlab a, const float* __restrict__ clip, int skip) {
    if (skip && clip[2] != 0.f) return;                     // a skipped step is no step: bias correction continues where it was
    const int i = threadIdx.x;
    if (i < a.nt) a.step[i][0] += 1.f;
}

// ---------------------------------------------------------------------------------------------- global gradient norm
struct NormSlab {                   // 780 B of kernarg
    const float* g[kAdamSlab];
    int first_chunk[kAdamSlab + 1];
    int n[kAdamSlab];
    int nt;
};

__global__ __launch_bounds__(256) void sumsq_kernel(const NormSlab a, float* __restrict__ partial) {
    __shared__ float wsum[4];
    const int nchunks = a.first_chunk[a.nt];
    int ti = 0;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        while (c >= a.first_chunk[ti + 1]) ++ti;
        const float* __restrict__ g = a.g[ti];
        const int n = a.n[ti], base = (c - a.first_chunk[ti]) * kAdamChunk;
        float s = 0.f;                                       // elements past the end add nothing: x + 0 is exact
#pragma unroll
        for (int j = 0; j < kAdamChunk / 256; ++j) {
            const int i = base + j * 256 + (int)threadIdx.x;
            const float x = i < n ? g[i] : 0.f;
            const float q = x * x;
            s = j == 0 ? q : s + q;
        }
        s = wave_sum(s);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) partial[c] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void norm_finalize_kernel(const float* __restrict__ partial, int npartial, double max_norm,
                                                            float* __restrict__ clip, float* __restrict__ nonfinite_steps) {
    __shared__ double wsum[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < npartial; i += 256) s += (double)partial[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sum = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        const float total = (float)sqrt(sum);
        const double q = max_norm / ((double)total + 1e-6);
        const float coef = (float)(q < 1.0 ? q : (q != q ? q : 1.0));       // clamp(max = 1): a NaN stays a NaN, as in torch
        const bool bad = !(fabsf(total) <= 3.402823466e+38f);               // inf or NaN
        clip[0] = total; clip[1] = coef; clip[2] = bad ? 1.f : 0.f; clip[3] = 0.f;
        if (bad && nonfinite_steps) nonfinite_steps[0] += 1.f;
    }
}

struct ScaleSlab {
    float* p[kAdamSlab];
    int first_chunk[kAdamSlab + 1];
    int n[kAdamSlab];
    int nt;
};

__global__ __launch_bounds__(256) void scale_kernel(const ScaleSlab a, const float* __restrict__ clip) {
    const float coef = clip[1];
    const int nchunks = a.first_chunk[a.nt];
    int ti = 0;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        while (c >= a.first_chunk[ti + 1]) ++ti;
        float* __restrict__ p = a.p[ti];
        const int n = a.n[ti], base = (c - a.first_chunk[ti]) * kAdamChunk;
#pragma unroll
        for (int j = 0; j < kAdamChunk / 256; ++j) {
            const int i = base + j * 256 + (int)threadIdx.x;
            if (i < n) p[i] = p[i] * coef;
        }
    }
}

// Fills the chunk table of one slab of a tensor list (shared by the three list kernels above); returns the slab's chunk count.
template <typename Slab>
static int fill_chunks(Slab& a, const long* numel, int t0, int ntensors) {
    a.nt = ntensors - t0 < kAdamSlab ? ntensors - t0 : kAdamSlab;
    int chunks = 0;
    for (int i = 0; i < a.nt; ++i) {
        const long n = numel[t0 + i];
        a.n[i] = (int)n;
        a.first_chunk[i] = chunks;
        chunks += (int)((n + kAdamChunk - 1) / kAdamChunk);
    }
    for (int i = a.nt; i <= kAdamSlab; ++i) a.first_chunk[i] = chunks;
    for (int i = a.nt; i < kAdamSlab; ++i) a.n[i] = 0;
    return chunks;
}

// Total chunk count of a tensor list, or a negative code (every element count in (0, 2^30], at most 2^30 chunks).
static long list_chunks(const long* numel, int ntensors) {
    long chunks = 0;
    for (int i = 0; i < ntensors; ++i) {
        if (numel[i] <= 0 || numel[i] > (1L << 30)) return NRGBD_E_SHAPE;
        chunks += (numel[i] + kAdamChunk - 1) / kAdamChunk;
    }
    return chunks > (1L << 30) ? (long)NRGBD_E_SHAPE : chunks;
}

template <bool CLIPPED>
static int adam_launch(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                       float* const* steps, const long* numel, int ntensors, double lr, double beta1, double beta2, double eps,
                       double weight_decay, int maximize, const float* clip, int skip, void* stream) {
    if (ntensors < 0) return NRGBD_E_SHAPE;
    if (ntensors == 0) return NRGBD_OK;
    if (!params || !grads || !exp_avg || !exp_avg_sq || !steps || !numel) return NRGBD_E_NULL;
    for (int t0 = 0; t0 < ntensors; t0 += kAdamSlab) {
        AdamSlab a;
        a.nt = ntensors - t0 < kAdamSlab ? ntensors - t0 : kAdamSlab;
        int chunks = 0;
        for (int i = 0; i < a.nt; ++i) {
            const long n = numel[t0 + i];
            if (!params[t0 + i] || !grads[t0 + i] || !exp_avg[t0 + i] || !exp_avg_sq[t0 + i] || !steps[t0 + i]) return NRGBD_E_NULL;
            if (n <= 0 || n > (1L << 30)) return NRGBD_E_SHAPE;
            a.p[i] = params[t0 + i]; a.g[i] = grads[t0 + i]; a.m[i] = exp_avg[t0 + i]; a.v[i] = exp_avg_sq[t0 + i];
            a.step[i] = steps[t0 + i];
            a.n[i] = (int)n;
            a.first_chunk[i] = chunks;
            chunks += (int)((n + kAdamChunk - 1) / kAdamChunk);
        }
        for (int i = a.nt; i <= kAdamSlab; ++i) a.first_chunk[i] = chunks;
        for (int i = a.nt; i < kAdamSlab; ++i) { a.p[i] = nullptr; a.g[i] = nullptr; a.m[i] = nullptr; a.v[i] = nullptr; a.step[i] = nullptr; a.n[i] = 0; }
        const int grid = chunks < 1024 ? chunks : 1024;
        if constexpr (CLIPPED) {
            hipLaunchKernelGGL(adam_clipped_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, lr, beta1, beta2, eps, weight_decay,
                               maximize, clip, skip);
            hipLaunchKernelGGL(adam_count_clipped_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, clip, skip);
        } else {
            hipLaunchKernelGGL(adam_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, lr, beta1, beta2, eps, weight_decay, maximize);
            hipLaunchKernelGGL(adam_count_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
        }
        NRGBD_CHECK_LAUNCH();
    }
    return NRGBD_OK;
}

}  // namespace nrgbd

extern "C" int nrgbd_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                               float* const* steps, const long* numel, int ntensors, double lr, double beta1, double beta2, double eps,
                               double weight_decay, int maximize, void* stream) {
    return nrgbd::adam_launch<false>(params, grads, exp_avg, exp_avg_sq, steps, numel, ntensors, lr, beta1, beta2, eps, weight_decay, maximize,
                                     nullptr, 0, stream);
}

extern "C" int nrgbd_adam_step_clipped(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                       float* const* steps, const long* numel, int ntensors, double lr, double beta1, double beta2,
                                       double eps, double weight_decay, int maximize, const float* clip, int skip_nonfinite, void* stream) {
    if (!clip) return NRGBD_E_NULL;
    if (skip_nonfinite != 0 && skip_nonfinite != 1) return NRGBD_E_ARG;
    return nrgbd::adam_launch<true>(params, grads, exp_avg, exp_avg_sq, steps, numel, ntensors, lr, beta1, beta2, eps, weight_decay, maximize,
                                    clip, skip_nonfinite, stream);
}

extern "C" long nrgbd_grad_norm_workspace(const long* numel, int ntensors) {
    if (ntensors < 0) return NRGBD_E_SHAPE;
    if (ntensors == 0) return 0;
    if (!numel) return NRGBD_E_NULL;
    const long chunks = nrgbd::list_chunks(numel, ntensors);
    return chunks < 0 ? chunks : chunks * (long)sizeof(float);
}

extern "C" int nrgbd_grad_norm(const float* const* grads, const long* numel, int ntensors, double max_norm, void* workspace,
                               size_t workspace_bytes, float* clip, float* nonfinite_steps, void* stream) {
    using namespace nrgbd;
    if (ntensors < 0 || !(max_norm > 0.0)) return NRGBD_E_SHAPE;         // max_norm <= 0 or NaN
    if (!clip || (ntensors > 0 && (!grads || !numel))) return NRGBD_E_NULL;
    const long total = ntensors > 0 ? list_chunks(numel, ntensors) : 0;
    if (total < 0) return (int)total;
    if (total > 0 && !workspace) return NRGBD_E_NULL;
    if (workspace_bytes < (size_t)total * sizeof(float)) return NRGBD_E_SHAPE;
    for (int i = 0; i < ntensors; ++i)
        if (!grads[i]) return NRGBD_E_NULL;
    float* partial = (float*)workspace;
    int done = 0;
    for (int t0 = 0; t0 < ntensors; t0 += kAdamSlab) {
        NormSlab a;
        const int chunks = fill_chunks(a, numel, t0, ntensors);
        for (int i = 0; i < kAdamSlab; ++i) a.g[i] = i < a.nt ? grads[t0 + i] : nullptr;
        const int grid = chunks < 1024 ? chunks : 1024;
        hipLaunchKernelGGL(sumsq_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, partial + done);
        NRGBD_CHECK_LAUNCH();
        done += chunks;
    }
    hipLaunchKernelGGL(norm_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, (int)total, max_norm, clip,
                       nonfinite_steps);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

extern "C" int nrgbd_scale_tensors(float* const* tensors, const long* numel, int ntensors, const float* clip, void* stream) {
    using namespace nrgbd;
    if (ntensors < 0) return NRGBD_E_SHAPE;
    if (!clip) return NRGBD_E_NULL;
    if (ntensors == 0) return NRGBD_OK;
    if (!tensors || !numel) return NRGBD_E_NULL;
    const long total = list_chunks(numel, ntensors);
    if (total < 0) return (int)total;
    for (int i = 0; i < ntensors; ++i)
        if (!tensors[i]) return NRGBD_E_NULL;
    for (int t0 = 0; t0 < ntensors; t0 += kAdamSlab) {
        ScaleSlab a;
        const int chunks = fill_chunks(a, numel, t0, ntensors);
        for (int i = 0; i < kAdamSlab; ++i) a.p[i] = i < a.nt ? tensors[t0 + i] : nullptr;
        const int grid = chunks < 1024 ? chunks : 1024;
        hipLaunchKernelGGL(scale_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, (const float*)clip);
        NRGBD_CHECK_LAUNCH();
    }
    return NRGBD_OK;
}
