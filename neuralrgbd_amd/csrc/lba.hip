// lba.hip — the local bundle adjustment (pose refinement) of ICP/opt_pose_numerical.py as three kernel types.
// Replaces the Adam loop of _opt_pose_warping (:28-170) / _opt_pose_warping_parallel (:172-303) and the pyramids of
// local_BA_direct(_parallel) (:306-417, mutils/misc.py:139 downsample_img).  Per iteration the reference runs the quaternion
// chain as scalar ATen ops, the warp, a mask, the L1 loss and their backward as separate kernels, a second gather pass for the
// pose gradient and torch.optim.Adam; here an iteration is TWO launches and stays on the device:
//   lba_grad_kernel    one (view, pixel) per lane, grid-stride over the pixels: project, load the 4 taps x 3 channels once,
//                      warped value, mask (warped != 0), residual r = w c - ref c, |r| and sign(r) c into the bilinear
//                      backward, the 12 products dY (x) [X 1]; workgroup partials [N][nwg][13] (12 pose terms, sum |r|).
//                      nwg <= kLbaMaxWg whatever the image size, so the serial reduction below stays short.
//   lba_update_kernel  ONE workgroup: fixed-order reduction of the partials (double, bitwise reproducible), the normaliser
//                      (nn.L1Loss mean), the chain rule dL/dR -> dL/duq through unitQ_to_quat + quaternion2Rotation
//                      (mutils/misc.py:459, :295: s = 1/|q|^2 on the diagonal only), the Adam step (optim.hip's arithmetic,
//                      torch.optim.adam._single_tensor_adam), R rebuilt from the new uq in the reference's fp32 operation
//                      order, and the loss appended to a device log.
// plus lba_pyramid_kernel, every avg_pool2d level of every plane in one launch.  No cross-workgroup waiting; no host sync.
#include "warp_depth.hpp"

namespace nrgbd {

constexpr int kLbaMaxWg = 256;                                 // workgroups per view of lba_grad_kernel (grid-stride beyond)
constexpr int kLbaMaxPlanes = 5 + 3 * NRGBD_MAX_V;            // ref (3) + sources (3 N) + depth + confidence

struct LbaPyramidArgs {
    const float* planes[kLbaMaxPlanes];
    float* out;
    long off[NRGBD_LBA_MAX_LEVELS + 1];                        // element offset of each level's block in out
    int k[NRGBD_LBA_MAX_LEVELS], h[NRGBD_LBA_MAX_LEVELS], w[NRGBD_LBA_MAX_LEVELS];
    int nplanes, nlevels, H, W;
};

// out[level][plane][y][x] = F.avg_pool2d(plane, k): the k x k window summed row by row in fp32, divided by k*k (ATen's CPU
// order); k = 1 copies (downsample_img returns its input).  Every level is pooled from the full-resolution plane.
__global__ __launch_bounds__(256) void lba_pyramid_kernel(const LbaPyramidArgs a) {
    const long total = a.off[a.nlevels];
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        int l = 0;
        while (e >= a.off[l + 1]) ++l;
        const long local = e - a.off[l];
        const int h = a.h[l], w = a.w[l], k = a.k[l];
        const long hw = (long)h * w;
        const int pl = (int)(local / hw);
        const int rem = (int)(local - (long)pl * hw);
        const int y = rem / w, x = rem - y * w;
        const float* src = a.planes[pl] + (size_t)y * k * a.W + (size_t)x * k;
        float s = 0.f;
        for (int dy = 0; dy < k; ++dy)
            for (int dx = 0; dx < k; ++dx) s += src[(size_t)dy * a.W + dx];
        a.out[e] = s / (float)(k * k);
    }
}

struct LbaGradArgs {
    const float* ref; const float* src; const float* dmap; const float* conf; const float* K; const float* rays;
    const float* state; float* partial;
    int N, H, W, nwg;
};

// grid (nwg, N): sum over the pixels of view n of |r| and of sign(r) c d(warped)/d(R_n, t_n), r = warped c - ref c where
// warped != 0 (per channel, opt_pose_numerical.py:258-266).  The normaliser is applied by lba_update_kernel.
__global__ __launch_bounds__(256) void lba_grad_kernel(const LbaGradArgs a) {
    __shared__ float red[4][13];
    const size_t hw = (size_t)a.H * a.W;
    const int n = blockIdx.y;
    const float* __restrict__ R = a.state + (size_t)NRGBD_LBA_STATE * n + 6;
    const float* __restrict__ t = a.state + (size_t)NRGBD_LBA_STATE * n + 3;
    float acc[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) acc[i] = 0.f;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < hw; p += (size_t)a.nwg * 256) {
        const DepthWarpPoint q = depth_warp_point(a.K, R, t, a.rays[p], a.rays[hw + p], a.rays[2 * hw + p], a.dmap[p], a.W, a.H);
        const DepthWarpTaps k = depth_warp_taps(q.ix, q.iy, a.W, a.H);
        const float c = a.conf[p];
        float gix = 0.f, giy = 0.f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* pl = a.src + ((size_t)n * 3 + ch) * hw;
            const float a00 = pl[k.onw], a01 = pl[k.one], a10 = pl[k.osw], a11 = pl[k.ose];
            const float wv = lerp4(a00, a01, a10, a11, k.b);               // = warp_depth_fwd's value
            if (wv != 0.f) {                                                // mask_img = 1 - (warped == 0)
                const float r = wv * c - a.ref[(size_t)ch * hw + p] * c;
                acc[12] += fabsf(r);
                const float g = r > 0.f ? c : (r < 0.f ? -c : 0.f);        // sign(0) = 0
                depth_warp_tap_grad(k, g, a00, a01, a10, a11, gix, giy);
            }
        }
        float dY[3];
        depth_warp_dY(a.K, q, gix, giy, a.W, a.H, dY);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            acc[3 * i + 0] = __builtin_fmaf(dY[i], q.X[0], acc[3 * i + 0]);
            acc[3 * i + 1] = __builtin_fmaf(dY[i], q.X[1], acc[3 * i + 1]);
            acc[3 * i + 2] = __builtin_fmaf(dY[i], q.X[2], acc[3 * i + 2]);
            acc[9 + i] += dY[i];
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 13; ++i) {
        const float s = wave_sum(acc[i]);
        if (lane == 0) red[wv][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < 13)
        a.partial[((size_t)n * a.nwg + blockIdx.x) * 13 + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// R = quaternion2Rotation(unitQ_to_quat(uq)) in the reference's fp32 operation order (mutils/misc.py:459-472, :295-331;
// the library is built with -ffp-contract=off, so every product and sum below is rounded on its own like the ATen ops).
__device__ __forceinline__ void lba_uq_to_R(const float* uq, float* R) {
    const float ux = uq[0], uy = uq[1], uz = uq[2];
    const float al = ux * ux + uy * uy + uz * uz;
    const float w = (2.f * ux) / (al + 1.f), x = (2.f * uy) / (al + 1.f), y = (2.f * uz) / (al + 1.f);
    const float z = (1.f - al) / (1.f + al);
    const float s = 1.f / (w * w + x * x + y * y + z * z);
    R[0] = 1.f - 2.f * s * (y * y + z * z);
    R[4] = 1.f - 2.f * s * (x * x + z * z);
    R[8] = 1.f - 2.f * s * (x * x + y * y);
    R[1] = 2.f * (x * y - w * z);
    R[3] = 2.f * (x * y + w * z);
    R[2] = 2.f * (x * z + w * y);
    R[6] = 2.f * (x * z - w * y);
    R[5] = 2.f * (y * z - w * x);
    R[7] = 2.f * (y * z + w * x);
}

// dL/duq from G = dL/dR [3][3] (row-major) at uq, in double: the derivative autograd takes through the two functions above,
// s included (w = q[3], x = q[0], y = q[1], z = q[2]; unitQ_to_quat puts uq_x into w).
__device__ __forceinline__ void lba_grad_uq(const float* uq, const double* G, double* g) {
    const double a0 = uq[0], a1 = uq[1], a2 = uq[2];
    const double A = a0 * a0 + a1 * a1 + a2 * a2, D = A + 1.0;
    const double w = 2.0 * a0 / D, x = 2.0 * a1 / D, y = 2.0 * a2 / D, z = (1.0 - A) / D;
    const double s = 1.0 / (w * w + x * x + y * y + z * z);
    const double dLds = -2.0 * (G[0] * (y * y + z * z) + G[4] * (x * x + z * z) + G[8] * (x * x + y * y));
    const double dLdn = -dLds * s * s;                                  // n = |q|^2, s = 1/n
    const double gw = dLdn * 2.0 * w + 2.0 * (-G[1] * z + G[3] * z + G[2] * y - G[6] * y - G[5] * x + G[7] * x);
    const double gx = dLdn * 2.0 * x - 4.0 * s * x * (G[4] + G[8]) +
                      2.0 * (G[1] * y + G[3] * y + G[2] * z + G[6] * z - G[5] * w + G[7] * w);
    const double gy = dLdn * 2.0 * y - 4.0 * s * y * (G[0] + G[8]) +
                      2.0 * (G[1] * x + G[3] * x + G[2] * w - G[6] * w + G[5] * z + G[7] * z);
    const double gz = dLdn * 2.0 * z - 4.0 * s * z * (G[0] + G[4]) +
                      2.0 * (-G[1] * w + G[3] * w + G[2] * x + G[6] * x + G[5] * y + G[7] * y);
    const double dot = gw * a0 + gx * a1 + gy * a2;
    const double D2 = D * D;
    g[0] = 2.0 * gw / D - 4.0 * a0 * (dot + gz) / D2;
    g[1] = 2.0 * gx / D - 4.0 * a1 * (dot + gz) / D2;
    g[2] = 2.0 * gy / D - 4.0 * a2 * (dot + gz) / D2;
}

// One Adam element: optim.hip's arithmetic (torch.optim.adam._single_tensor_adam, fp32, betas .9 / .999, eps 1e-8).
__device__ __forceinline__ void lba_adam(float& p, float& m, float& v, float g, float step_size, float bc2_sqrt) {
    const float w1 = (float)(1.0 - 0.9), b2 = (float)0.999, w2 = (float)(1.0 - 0.999), eps = (float)1e-8;
    m = m + (g - m) * w1;
    v = v * b2 + w2 * g * g;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p - step_size * (m / denom);
}

struct LbaUpdateArgs {
    const float* partial; const float* init; float* state; float* loss_log;
    double lr;
    int nwg, N, joint, step, opt_R, opt_t, log_stride, log_slot;
    double norm;                                               // nn.L1Loss's element count: 3 h w (x N when joint)
};

// ONE workgroup of 256.  step 0: state <- init (uq, t), moments 0, R from uq.  step >= 1: reduce, log, Adam step number `step`.
// Reduction: thread w takes workgroup row w of every view (all its loads independent: one memory latency, not nwg / 64 of them),
// then a fixed tree — the double xor tree inside each wave, the four wave sums in a fixed order.
__global__ __launch_bounds__(256) void lba_update_kernel(const LbaUpdateArgs a) {
    __shared__ double wsum[4][NRGBD_MAX_V][13];
    __shared__ double red[NRGBD_MAX_V][13];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (a.step > 0) {
        const int w = threadIdx.x;
        for (int n0 = 0; n0 < a.N; n0 += 4) {                      // four views' loads in flight at once
            float v[4][13];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 13; ++i)
                    v[j][i] = (w < a.nwg && n0 + j < a.N) ? a.partial[((size_t)(n0 + j) * a.nwg + w) * 13 + i] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (n0 + j >= a.N) break;
#pragma unroll
                for (int i = 0; i < 13; ++i) {
                    const double s = wave_sum((double)v[j][i]);
                    if (lane == 0) wsum[wv][n0 + j][i] = s;
                }
            }
        }
        __syncthreads();
        for (int pr = threadIdx.x; pr < a.N * 13; pr += 256) {
            const int n = pr / 13, i = pr - 13 * n;
            red[n][i] = (wsum[0][n][i] + wsum[1][n][i]) + (wsum[2][n][i] + wsum[3][n][i]);
        }
        __syncthreads();
    }
    const int n = threadIdx.x;
    if (n >= a.N) return;
    float* st = a.state + (size_t)NRGBD_LBA_STATE * n;
    if (a.step == 0) {
        for (int i = 0; i < 6; ++i) st[i] = a.init[6 * n + i];
        for (int i = 15; i < 27; ++i) st[i] = 0.f;
        lba_uq_to_R(st, st + 6);
        return;
    }
    if (a.joint) {
        if (n == 0) {
            double l = 0.0;
            for (int j = 0; j < a.N; ++j) l += red[j][12];
            a.loss_log[a.log_slot] = (float)(l / a.norm);
        }
    } else {
        a.loss_log[(size_t)n * a.log_stride + a.log_slot] = (float)(red[n][12] / a.norm);
    }
    const double t = (double)a.step;
    const float step_size = (float)(a.lr / (1.0 - pow(0.9, t)));
    const float bc2_sqrt = (float)sqrt(1.0 - pow(0.999, t));
    if (a.opt_t) {
        for (int i = 0; i < 3; ++i)
            lba_adam(st[3 + i], st[15 + i], st[18 + i], (float)(red[n][9 + i] / a.norm), step_size, bc2_sqrt);
    }
    if (a.opt_R) {
        double G[9], g[3];
        for (int i = 0; i < 9; ++i) G[i] = red[n][i] / a.norm;
        lba_grad_uq(st, G, g);
        for (int i = 0; i < 3; ++i) lba_adam(st[i], st[21 + i], st[24 + i], (float)g[i], step_size, bc2_sqrt);
        lba_uq_to_R(st, st + 6);
    }
}

}  // namespace nrgbd

extern "C" int nrgbd_lba_pyramid(const float* const* planes, int nplanes, int H, int W, const int* ks, int nlevels, float* out,
                                 void* stream) {
    using namespace nrgbd;
    if (!planes || !ks || !out) return NRGBD_E_NULL;
    if (nplanes <= 0 || nplanes > kLbaMaxPlanes || nlevels <= 0 || nlevels > NRGBD_LBA_MAX_LEVELS || H <= 0 || W <= 0)
        return NRGBD_E_SHAPE;
    LbaPyramidArgs a;
    a.out = out; a.nplanes = nplanes; a.nlevels = nlevels; a.H = H; a.W = W;
    for (int i = 0; i < kLbaMaxPlanes; ++i) {
        if (i < nplanes && !planes[i]) return NRGBD_E_NULL;
        a.planes[i] = i < nplanes ? planes[i] : nullptr;
    }
    a.off[0] = 0;
    for (int l = 0; l < NRGBD_LBA_MAX_LEVELS; ++l) {
        const int k = l < nlevels ? ks[l] : 1;
        if (k <= 0) return NRGBD_E_SHAPE;
        a.k[l] = k; a.h[l] = H / k; a.w[l] = W / k;
        if (l < nlevels && (a.h[l] == 0 || a.w[l] == 0)) return NRGBD_E_SHAPE;
        a.off[l + 1] = a.off[l] + (l < nlevels ? (long)nplanes * a.h[l] * a.w[l] : 0);
    }
    const long blocks = (a.off[nlevels] + 255) / 256;
    hipLaunchKernelGGL(lba_pyramid_kernel, dim3(blocks < 4096 ? (int)blocks : 4096), dim3(256), 0, (hipStream_t)stream, a);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

extern "C" int nrgbd_lba_workgroups(int H, int W) {
    const int n = nrgbd::ceil_div((long)H * W, 256);
    return n < nrgbd::kLbaMaxWg ? n : nrgbd::kLbaMaxWg;
}

extern "C" int nrgbd_lba_grad(const float* ref, const float* src, const float* dmap, const float* conf, const float* K,
                              const float* rays, const float* state, float* partial, int N, int H, int W, void* stream) {
    using namespace nrgbd;
    if (!ref || !src || !dmap || !conf || !K || !rays || !state || !partial) return NRGBD_E_NULL;
    if (N <= 0 || N > NRGBD_MAX_V || H <= 0 || W <= 0) return NRGBD_E_SHAPE;
    const int nwg = nrgbd_lba_workgroups(H, W);
    LbaGradArgs a{ref, src, dmap, conf, K, rays, state, partial, N, H, W, nwg};
    hipLaunchKernelGGL(lba_grad_kernel, dim3(nwg, N), dim3(256), 0, (hipStream_t)stream, a);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

extern "C" int nrgbd_lba_update(const float* partial, int nwg, const float* init, float* state, float* loss_log, int log_stride,
                                int log_slot, int N, int H, int W, int joint, int step, double lr, int opt_R, int opt_t,
                                void* stream) {
    using namespace nrgbd;
    if (!state) return NRGBD_E_NULL;
    if (step == 0 && !init) return NRGBD_E_NULL;
    if (step > 0 && (!partial || !loss_log)) return NRGBD_E_NULL;
    if (N <= 0 || N > NRGBD_MAX_V || H <= 0 || W <= 0 || nwg <= 0 || nwg > kLbaMaxWg || step < 0 || log_slot < 0 ||
        (!joint && log_slot >= log_stride))
        return NRGBD_E_SHAPE;
    if ((joint != 0 && joint != 1) || (opt_R != 0 && opt_R != 1) || (opt_t != 0 && opt_t != 1)) return NRGBD_E_ARG;
    LbaUpdateArgs a;
    a.partial = partial; a.init = init; a.state = state; a.loss_log = loss_log; a.lr = lr;
    a.nwg = nwg; a.N = N; a.joint = joint; a.step = step; a.opt_R = opt_R; a.opt_t = opt_t;
    a.log_stride = log_stride; a.log_slot = log_slot;
    a.norm = 3.0 * (double)H * (double)W * (joint ? (double)N : 1.0);
    hipLaunchKernelGGL(lba_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}
