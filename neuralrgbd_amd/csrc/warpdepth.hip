// warpdepth.hip — photometric warp through a per-pixel depth map (local bundle adjustment), forward and backward.
// Replaces warping/homography.py:479-528 (back_warp_th_Rt_msrc) and :530-575 (back_warp_th_Rt); the backward kernel
// replaces what torch autograd builds for ICP/opt_pose_numerical.py:245-294, where the warped sources are differentiated
// w.r.t. the N rigid motions (R_n, t_n) being refined.  Same sampling core as the plane sweep (zeros padding, ATen
// un-normalisation), with X = dmap[p] ray_p instead of a plane: Y = R X + t, P = K Y, (u, v) = P_xy / P_z (no epsilon,
// homography.py:510), g = (u - cx)/cx.  The matrix products are fma chains over k, the order the reference's 4x4 matmuls
// execute on CPU (oracle/nrgbd_oracle.c::depth_warp_coords, pinned against the live reference).  The per-pixel arithmetic lives
// in warp_depth.hpp, shared with the fused loss + gradient of the local bundle adjustment (lba.hip).
// HBM-bound: src [N][C][H][W] is gathered (L2-resident, 4 taps x C), out written once, coalesced along x.
#include "warp_depth.hpp"

namespace nrgbd {

struct DepthWarpArgs {
    const float* src; const float* dmap; const float* K; const float* R; const float* t; const float* rays;
    const float* g_out; float* out; float* partial;
    int N, C, H, W, nwg;
};

// grid (ceil(HW/256), N): one lane = one reference pixel of one view
__global__ __launch_bounds__(256) void warp_depth_fwd_kernel(const DepthWarpArgs a) {
    const size_t hw = (size_t)a.H * a.W;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (p >= hw) return;
    const DepthWarpPoint q = depth_warp_point(a.K, a.R + 9 * n, a.t + 3 * n, a.rays[p], a.rays[hw + p], a.rays[2 * hw + p],
                                              a.dmap[p], a.W, a.H);
    const Bilinear b = bilinear_zeros(q.ix, q.iy, a.W, a.H);
    const size_t onw = (size_t)b.y0 * a.W + b.x0, one = (size_t)b.y0 * a.W + b.x1;
    const size_t osw = (size_t)b.y1 * a.W + b.x0, ose = (size_t)b.y1 * a.W + b.x1;
    for (int c = 0; c < a.C; ++c) {
        const float* pl = a.src + ((size_t)n * a.C + c) * hw;
        a.out[((size_t)n * a.C + c) * hw + p] = lerp4(pl[onw], pl[one], pl[osw], pl[ose], b);
    }
}

// d sum(out g_out) / d(R_n, t_n): per lane the 12 terms dY (x) [X 1], reduced per workgroup into partial[n][wg][12]
__global__ __launch_bounds__(256) void warp_depth_bwd_kernel(const DepthWarpArgs a) {
    __shared__ float red[4][12];
    const size_t hw = (size_t)a.H * a.W;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    float g12[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) g12[i] = 0.f;
    if (p < hw) {
        const DepthWarpPoint q = depth_warp_point(a.K, a.R + 9 * n, a.t + 3 * n, a.rays[p], a.rays[hw + p],
                                                  a.rays[2 * hw + p], a.dmap[p], a.W, a.H);
        const DepthWarpTaps k = depth_warp_taps(q.ix, q.iy, a.W, a.H);   // weights already zero for taps outside the image
        float gix = 0.f, giy = 0.f;
        for (int c = 0; c < a.C; ++c) {
            const float* pl = a.src + ((size_t)n * a.C + c) * hw;
            const float g = a.g_out[((size_t)n * a.C + c) * hw + p];
            depth_warp_tap_grad(k, g, pl[k.onw], pl[k.one], pl[k.osw], pl[k.ose], gix, giy);
        }
        float dY[3];
        depth_warp_dY(a.K, q, gix, giy, a.W, a.H, dY);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            g12[3 * i + 0] = dY[i] * q.X[0]; g12[3 * i + 1] = dY[i] * q.X[1]; g12[3 * i + 2] = dY[i] * q.X[2];
            g12[9 + i] = dY[i];
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const float s = wave_sum(g12[i]);
        if (lane == 0) red[wv][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < 12)
        a.partial[((size_t)n * a.nwg + blockIdx.x) * 12 + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// partial[n][nwg][12] -> g_R[n][9], g_t[n][3]: fixed-order double-precision sum (bitwise reproducible)
__global__ __launch_bounds__(64) void warp_depth_bwd_finalize(const float* __restrict__ partial, int nwg,
                                                              float* __restrict__ g_R, float* __restrict__ g_t) {
    const int n = blockIdx.x, i = threadIdx.x;
    if (i >= 12) return;
    double s = 0.0;
    for (int w = 0; w < nwg; ++w) s += (double)partial[((size_t)n * nwg + w) * 12 + i];
    if (i < 9) g_R[9 * n + i] = (float)s;
    else g_t[3 * n + (i - 9)] = (float)s;
}

}  // namespace nrgbd

extern "C" int nrgbd_warp_depth_fwd(const float* src, const float* dmap, const float* K, const float* R, const float* t,
                                    const float* rays, float* out, int N, int C, int H, int W, void* stream) {
    using namespace nrgbd;
    if (!src || !dmap || !K || !R || !t || !rays || !out) return NRGBD_E_NULL;
    if (N <= 0 || N > 65535 || C <= 0 || H <= 0 || W <= 0) return NRGBD_E_SHAPE;
    DepthWarpArgs a{src, dmap, K, R, t, rays, nullptr, out, nullptr, N, C, H, W, 0};
    hipLaunchKernelGGL(warp_depth_fwd_kernel, dim3(ceil_div((long)H * W, 256), N), dim3(256), 0, (hipStream_t)stream, a);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

extern "C" int nrgbd_warp_depth_bwd_workgroups(int H, int W) { return nrgbd::ceil_div((long)H * W, 256); }

extern "C" int nrgbd_warp_depth_bwd(const float* src, const float* dmap, const float* K, const float* R, const float* t,
                                    const float* rays, const float* g_out, float* partial, float* g_R, float* g_t, int N,
                                    int C, int H, int W, void* stream) {
    using namespace nrgbd;
    if (!src || !dmap || !K || !R || !t || !rays || !g_out || !partial || !g_R || !g_t) return NRGBD_E_NULL;
    if (N <= 0 || N > 65535 || C <= 0 || H <= 0 || W <= 0) return NRGBD_E_SHAPE;
    const int nwg = ceil_div((long)H * W, 256);
    DepthWarpArgs a{src, dmap, K, R, t, rays, g_out, nullptr, partial, N, C, H, W, nwg};
    hipLaunchKernelGGL(warp_depth_bwd_kernel, dim3(nwg, N), dim3(256), 0, (hipStream_t)stream, a);
    NRGBD_CHECK_LAUNCH();
    hipLaunchKernelGGL(warp_depth_bwd_finalize, dim3(N), dim3(64), 0, (hipStream_t)stream, partial, nwg, g_R, g_t);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}
