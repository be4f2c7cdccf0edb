// warp_depth.hpp — the per-pixel arithmetic of the photometric warp through a depth map (warping/homography.py:479-575,
// back_warp_th_Rt_msrc / back_warp_th_Rt) and of its gradient w.r.t. the rigid motion, shared by warpdepth.hip (the
// reference-named operator and its autograd backward) and lba.hip (the fused loss + gradient of the local bundle
// adjustment), so that both compute the same bits.  X = dmap[p] ray_p, Y = R X + t, P = K Y, (u, v) = P_xy / P_z (no epsilon,
// homography.py:510), g = (u - cx)/cx.  The matrix products are fma chains over k, the order the reference's 4x4 matmuls
// execute on CPU (oracle/nrgbd_oracle.c::depth_warp_coords, pinned against the live reference).
#pragma once
#include "common.hpp"

namespace nrgbd {

struct DepthWarpPoint { float X[3], P[3], ix, iy; };

__device__ __forceinline__ DepthWarpPoint depth_warp_point(const float* __restrict__ K, const float* __restrict__ R,
                                                           const float* __restrict__ t, float rx, float ry, float rz,
                                                           float d, int W, int H) {
    DepthWarpPoint q;
    q.X[0] = d * rx; q.X[1] = d * ry; q.X[2] = d * rz;
    float Y[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float s = R[3 * i] * q.X[0];
        s = __builtin_fmaf(R[3 * i + 1], q.X[1], s);
        s = __builtin_fmaf(R[3 * i + 2], q.X[2], s);
        Y[i] = __builtin_fmaf(t[i], 1.0f, s);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float s = K[3 * i] * Y[0];
        s = __builtin_fmaf(K[3 * i + 1], Y[1], s);
        s = __builtin_fmaf(K[3 * i + 2], Y[2], s);
        q.P[i] = s;
    }
    const float u = q.P[0] / q.P[2], v = q.P[1] / q.P[2];
    const float cx = K[2], cy = K[5];
    q.ix = unnormalize((u - cx) / cx, (float)W, false);
    q.iy = unnormalize((v - cy) / cy, (float)H, false);
    return q;
}

// The four taps of a sample position: forward weights (zeroed outside the image) and clamped offsets (bilinear_zeros), plus
// what the backward needs — the fractional position and the in-bounds flag of each tap (ATen grid_sampler_2d_backward adds a
// tap's term only when it is inside).
struct DepthWarpTaps {
    Bilinear b;
    float fx, fy;
    bool v00, v01, v10, v11;
    size_t onw, one, osw, ose;
};

__device__ __forceinline__ DepthWarpTaps depth_warp_taps(float ix, float iy, int W, int H) {
    DepthWarpTaps k;
    k.b = bilinear_zeros(ix, iy, W, H);
    const float x0f = floorf(ix), y0f = floorf(iy);
    k.fx = ix - x0f; k.fy = iy - y0f;
    const float wm = (float)(W - 1), hm = (float)(H - 1);
    const bool vx0 = (x0f >= 0.f) && (x0f <= wm), vx1 = (x0f + 1.f >= 0.f) && (x0f + 1.f <= wm);
    const bool vy0 = (y0f >= 0.f) && (y0f <= hm), vy1 = (y0f + 1.f >= 0.f) && (y0f + 1.f <= hm);
    k.v00 = vx0 && vy0; k.v01 = vx1 && vy0; k.v10 = vx0 && vy1; k.v11 = vx1 && vy1;
    k.onw = (size_t)k.b.y0 * W + k.b.x0; k.one = (size_t)k.b.y0 * W + k.b.x1;
    k.osw = (size_t)k.b.y1 * W + k.b.x0; k.ose = (size_t)k.b.y1 * W + k.b.x1;
    return k;
}

// One channel's contribution g * d(sample)/d(ix, iy) to (gix, giy); a00..a11 are the raw loads at the clamped offsets.
__device__ __forceinline__ void depth_warp_tap_grad(const DepthWarpTaps& k, float g, float a00, float a01, float a10, float a11,
                                                    float& gix, float& giy) {
    const float v00 = k.v00 ? a00 : 0.f, v01 = k.v01 ? a01 : 0.f;
    const float v10 = k.v10 ? a10 : 0.f, v11 = k.v11 ? a11 : 0.f;
    gix = __builtin_fmaf(g, __builtin_fmaf(v11 - v10, k.fy, (v01 - v00) * (1.f - k.fy)), gix);
    giy = __builtin_fmaf(g, __builtin_fmaf(v11 - v01, k.fx, (v10 - v00) * (1.f - k.fx)), giy);
}

// (d/d ix, d/d iy) -> dY = K^T dP through the un-normalisation and the perspective division; the pose gradient of the pixel
// is then dY (x) [X 1].
__device__ __forceinline__ void depth_warp_dY(const float* __restrict__ K, const DepthWarpPoint& q, float gix, float giy,
                                              int W, int H, float dY[3]) {
    const float cx = K[2], cy = K[5];
    const float du = gix * (0.5f * (float)W) / cx, dv = giy * (0.5f * (float)H) / cy;
    const float ipz = 1.f / q.P[2];
    const float dP0 = du * ipz, dP1 = dv * ipz, dP2 = -(du * q.P[0] + dv * q.P[1]) * ipz * ipz;
#pragma unroll
    for (int i = 0; i < 3; ++i) dY[i] = K[i] * dP0 + K[3 + i] * dP1 + K[6 + i] * dP2;   // (K^T dP)_i
}

}  // namespace nrgbd
