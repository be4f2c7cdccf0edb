// resample.hpp — the per-voxel body of the rigid 3-D resample of a depth-probability volume: ONE piece of source for
// resample.hip (which writes the resampled volume, PREDICT) and keyframe.hip (which reduces it over the candidates on the
// fly, the LBA keyframe maps), the way warp_depth.hpp serves warpdepth.hip and lba.hip.  Every operation below is in the
// reference's order (warping/homography.py:673-716 and ATen's GridSampler); the library is compiled with
// -ffp-contract=off, so both users get the same bits.
#pragma once
#include "common.hpp"

namespace nrgbd {

struct ResampleArgs {
    const float* dpv; const float* T; const float* rays; const float* d_candi;
    float* out;
    float tan_hh, tan_hv, z_half, z_radius, pad, lo, hi;
    int do_clamp, D, h, w;   // D = planes of the source volume; the number of output planes (d_candi's length) is the launch's
};

// ATen GridSampler.h clip_coordinates: min(size-1, max(x, 0)) with std::min/max NaN behaviour
__device__ __forceinline__ float clip_border(float x, float hi) {
    x = (x < 0.f) ? 0.f : x;
    return (x < hi) ? x : hi;
}

// The resampled (and clamped) value at the point d * ray, ray = (rx, ry, rz), of the bordered source volume a.dpv.
// Every tap index is clipped into the volume (a NaN / infinite coordinate lands on size-1), so no load leaves it.
__device__ __forceinline__ float dpv_resample_voxel(const ResampleArgs& a, float rx, float ry, float rz, float d) {
    // homography.py:679-682  X = d * ray
    const float X = d * rx, Y = d * ry, Z = d * rz;
    // :698-702  rel_extM @ [X Y Z 1]^T  (K=4 fma chain)
    float q[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float acc = a.T[4 * r] * X;
        acc = __builtin_fmaf(a.T[4 * r + 1], Y, acc);
        acc = __builtin_fmaf(a.T[4 * r + 2], Z, acc);
        acc = __builtin_fmaf(a.T[4 * r + 3], 1.f, acc);
        q[r] = acc;
    }
    // :705-710
    const float den = q[2] + 1e-10f;
    const float wq = q[3] + 1e-10f;
    const float gx = ((q[0] / den) / a.tan_hh) / wq;
    const float gy = ((q[1] / den) / a.tan_hv) / wq;
    const float gz = ((q[2] - a.z_half) / a.z_radius) / wq;
    // :716  F.grid_sample 3-D: bilinear, padding 'border', align_corners=False
    const float fx = clip_border(unnormalize(gx, (float)a.w, false), (float)(a.w - 1));
    const float fy = clip_border(unnormalize(gy, (float)a.h, false), (float)(a.h - 1));
    const float fz = clip_border(unnormalize(gz, (float)a.D, false), (float)(a.D - 1));
    const float x0f = floorf(fx), y0f = floorf(fy), z0f = floorf(fz);
    const int x0 = (int)x0f, y0 = (int)y0f, z0 = (int)z0f;
    const float ex = (x0f + 1.f) - fx, ey = (y0f + 1.f) - fy, ez = (z0f + 1.f) - fz;
    const float wx = fx - x0f, wy = fy - y0f, wz = fz - z0f;

    // a tap on one of the 6 faces reads pad (:873-887); a tap beyond size-1 is dropped
    auto tap = [&](int zz, int yy, int xx) -> float {
        const bool face = (zz == 0) | (yy == 0) | (xx == 0) | (zz == a.D - 1) | (yy == a.h - 1) | (xx == a.w - 1);
        return face ? a.pad : a.dpv[((size_t)zz * a.h + yy) * a.w + xx];
    };
    const bool vx1 = x0 + 1 < a.w, vy1 = y0 + 1 < a.h, vz1 = z0 + 1 < a.D;
    const int x1 = vx1 ? x0 + 1 : x0, y1 = vy1 ? y0 + 1 : y0, z1 = vz1 ? z0 + 1 : z0;
    float acc = 0.f;
    acc += tap(z0, y0, x0) * (ex * ey * ez);
    if (vx1) acc += tap(z0, y0, x1) * (wx * ey * ez);
    if (vy1) acc += tap(z0, y1, x0) * (ex * wy * ez);
    if (vx1 && vy1) acc += tap(z0, y1, x1) * (wx * wy * ez);
    if (vz1) acc += tap(z1, y0, x0) * (ex * ey * wz);
    if (vz1 && vx1) acc += tap(z1, y0, x1) * (wx * ey * wz);
    if (vz1 && vy1) acc += tap(z1, y1, x0) * (ex * wy * wz);
    if (vz1 && vx1 && vy1) acc += tap(z1, y1, x1) * (wx * wy * wz);
    if (a.do_clamp) acc = fminf(fmaxf(acc, a.lo), a.hi);
    return acc;
}

}  // namespace nrgbd
