// tsdf_raycast.hip — the fused TSDF volume (tsdf.hip) seen from a camera: per pixel, a ray marched to the first zero crossing of the
// trilinear interpolant; z-depth and, when asked, the surface normal in the camera frame (neuralrgbd_amd/fusion.py: TSDFVolume.raycast,
// FusionVideoStream.render).
//
// No counterpart in the reference.  The operation sequence is written out in include/nrgbd.h and restated in numpy by
// tests/tsdf_raycast_ref.py, which reproduces every stored value bit for bit: fp32, one IEEE operation per operation of the header
// (the library is built with -ffp-contract=off; IEEE divisions and sqrtf), no atomics, no workspace, the volume is only read.
//
// tsdf_raycast_kernel<NORMAL>  one launch, one ray per lane.  A 256-lane workgroup owns a 16 x 16 pixel tile and each of its waves an
//                              8 x 8 quarter of it, so the rays of a wave walk neighbouring voxels and share cache lines.  Per sample
//                              the eight weights of the cell are requested together; the eight TSDF values only where all eight
//                              weights pass (unobserved space costs half the traffic).  All lanes of a wave share the step counter k
//                              and the wave leaves the loop when none of its lanes has a sample left (hit, past z1, or k at the cap).
//                              Bound by the latency of two dependent groups of gathered loads per sample, not by bytes: no LDS, no
//                              scratch (kernel-resource-usage, gfx950, -O3: 42 VGPRs with and without normals).
// tsdf_raycast_kernel<NORMAL, TsdfRayColour>  the same march, and at a hit whose cell passes the weight test (the normal's rule) the
//                              trilinear interpolant of the three colour planes, 24 more gathered loads; (0, 0, 0) elsewhere.  The
//                              colour arguments are an optional parameter pack: without them the kernel is the instruction stream it
//                              was before colour.  44 VGPRs with normals, 46 without, no scratch.
#include "common.hpp"

namespace nrgbd {

constexpr int kRaycastMaxSteps = NRGBD_TSDF_RAYCAST_MAX_STEPS;
constexpr int kRaycastTile = NRGBD_TSDF_RAYCAST_TILE;            // 16: the workgroup's pixel tile; a wave owns an 8 x 8 quarter
constexpr long kRaycastMaxVoxels = 1L << 31;
constexpr float kRayFltMax = 3.402823466e+38f;

struct TsdfView {
    float r[12];                        // float32(extM[:3,:4]) row-major, world -> camera
    float c[3];                         // the camera centre in the world
    float ox, oy, oz, vs;
    float fx, fy, cx, cy;
    float d_near, d_far, w_min, step;
    int X, Y, Z, H, W;
};

struct TsdfCell {
    size_t base;                        // linear index of corner (ix, iy, iz)
    float fx, fy, fz;
};

__device__ __forceinline__ float ray_lerp(float a, float b, float f) { return a + f * (b - a); }

// The cell of grid position p (0 <= p_a <= N_a - 1 on every axis): i_a = min((int)floorf(p_a), N_a - 2), f_a = p_a - (float)i_a.
__device__ __forceinline__ TsdfCell ray_cell(const TsdfView& v, float px, float py, float pz) {
    const int ix = min((int)floorf(px), v.X - 2), iy = min((int)floorf(py), v.Y - 2), iz = min((int)floorf(pz), v.Z - 2);
    TsdfCell c;
    c.base = ((size_t)iz * (size_t)v.Y + (size_t)iy) * (size_t)v.X + (size_t)ix;
    c.fx = px - (float)ix;
    c.fy = py - (float)iy;
    c.fz = pz - (float)iz;
    return c;
}

// The eight corners of a cell, requested together: a[0..7] = (x0 y0 z0) (x1 y0 z0) (x0 y1 z0) (x1 y1 z0) (x0 y0 z1) ... (x1 y1 z1).
__device__ __forceinline__ void ray_corners(const float* __restrict__ a, size_t base, size_t sy, size_t sz, float (&c)[8]) {
    const float* p = a + base;
    c[0] = p[0];       c[1] = p[1];           c[2] = p[sy];      c[3] = p[sy + 1];
    c[4] = p[sz];      c[5] = p[sz + 1];      c[6] = p[sz + sy]; c[7] = p[sz + sy + 1];
}

__device__ __forceinline__ bool ray_observed(const float (&w)[8], float w_min) {                 // a NaN fails
    return w[0] >= w_min && w[1] >= w_min && w[2] >= w_min && w[3] >= w_min && w[4] >= w_min && w[5] >= w_min && w[6] >= w_min &&
           w[7] >= w_min;
}

__device__ __forceinline__ bool ray_inside(const TsdfView& v, float px, float py, float pz) {    // a NaN fails
    return px >= 0.f && px <= (float)(v.X - 1) && py >= 0.f && py <= (float)(v.Y - 1) && pz >= 0.f && pz <= (float)(v.Z - 1);
}

// One axis of the slab test; false: the ray misses the interpolation domain [0, n - 1] of this axis.
__device__ __forceinline__ bool ray_slab(float go, float gd, int n, float& z0, float& z1) {
    const float last = (float)(n - 1);
    if (gd != 0.f) {
        const float ta = (0.f - go) / gd, tb = (last - go) / gd;
        z0 = fmaxf(z0, fminf(ta, tb));
        z1 = fminf(z1, fmaxf(ta, tb));
        return true;
    }
    return go >= 0.f && go <= last;
}

// The trilinear interpolant of eight corners, the nesting T uses: x, then y, then z.
__device__ __forceinline__ float ray_trilinear(const float (&t)[8], const TsdfCell& c) {
    const float c00 = ray_lerp(t[0], t[1], c.fx), c10 = ray_lerp(t[2], t[3], c.fx);
    const float c01 = ray_lerp(t[4], t[5], c.fx), c11 = ray_lerp(t[6], t[7], c.fx);
    return ray_lerp(ray_lerp(c00, c10, c.fy), ray_lerp(c01, c11, c.fy), c.fz);
}

// The coloured form's further kernel arguments; the colourless form has none (an empty pack: the kernel it was before colour).
struct TsdfRayColour {
    const float* color;                 // the volume's planes [3][Z][Y][X]
    float* rgb;                         // [3][H][W]
};

__device__ __forceinline__ TsdfRayColour ray_colour() { return TsdfRayColour(); }
__device__ __forceinline__ const TsdfRayColour& ray_colour(const TsdfRayColour& k) { return k; }

template <bool NORMAL, class... Colour>
__global__ __launch_bounds__(256) void tsdf_raycast_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                           float* __restrict__ depth, float* __restrict__ normal, const TsdfView v,
                                                           const Colour... colour) {
    constexpr bool COLOR = sizeof...(Colour) != 0;
    const TsdfRayColour k = ray_colour(colour...);
    const float* __restrict__ const color = k.color;
    float* __restrict__ const rgb = k.rgb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = (int)blockIdx.x * kRaycastTile + (wave & 1) * 8 + (lane & 7);
    const int py = (int)blockIdx.y * kRaycastTile + (wave >> 1) * 8 + (lane >> 3);
    const bool pixel = px < v.W && py < v.H;
    const size_t sy = (size_t)v.X, sz = (size_t)v.X * (size_t)v.Y;

    const float xn = (((float)px + 0.5f) - v.cx) / v.fx;
    const float yn = (((float)py + 0.5f) - v.cy) / v.fy;
    const float dx = (v.r[0] * xn + v.r[4] * yn) + v.r[8];
    const float dy = (v.r[1] * xn + v.r[5] * yn) + v.r[9];
    const float dz = (v.r[2] * xn + v.r[6] * yn) + v.r[10];
    const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
    const float dzs = v.step / len;
    const float gox = (v.c[0] - v.ox) / v.vs, goy = (v.c[1] - v.oy) / v.vs, goz = (v.c[2] - v.oz) / v.vs;
    const float gdx = dx / v.vs, gdy = dy / v.vs, gdz = dz / v.vs;
    float z0 = v.d_near, z1 = v.d_far;
    bool live = pixel && v.X >= 2 && v.Y >= 2 && v.Z >= 2;
    live = ray_slab(gox, gdx, v.X, z0, z1) && live;
    live = ray_slab(goy, gdy, v.Y, z0, z1) && live;
    live = ray_slab(goz, gdz, v.Z, z0, z1) && live;
    live = live && z0 <= z1;                                        // a NaN fails

    float hit = 0.f;
    bool found = false, have_prev = false;
    float T_prev = 0.f, z_prev = 0.f;
    for (int k = 0; k < kRaycastMaxSteps; ++k) {
        const float zk = z0 + (float)k * dzs;
        live = live && zk <= z1;
        if (__ballot(live) == 0) break;                             // wave-uniform: every lane is done
        if (!live) continue;
        const float sx = gox + zk * gdx, sy_ = goy + zk * gdy, sz_ = goz + zk * gdz;
        bool valid = ray_inside(v, sx, sy_, sz_);
        float T = 0.f;
        if (valid) {
            const TsdfCell c = ray_cell(v, sx, sy_, sz_);
            float w[8];
            ray_corners(weight, c.base, sy, sz, w);
            valid = ray_observed(w, v.w_min);
            if (valid) {
                float t[8];
                ray_corners(tsdf, c.base, sy, sz, t);
                const float c00 = ray_lerp(t[0], t[1], c.fx), c10 = ray_lerp(t[2], t[3], c.fx);
                const float c01 = ray_lerp(t[4], t[5], c.fx), c11 = ray_lerp(t[6], t[7], c.fx);
                T = ray_lerp(ray_lerp(c00, c10, c.fy), ray_lerp(c01, c11, c.fy), c.fz);
            }
        }
        if (valid && have_prev && T_prev > 0.f && T <= 0.f) {
            const float q = T_prev / (T_prev - T);
            hit = z_prev + dzs * q;
            found = true;
            live = false;
            continue;
        }
        have_prev = valid;
        T_prev = T;
        z_prev = zk;
    }
    if (!pixel) return;
    const size_t at = (size_t)py * (size_t)v.W + (size_t)px;
    depth[at] = hit;                                                // 0: no surface
    if (!NORMAL && !COLOR) return;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    float col[3] = {0.f, 0.f, 0.f};
    if (found) {
        const float hx = gox + hit * gdx, hy = goy + hit * gdy, hz = goz + hit * gdz;
        if (ray_inside(v, hx, hy, hz)) {
            const TsdfCell c = ray_cell(v, hx, hy, hz);
            float w[8];
            ray_corners(weight, c.base, sy, sz, w);
            if (ray_observed(w, v.w_min)) {
                if (NORMAL) {
                    float t[8];
                    ray_corners(tsdf, c.base, sy, sz, t);
                    const float gx = ray_lerp(ray_lerp(t[1] - t[0], t[3] - t[2], c.fy), ray_lerp(t[5] - t[4], t[7] - t[6], c.fy), c.fz);
                    const float gy = ray_lerp(ray_lerp(t[2] - t[0], t[3] - t[1], c.fx), ray_lerp(t[6] - t[4], t[7] - t[5], c.fx), c.fz);
                    const float gz = ray_lerp(ray_lerp(t[4] - t[0], t[5] - t[1], c.fx), ray_lerp(t[6] - t[2], t[7] - t[3], c.fx), c.fy);
                    const float g = sqrtf((gx * gx + gy * gy) + gz * gz);
                    if (g > 0.f && g <= kRayFltMax) {                    // a NaN fails
                        const float ux = gx / g, uy = gy / g, uz = gz / g;
                        nx = (v.r[0] * ux + v.r[1] * uy) + v.r[2] * uz;
                        ny = (v.r[4] * ux + v.r[5] * uy) + v.r[6] * uz;
                        nz = (v.r[8] * ux + v.r[9] * uy) + v.r[10] * uz;
                    }
                }
                if (COLOR) {                                         // whatever the gradient is
                    const size_t volume = sz * (size_t)v.Z;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        float t[8];
                        ray_corners(color + j * volume, c.base, sy, sz, t);
                        col[j] = ray_trilinear(t, c);
                    }
                }
            }
        }
    }
    const size_t plane = (size_t)v.H * (size_t)v.W;
    if (NORMAL) {
        normal[at] = nx;
        normal[plane + at] = ny;
        normal[2 * plane + at] = nz;
    }
    if (COLOR) {
        rgb[at] = col[0];
        rgb[plane + at] = col[1];
        rgb[2 * plane + at] = col[2];
    }
}

static bool ray_finite(float x) { return x >= -kRayFltMax && x <= kRayFltMax; }
static bool ray_positive(float x) { return x > 0.f && x <= kRayFltMax; }

}  // namespace nrgbd

namespace nrgbd {

// The checks nrgbd_tsdf_raycast_f32 and its coloured form share, in the documented order, and the view.
static int ray_view(TsdfView& v, int X, int Y, int Z, float ox, float oy, float oz, float voxel_size, const float* pose, const float* centre,
                    float fx, float fy, float cx, float cy, int H, int W, float d_near, float d_far, float w_min, float step) {
    if (X <= 0 || Y <= 0 || Z <= 0 || H <= 0 || W <= 0) return NRGBD_E_SHAPE;
    if ((long)X * Y > kRaycastMaxVoxels || (long)X * Y * Z > kRaycastMaxVoxels) return NRGBD_E_SHAPE;
    if (H > NRGBD_TSDF_RAYCAST_MAX_SIDE || W > NRGBD_TSDF_RAYCAST_MAX_SIDE) return NRGBD_E_SHAPE;
    if (!ray_positive(voxel_size) || !ray_positive(step) || !ray_positive(fx) || !ray_positive(fy)) return NRGBD_E_ARG;
    if (!(d_near < d_far) || w_min != w_min) return NRGBD_E_ARG;    // a NaN bound included
    for (int i = 0; i < 12; ++i) {
        if (!ray_finite(pose[i])) return NRGBD_E_ARG;
        v.r[i] = pose[i];
    }
    for (int i = 0; i < 3; ++i) {
        if (!ray_finite(centre[i])) return NRGBD_E_ARG;
        v.c[i] = centre[i];
    }
    v.ox = ox; v.oy = oy; v.oz = oz; v.vs = voxel_size;
    v.fx = fx; v.fy = fy; v.cx = cx; v.cy = cy;
    v.d_near = d_near; v.d_far = d_far; v.w_min = w_min; v.step = step;
    v.X = X; v.Y = Y; v.Z = Z; v.H = H; v.W = W;
    return NRGBD_OK;
}

}  // namespace nrgbd

// no counterpart in the reference: see the header of this file and include/nrgbd.h
extern "C" int nrgbd_tsdf_raycast_f32(const float* tsdf, const float* weight, int X, int Y, int Z, float ox, float oy, float oz,
                                      float voxel_size, const float* pose, const float* centre, float fx, float fy, float cx, float cy,
                                      int H, int W, float d_near, float d_far, float w_min, float step, float* depth, float* normal,
                                      void* stream) {
    using namespace nrgbd;
    if (!tsdf || !weight || !pose || !centre || !depth) return NRGBD_E_NULL;
    TsdfView v;
    const int rc = ray_view(v, X, Y, Z, ox, oy, oz, voxel_size, pose, centre, fx, fy, cx, cy, H, W, d_near, d_far, w_min, step);
    if (rc != NRGBD_OK) return rc;
    const dim3 grid((unsigned)ceil_div(W, kRaycastTile), (unsigned)ceil_div(H, kRaycastTile));
    if (normal)
        hipLaunchKernelGGL(tsdf_raycast_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, tsdf, weight, depth, normal, v);
    else
        hipLaunchKernelGGL(tsdf_raycast_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, tsdf, weight, depth, normal, v);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

// no counterpart in the reference: the same march, and the trilinear colour at the hit
extern "C" int nrgbd_tsdf_raycast_color_f32(const float* tsdf, const float* weight, const float* color, int X, int Y, int Z, float ox,
                                            float oy, float oz, float voxel_size, const float* pose, const float* centre, float fx,
                                            float fy, float cx, float cy, int H, int W, float d_near, float d_far, float w_min, float step,
                                            float* depth, float* normal, float* rgb, void* stream) {
    using namespace nrgbd;
    if (!tsdf || !weight || !pose || !centre || !depth || !color || !rgb) return NRGBD_E_NULL;
    TsdfView v;
    const int rc = ray_view(v, X, Y, Z, ox, oy, oz, voxel_size, pose, centre, fx, fy, cx, cy, H, W, d_near, d_far, w_min, step);
    if (rc != NRGBD_OK) return rc;
    const dim3 grid((unsigned)ceil_div(W, kRaycastTile), (unsigned)ceil_div(H, kRaycastTile));
    if (normal)
        hipLaunchKernelGGL((tsdf_raycast_kernel<true, TsdfRayColour>), grid, dim3(256), 0, (hipStream_t)stream, tsdf, weight, depth, normal, v,
                           TsdfRayColour{color, rgb});
    else
        hipLaunchKernelGGL((tsdf_raycast_kernel<false, TsdfRayColour>), grid, dim3(256), 0, (hipStream_t)stream, tsdf, weight, depth, normal, v,
                           TsdfRayColour{color, rgb});
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}
