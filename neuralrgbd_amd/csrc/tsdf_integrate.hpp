// tsdf_integrate.hpp — what the integration of a depth frame (tsdf.hip, nrgbd_tsdf_integrate_f32 and its coloured form) and its
// inverse (tsdf_reint.hip, nrgbd_tsdf_reintegrate_f32: a frame taken out of the volume and put back at another pose) share: the frame,
// the per-voxel chain up to (t, w), the colour pixel, the running average and its inverse, the lane group's update built from them
// (tsdf_update_group), the entries' argument checks and the launch grid.  They exist once, here, so that what one launch adds is what
// the other removes, bit for bit.
#pragma once
#include "tsdf_extract.hpp"      // kFltMax, tsdf_voxels, tsdf_positive

namespace nrgbd {

struct TsdfFrame {
    float r[12];                        // float32(extM[:3,:4]) row-major: r00 r01 r02 tx | r10 r11 r12 ty | r20 r21 r22 tz
    float ox, oy, oz, vs;
    float fx, fy, cx, cy;
    float trunc, d_near, d_far, w_max, gate_thr;
    int X, Y, H, W;
    int x0, y0, z0, x1, y1, z1;         // half-open voxel box
};

// What does not depend on x: the lattice row's contribution to the three camera coordinates.
struct TsdfRow {
    float bx, cx, by, cy, bz, cz;       // r01 yw, r02 zw | r11 yw, r12 zw | r21 yw, r22 zw
};

__device__ __forceinline__ TsdfRow tsdf_row(const TsdfFrame& f, int iy, int iz) {
    const float yw = f.oy + f.vs * (float)iy;
    const float zw = f.oz + f.vs * (float)iz;
    TsdfRow r;
    r.bx = f.r[1] * yw; r.cx = f.r[2] * zw;
    r.by = f.r[5] * yw; r.cy = f.r[6] * zw;
    r.bz = f.r[9] * yw; r.cz = f.r[10] * zw;
    return r;
}

// The colour image of nrgbd_tsdf_integrate_color_f32: its size and intrinsics, the affine c = image * a + b per channel.
struct TsdfImage {
    float fx, fy, cx, cy;
    float a[3], b[3];
    int H, W;
    size_t volume;                      // X Y Z: the distance between two colour planes
};

// The chain of include/nrgbd.h up to t and w for lattice column ix of a row; false: the voxel is skipped.  COLOR: the two quotients of
// the projection as well (xq = xc / zc, yq = yc / zc: the colour image is projected with the same ones).
template <bool COLOR>
__device__ __forceinline__ bool tsdf_observe(const TsdfFrame& f, const TsdfRow& row, int ix, const float* __restrict__ depth,
                                             const float* __restrict__ gate, const float* __restrict__ wmap, float& t, float& w,
                                             float& xq, float& yq) {
    const float xw = f.ox + f.vs * (float)ix;
    const float xc = ((f.r[0] * xw + row.bx) + row.cx) + f.r[3];
    const float yc = ((f.r[4] * xw + row.by) + row.cy) + f.r[7];
    const float zc = ((f.r[8] * xw + row.bz) + row.cz) + f.r[11];
    if (!(zc > 0.f)) return false;
    const float xz = xc / zc, yz = yc / zc;
    const float u = f.fx * xz + f.cx;
    const float v = f.fy * yz + f.cy;
    if (COLOR) {
        xq = xz;
        yq = yz;
    }
    if (!(u >= 0.f && u < (float)f.W && v >= 0.f && v < (float)f.H)) return false;       // a NaN fails
    const int iu = (int)floorf(u), iv = (int)floorf(v);                                  // 0 <= iu < W, 0 <= iv < H
    const size_t p = (size_t)iv * (size_t)f.W + (size_t)iu;
    const float d = depth[p];
    if (!(fabsf(d) <= kFltMax && d > f.d_near && d <= f.d_far)) return false;
    if (gate && !(gate[p] >= f.gate_thr)) return false;
    w = wmap ? wmap[p] : 1.f;
    if (!(w <= kFltMax && w > 0.f)) return false;
    const float s = d - zc;
    if (s < -f.trunc) return false;
    t = fminf(1.f, s / f.trunc);
    return true;
}

__device__ __forceinline__ void tsdf_average(float& T, float& Wt, float t, float w, float w_max) {
    T = (T * Wt + t * w) / (Wt + w);
    Wt = fminf(Wt + w, w_max);
}

// The pixel of the colour image a voxel sees (clamped into the image: colour never vetoes a distance update), through the affine.
// false: one of the three values is not finite and the voxel's colour keeps its bits.
__device__ __forceinline__ bool tsdf_colour(const TsdfImage& m, const float* __restrict__ image, float xq, float yq, float (&c)[3]) {
    float uc = m.fx * xq + m.cx;
    float vc = m.fy * yq + m.cy;
    uc = fminf(fmaxf(uc, 0.f), (float)(m.W - 1));
    vc = fminf(fmaxf(vc, 0.f), (float)(m.H - 1));
    const int icu = (int)floorf(uc), icv = (int)floorf(vc);
    const size_t plane = (size_t)m.H * (size_t)m.W;
    const float* px = image + ((size_t)icv * (size_t)m.W + (size_t)icu);
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = px[j * plane] * m.a[j] + m.b[j];
    return fabsf(c[0]) <= kFltMax && fabsf(c[1]) <= kFltMax && fabsf(c[2]) <= kFltMax;                // a NaN fails
}

// C' = (C * Wt + c * w) / (Wt + w) with the OLD Wt: the denominator of T'
__device__ __forceinline__ float tsdf_blend(float C, float Wt, float c, float w) { return (C * Wt + c * w) / (Wt + w); }

// The coloured form's further kernel arguments; the colourless form has none (an empty pack: the kernel it was before colour).
struct TsdfColour {
    float* color;                       // [3][Z][Y][X]
    const float* image;                 // [3][Hc][Wc]
    TsdfImage m;
};

__device__ __forceinline__ TsdfColour tsdf_colour_args() { return TsdfColour(); }
__device__ __forceinline__ const TsdfColour& tsdf_colour_args(const TsdfColour& k) { return k; }

// The second pose of a remove-and-add launch and the floor under which a removal empties the voxel.
struct TsdfRepose {
    float r[12];                        // float32(extM_add[:3,:4]); unused without ADD
    float w_floor;
};

// Wn = Wt - w, and whether the voxel survives the removal (a NaN Wn does not)
__device__ __forceinline__ bool tsdf_remaining(float Wt, float w, float w_floor, float& Wn) {
    Wn = Wt - w;
    return Wn > w_floor;
}

// C' = (C * Wt - c * w) / Wn with the stored Wt: the inverse of tsdf_blend
__device__ __forceinline__ float tsdf_unblend(float C, float Wt, float c, float w, float Wn) { return (C * Wt - c * w) / Wn; }

// T' = fminf(1, fmaxf(-1, (T * Wt - t * w) / Wn)), W' = Wn; an emptied voxel is (0, 0)
__device__ __forceinline__ void tsdf_unaverage(float& T, float& Wt, float t, float w, float Wn, bool stays) {
    T = stays ? fminf(1.f, fmaxf(-1.f, tsdf_unblend(T, Wt, t, w, Wn))) : 0.f;
    Wt = stays ? Wn : 0.f;
}

__device__ __forceinline__ void tsdf_load4(const float* p, float (&v)[4]) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}

__device__ __forceinline__ void tsdf_store4(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }

// The update of one lane group of N voxels (4: VEC, 16-byte accesses; 1: a voxel) starting at lattice column ix0 of a row: the loop
// body of tsdf_reintegrate_kernel (REMOVE, or REMOVE and ADD) and of tsdf_integrate_kernel's element form (ADD alone, f == fa; its
// VEC form keeps a spelling of its own in tsdf.hip, which measured faster).  REMOVE: the chain with f's pose, and the observation
// subtracted from the weighted sums of the voxels that pass.  ADD: the chain with fa's pose and the running average.  Either way the
// planes are loaded only when a voxel passes, colour is formed with the old weights before the distance replaces them, and a group
// that was loaded is stored once per plane.
template <int N, bool REMOVE, bool ADD, bool COLOR>
__device__ __forceinline__ void tsdf_update_group(float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color,
                                                  const float* __restrict__ depth, const float* __restrict__ gate,
                                                  const float* __restrict__ wmap, const float* __restrict__ image, const TsdfFrame& f,
                                                  const TsdfFrame& fa, const TsdfImage& m, float w_floor, int iy, int iz, int ix0,
                                                  size_t at) {
    float T[N], Wt[N], C[3][N];
    bool have = false, have_c = false;
    auto load = [&](const float* p, float (&v)[N]) {
        if constexpr (N == 4) tsdf_load4(p + at, v);
        else v[0] = p[at];
    };
    auto store = [&](float* p, const float (&v)[N]) {
        if constexpr (N == 4) tsdf_store4(p + at, v);
        else p[at] = v[0];
    };
    if (REMOVE) {                                                   // its chain ends with this scope
        const TsdfRow row = tsdf_row(f, iy, iz);
        float t[N], w[N], xq[N], yq[N];
        bool ok[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int ix = ix0 + j;
            t[j] = w[j] = xq[j] = yq[j] = 0.f;
            ok[j] = ix >= f.x0 && ix < f.x1 && tsdf_observe<COLOR>(f, row, ix, depth, gate, wmap, t[j], w[j], xq[j], yq[j]);
            have = have || ok[j];
        }
        if (have) {
            load(tsdf, T);
            load(weight, Wt);
            float Wn[N];
            bool stays[N];
#pragma unroll
            for (int j = 0; j < N; ++j) stays[j] = tsdf_remaining(Wt[j], w[j], w_floor, Wn[j]);
            if (COLOR) {                                            // with the stored weights, before the removal replaces them
                float c[N][3];
                bool fin[N];
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    c[j][0] = c[j][1] = c[j][2] = 0.f;
                    fin[j] = ok[j] && tsdf_colour(m, image, xq[j], yq[j], c[j]);
                    have_c = have_c || fin[j] || (ok[j] && !stays[j]);
                }
                if (have_c) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        load(color + k * m.volume, C[k]);
#pragma unroll
                        for (int j = 0; j < N; ++j) {
                            if (ok[j] && !stays[j]) C[k][j] = 0.f;
                            else if (fin[j]) C[k][j] = tsdf_unblend(C[k][j], Wt[j], c[j][k], w[j], Wn[j]);
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (ok[j]) tsdf_unaverage(T[j], Wt[j], t[j], w[j], Wn[j], stays[j]);
        }
    }
    if (ADD) {                                                      // on the values in registers, where the removal loaded them
        const TsdfRow row = tsdf_row(fa, iy, iz);
        float t[N], w[N], xq[N], yq[N];
        bool ok[N], any = false;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int ix = ix0 + j;
            t[j] = w[j] = xq[j] = yq[j] = 0.f;
            ok[j] = ix >= fa.x0 && ix < fa.x1 && tsdf_observe<COLOR>(fa, row, ix, depth, gate, wmap, t[j], w[j], xq[j], yq[j]);
            any = any || ok[j];
        }
        if (any) {
            if (!have) {
                load(tsdf, T);
                load(weight, Wt);
                have = true;
            }
            if (COLOR) {                                            // with the old weights, before the average replaces them
                float c[N][3];
                bool fin[N], any_fin = false;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    c[j][0] = c[j][1] = c[j][2] = 0.f;
                    fin[j] = ok[j] && tsdf_colour(m, image, xq[j], yq[j], c[j]);
                    any_fin = any_fin || fin[j];
                }
                if (any_fin) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        if (!have_c) load(color + k * m.volume, C[k]);
#pragma unroll
                        for (int j = 0; j < N; ++j)
                            if (fin[j]) C[k][j] = tsdf_blend(C[k][j], Wt[j], c[j][k], w[j]);
                    }
                    have_c = true;
                }
            }
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (ok[j]) tsdf_average(T[j], Wt[j], t[j], w[j], fa.w_max);
        }
    }
    if (!have) return;
    store(tsdf, T);
    store(weight, Wt);
    if (COLOR && have_c) {
#pragma unroll
        for (int k = 0; k < 3; ++k) store(color + k * m.volume, C[k]);
    }
}

// The colour entries' image: intrinsics, affine (a [3], then b [3]), size, and the distance between two colour planes of the grid.
static inline TsdfImage tsdf_image(int X, int Y, int Z, int Hc, int Wc, float fxc, float fyc, float cxc, float cyc, const float* affine) {
    TsdfImage m;
    m.fx = fxc; m.fy = fyc; m.cx = cxc; m.cy = cyc;
    for (int j = 0; j < 3; ++j) {
        m.a[j] = affine[j];
        m.b[j] = affine[3 + j];
    }
    m.H = Hc; m.W = Wc;
    m.volume = (size_t)(X > 0 ? X : 0) * (size_t)(Y > 0 ? Y : 0) * (size_t)(Z > 0 ? Z : 0);
    return m;
}

// Whether the VEC form may run: rows of whole 16-byte groups (X % 4 == 0, which holds for every plane) in 16-byte aligned planes.
template <class... Plane>
static inline bool tsdf_vec_ok(int X, const Plane*... planes) {
    return X % 4 == 0 && ((... | (uintptr_t)planes) & 15) == 0;
}

// The checks the integrations share, in the documented order (m: the colour entry's image, else NULL), and the frame.
static inline int tsdf_frame(TsdfFrame& f, int X, int Y, int Z, float ox, float oy, float oz, float voxel_size, int H, int W, const float* pose,
                             float fx, float fy, float cx, float cy, float trunc, float d_near, float d_far, float w_max, float gate_thr,
                             const int* box, const TsdfImage* m) {
    const long n = tsdf_voxels(X, Y, Z);
    if (n < 0) return (int)n;
    if (H <= 0 || W <= 0) return NRGBD_E_SHAPE;
    if (m && (m->H <= 0 || m->W <= 0)) return NRGBD_E_SHAPE;
    f.x0 = f.y0 = f.z0 = 0;
    f.x1 = X; f.y1 = Y; f.z1 = Z;
    if (box) {
        f.x0 = box[0]; f.y0 = box[1]; f.z0 = box[2];
        f.x1 = box[3]; f.y1 = box[4]; f.z1 = box[5];
        if (f.x0 < 0 || f.y0 < 0 || f.z0 < 0 || f.x1 > X || f.y1 > Y || f.z1 > Z) return NRGBD_E_SHAPE;
        if (f.x0 >= f.x1 || f.y0 >= f.y1 || f.z0 >= f.z1) return NRGBD_E_SHAPE;
    }
    if (!tsdf_positive(voxel_size) || !tsdf_positive(trunc) || !tsdf_positive(w_max)) return NRGBD_E_ARG;
    if (!(d_near < d_far)) return NRGBD_E_ARG;                   // a NaN bound included
    if (m) {
        const float k[10] = {m->fx, m->fy, m->cx, m->cy, m->a[0], m->a[1], m->a[2], m->b[0], m->b[1], m->b[2]};
        for (int i = 0; i < 10; ++i)
            if (!(fabsf(k[i]) <= kFltMax)) return NRGBD_E_ARG;   // a NaN fails
    }
    for (int i = 0; i < 12; ++i) f.r[i] = pose[i];
    f.ox = ox; f.oy = oy; f.oz = oz; f.vs = voxel_size;
    f.fx = fx; f.fy = fy; f.cx = cx; f.cy = cy;
    f.trunc = trunc; f.d_near = d_near; f.d_far = d_far; f.w_max = w_max; f.gate_thr = gate_thr;
    f.X = X; f.Y = Y; f.H = H; f.W = W;
    return NRGBD_OK;
}

static inline dim3 tsdf_integrate_grid(const TsdfFrame& f, bool vec) {
    const int units = vec ? (f.x1 + 3) / 4 - f.x0 / 4 : f.x1 - f.x0;
    const int rows = f.y1 - f.y0, slices = f.z1 - f.z0;
    return dim3((unsigned)ceil_div(units, 64), (unsigned)(ceil_div(rows, 4) < 65535 ? ceil_div(rows, 4) : 65535),
                (unsigned)(slices < 65535 ? slices : 65535));
}

}  // namespace nrgbd
