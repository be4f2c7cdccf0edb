// tsdf_reint.hip — a fused depth frame taken out of the TSDF volume again, and put back at a corrected pose in the same launch
// (neuralrgbd_amd/fusion.py: TSDFVolume.deintegrate / reintegrate, FusionVideoStream.repose / retrack).
//
// No counterpart in the reference.  The arithmetic is written out in include/nrgbd.h (nrgbd_tsdf_reintegrate_f32) and restated in numpy
// by tests/tsdf_deint_ref.py, which reproduces every stored value bit for bit: fp32, one IEEE operation per operation of the header
// (-ffp-contract=off: no fused multiply-add, no reciprocal), no atomics, the same bits in every run.  The frame, the chain up to
// (t, w), the colour pixel and the running average are tsdf_integrate.hpp's — the device code the integration runs — so what this
// launch removes is what that one added.
//
// tsdf_reintegrate_kernel<VEC, ADD>  block (64, 4) and the lane's four x-neighbours (VEC) or one voxel of tsdf_integrate_kernel.  Per
//                             lane group: the chain with pose_remove; where a voxel passes, the group's planes are loaded and the
//                             observation is subtracted from the weighted sums (a voxel whose weight falls to w_floor is fresh
//                             again: 0, 0); ADD: then the chain with pose_add and the unchanged integration update on the values in
//                             registers.  The removal chain is dead before the addition chain starts — only the loaded planes live
//                             across it.  A group that neither pose updates is neither loaded nor stored; any other is loaded once and
//                             stored once per plane, whichever of the two touched it.  Voxels are independent, so ADD is by
//                             definition the bits of the removal launch followed by nrgbd_tsdf_integrate_f32.
// tsdf_reintegrate_kernel<VEC, ADD, TsdfColour>  the same with the three colour planes: the colour pixel of a removed observation is
//                             subtracted with the weights of T (when its three values are finite), an emptied voxel's colour is 0;
//                             the colour planes are loaded only when one of the lane's voxels changes its colour.
//                             Resources (kernel-resource-usage remarks, gfx950, -O3), VGPRs / waves per SIMD, ScratchSize 0 and no
//                             LDS in every form:
//                               colourless  VEC: remove 52 / 8, remove-and-add 77 / 6; element: 26 / 8, 32 / 7
//                               coloured    VEC: remove 100 / 4, remove-and-add 122 / 4; element: remove 34 / 7
//                             The coloured element form is not built remove-and-add: with two poses, the frame, the image and its
//                             lane masks it runs out of scalar registers and the compiler reserves scratch for them, so the entry
//                             launches its removal and then nrgbd_tsdf_integrate_color_f32's kernel (the fallback for X % 4 != 0 or
//                             misaligned planes; the same bits by definition).
//                             One more IEEE division per removed voxel (three more with colour) beside the chain's.
#include "tsdf_integrate.hpp"

namespace nrgbd {

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

// One lane group of N voxels (4: VEC, 16-byte accesses; 1: a voxel) starting at lattice column ix0 of a row.
template <int N, bool ADD, bool COLOR>
__device__ __forceinline__ void tsdf_reintegrate_group(float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color,
                                                       const float* __restrict__ depth, const float* __restrict__ gate,
                                                       const float* __restrict__ wmap, const float* __restrict__ image,
                                                       const TsdfFrame& f, const TsdfFrame& fa, const TsdfImage& m, float w_floor,
                                                       int iy, int iz, int ix0, size_t at) {
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
    {                                                               // the removal: its chain ends with this scope
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
    if (ADD) {                                                      // tsdf_integrate_kernel's update on the values in registers
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

// block (64, 4): threadIdx.x walks x (groups of four voxels, or voxels), threadIdx.y rows; blockIdx.y / .z stride over rows and slices
template <bool VEC, bool ADD, class... Colour>
__global__ __launch_bounds__(256) void tsdf_reintegrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                               const float* __restrict__ depth, const float* __restrict__ gate,
                                                               const float* __restrict__ wmap, const TsdfFrame f, const TsdfRepose q,
                                                               const Colour... colour) {
    constexpr bool COLOR = sizeof...(Colour) != 0;
    const TsdfColour k = tsdf_colour_args(colour...);
    const long at = (long)(VEC ? (f.x0 >> 2) : f.x0) + (long)(blockIdx.x * 64 + threadIdx.x);
    if (at >= (VEC ? (long)((f.x1 + 3) >> 2) : (long)f.x1)) return;
    const int unit = (int)at;
    TsdfFrame fa = f;                                               // the frame at pose_add: everything but the pose is shared
    if (ADD) {
#pragma unroll
        for (int i = 0; i < 12; ++i) fa.r[i] = q.r[i];
    }
    for (int iz = f.z0 + (int)blockIdx.z; iz < f.z1; iz += (int)gridDim.z) {
        for (int iy = f.y0 + (int)(blockIdx.y * 4 + threadIdx.y); iy < f.y1; iy += (int)gridDim.y * 4) {
            const size_t base = ((size_t)iz * (size_t)f.Y + (size_t)iy) * (size_t)f.X;
            if (VEC)
                tsdf_reintegrate_group<4, ADD, COLOR>(tsdf, weight, k.color, depth, gate, wmap, k.image, f, fa, k.m, q.w_floor, iy, iz,
                                                      4 * unit, base + 4 * (size_t)unit);
            else
                tsdf_reintegrate_group<1, ADD, COLOR>(tsdf, weight, k.color, depth, gate, wmap, k.image, f, fa, k.m, q.w_floor, iy, iz,
                                                      unit, base + (size_t)unit);
        }
    }
}

// The launch of both entries: the form (VEC / element, remove / remove-and-add) chosen on the host.
template <class... Colour>
static void tsdf_reintegrate_launch(bool vec, bool add, const TsdfFrame& f, const TsdfRepose& q, float* tsdf, float* weight,
                                    const float* depth, const float* gate, const float* wmap, hipStream_t st, const Colour&... colour) {
    const dim3 grid = tsdf_integrate_grid(f, vec), block(64, 4);
    if (vec && add)
        hipLaunchKernelGGL((tsdf_reintegrate_kernel<true, true, Colour...>), grid, block, 0, st, tsdf, weight, depth, gate, wmap, f, q, colour...);
    else if (vec)
        hipLaunchKernelGGL((tsdf_reintegrate_kernel<true, false, Colour...>), grid, block, 0, st, tsdf, weight, depth, gate, wmap, f, q, colour...);
    else if (add) {
        // the coloured element form is not built remove-and-add (its scalar registers spill into scratch): the entry splits it
        if constexpr (sizeof...(Colour) == 0)
            hipLaunchKernelGGL((tsdf_reintegrate_kernel<false, true>), grid, block, 0, st, tsdf, weight, depth, gate, wmap, f, q);
    } else
        hipLaunchKernelGGL((tsdf_reintegrate_kernel<false, false, Colour...>), grid, block, 0, st, tsdf, weight, depth, gate, wmap, f, q, colour...);
}

static bool tsdf_floor_ok(float w_floor) { return w_floor >= 0.f && w_floor <= kFltMax; }              // a NaN fails

static TsdfRepose tsdf_repose(const float* pose_add, float w_floor) {
    TsdfRepose q;
    for (int i = 0; i < 12; ++i) q.r[i] = pose_add ? pose_add[i] : 0.f;
    q.w_floor = w_floor;
    return q;
}

}  // namespace nrgbd

// no counterpart in the reference: see the header of this file and include/nrgbd.h
extern "C" int nrgbd_tsdf_reintegrate_f32(float* tsdf, float* weight, int X, int Y, int Z, float ox, float oy, float oz, float voxel_size,
                                          const float* depth, const float* gate, const float* wmap, const float* pose_remove,
                                          const float* pose_add, int H, int W, float fx, float fy, float cx, float cy, float trunc,
                                          float d_near, float d_far, float w_max, float w_floor, float gate_thr, const int* box,
                                          void* stream) {
    using namespace nrgbd;
    if (!tsdf || !weight || !depth || !pose_remove) return NRGBD_E_NULL;
    TsdfFrame f;
    const int rc = tsdf_frame(f, X, Y, Z, ox, oy, oz, voxel_size, H, W, pose_remove, fx, fy, cx, cy, trunc, d_near, d_far, w_max, gate_thr,
                              box, nullptr);
    if (rc != NRGBD_OK) return rc;
    if (!tsdf_floor_ok(w_floor)) return NRGBD_E_ARG;
    const bool vec = X % 4 == 0 && (((uintptr_t)tsdf | (uintptr_t)weight) & 15) == 0;
    tsdf_reintegrate_launch(vec, pose_add != nullptr, f, tsdf_repose(pose_add, w_floor), tsdf, weight, depth, gate, wmap, (hipStream_t)stream);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

// no counterpart in the reference: the same launch on a colour volume
extern "C" int nrgbd_tsdf_reintegrate_color_f32(float* tsdf, float* weight, float* color, int X, int Y, int Z, float ox, float oy, float oz,
                                                float voxel_size, const float* depth, const float* gate, const float* wmap,
                                                const float* pose_remove, const float* pose_add, int H, int W, float fx, float fy,
                                                float cx, float cy, float trunc, float d_near, float d_far, float w_max, float w_floor,
                                                float gate_thr, const int* box, const float* image, int Hc, int Wc, float fxc, float fyc,
                                                float cxc, float cyc, const float* affine, void* stream) {
    using namespace nrgbd;
    if (!tsdf || !weight || !depth || !pose_remove || !color || !image || !affine) return NRGBD_E_NULL;
    TsdfImage m;
    m.fx = fxc; m.fy = fyc; m.cx = cxc; m.cy = cyc;
    for (int j = 0; j < 3; ++j) {
        m.a[j] = affine[j];
        m.b[j] = affine[3 + j];
    }
    m.H = Hc; m.W = Wc;
    m.volume = (size_t)(X > 0 ? X : 0) * (size_t)(Y > 0 ? Y : 0) * (size_t)(Z > 0 ? Z : 0);
    TsdfFrame f;
    const int rc = tsdf_frame(f, X, Y, Z, ox, oy, oz, voxel_size, H, W, pose_remove, fx, fy, cx, cy, trunc, d_near, d_far, w_max, gate_thr,
                              box, &m);
    if (rc != NRGBD_OK) return rc;
    if (!tsdf_floor_ok(w_floor)) return NRGBD_E_ARG;
    const bool vec = X % 4 == 0 && (((uintptr_t)tsdf | (uintptr_t)weight | (uintptr_t)color) & 15) == 0;      // X % 4 == 0: every plane
    const TsdfColour k = {color, image, m};
    const bool split = !vec && pose_add;            // the element form: the removal, then the integration launch itself (the same bits)
    tsdf_reintegrate_launch(vec, pose_add != nullptr && !split, f, tsdf_repose(split ? nullptr : pose_add, w_floor), tsdf, weight, depth, gate,
                            wmap, (hipStream_t)stream, k);
    NRGBD_CHECK_LAUNCH();
    if (split)
        return nrgbd_tsdf_integrate_color_f32(tsdf, weight, color, X, Y, Z, ox, oy, oz, voxel_size, depth, gate, gate_thr, wmap, H, W, pose_add,
                                              fx, fy, cx, cy, trunc, d_near, d_far, w_max, box, image, Hc, Wc, fxc, fyc, cxc, cyc, affine,
                                              stream);
    return NRGBD_OK;
}
