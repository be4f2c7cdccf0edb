// tsdf_reint.hip — a fused depth frame taken out of the TSDF volume again, and put back at a corrected pose in the same launch
// (neuralrgbd_amd/fusion.py: TSDFVolume.deintegrate / reintegrate, FusionVideoStream.repose / retrack).
//
// No counterpart in the reference.  The arithmetic is written out in include/nrgbd.h (nrgbd_tsdf_reintegrate_f32) and restated in numpy
// by tests/tsdf_deint_ref.py, which reproduces every stored value bit for bit: fp32, one IEEE operation per operation of the header
// (-ffp-contract=off: no fused multiply-add, no reciprocal), no atomics, the same bits in every run.  The lane group's update —
// removal and addition — is tsdf_integrate.hpp's tsdf_update_group, built from the helpers the integration kernel runs (its element
// form calls the same group; its VEC form spells the addition out once more), so what this launch removes is what that one added.
//
// tsdf_reintegrate_kernel<VEC, ADD>  block (64, 4) and the lane's four x-neighbours (VEC) or one voxel of tsdf_integrate_kernel.  Per
//                             lane group: the chain with pose_remove; where a voxel passes, the group's planes are loaded and the
//                             observation is subtracted from the weighted sums (a voxel whose weight falls to w_floor is fresh
//                             again: 0, 0); ADD: then the chain with pose_add and the integration update on the values in
//                             registers.  The removal chain is dead before the addition chain starts — only the loaded planes live
//                             across it.  A group that neither pose updates is neither loaded nor stored; any other is loaded once and
//                             stored once per plane, whichever of the two touched it.  Voxels are independent, so ADD gives the
//                             bits of the removal launch followed by nrgbd_tsdf_integrate_f32.
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
                tsdf_update_group<4, true, ADD, COLOR>(tsdf, weight, k.color, depth, gate, wmap, k.image, f, fa, k.m, q.w_floor, iy, iz,
                                                     4 * unit, base + 4 * (size_t)unit);
            else
                tsdf_update_group<1, true, ADD, COLOR>(tsdf, weight, k.color, depth, gate, wmap, k.image, f, fa, k.m, q.w_floor, iy, iz,
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
    tsdf_reintegrate_launch(tsdf_vec_ok(X, tsdf, weight), pose_add != nullptr, f, tsdf_repose(pose_add, w_floor), tsdf, weight, depth, gate,
                            wmap, (hipStream_t)stream);
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
    const TsdfImage m = tsdf_image(X, Y, Z, Hc, Wc, fxc, fyc, cxc, cyc, affine);
    TsdfFrame f;
    const int rc = tsdf_frame(f, X, Y, Z, ox, oy, oz, voxel_size, H, W, pose_remove, fx, fy, cx, cy, trunc, d_near, d_far, w_max, gate_thr,
                              box, &m);
    if (rc != NRGBD_OK) return rc;
    if (!tsdf_floor_ok(w_floor)) return NRGBD_E_ARG;
    const bool vec = tsdf_vec_ok(X, tsdf, weight, color);
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
