// resample.hip — PREDICT: rigid 3-D resample of the depth-probability volume (K10).
// Replaces warping/homography.py:654-723 (resample_vol_cuda, d_candi_new = None or given), :873-887
// (_set_vol_border) and the clamp of test_utils/test_KVNet.py:54-59.
//
// The reference builds the [1,D,h,w,3] back-projected point grid on the HOST in a Python loop and
// copies it to the device every frame (:673-682), then syncs twice for z min/max (:689-690).
// Here the point of voxel (k,y,x) is generated in-kernel from the ray table and d_candi, the pose
// is read from device memory, and the border overwrite is applied on the fly to the 8 taps, so the
// step is one HBM-bound launch (read D*hw, write D*hw floats) with no host round trip.
#include "resample.hpp"

namespace nrgbd {

// the per-voxel arithmetic (point, pose chain, taps, clamp) is dpv_resample_voxel of resample.hpp, shared with keyframe.hip
__global__ __launch_bounds__(256) void dpv_resample_kernel(const ResampleArgs a) {
    const size_t hw = (size_t)a.h * a.w;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (p >= hw) return;
    a.out[(size_t)k * hw + p] = dpv_resample_voxel(a, a.rays[p], a.rays[hw + p], a.rays[2 * hw + p], a.d_candi[k]);
}

}  // namespace nrgbd

extern "C" int nrgbd_dpv_resample_to(const float* dpv, const float* T, const float* rays,
                                     const float* d_candi_out, float tan_hh, float tan_hv, float z_half,
                                     float z_radius, float pad_value, int do_clamp, float clamp_lo,
                                     float clamp_hi, float* out, int D_src, int D_out, int h, int w, void* stream) {
    using namespace nrgbd;
    if (!dpv || !T || !rays || !d_candi_out || !out) return NRGBD_E_NULL;
    if (dpv == out) return NRGBD_E_ARG;
    if (D_src <= 0 || D_src > 65535 || D_out <= 0 || D_out > 65535 || h <= 0 || w <= 0) return NRGBD_E_SHAPE;
    ResampleArgs a{dpv, T, rays, d_candi_out, out, tan_hh, tan_hv, z_half, z_radius, pad_value,
                   clamp_lo, clamp_hi, do_clamp, D_src, h, w};
    dim3 grid(ceil_div((long)h * w, 256), D_out);
    hipLaunchKernelGGL(dpv_resample_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

extern "C" int nrgbd_dpv_resample(const float* dpv, const float* T, const float* rays,
                                  const float* d_candi, float tan_hh, float tan_hv, float z_half,
                                  float z_radius, float pad_value, int do_clamp, float clamp_lo,
                                  float clamp_hi, float* out, int D, int h, int w, void* stream) {
    return nrgbd_dpv_resample_to(dpv, T, rays, d_candi, tan_hh, tan_hv, z_half, z_radius, pad_value, do_clamp, clamp_lo,
                                 clamp_hi, out, D, D, h, w, stream);
}
