// keyframe.hip — the depth / confidence maps the local bundle adjustment reads, from the R-Net's log-DPV in ONE launch.
// Replaces, per frame of the LBA driver (test_KVNet_LBA.py:414-423, :455, :495):
//     BV_tmp   = resample_vol_cuda(BVs_measure, inv(pose_next), ..., d_candi_new=d_candi, pad).clamp(-1000, 0)
//     dmap_ref = depth_val_regression(BVs_measure);  conf_ref = exp(max_k BVs_measure) ** 2
//     dmap_kf  = depth_val_regression(BV_tmp);       conf_kf  = exp(max_k BV_tmp) ** 2
// i.e. nrgbd_dpv_resample_to + 4 x nrgbd_depth_regress + ATen exp / pow: 7 D hw floats of HBM traffic and a [D,H,W]
// temporary at IMAGE size (25 MB at 64 x 256 x 384, 201 MB at 768 x 1024) for four [H,W] maps.  Here the resampled volume
// is never written: every sample is reduced over the candidates as it is produced (reads: the volume once through the
// caches for the gathers, once coalesced for the reference maps).
//
// Work split: a workgroup owns a 16 x 4 PIXEL TILE (neighbouring pixels sample neighbouring texels: a wave's 8 taps fall
// into a few 64-byte row segments of two planes) and its 4 waves split the candidates: wave `part` samples candidates
// part, part + 4, ... of all 64 pixels.  One thread per pixel would run 8 Do dependent gathers and Do expf in a row, the
// shape that made depth_regress_kernel latency-bound (softmax.hip, above logsoftmax_d4_kernel); here a thread has the
// gathers of KC / 4 independent candidates to overlap.
// Arithmetic: the sample is dpv_resample_voxel (resample.hpp: resample.hip's own body, so the bits are the resampled
// volume's); the per-candidate terms expf(v_k) * d_k go through LDS and wave 0 adds them in candidate order k = 0 .. Do-1
// from 0.f — depth_regress_kernel's association, bit for bit; the maximum is exact in any order; conf = c * c with
// c = exp_rn(max) as export_depth_u16_kernel.  Capture-safe: no allocation, no host read, pose read from device memory.
#include "resample.hpp"

namespace nrgbd {

constexpr int kKfTileW = 16, kKfTileH = 4;     // 64 pixels = the lanes of a wave
constexpr int kKfParts = 4;                    // waves per workgroup = candidate subsets
constexpr int kKfChunk = 64;                   // candidates per LDS round: 16 per wave, 16 KB of terms

struct KeyframeArgs {
    ResampleArgs rs;                 // rs.d_candi = the OUTPUT candidates, rs.out unused
    const float* d_candi_src;
    float *dmap_kf, *conf_kf, *dmap_ref, *conf_ref;
    int D_out;
};

// sum_k expf(v_k) * d[k] in candidate order and max_k v_k over n candidates, v_k = value(k); every thread of the workgroup
// calls it; wave 0 returns the sum, every wave the maximum of ITS candidates (combined by the caller).
template <class F>
__device__ __forceinline__ void kf_regress(int n, const float* __restrict__ d, F value, float (*term)[64], int lane, int part,
                                           float& acc, float& m) {
    acc = 0.f;
    m = -INFINITY;
    for (int k0 = 0; k0 < n; k0 += kKfChunk) {
#pragma unroll 4
        for (int t = 0; t < kKfChunk / kKfParts; ++t) {
            const int k = k0 + part + kKfParts * t;
            const int kc = k < n ? k : n - 1;            // the tail samples a valid candidate and drops it: no divergent loads
            const float v = value(kc);
            if (k < n) {
                term[k - k0][lane] = expf(v) * d[kc];
                m = fmaxf(m, v);
            }
        }
        __syncthreads();
        if (part == 0) {
            const int cnt = (n - k0 < kKfChunk) ? n - k0 : kKfChunk;
            for (int j = 0; j < cnt; ++j) acc = acc + term[j][lane];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void dpv_keyframe_maps_kernel(const KeyframeArgs a) {
    __shared__ float term[kKfChunk][64];
    __shared__ float red[kKfParts][64];
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int px = blockIdx.x * kKfTileW + (lane & (kKfTileW - 1));
    const int py = blockIdx.y * kKfTileH + (lane / kKfTileW);
    const bool in = px < a.rs.w && py < a.rs.h;
    const size_t hw = (size_t)a.rs.h * a.rs.w;
    // a lane outside the image works on the clamped pixel and writes nothing
    const size_t p = (size_t)(py < a.rs.h ? py : a.rs.h - 1) * a.rs.w + (px < a.rs.w ? px : a.rs.w - 1);
    float acc, m;

    if (a.dmap_kf || a.conf_kf) {
        const float rx = a.rs.rays[p], ry = a.rs.rays[hw + p], rz = a.rs.rays[2 * hw + p];
        kf_regress(a.D_out, a.rs.d_candi,
                   [&](int k) { return dpv_resample_voxel(a.rs, rx, ry, rz, a.rs.d_candi[k]); }, term, lane, part, acc, m);
        red[part][lane] = m;
        __syncthreads();
        if (part == 0 && in) {
            m = fmaxf(fmaxf(red[0][lane], red[1][lane]), fmaxf(red[2][lane], red[3][lane]));
            const float c = exp_rn(m);
            if (a.dmap_kf) a.dmap_kf[p] = acc;
            if (a.conf_kf) a.conf_kf[p] = c * c;
        }
        __syncthreads();
    }
    if (a.dmap_ref || a.conf_ref) {
        const float* __restrict__ src = a.rs.dpv + p;
        kf_regress(a.rs.D, a.d_candi_src, [&](int k) { return src[(size_t)k * hw]; }, term, lane, part, acc, m);
        red[part][lane] = m;
        __syncthreads();
        if (part == 0 && in) {
            m = fmaxf(fmaxf(red[0][lane], red[1][lane]), fmaxf(red[2][lane], red[3][lane]));
            const float c = exp_rn(m);
            if (a.dmap_ref) a.dmap_ref[p] = acc;
            if (a.conf_ref) a.conf_ref[p] = c * c;
        }
    }
}

}  // namespace nrgbd

extern "C" int nrgbd_dpv_keyframe_maps(const float* dpv, const float* T, const float* rays, const float* d_candi_out,
                                       const float* d_candi_src, float tan_hh, float tan_hv, float z_half, float z_radius,
                                       float pad_value, int do_clamp, float clamp_lo, float clamp_hi, float* dmap_kf,
                                       float* conf_kf, float* dmap_ref, float* conf_ref, int D_src, int D_out, int h, int w,
                                       void* stream) {
    using namespace nrgbd;
    const bool want_kf = dmap_kf || conf_kf, want_ref = dmap_ref || conf_ref;
    if (!dpv || (!want_kf && !want_ref)) return NRGBD_E_NULL;
    if (want_kf && (!T || !rays || !d_candi_out)) return NRGBD_E_NULL;
    if (want_ref && !d_candi_src) return NRGBD_E_NULL;
    if (D_src <= 0 || D_src > 65535 || D_out <= 0 || D_out > 65535 || h <= 0 || w <= 0) return NRGBD_E_SHAPE;
    KeyframeArgs a{{dpv, T, rays, d_candi_out, nullptr, tan_hh, tan_hv, z_half, z_radius, pad_value, clamp_lo, clamp_hi,
                    do_clamp, D_src, h, w},
                   d_candi_src, dmap_kf, conf_kf, dmap_ref, conf_ref, D_out};
    dim3 grid(ceil_div(w, kKfTileW), ceil_div(h, kKfTileH));
    if (grid.y > 65535) return NRGBD_E_SHAPE;
    hipLaunchKernelGGL(dpv_keyframe_maps_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}
