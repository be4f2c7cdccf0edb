// consistency.hip — multi-view depth consistency: a depth map cross-checked against other views' maps before it is fused
// (neuralrgbd_amd/fusion.py: filter_depth, FusionVideoStream(consistency=k); ops.depth_consistency).
//
// No counterpart in the reference, which stops at the maps.  The operation sequence per pixel is written out in include/nrgbd.h and
// restated in numpy by tests/consistency_ref.py: fp32, one IEEE operation per operation of the header (the library is built with
// -ffp-contract=off), no atomics, no workspace, no LDS: the same inputs give the same bits in every run.
//
// depth_consistency_kernel   one reference pixel per lane, one wave on a 32 x 2 pixel tile, 2 x 2 waves per workgroup: neighbouring
//                            lanes project to neighbouring source pixels, and the sources of a video are a few centimetres and
//                            hundredths of a radian away, so a wave's gather touches about two row segments of 128 bytes, and its
//                            own loads and stores are two such segments.  (tsdf_raycast.hip's 8 x 8 tile was measured first: 8 row
//                            segments of 32 bytes per access; at 768 x 1024 with 16 gated sources 46.7 us against 28.2 us for 32 x 2
//                            and 27.1 us for 64 x 1, without gates 27.1 / 24.5 / 24.6 us; 32 x 2 keeps some height for a camera
//                            that rolls.)  The transforms and the maps' offsets are kernel arguments (wave-uniform, 992 bytes in
//                            all) and the source loop runs to the runtime n_src.  A valid pixel requests a source's depth and gate
//                            together, at pixel 0 of the map where its projection falls outside, so that the loads of several
//                            sources can be in flight at once; an invalid pixel issues no source load.  Reads (1 + n_src) maps
//                            (twice that with gates) and writes up to two with plain vector stores.  27 VGPRs, no scratch.  Per
//                            source a lane spends two IEEE divisions and about 20 other fp32 operations: without gates the launch
//                            is nearer to that arithmetic than to the bytes (tools/bench_consistency.py).
#include "common.hpp"

namespace nrgbd {

constexpr int kConsMaxSrc = NRGBD_CONSISTENCY_MAX_SRC;
constexpr int kConsMaxSide = 1 << 15;
constexpr int kConsWaveW = 32, kConsWaveH = 64 / kConsWaveW;                 // a wave's pixel tile: 32 x 2 (measured, see above)
constexpr int kConsTileW = 2 * kConsWaveW, kConsTileH = 2 * kConsWaveH;      // the workgroup's: 2 x 2 waves
constexpr float kConsFltMax = 3.402823466e+38f;

struct ConsistencyArgs {
    const float* depth; const float* gate; const float* src_depth; const float* src_gate;
    float* votes; float* depth_out;
    long off[kConsMaxSrc];                                     // source s is the map at src_depth + off[s]
    float T[kConsMaxSrc][12];                                  // reference camera -> source camera s, [3][4] row-major
    int H, W, n_src, min_views;
    float gate_thr, d_near, d_far, fx, fy, cx, cy, rel_thr;
};
static_assert(sizeof(ConsistencyArgs) < 1024, "the arguments stay under 1 KB");

__device__ __forceinline__ bool cons_valid(float d, float d_near, float d_far) {
    return d > d_near && d <= d_far && d <= kConsFltMax;      // a NaN fails
}

__global__ __launch_bounds__(256) void depth_consistency_kernel(const ConsistencyArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = (int)blockIdx.x * kConsTileW + (wave & 1) * kConsWaveW + (lane % kConsWaveW);
    const int y = (int)blockIdx.y * kConsTileH + (wave >> 1) * kConsWaveH + (lane / kConsWaveW);
    if (x >= a.W || y >= a.H) return;
    const size_t at = (size_t)y * (size_t)a.W + (size_t)x;
    const float d = a.depth[at];
    bool ok = cons_valid(d, a.d_near, a.d_far);
    if (ok && a.gate) ok = a.gate[at] >= a.gate_thr;
    int agree = -1;
    if (ok) {
        agree = 0;
        const float xn = (((float)x + 0.5f) - a.cx) / a.fx;
        const float yn = (((float)y + 0.5f) - a.cy) / a.fy;
        const float px = xn * d, py = yn * d, pz = d;
        const float Wf = (float)a.W, Hf = (float)a.H;
#pragma unroll 4
        for (int s = 0; s < a.n_src; ++s) {
            const float* T = a.T[s];
            const float qx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
            const float qy = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
            const float qz = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
            const float u = a.fx * (qx / qz) + a.cx;
            const float v = a.fy * (qy / qz) + a.cy;
            const bool in = qz > 0.f && u >= 0.f && u < Wf && v >= 0.f && v < Hf;      // a NaN fails
            const int iu = (int)floorf(in ? u : 0.f), iv = (int)floorf(in ? v : 0.f);
            const size_t as = (size_t)a.off[s] + ((size_t)iv * (size_t)a.W + (size_t)iu);
            const float ds = a.src_depth[as];
            const float gs = a.src_gate ? a.src_gate[as] : 0.f;
            bool hit = in && cons_valid(ds, a.d_near, a.d_far);
            if (a.src_gate) hit = hit && gs >= a.gate_thr;
            hit = hit && fabsf(ds - qz) <= a.rel_thr * qz;     // a NaN fails
            agree += hit ? 1 : 0;
        }
    }
    if (a.votes) a.votes[at] = (float)agree;
    if (a.depth_out) a.depth_out[at] = agree >= a.min_views && ok ? d : 0.f;
}

static bool cons_pos(float x) { return x > 0.f && x <= kConsFltMax; }
static bool cons_fin(float x) { return x >= -kConsFltMax && x <= kConsFltMax; }

}  // namespace nrgbd

// no counterpart in the reference: see the header of this file and include/nrgbd.h
extern "C" int nrgbd_depth_consistency_f32(const float* depth, const float* gate, float gate_thr, int H, int W, float d_near, float d_far,
                                           float fx, float fy, float cx, float cy, const float* src_depth, const float* src_gate,
                                           long src_stride, const int* src_slots, const float* src_T, int n_src, float rel_thr,
                                           int min_views, float* votes, float* depth_out, void* stream) {
    using namespace nrgbd;
    if (!depth || (!votes && !depth_out)) return NRGBD_E_NULL;
    if (n_src > 0 && (!src_depth || !src_slots || !src_T)) return NRGBD_E_NULL;
    if (n_src > 0 && ((gate != nullptr) != (src_gate != nullptr))) return NRGBD_E_NULL;
    if (H <= 0 || W <= 0 || H > kConsMaxSide || W > kConsMaxSide) return NRGBD_E_SHAPE;
    if (n_src < 0 || n_src > kConsMaxSrc || min_views < 0) return NRGBD_E_SHAPE;
    if (n_src > 0 && src_stride < (long)H * W) return NRGBD_E_SHAPE;
    for (int s = 0; s < n_src; ++s)
        if (src_slots[s] < 0) return NRGBD_E_SHAPE;
    if (!cons_pos(fx) || !cons_pos(fy) || !cons_fin(cx) || !cons_fin(cy) || !cons_pos(rel_thr)) return NRGBD_E_ARG;
    if (!(d_near < d_far)) return NRGBD_E_ARG;                  // a NaN bound included
    if (gate && gate_thr != gate_thr) return NRGBD_E_ARG;
    for (int i = 0; i < 12 * n_src; ++i)
        if (!cons_fin(src_T[i])) return NRGBD_E_ARG;
    ConsistencyArgs a;
    a.depth = depth; a.gate = gate; a.src_depth = src_depth; a.src_gate = n_src > 0 ? src_gate : nullptr;
    a.votes = votes; a.depth_out = depth_out;
    for (int s = 0; s < kConsMaxSrc; ++s) {
        a.off[s] = s < n_src ? (long)src_slots[s] * src_stride : 0;
        for (int k = 0; k < 12; ++k) a.T[s][k] = s < n_src ? src_T[12 * s + k] : 0.f;
    }
    a.H = H; a.W = W; a.n_src = n_src; a.min_views = min_views;
    a.gate_thr = gate_thr; a.d_near = d_near; a.d_far = d_far; a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.rel_thr = rel_thr;
    const dim3 grid((unsigned)ceil_div(W, kConsTileW), (unsigned)ceil_div(H, kConsTileH));
    hipLaunchKernelGGL(depth_consistency_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}
