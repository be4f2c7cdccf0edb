// costvol_bwd.hip — backward of the fused plane-sweep cost volume (training, BASELINE config 4).
// Replaces what autograd does for warping/homography.py:293-331 in the reference: grid_sample backward
// (a scatter-add of the bilinear weights into the source features), the broadcast subtraction and the
// channel sum.  Nothing of the [D,C,h,w] warped tensors is materialised in either direction.
//
//   cost[k,p] = sum_v (1/sigma) sum_c dist( s_c(v,k,p) - ref_c(p) ),   s_c = sum_tap w_tap * src_v[c, tap]
//   L2:  dcost/ds_c = 2 (s_c - ref_c) / sigma      L1:  sign(s_c - ref_c) / sigma
//   g_src[v, tap, c] += w_tap * dcost/ds_c * g[k,p]        (scatter: many pixels/candidates hit one texel)
//   g_ref[p, c]      -= sum_{k,v} dcost/ds_c * g[k,p]      (register accumulation)
// Two kernels.  costvol_bwd_lds_kernel (grids whose 16-byte channel word of one source view fits in LDS, i.e. the
// training grids): the scatter goes into LDS with ds_add_f32 and leaves the workgroup once, as plain coalesced
// stores of per-slice partial sums that costvol_bwd_reduce_kernel adds in a fixed order — no global atomics at
// all.  costvol_bwd_kernel (larger grids): the same sample loop with global atomics; measured on MI355X at
// 64x96x64, V = 4, C = 67 it spends 4.9 of its 5.2 ms waiting on those atomics, the LDS kernel takes the rest.
// Sampling positions are recomputed exactly as in the forward kernels (no gradient flows to the poses:
// they are inputs, as in the reference where they come from the dataset).
#include "costvol_bwd.hpp"

namespace nrgbd {

// Developer builds only (NRGBD_BWD_ABL): 1 = no atomics, 2 = no tap loads, 4 = conflict-free LDS addresses (results invalid).
#ifdef NRGBD_DEV
#define NRGBD_BWD_ABL_BITS(abl) (abl)
#else
#define NRGBD_BWD_ABL_BITS(abl) 0
#endif

// grid (ceil(hw/64), kchunks, Cp/4), block 64: one lane = one pixel x one slice of consecutive depth candidates x
// one 16-byte channel word, over all views (costvol_bwd_sweep); a flushed tap gradient is one global atomic.
__global__ __launch_bounds__(64) void costvol_bwd_kernel(const CostvolBwdArgs a, const int kchunks, const int abl_) {
    const int abl = NRGBD_BWD_ABL_BITS(abl_);
    const int hw = a.h * a.w;
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= hw) return;
    const int per = (a.D + kchunks - 1) / kchunks;
    const int k_begin = blockIdx.y * per, k_end = min(a.D, k_begin + per);
    const int i = blockIdx.z;                      // channel word
    const float rx = a.rays[p], ry = a.rays[hw + p], rz = a.rays[2 * hw + p];
    const float4 r = *reinterpret_cast<const float4*>(a.ref + (size_t)p * a.Cp + 4 * i);
    float gr[4] = {0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < a.V; ++v) {
        float* gs = a.g_src + (size_t)v * hw * a.Cp + 4 * i;
        costvol_bwd_sweep(a, abl, p, v, i, k_begin, k_end, rx, ry, rz, r, gr,
                          [&](int tex, int e, float x) { atomicAdd(gs + (size_t)tex * a.Cp + e, x); });
    }
    float* go = a.g_ref + (size_t)p * a.Cp + 4 * i;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (gr[e] != 0.f) atomicAdd(go + e, gr[e]);
}

constexpr int kBwdThreads = 1024;
constexpr size_t kBwdLdsMax = 144 * 1024;   // of the 160 KB of a CU

// grid (kchunks, Cp/4, V), block 1024, LDS 16*h*w bytes: one workgroup = one source view x one 16-byte channel word
// x one slice of consecutive depth candidates, over ALL pixels.  The gradient of that word of the view lives in LDS
// as four component planes [4][h*w] (adjacent pixels sample adjacent texels -> adjacent banks); a lane walks the
// candidates of a pixel (costvol_bwd_sweep), a flushed tap gradient is one LDS atomic.
//   part_src [kchunks][V][Cp/4][h*w][4]   partial g_src of this slice (every element written)
//   part_ref [kchunks][V][Cp/4][h*w][4]   partial g_ref of this slice and view
__global__ __launch_bounds__(kBwdThreads) void costvol_bwd_lds_kernel(const CostvolBwdArgs a, const int kchunks, const int abl_,
                                                                      float* __restrict__ part_src, float* __restrict__ part_ref) {
    const int abl = NRGBD_BWD_ABL_BITS(abl_);
    extern __shared__ float gl[];
    const int hw = a.h * a.w, words = a.Cp >> 2;
    const int kc = blockIdx.x, i = blockIdx.y, v = blockIdx.z, tid = threadIdx.x;
    for (int t = tid; t < 4 * hw; t += kBwdThreads) gl[t] = 0.f;
    __syncthreads();
    const int per = (a.D + kchunks - 1) / kchunks;
    const int k_begin = kc * per, k_end = min(a.D, k_begin + per);
    const size_t slab = (((size_t)kc * a.V + v) * words + i) * hw;

    for (int p = tid; p < hw; p += kBwdThreads) {
        const float rx = a.rays[p], ry = a.rays[hw + p], rz = a.rays[2 * hw + p];
        const float4 r = *reinterpret_cast<const float4*>(a.ref + (size_t)p * a.Cp + 4 * i);
        float gr[4] = {0.f, 0.f, 0.f, 0.f};
        costvol_bwd_sweep(a, abl, p, v, i, k_begin, k_end, rx, ry, rz, r, gr,
                          [&](int tex, int e, float x) { atomicAdd(gl + e * hw + ((abl & 4) ? p : tex), x); });
        *reinterpret_cast<float4*>(part_ref + (slab + p) * 4) = make_float4(gr[0], gr[1], gr[2], gr[3]);
    }
    __syncthreads();
    for (int t = tid; t < hw; t += kBwdThreads)
        *reinterpret_cast<float4*>(part_src + (slab + t) * 4) = make_float4(gl[t], gl[hw + t], gl[2 * hw + t], gl[3 * hw + t]);
}

// One thread per (view or reference, texel, channel word): adds the slices (and, for the reference image, the views)
// in index order and writes the NHWC gradients.
__global__ __launch_bounds__(256) void costvol_bwd_reduce_kernel(const float* __restrict__ part_src, const float* __restrict__ part_ref,
                                                                 float* __restrict__ g_src, float* __restrict__ g_ref,
                                                                 int V, int words, int hw, int kchunks) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)(V + 1) * hw * words;
    if (idx >= total) return;
    const int word = (int)(idx % words);
    const int t = (int)((idx / words) % hw);
    const int vv = (int)(idx / ((size_t)words * hw));
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vv < V) {
        for (int kc = 0; kc < kchunks; ++kc) {
            const float4 q = *reinterpret_cast<const float4*>(part_src + ((((size_t)kc * V + vv) * words + word) * hw + t) * 4);
            s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w;
        }
        *reinterpret_cast<float4*>(g_src + ((size_t)vv * hw + t) * (4 * words) + 4 * word) = s;
    } else {
        for (int kc = 0; kc < kchunks; ++kc)
            for (int v = 0; v < V; ++v) {
                const float4 q = *reinterpret_cast<const float4*>(part_ref + ((((size_t)kc * V + v) * words + word) * hw + t) * 4);
                s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w;
            }
        *reinterpret_cast<float4*>(g_ref + (size_t)t * (4 * words) + 4 * word) = s;
    }
}

// Depth slices of the LDS kernel: as many as keep the grid within one wave of workgroups (one per CU: its LDS
// plane fills most of the CU), at most 16.  0 = the grid does not fit in LDS (global-atomic kernel).
static int bwd_lds_kchunks(int V, int Cp, int D, int h, int w, int* out) {
    *out = 0;
    if ((size_t)h * w * 16 > kBwdLdsMax) return NRGBD_OK;
    int dev = 0, ncu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return (int)e;
    int kc = ncu / (V * (Cp >> 2));
    kc = kc < 1 ? 1 : (kc > 16 ? 16 : kc);
    *out = kc > D ? D : kc;
    return NRGBD_OK;
}

}  // namespace nrgbd

extern "C" int nrgbd_costvol_bwd_workspace(int V, int Cp, int D, int h, int w, size_t* bytes) {
    using namespace nrgbd;
    if (!bytes) return NRGBD_E_NULL;
    if (costvol_bwd_check_shape(V, Cp, Cp, D, h, w, NRGBD_DIST_L2) != NRGBD_OK) return NRGBD_E_SHAPE;
    int kc = 0;
    const int rc = bwd_lds_kchunks(V, Cp, D, h, w, &kc);
    if (rc != NRGBD_OK) return rc;
    *bytes = 2 * (size_t)kc * V * (Cp >> 2) * h * w * 4 * sizeof(float);
    return NRGBD_OK;
}

extern "C" int nrgbd_costvol_bwd(const float* ref_nhwc, const float* src_nhwc, const float* KR, const float* Kt,
                                 const float* rays, const float* d_candi, float cx, float cy, float sigma,
                                 int dist, int align_corners, const float* g_cost, float* g_ref, float* g_src,
                                 int V, int C, int Cp, int D, int h, int w, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    using namespace nrgbd;
    const CostvolBwdArgs a{ref_nhwc, src_nhwc, KR, Kt, rays, d_candi, g_cost, g_ref, g_src, cx, cy, sigma,
                           dist, align_corners, V, C, Cp, D, h, w};
    int rc = costvol_bwd_check(a);
    if (rc != NRGBD_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t hw = (size_t)h * w;
    const int abl = dev_env_int("NRGBD_BWD_ABL");
    int lds_kc = 0;
    rc = bwd_lds_kchunks(V, Cp, D, h, w, &lds_kc);
    if (rc != NRGBD_OK) return rc;
    if (lds_kc > 0) {
        const size_t half = (size_t)lds_kc * V * (Cp >> 2) * hw * 4;   // floats per partial array
        if (!workspace) return NRGBD_E_NULL;
        if (workspace_bytes < 2 * half * sizeof(float)) return NRGBD_E_SHAPE;
        if ((uintptr_t)workspace & 15) return NRGBD_E_ALIGN;
        float* part_src = static_cast<float*>(workspace);
        float* part_ref = part_src + half;
        const size_t lds = hw * 16;
        hipError_t e = hipSuccess;
        if (lds > 64 * 1024)   // the function's opt-in: always the maximum, never this call's size (a hipGraph replay runs under the current value)
            e = set_max_dynamic_lds(reinterpret_cast<const void*>(&costvol_bwd_lds_kernel), 160 * 1024);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(costvol_bwd_lds_kernel, dim3(lds_kc, Cp >> 2, V), dim3(kBwdThreads), lds, s, a, lds_kc, abl, part_src, part_ref);
        NRGBD_CHECK_LAUNCH();
        const size_t total = (size_t)(V + 1) * hw * (Cp >> 2);
        hipLaunchKernelGGL(costvol_bwd_reduce_kernel, dim3((unsigned)ceil_div((long)total, 256)), dim3(256), 0, s,
                           part_src, part_ref, g_src, g_ref, V, Cp >> 2, (int)hw, lds_kc);
        NRGBD_CHECK_LAUNCH();
        return NRGBD_OK;
    }
    hipError_t e = hipMemsetAsync(g_ref, 0, hw * Cp * sizeof(float), s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(g_src, 0, (size_t)V * hw * Cp * sizeof(float), s);
    if (e != hipSuccess) return (int)e;
    // slices of consecutive candidates: long enough for the register run-accumulation, parallelism comes from
    // the channel-word axis of the grid
    const int kchunks = D >= 32 ? 4 : (D >= 8 ? 2 : 1);
    hipLaunchKernelGGL(costvol_bwd_kernel, dim3(ceil_div((long)hw, 64), kchunks, Cp >> 2), dim3(64), 0, s, a, kchunks, abl);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}
