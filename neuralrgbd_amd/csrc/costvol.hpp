// costvol.hpp — argument block and launchers shared by the cost-volume kernels.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace nrgbd {

struct CostvolArgs {
    const float* ref;      // [h][w][Cp]
    const float* src;      // [V][h][w][Cp]
    const float* KR;       // [V][9]
    const float* Kt;       // [V][3]
    const float* rays;     // [3][hw]
    const float* d_candi;  // [D]
    float* out_cost;       // [D][hw] or null
    float* out_logp;       // [D][hw] or null
    float cx, cy, sigma;
    int dist, align;
    int V, C, Cp, D, h, w;
    int nsingle;           // LDS generation: leading candidates that get a workgroup each (set by the launcher)
    int debug;             // developer bits, honoured only in -DNRGBD_DEV builds (env NRGBD_ABLATE).  LDS and quad generations: 1 = no staging
                           // (every tap from global memory), 2 = no math; LDS generation only: 4 = XCD-owned tile order, 8 = singles on any
                           // grid, (g+1)<<8 = run candidate group g only.  16, 32 and 64 mean nothing any more (costvol_quad.hip, "tried and rejected")
    int nchunk, kchunk;    // quad generation: candidate chunks per tile / candidates per chunk (set by the launcher)
    int fuse_softmax;      // quad generation: the workgroup owns all D candidates and also writes out_logp
    float rcx, rcy, rsigma;  // quad generation: RN(1/cx), RN(1/cy), RN(1/sigma) (host, double precision) for div_by_const
    long long* trace;      // developer builds: per-workgroup phase clocks [workgroups][24] (tools/cv_trace.py); null in the product library
};

// Developer ablation bits are compiled out of the product library: a stray environment variable must never change results.
#ifdef NRGBD_DEV
#define NRGBD_DBG(a, bits) ((a).debug & (bits))
#else
#define NRGBD_DBG(a, bits) 0
#endif

enum { NRGBD_GEN_AUTO = 0, NRGBD_GEN_GATHER = 1, NRGBD_GEN_LDS = 2, NRGBD_GEN_QUAD = 3 };

// Cp / 4 values with an instantiation of the gather kernel's register-cached form and of the LDS generation: the two launch
// switches and costvol_lds_supported are generated from this one list
#define NRGBD_CP4_CASES(X) X(1) X(2) X(3) X(4) X(8) X(9) X(16) X(17)

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (N > 0) {
        static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

// Bilinear tap weights with zeros padding (a corner outside the image contributes nothing), the un-clamped integer corner and
// which of its rows / columns lie inside the image.  (bilinear_zeros of common.hpp also returns the CLAMPED integer corners,
// which the staged kernels do not need.)
struct TapW {
    float nw, ne, sw, se, x0f, y0f;
    bool vx0, vx1, vy0, vy1;
    __device__ __forceinline__ bool any() const { return (vx0 || vx1) && (vy0 || vy1); }   // some tap lies inside the image (lane masks: scalar-unit work)
};
__device__ __forceinline__ TapW tap_weights(float ix, float iy, float wf, float hf) {
    TapW t;
    t.x0f = floorf(ix); t.y0f = floorf(iy);
    const float fx = ix - t.x0f, fy = iy - t.y0f, ex = 1.f - fx, ey = 1.f - fy;
    const float x1f = t.x0f + 1.f, y1f = t.y0f + 1.f;
    t.vx0 = (t.x0f >= 0.f) && (t.x0f <= wf - 1.f); t.vx1 = (x1f >= 0.f) && (x1f <= wf - 1.f);
    t.vy0 = (t.y0f >= 0.f) && (t.y0f <= hf - 1.f); t.vy1 = (y1f >= 0.f) && (y1f <= hf - 1.f);
    t.nw = (t.vx0 && t.vy0) ? ey * ex : 0.f; t.ne = (t.vx1 && t.vy0) ? ey * fx : 0.f;
    t.sw = (t.vx0 && t.vy1) ? fy * ex : 0.f; t.se = (t.vx1 && t.vy1) ? fy * fx : 0.f;
    return t;
}

// |s| or s*s accumulated into `acc` (metric fixed at compile time: no branch inside a channel loop)
template <int DIST>
__device__ __forceinline__ float dist_acc(float s, float acc) {
    if constexpr (DIST == NRGBD_DIST_L2) return __builtin_fmaf(s, s, acc);
    else return acc + fabsf(s);
}

// All four taps out of view: distance of the first `ncomp` channels of a reference word to the zero vector
__device__ __forceinline__ float zero_sample_dist(float rx, float ry, float rz, float rw, int ncomp, int dist, float acc) {
    const float c4[4] = {rx, ry, rz, rw};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e < ncomp) {
            const float s = 0.f - c4[e];
            acc = (dist == NRGBD_DIST_L2) ? dist_acc<NRGBD_DIST_L2>(s, acc) : dist_acc<NRGBD_DIST_L1>(s, acc);
        }
    return acc;
}

// costvol_lds.hip: LDS-staged generation (returns NRGBD_E_SHAPE when Cp/4 has no instantiation)
int launch_costvol_lds(const CostvolArgs& a, hipStream_t stream);
bool costvol_lds_supported(int cp4);
// costvol_quad.hip: generation 3 (4 lanes per (pixel, candidate), conflict-free LDS taps, fused log-softmax)
bool costvol_quad_supported(const CostvolArgs& a);
int launch_costvol_quad(const CostvolArgs& a, hipStream_t stream, bool* did_softmax);
// softmax.hip
int launch_logsoftmax_d(const float* a, const float* b, float scale, float* out, int D, size_t n,
                        hipStream_t stream);

}  // namespace nrgbd
