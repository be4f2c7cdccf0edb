// costvol_bwd.hpp — what the cost-volume backward kernels share: the argument block, the argument checks of the C entries and
// THE sample loop.  costvol_bwd.hip (global float atomics; LDS float atomics + fixed-order reduce) and costvol_bwd_det.hip (fixed
// point, bit-reproducible) differ only in the candidate range a lane walks and in where a flushed tap gradient goes.
#pragma once
#include <limits.h>

#include "costvol.hpp"

namespace nrgbd {

struct CostvolBwdArgs {
    const float* ref; const float* src; const float* KR; const float* Kt; const float* rays;
    const float* d_candi; const float* g_cost;
    float* g_ref; float* g_src;
    float cx, cy, sigma;
    int dist, align, V, C, Cp, D, h, w;
};

// The argument checks the four C entries share, in the order (null,) shape, align, arg: the first that fails is the return code.
// h * w is bounded last because the sample loop indexes texels with int (4 h w: the four component planes of a channel word).
// The _workspace queries, which know neither C nor dist, pass C = Cp and NRGBD_DIST_L2 and answer NRGBD_E_SHAPE for any refusal
// (an unpadded Cp has always been a shape error there).
inline int costvol_bwd_check_shape(int V, int C, int Cp, int D, int h, int w, int dist) {
    if (V <= 0 || V > NRGBD_MAX_V || C <= 0 || D <= 0 || D > NRGBD_MAX_D || h <= 0 || w <= 0) return NRGBD_E_SHAPE;
    if ((Cp & 3) || Cp < C || Cp - C > 3) return NRGBD_E_ALIGN;
    if (dist != NRGBD_DIST_L2 && dist != NRGBD_DIST_L1) return NRGBD_E_ARG;
    if ((long long)h * w > INT_MAX / 4) return NRGBD_E_SHAPE;
    return NRGBD_OK;
}

inline int costvol_bwd_check(const CostvolBwdArgs& a) {
    if (!a.ref || !a.src || !a.KR || !a.Kt || !a.rays || !a.d_candi || !a.g_cost || !a.g_ref || !a.g_src) return NRGBD_E_NULL;
    return costvol_bwd_check_shape(a.V, a.C, a.Cp, a.D, a.h, a.w, a.dist);
}

// The sweep of one (pixel p, source view v, 16-byte channel word i) over the depth candidates [k_begin, k_end): (rx, ry, rz) is the
// pixel's ray, r its word of the reference features; the word's share of g_ref is subtracted from gr, its share of g_src goes to
// emit(texel, e, value): texel = y * w + x of a tap in view v, e the component of the word.
// Sampling positions are recomputed exactly as in the forward kernels.  Consecutive candidates of a pixel sample neighbouring
// positions along its epipolar line — for the far planes the SAME 2x2 source cell for several candidates in a row — so the four
// tap gradients are accumulated in registers (fma in candidate order) while the cell stays the same and emitted only when it
// changes, and once at the end: 4-8x fewer atomics than one per (pixel, candidate, view, channel); the kernels are atomic-bound.
// Zero register terms (an invalid tap: weight 0, a dead channel, a padding lane) are not emitted.
// abl: developer ablation bits (NRGBD_BWD_ABL), 1 = nothing emitted, 2 = no tap loads (results invalid); a constexpr 0 in the product
// library.
template <class Emit>
__device__ __forceinline__ void costvol_bwd_sweep(const CostvolBwdArgs& a, const int abl, const int p, const int v, const int i,
                                                  const int k_begin, const int k_end, const float rx, const float ry, const float rz,
                                                  const float4 r, float (&gr)[4], Emit emit) {
    const int hw = a.h * a.w;
    const float wf = (float)a.w, hf = (float)a.h;
    const int ncomp = min(4, a.C - 4 * i);         // valid components of this word
    const SweepTerm st = make_sweep_term(a.KR + 9 * v, a.Kt + 3 * v, rx, ry, rz);
    const float* sv = a.src + (size_t)v * hw * a.Cp + 4 * i;
    // register accumulator of the current cell: 4 taps x 4 components
    float acc[4][4];
    float cx0 = -1e30f, cy0 = -1e30f;              // floor of the current cell (never matches initially)
    int o[4] = {0, 0, 0, 0};
    bool have = false;
    auto flush = [&]() {
        if (!have) return;
#pragma unroll
        for (int tpi = 0; tpi < 4; ++tpi)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (acc[tpi][e] != 0.f && !(abl & 1)) emit(o[tpi], e, acc[tpi][e]);
    };
    for (int k = k_begin; k < k_end; ++k) {
        const float gk = a.g_cost[(size_t)k * hw + p] / a.sigma;
        float ix, iy;
        sweep_sample_pos(st, a.d_candi[k], a.cx, a.cy, wf, hf, a.align != 0, ix, iy);
        const Bilinear b = bilinear_zeros(ix, iy, a.w, a.h);
        const float x0f = floorf(ix), y0f = floorf(iy);
        if (!(x0f == cx0 && y0f == cy0)) {          // new cell (also taken for NaN positions)
            flush();
            cx0 = x0f; cy0 = y0f; have = true;
            o[0] = b.y0 * a.w + b.x0; o[1] = b.y0 * a.w + b.x1;
            o[2] = b.y1 * a.w + b.x0; o[3] = b.y1 * a.w + b.x1;
#pragma unroll
            for (int tpi = 0; tpi < 4; ++tpi)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[tpi][e] = 0.f;
        }
        if (gk == 0.f) continue;
        float4 A = r, B = r, Cc = r, Dd = r;
        if (!(abl & 2)) {
            A = *reinterpret_cast<const float4*>(sv + (size_t)o[0] * a.Cp);
            B = *reinterpret_cast<const float4*>(sv + (size_t)o[1] * a.Cp);
            Cc = *reinterpret_cast<const float4*>(sv + (size_t)o[2] * a.Cp);
            Dd = *reinterpret_cast<const float4*>(sv + (size_t)o[3] * a.Cp);
        }
        const float df[4] = {lerp4(A.x, B.x, Cc.x, Dd.x, b) - r.x, lerp4(A.y, B.y, Cc.y, Dd.y, b) - r.y,
                             lerp4(A.z, B.z, Cc.z, Dd.z, b) - r.z, lerp4(A.w, B.w, Cc.w, Dd.w, b) - r.w};
        const float wt[4] = {b.nw, b.ne, b.sw, b.se};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= ncomp) continue;
            const float ds = (a.dist == NRGBD_DIST_L2) ? 2.f * df[e] : (df[e] > 0.f ? 1.f : (df[e] < 0.f ? -1.f : 0.f));
            const float c = ds * gk;
            gr[e] -= c;
#pragma unroll
            for (int tpi = 0; tpi < 4; ++tpi) acc[tpi][e] = __builtin_fmaf(wt[tpi], c, acc[tpi][e]);
        }
    }
    flush();
}

}  // namespace nrgbd
