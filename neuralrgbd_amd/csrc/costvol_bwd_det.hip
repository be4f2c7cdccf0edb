// costvol_bwd_det.hip — the cost-volume backward of costvol_bwd.hip with bit-reproducible results (opt-in: ops.costvol_bwd(...,
// deterministic=True), neuralrgbd_amd.autograd.deterministic()).  Same mathematics, same sample cell and fractions (make_sweep_term,
// sweep_sample_pos, bilinear_zeros, lerp4 of common.hpp: the forward's bits), L2 and L1, both align_corners values, any ray table,
// any candidate order.  No floating-point atomic anywhere in this file.
//
// g_ref[p, c] is a sum over (view, candidate) of ONE pixel: a lane owns (pixel, 16-byte channel word), walks v = 0..V-1 and
// k = 0..D-1 in index order and keeps the sum in registers.  One fixed order, one plain store.
//
// g_src[v, texel, c] is a scatter: many (pixel, candidate) samples land on one texel in an order the hardware decides.  It is summed
// in fixed point, which makes the order irrelevant (integer addition is associative):
//   pass 1  (costvol_bwd_det_sweep<0>)  the sample loop.  A lane keeps the four tap gradients of the current 2x2 source cell in
//           registers while consecutive candidates stay in that cell (fma in candidate order, like costvol_bwd.hip) and emits them
//           when the cell changes: the emitted fp32 values are the TERMS.  Each term's absolute bit pattern goes into a uint32 plane
//           with an integer atomic max (non-negative floats order like unsigned integers).
//   pass 2  (costvol_bwd_det_sweep<1>)  the same device function again: the same terms, bit for bit (the library is compiled with
//           -ffp-contract=off and without fast-math: every operation is individually rounded IEEE arithmetic, so two instantiations
//           of one expression cannot differ).  With E the exponent of the element's largest |term| (from pass 1) a term is scaled
//           by the exact power of two 2^(S - E), rounded ONCE to an integer (round to nearest even) and added to an int64 plane with
//           an integer atomic.  This pass also writes g_ref.
//   pass 3  (costvol_bwd_det_convert)  one lane per (view, texel, channel word): int64 -> double -> times 2^(E - S) (exact) -> ONE
//           rounding to fp32, written as a float4 of the NHWC gradient.  The padding lanes C .. Cp-1 never receive a term: exactly 0.
// S = min(40, 61 - ceil(log2(h w D))): the largest scaled term is below 2^(S+1) and an element receives at most h w D terms (a
// sample emits at most one term per tap, its four taps are different texels), so |sum| < 2^62: the int64 cannot overflow.  Shapes
// with S < 32 (h w D > 2^29) are refused (NRGBD_E_SHAPE).
//
// Error of an element with n terms t_i, M = max |t_i| in [2^E, 2^(E+1)), against the exact sum of the same terms:
//   quantisation  each term is rounded to a multiple of 2^(E-S): at most 2^(E-S-1) <= M 2^-(S+1) each, n M 2^-41 in all at S = 40
//                 (n M 2^-33 at the refusal limit S = 32);
//   conversion    (double) of the int64 is exact below 2^53 and off by at most 2^-53 relative above; the scaling is exact; the one
//                 rounding to fp32 adds u |sum|, u = 2^-24.
// tests/costvol_bwd_exact.py bounds an element by gamma(C0 + n) A + ..., A = sum |t_i| >= M, gamma(m) ~ m 2^-24, where n - 1 of the
// roundings in gamma are the additions of an fp32 summation in any order.  This path replaces those n - 1 roundings (up to
// (n - 1) 2^-24 A) by n 2^-(S+1) M + 2^-24 |sum| <= (n 2^-33 + 2^-24) A: inside the same 1 x bound with room to spare, for any n.
// (The terms themselves — weights, lerp4, difference, ds * g, the run fma — come from costvol_bwd_sweep of costvol_bwd.hpp, the one
// function that costvol_bwd.hip's kernels call too: the C0 part.)
//
// Special values.  An element all of whose terms are zero (or that receives none) is exactly +0.  An element that receives a
// non-finite term (Inf or NaN: non-finite features or g_cost) is NaN — also where the atomic kernels would give an infinity.
// g_ref propagates non-finite values like any fp32 sum.
//
// Reproducibility.  The launch geometry depends on the shape arguments only: (ceil(h w / 256), Cp / 4) workgroups of 256 lanes
// for the sweeps, no depth slicing, no LDS, nothing derived from the device's CU count (costvol_bwd.hip's LDS slice count is
// CUs / (V Cp / 4): its summation order changes with the part; this path's results do not).  One path for every grid.  The
// workspace (12 bytes per g_src element) is cleared by the entry itself on the caller's stream; every output element is written;
// nothing is read before it is written.  Every loop's trip count is a shape argument; no workgroup waits for another; no
// allocation, no host synchronisation: capture-safe like every other entry.
//
// Layout of the planes: [V][Cp][h w] (component planes, like the LDS kernel's), so the 64 lanes of a wave — 64 neighbouring pixels,
// which sample neighbouring texels — issue each atomic on one or two contiguous runs instead of 64 addresses 4 Cp bytes apart.
#include "costvol_bwd.hpp"

namespace nrgbd {

struct CostvolBwdDetArgs : CostvolBwdArgs {
    unsigned long long* sum;   // [V][Cp][hw] two's-complement int64 sums of the scaled terms
    unsigned int* mx;          // [V][Cp][hw] largest |term| as fp32 bits
    int S;                     // scaled exponent of an element's largest term
};

constexpr int kDetThreads = 256;

// Exponent field of the element's scale: E + 127 with subnormal maxima counted as 2^-126.
__device__ __forceinline__ int det_exp_field(unsigned int m) {
    const int e = (int)(m >> 23);
    return e < 1 ? 1 : e;
}

// 2^n as a double, n in [-1022, 1023]
__device__ __forceinline__ double det_pow2(int n) {
    return __longlong_as_double((long long)(1023 + n) << 52);
}

// PASS 0: maxima of |term|.  PASS 1: scaled integer sums + g_ref.  One lane = one pixel x one 16-byte channel word, all views, all
// candidates (costvol_bwd_sweep); pass 0 never reads gr, so its sum is dead code there.
template <int PASS>
__global__ __launch_bounds__(kDetThreads) void costvol_bwd_det_sweep(const CostvolBwdDetArgs a) {
    const int hw = a.h * a.w;
    const int p = blockIdx.x * kDetThreads + threadIdx.x;
    if (p >= hw) return;
    const int i = blockIdx.y;                      // channel word
    const float rx = a.rays[p], ry = a.rays[hw + p], rz = a.rays[2 * hw + p];
    const float4 r = *reinterpret_cast<const float4*>(a.ref + (size_t)p * a.Cp + 4 * i);
    float gr[4] = {0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < a.V; ++v) {
        const size_t plane = ((size_t)v * a.Cp + 4 * i) * hw;        // component e of this word: plane + e * hw + texel
        costvol_bwd_sweep(a, 0, p, v, i, 0, a.D, rx, ry, rz, r, gr, [&](int tex, int e, float t) {
            const size_t at = plane + (size_t)e * hw + tex;
            if (PASS == 0) {
                const unsigned int bits = __float_as_uint(t) & 0x7fffffffu;
                // the plane only grows during this kernel: a value read here, however stale, is a lower bound of the final
                // maximum, so skipping the atomic when it already covers `bits` cannot change the result
                if (bits > __hip_atomic_load(a.mx + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    atomicMax(a.mx + at, bits);
            } else {
                const unsigned int m = a.mx[at];
                if (m >= 0x7f800000u) return;              // a non-finite term landed here: pass 3 writes NaN
                const long long q = __double2ll_rn((double)t * det_pow2(a.S + 127 - det_exp_field(m)));
                if (q != 0) atomicAdd(a.sum + at, (unsigned long long)q);
            }
        });
    }
    if (PASS == 1)
        *reinterpret_cast<float4*>(a.g_ref + (size_t)p * a.Cp + 4 * i) = make_float4(gr[0], gr[1], gr[2], gr[3]);
}

// One lane per (view, channel word, texel), texel fastest: the planes are read in runs, g_src is written as float4.
__global__ __launch_bounds__(256) void costvol_bwd_det_convert(const unsigned long long* __restrict__ sum,
                                                               const unsigned int* __restrict__ mx, float* __restrict__ g_src,
                                                               int V, int words, int hw, int S) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)V * words * hw) return;
    const int t = (int)(idx % hw);
    const int word = (int)((idx / hw) % words);
    const int v = (int)(idx / ((size_t)hw * words));
    const int Cp = 4 * words;
    const size_t plane = ((size_t)v * Cp + 4 * word) * hw + t;
    float out[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned int m = mx[plane + (size_t)e * hw];
        const long long s = (long long)sum[plane + (size_t)e * hw];
        out[e] = m == 0u ? 0.f : (m >= 0x7f800000u ? __builtin_nanf("") : (float)((double)s * det_pow2(det_exp_field(m) - 127 - S)));
    }
    *reinterpret_cast<float4*>(g_src + ((size_t)v * hw + t) * Cp + 4 * word) = make_float4(out[0], out[1], out[2], out[3]);
}

// S of the file header, or -1 where the shape is refused.
static int det_scale_exponent(int D, int h, int w) {
    const unsigned long long n = (unsigned long long)h * (unsigned long long)w * (unsigned long long)D;
    int lg = 0;
    while ((1ull << lg) < n) ++lg;                 // ceil(log2 n), n <= 2^31 * 2^8
    const int S = 61 - lg < 40 ? 61 - lg : 40;
    return S < 32 ? -1 : S;
}

}  // namespace nrgbd

extern "C" int nrgbd_costvol_bwd_det_workspace(int V, int Cp, int D, int h, int w, size_t* bytes) {
    using namespace nrgbd;
    if (!bytes) return NRGBD_E_NULL;
    if (costvol_bwd_check_shape(V, Cp, Cp, D, h, w, NRGBD_DIST_L2) != NRGBD_OK || det_scale_exponent(D, h, w) < 0) return NRGBD_E_SHAPE;
    *bytes = (size_t)V * Cp * h * w * (sizeof(unsigned long long) + sizeof(unsigned int));
    return NRGBD_OK;
}

extern "C" int nrgbd_costvol_bwd_det(const float* ref_nhwc, const float* src_nhwc, const float* KR, const float* Kt,
                                     const float* rays, const float* d_candi, float cx, float cy, float sigma,
                                     int dist, int align_corners, const float* g_cost, float* g_ref, float* g_src,
                                     int V, int C, int Cp, int D, int h, int w, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    using namespace nrgbd;
    if (!workspace) return NRGBD_E_NULL;
    CostvolBwdDetArgs a{{ref_nhwc, src_nhwc, KR, Kt, rays, d_candi, g_cost, g_ref, g_src, cx, cy, sigma,
                         dist, align_corners, V, C, Cp, D, h, w}};
    const int rc = costvol_bwd_check(a);
    if (rc != NRGBD_OK) return rc;
    a.S = det_scale_exponent(D, h, w);
    if (a.S < 0) return NRGBD_E_SHAPE;
    const size_t hw = (size_t)h * w, n = (size_t)V * Cp * hw;
    const size_t need = n * (sizeof(unsigned long long) + sizeof(unsigned int));
    if (workspace_bytes < need) return NRGBD_E_SHAPE;
    if ((uintptr_t)workspace & 15) return NRGBD_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    a.sum = static_cast<unsigned long long*>(workspace);
    a.mx = reinterpret_cast<unsigned int*>(a.sum + n);
    hipError_t e = hipMemsetAsync(workspace, 0, need, s);
    if (e != hipSuccess) return (int)e;
    const dim3 grid(ceil_div((long)hw, kDetThreads), Cp >> 2);
    hipLaunchKernelGGL(costvol_bwd_det_sweep<0>, grid, dim3(kDetThreads), 0, s, a);
    NRGBD_CHECK_LAUNCH();
    hipLaunchKernelGGL(costvol_bwd_det_sweep<1>, grid, dim3(kDetThreads), 0, s, a);
    NRGBD_CHECK_LAUNCH();
    hipLaunchKernelGGL(costvol_bwd_det_convert, dim3((unsigned)ceil_div((long)n / 4, 256)), dim3(256), 0, s, a.sum, a.mx, g_src,
                       V, Cp >> 2, (int)hw, a.S);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}
