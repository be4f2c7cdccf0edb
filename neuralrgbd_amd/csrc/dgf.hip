// dgf.hip — the guided-filter refinement net (KVNET(refineNet_name='DGF'); neuralrgbd_amd/nets.py: DGFRefineNet), one launch.
//
// Replaces models/Refine.py:620-641 (RefineNet_DGF.forward: F.upsample(align_corners=True), the 3 -> 64 -> 1 per-pixel network,
// GuidedFilter), models/GF/guided_filter.py:54-97 and models/GF/box_filter.py: 82 launches over image-size temporaries when
// written with torch device operations (tools/bench_dgf.py).
//
// The reference's box filter takes differences of fp32 cumsums and its variance is E[x^2] - E[x]^2: both cancel, and on smooth
// images its fp32 output is metres off (README, "DGF").  This kernel computes the SAME function in the centred form — direct sums over
// the clipped 3 x 3 window, var = sum (x - mx)^2 / N —, which agrees with the reference evaluated in float64 to 1e-9 and stays
// within 1e-4 m of it in fp32.  It does not reproduce the reference's fp32 bits, on purpose.
//
// Per image pixel p, in this operation sequence (fp32; separate multiplies and adds except where an fma is written out; every
// division is an IEEE division):
//   y   bilinear, align_corners = True, coordinates in integers: num = i (h - 1), i0 = num / (H - 1),
//       lam = float(num % (H - 1)) / float(H - 1), i1 = min(i0 + 1, h - 1); the same along columns;
//       y = (1 - lr) ((1 - lc) d00 + lc d01) + lr ((1 - lc) d10 + lc d11)
//   x   b2 + sum_k w2[k] max(0, b1[k] + w1[k][0] r + w1[k][1] g + w1[k][2] b), k ascending, every multiply-add an fma
//   W(p) the 3 x 3 neighbourhood clipped to the image, N = |W| in {4, 6, 9}; sums in row-major order
//       mx = sum x / N, my = sum y / N, var = sum (x - mx)^2 / N, cov = sum (x - mx)(y - my) / N
//       A = cov / (var + eps), b = my - A mx
//   out = (sum_W A / N) x + (sum_W b / N)
//
// A workgroup of 256 lanes owns a 16 x 64 tile: x and y on tile + 2 into LDS (6 positions per lane; the 321 weights are wave-uniform
// loads, shared by the lane's six positions), A and b on tile + 1 into LDS, then 4 pixels of a row per lane.  For a position outside
// the image nothing is read at that position and nothing is stored: in stage 1 its lane slot stays in the wave and runs the network
// on zeros and the lerp on depth_lr's first elements (in-bounds loads, results discarded); in stages 2 and 3 such a neighbour's LDS
// index falls back to the window's centre and the value takes no part in the sums.  With n = 2 targets the network and the guide
// statistics are computed once; a target's operations do not depend on n, so its bits equal those of an n = 1 call.  No atomics, no
// workspace: capturable, and the same bits in every run.  Stores are 16 bytes per lane where the address allows it, element stores
// otherwise.
// Traffic: 12 bytes read and 4 n written per pixel; the halo re-evaluates 1360 / 1024 = 1.33 x of the network (5 VALU operations per
// hidden unit and position).  Measured: 13.5 / 16.1 us (n = 1 / 2) at 256 x 384 — 96 workgroups, one workgroup's dependent chain —
// and 23.9 / 29.4 us at 768 x 1024, 0.065 of the HBM peak: wave64 VALU issue binds it there.
#include "common.hpp"

namespace nrgbd {

constexpr int kDgfTy = NRGBD_DGF_TILE_Y, kDgfTx = NRGBD_DGF_TILE_X;       // 16 x 64
constexpr int kDgfXh = kDgfTy + 4, kDgfXw = kDgfTx + 4;                  // x, y: tile + 2
constexpr int kDgfAh = kDgfTy + 2, kDgfAw = kDgfTx + 2;                  // A, b: tile + 1
constexpr int kDgfHidden = 64;
constexpr int kDgfPos = (kDgfXh * kDgfXw + 255) / 256;                  // 6 positions of tile + 2 per lane
constexpr int kDgfMaxExtent = 16384;

template <int NT>
__global__ __launch_bounds__(256) void dgf_refine_kernel(const float* __restrict__ depth_lr, int h, int w,
                                                         const float* __restrict__ img, int H, int W,
                                                         const float* __restrict__ w1, const float* __restrict__ b1,
                                                         const float* __restrict__ w2, const float* __restrict__ b2, float eps,
                                                         float* __restrict__ out) {
    __shared__ float s_x[kDgfXh * kDgfXw];
    __shared__ float s_y[NT][kDgfXh * kDgfXw];
    __shared__ float s_A[NT][kDgfAh * kDgfAw];
    __shared__ float s_b[NT][kDgfAh * kDgfAw];
    __shared__ int s_i0[kDgfXh + kDgfXw];            // rows of tile + 2, then its columns: the low-resolution index ...
    __shared__ float s_lam[kDgfXh + kDgfXw];         // ... and the interpolation weight

    const int tid = threadIdx.x;
    const int ty0 = blockIdx.y * kDgfTy, tx0 = blockIdx.x * kDgfTx;
    const size_t plane = (size_t)H * W;

    // 0. the interpolation tables of the rows and columns of tile + 2 that lie inside the image
    if (tid < kDgfXh + kDgfXw) {
        const bool row = tid < kDgfXh;
        const int i = row ? ty0 - 2 + tid : tx0 - 2 + (tid - kDgfXh);
        const int lo = row ? h : w, hi = row ? H : W;
        if (i >= 0 && i < hi) {
            const int num = i * (lo - 1);
            const int q = num / (hi - 1);
            s_i0[tid] = q;
            s_lam[tid] = (float)(num - q * (hi - 1)) / (float)(hi - 1);
        }
    }

    __syncthreads();

    // 1. the guide x and the up-sampled targets y on tile + 2: the lane's positions side by side.  Every global load — the pixel's
    //    r, g, b and the four low-resolution depths per target — is issued before the network, whose 320 operations per position
    //    cover the latency; the weights are read once for all positions
    {
        float r[kDgfPos], g[kDgfPos], b[kDgfPos], acc[kDgfPos], d[NT][kDgfPos][4], lr[kDgfPos], lc[kDgfPos];
        bool in[kDgfPos];
        const float bias2 = b2[0];
#pragma unroll
        for (int j = 0; j < kDgfPos; ++j) {
            const int idx = tid + 256 * j;
            const int ry = idx / kDgfXw, rx = idx - ry * kDgfXw;
            const int gy = ty0 - 2 + ry, gx = tx0 - 2 + rx;
            in[j] = idx < kDgfXh * kDgfXw && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const size_t o = in[j] ? (size_t)gy * W + gx : 0;
            r[j] = in[j] ? img[o] : 0.f;
            g[j] = in[j] ? img[plane + o] : 0.f;
            b[j] = in[j] ? img[2 * plane + o] : 0.f;
            acc[j] = bias2;
            const int r0 = in[j] ? s_i0[ry] : 0, c0 = in[j] ? s_i0[kDgfXh + rx] : 0;
            lr[j] = in[j] ? s_lam[ry] : 0.f;
            lc[j] = in[j] ? s_lam[kDgfXh + rx] : 0.f;
            const int r1 = min(r0 + 1, h - 1), c1 = min(c0 + 1, w - 1);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float* dl = depth_lr + (size_t)t * h * w;
                d[t][j][0] = dl[(size_t)r0 * w + c0];
                d[t][j][1] = dl[(size_t)r0 * w + c1];
                d[t][j][2] = dl[(size_t)r1 * w + c0];
                d[t][j][3] = dl[(size_t)r1 * w + c1];
            }
        }
#pragma unroll 8
        for (int k = 0; k < kDgfHidden; ++k) {
            const float wr = w1[3 * k], wg = w1[3 * k + 1], wb = w1[3 * k + 2], bk = b1[k], vk = w2[k];
#pragma unroll
            for (int j = 0; j < kDgfPos; ++j) {
                const float hk = __builtin_fmaf(wb, b[j], __builtin_fmaf(wg, g[j], __builtin_fmaf(wr, r[j], bk)));
                acc[j] = __builtin_fmaf(vk, fmaxf(hk, 0.f), acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < kDgfPos; ++j) {
            if (!in[j]) continue;
            s_x[tid + 256 * j] = acc[j];
            const float er = 1.f - lr[j], ec = 1.f - lc[j];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float top = ec * d[t][j][0] + lc[j] * d[t][j][1];
                const float bot = ec * d[t][j][2] + lc[j] * d[t][j][3];
                s_y[t][tid + 256 * j] = er * top + lr[j] * bot;
            }
        }
    }
    __syncthreads();

    // 2. A and b on tile + 1.  The nine neighbours are read side by side (independent LDS reads); a neighbour outside the image is not
    //    read (its index falls back to the centre) and takes no part in the sums, which run in row-major order over the others
    for (int idx = tid; idx < kDgfAh * kDgfAw; idx += 256) {
        const int ay = idx / kDgfAw, ax = idx - ay * kDgfAw;
        const int gy = ty0 - 1 + ay, gx = tx0 - 1 + ax;
        if (gy < 0 || gy >= H || gx < 0 || gx >= W) continue;
        const int centre = (ay + 1) * kDgfXw + ax + 1;             // the window in the coordinates of tile + 2: rows ay .. ay + 2
        bool ok[9];
        int o[9];
        float xv[9], cx[9];
        int count = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int dy = k / 3, dx = k - 3 * dy;
            ok[k] = gy + dy - 1 >= 0 && gy + dy - 1 < H && gx + dx - 1 >= 0 && gx + dx - 1 < W;
            o[k] = ok[k] ? (ay + dy) * kDgfXw + ax + dx : centre;
            xv[k] = s_x[o[k]];
            count += ok[k] ? 1 : 0;
        }
        const float N = (float)count;
        float sx = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) sx = ok[k] ? sx + xv[k] : sx;
        const float mx = sx / N;
        float sv = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            cx[k] = xv[k] - mx;
            sv = ok[k] ? sv + cx[k] * cx[k] : sv;
        }
        const float den = sv / N + eps;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float yv[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) yv[k] = s_y[t][o[k]];
            float sy = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) sy = ok[k] ? sy + yv[k] : sy;
            const float my = sy / N;
            float sc = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) sc = ok[k] ? sc + cx[k] * (yv[k] - my) : sc;
            const float A = (sc / N) / den;
            s_A[t][idx] = A;
            s_b[t][idx] = my - A * mx;
        }
    }
    __syncthreads();

    // 3. the tile: 4 pixels of a row per lane; their windows share the 3 x 6 block of tile + 1 that starts at (py, px)
    {
        const int py = tid >> 4, px = (tid & 15) * 4;
        const int gy = ty0 + py, gx0 = tx0 + px;
        if (gy >= H || gx0 >= W) return;
        const int centre = (py + 1) * kDgfAw + px + 1;             // the lane's first pixel: inside the image
        bool rok[3], cok[6];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) rok[dy] = gy + dy - 1 >= 0 && gy + dy - 1 < H;
#pragma unroll
        for (int c = 0; c < 6; ++c) cok[c] = gx0 + c - 1 >= 0 && gx0 + c - 1 < W;
        float xc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) xc[e] = s_x[(py + 2) * kDgfXw + px + 2 + (gx0 + e < W ? e : 0)];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float av[3][6], bv[3][6];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    const int o = (rok[dy] && cok[c]) ? (py + dy) * kDgfAw + px + c : centre;
                    av[dy][c] = s_A[t][o];
                    bv[dy][c] = s_b[t][o];
                }
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float sa = 0.f, sb = 0.f;
                int count = 0;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const bool ok = rok[dy] && cok[e + dx];
                        sa = ok ? sa + av[dy][e + dx] : sa;
                        sb = ok ? sb + bv[dy][e + dx] : sb;
                        count += ok ? 1 : 0;
                    }
                const float N = (float)(count > 0 ? count : 1);    // count = 0 only for a pixel past the right edge: not stored
                v[e] = (sa / N) * xc[e] + sb / N;
            }
            float* p = out + (size_t)t * plane + (size_t)gy * W + gx0;
            if (gx0 + 3 < W && ((uintptr_t)p & 15) == 0) {
                *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (gx0 + e < W) p[e] = v[e];
            }
        }
    }
}

}  // namespace nrgbd

// Refine.py:620-641, GF/guided_filter.py:54-97, GF/box_filter.py (see the header of this file)
extern "C" int nrgbd_dgf_refine_f32(const float* depth_lr, int n, int h, int w, const float* img, int H, int W, const float* w1,
                                    const float* b1, const float* w2, const float* b2, float eps, float* out, void* stream) {
    using namespace nrgbd;
    if (!depth_lr || !img || !w1 || !b1 || !w2 || !b2 || !out) return NRGBD_E_NULL;
    if (h <= 0 || w <= 0 || H <= 0 || W <= 0 || H > kDgfMaxExtent || W > kDgfMaxExtent) return NRGBD_E_SHAPE;
    if (H % h != 0 || W % w != 0 || H / h != W / w || H / h < 2) return NRGBD_E_SHAPE;
    if (H <= 3 || W <= 3) return NRGBD_E_SHAPE;                  // guided_filter.py:74: h_x > 2 r + 1
    if (n != 1 && n != 2) return NRGBD_E_ARG;
    if (!(eps >= 0.f)) return NRGBD_E_ARG;                       // negative or NaN
    const dim3 grid((W + kDgfTx - 1) / kDgfTx, (H + kDgfTy - 1) / kDgfTy);
    if (n == 1)
        hipLaunchKernelGGL(dgf_refine_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, depth_lr, h, w, img, H, W, w1, b1, w2, b2, eps, out);
    else
        hipLaunchKernelGGL(dgf_refine_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, depth_lr, h, w, img, H, W, w1, b1, w2, b2, eps, out);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}
