// ingest.hip — the two memory movers in front of a frame of the video stream (neuralrgbd_amd/video.py: VideoDepthStream).
//
// frame_ingest_kernel   one uint8 camera frame -> the normalised fp32 planar image the network reads, written into a slot of the
//                       stream's frame ring.  Replaces the loaders' image preparation (mdataloader/scanNet.py:368-369,429-430 and
//                       utils/preprocess.py:14-35: PIL.Image.NEAREST resize to the network size, ToTensor, Normalize) and the upload of
//                       the fp32 result: per element ((float)u / 255.0f - mean_c) / std_c with two IEEE fp32 divisions in that order
//                       (-ffp-contract=off; `/` is the correctly rounded division) = ToTensor followed by Normalize bit for bit.
//                       Resize: nearest at pixel centres in integers, sy = ((2y + 1) Hin) / (2 Hout), sx likewise — Pillow's NEAREST.
// window_gather_kernel  the 2r + 1 slots of the ring -> the window [V,3,H,W] + [3,H,W] that DepthStream.step takes
//                       (test_KVNet.py:195,213: split_frame_list and the list of source images; torch.stack of the slots).
//
// Both write 16 bytes per lane to consecutive addresses (one wave = 1 KiB per store instruction) and use no LDS.  The ingest has two
// forms.  Wout % 4 == 0 (every network size): frame_ingest_rows_kernel, one workgroup row per (channel, output row) from the grid's
// y / z indices, a lane's four pixels from ONE integer division — the source column of the next pixel follows by adding
// (2 Win) / (2 Wout) and carrying the remainder, which is the same integer — and one more for the row.  Any other width:
// frame_ingest_kernel addresses the slot FLAT, 4 elements of [3][Hout][Wout] per lane: the slot is 16-byte aligned and so is every
// group, whatever Wout is; a group may straddle a row or a plane (the coordinates carry over), and the last 3 Hout Wout mod 4 elements
// go out as scalar stores.  The source is read through the caches: an interleaved frame is read once per channel (3.8 MB at
// 1296 x 968 against 9.4 MB written).  The wave64 VALU binds both: measured at 1296 x 968 -> 1024 x 768, 10.3 us for the flat
// form (ten integer divisions per lane) and 6.3 us for the row form (two, and the eight IEEE divisions of the arithmetic).
#include "common.hpp"

namespace nrgbd {

constexpr int kIngestMaxDim = 16384;        // (2x + 1) * Win < 2^31
constexpr int kGatherMaxV = 6;

struct IngestNorm {
    float mean[3];
    float stdv[3];
};

template <bool CHW, bool RESIZE>
__device__ __forceinline__ float ingest_element(const unsigned char* __restrict__ src, long pitch, int Hin, int Win, int Hout, int Wout,
                                                const IngestNorm& nm, int c, int y, int x) {
    const int sy = RESIZE ? ((2 * y + 1) * Hin) / (2 * Hout) : y;
    const int sx = RESIZE ? ((2 * x + 1) * Win) / (2 * Wout) : x;
    const size_t off = CHW ? ((size_t)c * Hin + sy) * (size_t)pitch + sx : (size_t)sy * (size_t)pitch + 3 * (size_t)sx + c;
    const float u = (float)src[off];
    return (u / 255.0f - nm.mean[c]) / nm.stdv[c];
}

template <bool CHW, bool RESIZE>
__global__ __launch_bounds__(256) void frame_ingest_kernel(const unsigned char* __restrict__ src, long pitch, int Hin, int Win,
                                                           const IngestNorm nm, float* __restrict__ dst, int Hout, int Wout) {
    const int total = 3 * Hout * Wout;                          // <= 3 * 2^28
    const int e0 = 4 * (int)(blockIdx.x * 256 + threadIdx.x);   // < total + 1024
    if (e0 >= total) return;
    const int plane = Hout * Wout;
    int c = e0 / plane;
    const int rem = e0 - c * plane;
    int y = rem / Wout;
    int x = rem - y * Wout;
    const int n = total - e0 < 4 ? total - e0 : 4;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = 0.f;
        if (j < n) {
            v[j] = ingest_element<CHW, RESIZE>(src, pitch, Hin, Win, Hout, Wout, nm, c, y, x);
            if (++x == Wout) {
                x = 0;
                if (++y == Hout) { y = 0; ++c; }
            }
        }
    }
    if (n == 4) {
        *reinterpret_cast<float4*>(dst + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < n; ++j) dst[e0 + j] = v[j];         // the tail: at most 3 elements of the whole image
    }
}

// Wout % 4 == 0.  grid = (ceil(Wout / 1024), Hout, 3); qstep = (2 Win) / (2 Wout), rstep = (2 Win) % (2 Wout).
template <bool CHW, bool RESIZE>
__global__ __launch_bounds__(256) void frame_ingest_rows_kernel(const unsigned char* __restrict__ src, long pitch, int Hin, int Win,
                                                                const IngestNorm nm, float* __restrict__ dst, int Hout, int Wout,
                                                                int qstep, int rstep) {
    const int c = blockIdx.z, y = blockIdx.y;
    const int x0 = 4 * (int)(blockIdx.x * 256 + threadIdx.x);
    if (x0 >= Wout) return;
    const int sy = RESIZE ? ((2 * y + 1) * Hin) / (2 * Hout) : y;
    const unsigned char* __restrict__ row = CHW ? src + ((size_t)c * Hin + sy) * (size_t)pitch : src + (size_t)sy * (size_t)pitch + c;
    int sx = x0, rem = 0;
    if (RESIZE) {
        const int num = (2 * x0 + 1) * Win;
        sx = num / (2 * Wout);
        rem = num - sx * (2 * Wout);
    }
    const float mean = nm.mean[c], stdv = nm.stdv[c];
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float u = (float)row[CHW ? sx : 3 * sx];
        v[j] = (u / 255.0f - mean) / stdv;
        if (RESIZE) {                                               // ((2 (x + 1) + 1) Win) / (2 Wout) from the quotient and remainder at x
            sx += qstep;
            rem += rstep;
            if (rem >= 2 * Wout) { rem -= 2 * Wout; ++sx; }
        } else {
            ++sx;
        }
    }
    *reinterpret_cast<float4*>(dst + ((size_t)c * Hout + y) * (size_t)Wout + x0) = make_float4(v[0], v[1], v[2], v[3]);
}

struct GatherSlots {
    int idx[kGatherMaxV + 1];
};

// blockIdx.y = image of the window (0 .. V - 1: sources, V: the reference); VEC: 16 bytes per lane, else one element per lane
template <bool VEC>
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ ring, long slot_stride, const GatherSlots slots, int V,
                                                            float* __restrict__ src, float* __restrict__ ref, int n) {
    const int img = blockIdx.y;
    const float* __restrict__ in = ring + (size_t)slots.idx[img] * (size_t)slot_stride;
    float* __restrict__ out = img < V ? src + (size_t)img * n : ref;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (VEC) {
        if (4 * i < n) reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(in)[i];
    } else {
        if (i < n) out[i] = in[i];
    }
}

}  // namespace nrgbd

extern "C" int nrgbd_frame_ingest_u8(const unsigned char* src, int Hin, int Win, long pitch, int layout, float mean0, float mean1,
                                     float mean2, float std0, float std1, float std2, float* dst, int Hout, int Wout, void* stream) {
    using namespace nrgbd;
    if (!src || !dst) return NRGBD_E_NULL;
    if (Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || Hin > kIngestMaxDim || Win > kIngestMaxDim || Hout > kIngestMaxDim ||
        Wout > kIngestMaxDim)
        return NRGBD_E_SHAPE;
    if (layout != 0 && layout != 1) return NRGBD_E_ARG;
    if (pitch < (layout == 0 ? 3L * Win : (long)Win)) return NRGBD_E_SHAPE;
    IngestNorm nm = {{mean0, mean1, mean2}, {std0, std1, std2}};
    for (int c = 0; c < 3; ++c)
        if (nm.stdv[c] == 0.f || !(fabsf(nm.stdv[c]) <= 3.402823466e+38f) || !(fabsf(nm.mean[c]) <= 3.402823466e+38f)) return NRGBD_E_ARG;
    if (((uintptr_t)dst & 15) != 0) return NRGBD_E_ALIGN;
    const long total = 3L * Hout * Wout;
    const dim3 grid((unsigned)ceil_div(total, 1024)), block(256);
    const bool resize = Hin != Hout || Win != Wout;
    hipStream_t st = (hipStream_t)stream;
    if (Wout % 4 == 0) {
        const dim3 rows((unsigned)ceil_div(Wout, 1024), Hout, 3);
        const int qstep = (2 * Win) / (2 * Wout), rstep = (2 * Win) % (2 * Wout);
        if (layout == 0) {
            if (resize) hipLaunchKernelGGL((frame_ingest_rows_kernel<false, true>), rows, block, 0, st, src, pitch, Hin, Win, nm, dst, Hout, Wout, qstep, rstep);
            else hipLaunchKernelGGL((frame_ingest_rows_kernel<false, false>), rows, block, 0, st, src, pitch, Hin, Win, nm, dst, Hout, Wout, qstep, rstep);
        } else {
            if (resize) hipLaunchKernelGGL((frame_ingest_rows_kernel<true, true>), rows, block, 0, st, src, pitch, Hin, Win, nm, dst, Hout, Wout, qstep, rstep);
            else hipLaunchKernelGGL((frame_ingest_rows_kernel<true, false>), rows, block, 0, st, src, pitch, Hin, Win, nm, dst, Hout, Wout, qstep, rstep);
        }
    } else if (layout == 0) {
        if (resize) hipLaunchKernelGGL((frame_ingest_kernel<false, true>), grid, block, 0, st, src, pitch, Hin, Win, nm, dst, Hout, Wout);
        else hipLaunchKernelGGL((frame_ingest_kernel<false, false>), grid, block, 0, st, src, pitch, Hin, Win, nm, dst, Hout, Wout);
    } else {
        if (resize) hipLaunchKernelGGL((frame_ingest_kernel<true, true>), grid, block, 0, st, src, pitch, Hin, Win, nm, dst, Hout, Wout);
        else hipLaunchKernelGGL((frame_ingest_kernel<true, false>), grid, block, 0, st, src, pitch, Hin, Win, nm, dst, Hout, Wout);
    }
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

extern "C" int nrgbd_window_gather(const float* ring, int R, long slot_stride, nrgbd_window_slots slots, int V, float* src, float* ref,
                                   int H, int W, void* stream) {
    using namespace nrgbd;
    static_assert(sizeof(nrgbd_window_slots) == sizeof(GatherSlots) && NRGBD_GATHER_MAX_V == kGatherMaxV, "header and kernel disagree");
    if (!ring || !src || !ref) return NRGBD_E_NULL;
    if (V < 1 || V > kGatherMaxV || R <= 0 || H <= 0 || W <= 0 || H > kIngestMaxDim || W > kIngestMaxDim) return NRGBD_E_SHAPE;
    const long n = 3L * H * W;
    if (slot_stride < n) return NRGBD_E_SHAPE;
    GatherSlots g;
    for (int i = 0; i <= kGatherMaxV; ++i) {
        g.idx[i] = i <= V ? slots.idx[i] : 0;
        if (g.idx[i] < 0 || g.idx[i] >= R) return NRGBD_E_SHAPE;
    }
    const bool vec = n % 4 == 0 && slot_stride % 4 == 0 && (((uintptr_t)ring | (uintptr_t)src | (uintptr_t)ref) & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(window_gather_kernel<true>, dim3((unsigned)ceil_div(n, 1024), V + 1), dim3(256), 0, st, ring, slot_stride, g, V, src,
                           ref, (int)n);
    else
        hipLaunchKernelGGL(window_gather_kernel<false>, dim3((unsigned)ceil_div(n, 256), V + 1), dim3(256), 0, st, ring, slot_stride, g, V, src,
                           ref, (int)n);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}
