// depth_ingest.hip — one ground-truth depth frame -> the labels and metric maps a training step reads
// (neuralrgbd_amd/train_video.py: DepthLabeler, TrainVideoStream).
//
// depth_ingest_kernel   one uint16 depth frame (millimetres) -> int64 labels at the plane-sweep grid and at the image size, and the
//                       masked fp32 metres at both sizes, in ONE launch.  Replaces the loaders' depth preparation
//                       (mdataloader/scanNet.py:372-422, mdataloader/misc.py:13-36: PIL NEAREST resizes of the frame and of its
//                       hole mask, `.float() * .001`, np.digitize against float64 candidates, the clamp to [0, n - 1]) and the
//                       upload of its results (8 bytes of label per image pixel against 2 bytes of depth per source pixel).
//
// Resize.  Pillow's NEAREST tabulates its source indices by accumulating a double; no integer formula reproduces that for every
// size pair (640 -> 96 is one that differs), so the source rows / columns come as int32 tables the host built by the same
// sequential accumulation.  Every table entry is clamped to the frame before it is used: a bad table reads a wrong pixel, never
// out of bounds.  The hole mask of the grid-size map is sampled through TWO resizes in the reference (raw -> image size -> grid), so
// it has tables of its own (the composition); at the image size the mask is the frame's own zeros.
// Labels.  np.digitize compares the fp32 metres, promoted, with float64 candidates.  The label is monotone in the raw value u, so it
// is #{k : T[k] <= u} with integer thresholds T the host derives exactly; the kernel compares integers only.  The thresholds travel
// BY VALUE with the launch (uint16, 1 KB per table: the entry reads them on the host, checks them, and drops the entries no uint16
// reaches), each workgroup copies the table of its part to LDS (int32, padded with 65536) and every pixel runs a branch-free binary
// search over it: log2(n) LDS reads, the first ones broadcasts.
// Shape.  A lane owns 4 consecutive pixels of one output row: 16 bytes of metres, 32 bytes of labels (two 16-byte stores).  The
// lanes are numbered flat over (row, group of 4): one integer division per lane.  Vector stores need rows that keep the alignment
// (width % 4 == 0, 16-byte aligned base); any other width, and the last lanes of a row, store element by element.  The workgroups
// of the image-size part come first in the grid, those of the plane-sweep part after them; a part whose two outputs are both NULL
// has no workgroups.  No atomics, no scratch, nothing but plain vector stores.
// Bound: 0.6 MB read and 1.3 MB written at 480 x 640 -> 256 x 384 / 64 x 96 is microseconds of HBM time: the launch and the
// dependent load chain (table -> depth -> LDS search -> store) set the duration, not the bandwidth.
#include "common.hpp"

namespace nrgbd {

constexpr int kDepthMaxDim = 16384;
constexpr int kDepthMaxThr = NRGBD_DEPTH_MAX_THRESHOLDS;      // 512

struct DepthThr {
    unsigned short t[kDepthMaxThr];     // the thresholds below 65536, non-decreasing; entries from n_eff on are not read
};

struct DepthPart {
    const int* __restrict__ rows;       // [Hout] source row of an output row
    const int* __restrict__ cols;       // [Wout]
    const int* __restrict__ mrows;      // [Hout] / [Wout] source row / column of the hole mask; NULL: the pixel's own
    const int* __restrict__ mcols;
    long long* __restrict__ labels;     // [Hout][Wout] or NULL
    float* __restrict__ metres;         // [Hout][Wout] or NULL
    int Hout, Wout;
    int n_eff;                          // thresholds in the table
    int n_max;                          // largest label = n - 1
    int step0;                          // first step of the search: a power of two with 2 step0 >= n
    int vec;                            // rows keep 16-byte alignment
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ void depth_part(const unsigned short* __restrict__ src, long pitch, int Hin, int Win, float scale,
                                           const DepthPart& P, const int* __restrict__ thr, int group) {
    const int gpr = (P.Wout + 3) >> 2;                          // groups of 4 per output row
    if (group >= P.Hout * gpr) return;
    const int y = group / gpr;
    const int x0 = (group - y * gpr) << 2;
    const int n = P.Wout - x0 < 4 ? P.Wout - x0 : 4;
    const unsigned short* __restrict__ row = src + (size_t)clampi(P.rows[y], Hin - 1) * (size_t)pitch;
    const unsigned short* __restrict__ mrow = P.mrows ? src + (size_t)clampi(P.mrows[y], Hin - 1) * (size_t)pitch : nullptr;
    float v[4];
    long long lab[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = 0.f;
        lab[j] = 0;
        if (j < n) {
            int u = row[clampi(P.cols[x0 + j], Win - 1)];
            if (mrow && mrow[clampi(P.mcols[x0 + j], Win - 1)] == 0) u = 0;       // a hole of the twice-resized mask
            v[j] = (float)u * scale;                                             // .float() * depth_scale: one fp32 product
            int lo = 0;                                                          // min(#{k : T[k] <= u}, 2 step0 - 1)
            for (int s = P.step0; s > 0; s >>= 1)
                if (thr[lo + s - 1] <= u) lo += s;
            lab[j] = lo < P.n_max ? lo : P.n_max;
        }
    }
    const size_t o = (size_t)y * (size_t)P.Wout + x0;
    if (P.vec && n == 4) {
        if (P.metres) *reinterpret_cast<float4*>(P.metres + o) = make_float4(v[0], v[1], v[2], v[3]);
        if (P.labels) {
            *reinterpret_cast<longlong2*>(P.labels + o) = make_longlong2(lab[0], lab[1]);
            *reinterpret_cast<longlong2*>(P.labels + o + 2) = make_longlong2(lab[2], lab[3]);
        }
    } else {
        for (int j = 0; j < n; ++j) {
            if (P.metres) P.metres[o + j] = v[j];
            if (P.labels) P.labels[o + j] = lab[j];
        }
    }
}

// grid = nb_full + nb_q workgroups of 256: [0, nb_full) the image-size part, the rest the plane-sweep grid
__global__ __launch_bounds__(256) void depth_ingest_kernel(const unsigned short* __restrict__ src, long pitch, int Hin, int Win,
                                                           float scale, const DepthPart full, const DepthPart q, const DepthThr tf,
                                                           const DepthThr tq, int nb_full) {
    __shared__ int thr[kDepthMaxThr];
    const bool is_full = (int)blockIdx.x < nb_full;
    const int n_eff = is_full ? full.n_eff : q.n_eff;
    for (int i = threadIdx.x; i < kDepthMaxThr; i += 256) {
        int t = 65536;
        if (i < n_eff) t = is_full ? tf.t[i] : tq.t[i];
        thr[i] = t;
    }
    __syncthreads();
    if (is_full)
        depth_part(src, pitch, Hin, Win, scale, full, thr, (int)(blockIdx.x * 256 + threadIdx.x));
    else
        depth_part(src, pitch, Hin, Win, scale, q, thr, (int)((blockIdx.x - nb_full) * 256 + threadIdx.x));
}

// host: the thresholds of one part, checked and packed; false when they are refused
static bool pack_thresholds(const int* thr, int n, DepthThr& out, DepthPart& P) {
    if (!thr || n < 1 || n > kDepthMaxThr) return false;
    int n_eff = 0;
    for (int k = 0; k < n; ++k) {
        if (thr[k] < 0 || thr[k] > 65536 || (k > 0 && thr[k] < thr[k - 1])) return false;
        if (thr[k] < 65536) out.t[n_eff++] = (unsigned short)thr[k];
    }
    for (int k = n_eff; k < kDepthMaxThr; ++k) out.t[k] = 0xFFFF;
    P.n_eff = n_eff;
    P.n_max = n - 1;
    int s = 1;
    while (2 * s < n) s *= 2;
    P.step0 = s;
    return true;
}

}  // namespace nrgbd

extern "C" int nrgbd_depth_ingest_u16(const unsigned short* depth, int Hin, int Win, long pitch, const int* rows_full,
                                      const int* cols_full, const int* rows_q, const int* cols_q, const int* mask_rows_q,
                                      const int* mask_cols_q, float depth_scale, const int* thr_q, int n_q, const int* thr_full,
                                      int n_full, long long* labels_q, long long* labels_full, float* dmap_raw, float* dmap_imgsize,
                                      int H, int W, int h, int w, void* stream) {
    using namespace nrgbd;
    if (!depth || !rows_full || !cols_full || !rows_q || !cols_q || !mask_rows_q || !mask_cols_q || !thr_q || !thr_full)
        return NRGBD_E_ARG;
    if (!labels_q && !labels_full && !dmap_raw && !dmap_imgsize) return NRGBD_E_ARG;
    const int dims[6] = {Hin, Win, H, W, h, w};
    for (int d : dims)
        if (d <= 0 || d > kDepthMaxDim) return NRGBD_E_ARG;
    if (pitch < Win) return NRGBD_E_ARG;
    if (!(depth_scale > 0.f) || !(depth_scale <= 3.402823466e+38f)) return NRGBD_E_ARG;
    DepthThr tf, tq;
    DepthPart full = {rows_full, cols_full, nullptr, nullptr, labels_full, dmap_imgsize, H, W, 0, 0, 1, 0};
    DepthPart q = {rows_q, cols_q, mask_rows_q, mask_cols_q, labels_q, dmap_raw, h, w, 0, 0, 1, 0};
    if (!pack_thresholds(thr_full, n_full, tf, full) || !pack_thresholds(thr_q, n_q, tq, q)) return NRGBD_E_ARG;
    full.vec = W % 4 == 0 && (((uintptr_t)labels_full | (uintptr_t)dmap_imgsize) & 15) == 0;
    q.vec = w % 4 == 0 && (((uintptr_t)labels_q | (uintptr_t)dmap_raw) & 15) == 0;
    const int nb_full = (labels_full || dmap_imgsize) ? ceil_div((long)H * ((W + 3) / 4), 256) : 0;
    const int nb_q = (labels_q || dmap_raw) ? ceil_div((long)h * ((w + 3) / 4), 256) : 0;
    hipLaunchKernelGGL(depth_ingest_kernel, dim3((unsigned)(nb_full + nb_q)), dim3(256), 0, (hipStream_t)stream, depth, pitch, Hin, Win,
                       depth_scale, full, q, tf, tq, nb_full);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}
