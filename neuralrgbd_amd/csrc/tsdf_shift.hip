// tsdf_shift.hip — the TSDF volume moved by whole voxels so that it follows the camera: what stays is copied to its new place, what
// enters starts empty, and what leaves is handed out as the spill volume in the same launch (neuralrgbd_amd/fusion.py:
// TSDFVolume.shift, follow_shift, FusionVideoStream(follow=...)).  The moving volume of Kintinuous / large-scale KinFu.
//
// No counterpart in the reference.  The semantics are written out in include/nrgbd.h (nrgbd_tsdf_shift_f32) and restated in numpy by
// tests/tsdf_shift_ref.py.  A pure copy: no arithmetic touches a value, so NaN payloads, signed zeros and denormals come through bit for
// bit; no LDS, no atomics, no workspace, the same bits in every run.
//
// tsdf_shift_kernel<FORM>     block (64, 4): threadIdx.x walks groups of four consecutive x of a dst row, threadIdx.y rows; blockIdx.y
//                             strides over rows, blockIdx.z over (plane unit, slice) pairs.  A colourless volume is one unit: a lane
//                             moves tsdf and weight together.  A colour volume is five units, one per plane.  A lane owns its four
//                             dst voxels in its unit's planes: it loads their sources (none where the source lies outside the grid:
//                             the voxels get +0.0f), stores them, and with spill rewrites, in the tsdf and the weight plane, exactly
//                             the source words it read — 0 where the voxel is not on the rim, its own bits where it is.  A source
//                             word has one reader, and that lane alone writes it, after its read: one launch without a hazard.
//                             Leaving voxels and the colour planes of src are never written.
//                               FORM 2  X % 4 == 0, sx % 4 == 0, both bases 16-byte aligned: a source group is a whole aligned group (or
//                                       wholly outside): global_load_dwordx4 / global_store_dwordx4, also for the spill store
//                               FORM 1  X % 4 == 0, bases aligned, another sx: the four sources straddle two groups: global_load_dword
//                                       x 4 per plane, global_store_dwordx4 to dst, global_store_dword for the spill
//                               FORM 0  any X, any base: dword accesses throughout, each x tested against X
//                             Why a colour volume is not moved five planes to a lane (the shape of the other TSDF kernels): measured
//                             at 256^3 (tools/bench_shift.py), ten streams 67 MB apart per lane ran at 131 us for (8,0,0), 1.05 of
//                             a device-to-device copy_ of the buffer and behind torch's slice copy; a plane per unit runs at 110 us,
//                             0.87 of the copy_.  Two planes to a lane are the faster shape on a colourless volume (34 us against
//                             36 us a plane), so that one keeps it.
//                             Plain loads and stores: every byte is touched once, so no cache policy has anything to keep, and the
//                             non-temporal forms only bypass the L1 on gfx950 (they were not tried here).
#include "tsdf_extract.hpp"     // tsdf_voxels

namespace nrgbd {

struct TsdfShift {
    int X, Y, Z;
    int sx, sy, sz;                     // |s_k| < n_k, or (X, 0, 0) when nothing is retained
    int spill;
    int units;                          // 1: (tsdf, weight) as one unit; 5: every plane of a colour volume its own
    size_t volume;                      // X Y Z: floats between two planes
};

// The rows of slice iz this lane walks, in NP consecutive planes from `src` / `dst` (the bases of the unit's first plane).
template <int NP, int FORM>
__device__ __forceinline__ void tsdf_shift_rows(float* __restrict__ src, float* __restrict__ dst, const TsdfShift& s, bool spill, int ix0,
                                                int iz, const bool (&in_x)[4], const bool (&rim_x)[4]) {
    const long jz = (long)iz + (long)s.sz;
    const bool in_z = jz >= 0 && jz < s.Z;
    const bool rim_z = (s.sz > 0 && iz == 0) || (s.sz < 0 && iz == s.Z - 1);
    for (int iy = (int)(blockIdx.y * 4 + threadIdx.y); iy < s.Y; iy += (int)gridDim.y * 4) {
        const long jy = (long)iy + (long)s.sy;
        const bool in_row = in_z && jy >= 0 && jy < s.Y;
        const bool rim_row = rim_z || (s.sy > 0 && iy == 0) || (s.sy < 0 && iy == s.Y - 1);
        float* const to = dst + ((size_t)iz * (size_t)s.Y + (size_t)iy) * (size_t)s.X + (size_t)ix0;
        // the source of dst voxel ix0 (only dereferenced where the row and the x are inside; ix0 + sx may be negative)
        float* const from = src + ((size_t)(in_row ? jz : 0) * (size_t)s.Y + (size_t)(in_row ? jy : 0)) * (size_t)s.X + ((long)ix0 + (long)s.sx);
        float v[NP][4];
        if (FORM == 2) {
            const bool in = in_row && in_x[0];                      // sx % 4 == 0 and X % 4 == 0: the group is inside or outside as one
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const float4 q = in ? *reinterpret_cast<const float4*>(from + p * s.volume) : make_float4(0.f, 0.f, 0.f, 0.f);
                v[p][0] = q.x; v[p][1] = q.y; v[p][2] = q.z; v[p][3] = q.w;
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) *reinterpret_cast<float4*>(to + p * s.volume) = make_float4(v[p][0], v[p][1], v[p][2], v[p][3]);
            if (spill && in && !rim_row) {                          // a rim row keeps every bit: nothing to write
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    *reinterpret_cast<float4*>(from + p * s.volume) = make_float4(rim_x[0] ? v[p][0] : 0.f, rim_x[1] ? v[p][1] : 0.f,
                                                                                  rim_x[2] ? v[p][2] : 0.f, rim_x[3] ? v[p][3] : 0.f);
            }
        } else {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[p][j] = in_row && in_x[j] ? from[p * s.volume + j] : 0.f;
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                if (FORM == 1) {
                    *reinterpret_cast<float4*>(to + p * s.volume) = make_float4(v[p][0], v[p][1], v[p][2], v[p][3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (ix0 + j < s.X) to[p * s.volume + j] = v[p][j];
                }
            }
            if (spill && in_row && !rim_row) {
#pragma unroll
                for (int p = 0; p < NP; ++p) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (in_x[j] && !rim_x[j]) from[p * s.volume + j] = 0.f;
                }
            }
        }
    }
}

// Resources (kernel-resource-usage remarks, gfx950, -O3), VGPRs / SGPRs; 8 waves per SIMD, ScratchSize 0 and no LDS in every form:
//   FORM 2: 28 / 84   FORM 1: 28 / 89   FORM 0: 27 / 95       (each holds both unit shapes: two planes to a lane and one)
// Global accesses in the compiled code, per lane and row: FORM 2 one global_load_dwordx4 and one global_store_dwordx4 per plane of the
// unit, and one more global_store_dwordx4 per spilled plane; FORM 1 four global_load_dword and one global_store_dwordx4 per plane,
// global_store_dword under spill; FORM 0 global_load_dword / global_store_dword only.  A lane's loads of a row are issued before its
// first store.
template <int FORM>
__global__ __launch_bounds__(256) void tsdf_shift_kernel(float* __restrict__ src, float* __restrict__ dst, const TsdfShift s) {
    const long first = 4L * (long)(blockIdx.x * 64 + threadIdx.x);   // in a long: the last block of a row of 2^31 - 1 voxels passes 2^31
    if (first >= (long)s.X) return;
    const int ix0 = (int)first;
    bool in_x[4], rim_x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ix = ix0 + j;
        const long jx = (long)ix + (long)s.sx;                      // sx may be X itself
        in_x[j] = ix < s.X && jx >= 0 && jx < s.X;
        rim_x[j] = (s.sx > 0 && ix == 0) || (s.sx < 0 && ix == s.X - 1);
    }
    const long pairs = (long)s.units * (long)s.Z;                   // at most 5 (2^31 - 1): a long
    for (long pair = (long)blockIdx.z; pair < pairs; pair += (long)gridDim.z) {
        const int unit = (int)(pair / s.Z), iz = (int)(pair - (long)unit * s.Z);
        if (s.units == 1) {                                         // a colourless volume: (tsdf, weight) by one lane
            tsdf_shift_rows<2, FORM>(src, dst, s, s.spill != 0, ix0, iz, in_x, rim_x);
        } else {                                                    // a colour volume: plane `unit`; the colour planes are never spilled
            const size_t at = (size_t)unit * s.volume;
            tsdf_shift_rows<1, FORM>(src + at, dst + at, s, s.spill != 0 && unit < 2, ix0, iz, in_x, rim_x);
        }
    }
}

static void tsdf_shift_launch(int form, const TsdfShift& s, float* src, float* dst, hipStream_t st) {
    const long pairs = (long)s.units * (long)s.Z;
    const dim3 grid((unsigned)ceil_div(ceil_div(s.X, 4), 64), (unsigned)(ceil_div(s.Y, 4) < 65535 ? ceil_div(s.Y, 4) : 65535),
                    (unsigned)(pairs < 65535 ? pairs : 65535)), block(64, 4);
    if (form == 2) hipLaunchKernelGGL((tsdf_shift_kernel<2>), grid, block, 0, st, src, dst, s);
    else if (form == 1) hipLaunchKernelGGL((tsdf_shift_kernel<1>), grid, block, 0, st, src, dst, s);
    else hipLaunchKernelGGL((tsdf_shift_kernel<0>), grid, block, 0, st, src, dst, s);
}

}  // namespace nrgbd

// no counterpart in the reference: see the header of this file and include/nrgbd.h
extern "C" int nrgbd_tsdf_shift_f32(float* src, float* dst, int planes, int X, int Y, int Z, int sx, int sy, int sz, int spill,
                                    void* stream) {
    using namespace nrgbd;
    if (!src || !dst) return NRGBD_E_NULL;
    if (planes != 2 && planes != 5) return NRGBD_E_SHAPE;
    const long n = tsdf_voxels(X, Y, Z);
    if (n < 0) return (int)n;
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst, bytes = (uintptr_t)planes * (uintptr_t)n * sizeof(float);
    if (a < b + bytes && b < a + bytes) return NRGBD_E_ARG;        // the two buffers overlap
    TsdfShift s;
    s.X = X; s.Y = Y; s.Z = Z;
    s.sx = sx; s.sy = sy; s.sz = sz;
    s.spill = spill != 0;
    s.units = planes == 5 ? 5 : 1;
    s.volume = (size_t)n;
    const auto beyond = [](int sh, int dim) { return sh >= dim || sh <= -dim; };
    if (beyond(sx, X) || beyond(sy, Y) || beyond(sz, Z)) {         // nothing is retained: every source lies outside
        s.sx = X;
        s.sy = s.sz = 0;
    }
    const bool vec = X % 4 == 0 && ((a | b) & 15) == 0;
    const int form = vec ? (s.sx % 4 == 0 ? 2 : 1) : 0;
    tsdf_shift_launch(form, s, src, dst, (hipStream_t)stream);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}
