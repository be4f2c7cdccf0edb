// tsdf_page.hip — the moving TSDF volume paged: 8^3 voxel blocks gathered out of a volume into a dense staging tensor, with a flag that
// says which of them hold anything, and scattered back into a volume (neuralrgbd_amd/fusion.py: BlockStore, TSDFVolume.shift(store=...),
// paged_extract, FusionVideoStream(follow_spill="page")).  What leaves the window goes to a host store and comes back bit for bit when
// the window covers it again: the re-entry scheme of Kintinuous and of voxel-hashing streaming.
//
// No counterpart in the reference.  The semantics are written out in include/nrgbd.h (nrgbd_tsdf_blocks_gather_f32,
// nrgbd_tsdf_blocks_scatter_f32) and restated in numpy by tests/tsdf_page_ref.py.  Pure copies: no arithmetic touches a value, so NaN
// payloads, signed zeros and denormals come through bit for bit; no atomics, no workspace, the same bits in every run.
//
// tsdf_page_kernel<NP, VEC, GATHER>   one workgroup of 128 lanes per block, the blocks on blockIdx.x (at most NRGBD_TSDF_MAX_BLOCKS = 2^20:
//                             no loop over blocks).  Lane t owns the four consecutive x (t & 1) * 4 .. + 3 of row (z, y) = (t >> 4,
//                             (t >> 1) & 7) of the block, in every plane: a quarter of a row pair, 16 bytes a plane.  On the staging
//                             side that is always one global_load_dwordx4 / global_store_dwordx4 (the staging tensor is 16-byte
//                             aligned and a lane's words start at a multiple of four).  On the volume side
//                               VEC, ox % 4 == 0   X % 4 == 0 and the base 16-byte aligned (the launch's choice) and this block's ox a
//                                       multiple of 4 (the workgroup's, uniform): the four voxels are one aligned group that lies
//                                       wholly inside the grid or wholly outside: one dwordx4 access a plane
//                               otherwise          dword accesses, each x tested against the grid
//                             A voxel outside the grid is neither loaded nor stored: gather writes +0.0f for it, scatter skips it.
//                             Gather's flag: every lane ORs the words it loaded (the bit patterns: -0.0 and NaN count), the OR is
//                             folded through the wave by a ballot of "non-zero", through LDS across the two waves, and lane 0 writes
//                             the int with a plain store.  A lane's loads of all planes are issued before its first store.
//                             Why one workgroup a block and not the shift kernel's rows: a block's 64 rows of 32 bytes lie a grid row
//                             apart wherever the block sits, so no lane order makes the volume side coalesce beyond 32 bytes; the
//                             staging side is the one that can be dense, and this shape makes it so — a wave writes 1 KiB of it
//                             contiguously a plane.  Measured by tools/bench_page.py against torch slice copies.
#include "tsdf_extract.hpp"     // tsdf_voxels

namespace nrgbd {

struct TsdfPage {
    int X, Y, Z;
    size_t volume;                      // X Y Z: floats between two planes
};

constexpr int kPageWords = NRGBD_TSDF_BLOCK * NRGBD_TSDF_BLOCK * NRGBD_TSDF_BLOCK;      // 512 words a plane of a block

// Resources (kernel-resource-usage remarks, gfx950, -O3), VGPRs / SGPRs; 8 waves per SIMD and ScratchSize 0 in every form; LDS 8 bytes
// (gather: the two waves' flags) or none (scatter):
//   gather   NP 2: VEC 20 / 34, element 14 / 28     NP 5: VEC 32 / 34, element 28 / 28
//   scatter  NP 2: VEC 15 / 32, element 16 / 30     NP 5: VEC 30 / 34, element 32 / 30
// (a VEC kernel holds both paths: the block's ox decides.)  Global accesses in the compiled code, per lane and plane: on the aligned
// path one global_load_dwordx4 and one global_store_dwordx4; on the element path four global_load_dword (gather) or four
// global_store_dword (scatter) on the volume side and one dwordx4 access on the staging side — except that in scatter the compiler sinks
// the last plane's first word under its own test: that plane moves as dwordx3 + dword.  The flag: one global_store_dword by lane 0.
template <int NP, bool VEC, bool GATHER>
__global__ __launch_bounds__(128) void tsdf_page_kernel(float* __restrict__ vol, const TsdfPage s, const int* __restrict__ origins,
                                                        float* __restrict__ blocks, int* __restrict__ nonempty) {
    __shared__ int wave_any[2];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    const int i0 = (t & 1) * 4, j = (t >> 1) & 7, k = t >> 4;
    const long ox = origins[3 * b], oy = origins[3 * b + 1], oz = origins[3 * b + 2];      // longs: o + 7 of any int stays exact
    const long x0 = ox + i0, y = oy + j, z = oz + k;
    const bool in_row = y >= 0 && y < s.Y && z >= 0 && z < s.Z;
    bool in_x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) in_x[i] = in_row && x0 + i >= 0 && x0 + i < s.X;
    // only dereferenced where the voxel is inside the grid
    float* const at = vol + ((size_t)(in_row ? z : 0) * (size_t)s.Y + (size_t)(in_row ? y : 0)) * (size_t)s.X + (x0);
    float* const staged = blocks + ((size_t)b * NP) * kPageWords + (size_t)t * 4;
    const bool vec = VEC && (ox & 3) == 0;                         // uniform in the workgroup; the group is inside or outside as one
    float4 q[NP];
    if (GATHER) {
        unsigned any = 0;
        if (vec) {                                                  // each path whole, loads to stores: the two are compiled apart
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                q[p] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (in_x[0]) q[p] = *reinterpret_cast<const float4*>(at + p * s.volume);
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                *reinterpret_cast<float4*>(staged + p * kPageWords) = q[p];
                any |= (__float_as_uint(q[p].x) | __float_as_uint(q[p].y)) | (__float_as_uint(q[p].z) | __float_as_uint(q[p].w));
            }
        } else {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                q[p].x = in_x[0] ? at[p * s.volume] : 0.f;
                q[p].y = in_x[1] ? at[p * s.volume + 1] : 0.f;
                q[p].z = in_x[2] ? at[p * s.volume + 2] : 0.f;
                q[p].w = in_x[3] ? at[p * s.volume + 3] : 0.f;
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                *reinterpret_cast<float4*>(staged + p * kPageWords) = q[p];
                any |= (__float_as_uint(q[p].x) | __float_as_uint(q[p].y)) | (__float_as_uint(q[p].z) | __float_as_uint(q[p].w));
            }
        }
        if (nonempty) {                                             // uniform: a kernel argument
            const bool wave = __ballot(any != 0) != 0;
            if ((t & 63) == 0) wave_any[t >> 6] = wave ? 1 : 0;
            __syncthreads();
            if (t == 0) nonempty[b] = wave_any[0] | wave_any[1];
        }
    } else {
#pragma unroll
        for (int p = 0; p < NP; ++p) q[p] = *reinterpret_cast<const float4*>(staged + p * kPageWords);
        if (vec) {
            if (in_x[0]) {
#pragma unroll
                for (int p = 0; p < NP; ++p) *reinterpret_cast<float4*>(at + p * s.volume) = q[p];
            }
        } else {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                if (in_x[0]) at[p * s.volume] = q[p].x;
                if (in_x[1]) at[p * s.volume + 1] = q[p].y;
                if (in_x[2]) at[p * s.volume + 2] = q[p].z;
                if (in_x[3]) at[p * s.volume + 3] = q[p].w;
            }
        }
    }
}

template <bool GATHER>
static void tsdf_page_launch(int planes, bool vec, const TsdfPage& s, float* vol, const int* origins, int n, float* blocks, int* nonempty,
                             hipStream_t st) {
    const dim3 grid((unsigned)n), block(128);
    if (planes == 2) {
        if (vec) hipLaunchKernelGGL((tsdf_page_kernel<2, true, GATHER>), grid, block, 0, st, vol, s, origins, blocks, nonempty);
        else hipLaunchKernelGGL((tsdf_page_kernel<2, false, GATHER>), grid, block, 0, st, vol, s, origins, blocks, nonempty);
    } else {
        if (vec) hipLaunchKernelGGL((tsdf_page_kernel<5, true, GATHER>), grid, block, 0, st, vol, s, origins, blocks, nonempty);
        else hipLaunchKernelGGL((tsdf_page_kernel<5, false, GATHER>), grid, block, 0, st, vol, s, origins, blocks, nonempty);
    }
}

// The two entries' checks, in the documented order: -> NRGBD_OK with `s` and `vec` filled, or the error.
static int tsdf_page_check(const float* vol, int planes, int X, int Y, int Z, const int* origins, int n, const float* blocks, TsdfPage& s,
                           bool& vec) {
    if (!vol || (n != 0 && (!origins || !blocks))) return NRGBD_E_NULL;
    if (planes != 2 && planes != 5) return NRGBD_E_SHAPE;
    const long voxels = tsdf_voxels(X, Y, Z);
    if (voxels < 0) return (int)voxels;
    if (n < 0 || n > NRGBD_TSDF_MAX_BLOCKS) return NRGBD_E_SHAPE;
    if (((uintptr_t)blocks & 15) != 0) return NRGBD_E_ARG;
    s.X = X; s.Y = Y; s.Z = Z;
    s.volume = (size_t)voxels;
    vec = X % 4 == 0 && ((uintptr_t)vol & 15) == 0;
    return NRGBD_OK;
}

}  // namespace nrgbd

// no counterpart in the reference: see the header of this file and include/nrgbd.h
extern "C" int nrgbd_tsdf_blocks_gather_f32(const float* vol, int planes, int X, int Y, int Z, const int* origins, int n, float* blocks,
                                            int* nonempty, void* stream) {
    using namespace nrgbd;
    TsdfPage s;
    bool vec;
    const int rc = tsdf_page_check(vol, planes, X, Y, Z, origins, n, blocks, s, vec);
    if (rc != NRGBD_OK) return rc;
    if (n == 0) return NRGBD_OK;
    tsdf_page_launch<true>(planes, vec, s, const_cast<float*>(vol), origins, n, blocks, nonempty, (hipStream_t)stream);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

// no counterpart in the reference: see the header of this file and include/nrgbd.h
extern "C" int nrgbd_tsdf_blocks_scatter_f32(float* vol, int planes, int X, int Y, int Z, const int* origins, int n, const float* blocks,
                                             void* stream) {
    using namespace nrgbd;
    TsdfPage s;
    bool vec;
    const int rc = tsdf_page_check(vol, planes, X, Y, Z, origins, n, blocks, s, vec);
    if (rc != NRGBD_OK) return rc;
    if (n == 0) return NRGBD_OK;
    tsdf_page_launch<false>(planes, vec, s, vol, origins, n, const_cast<float*>(blocks), nullptr, (hipStream_t)stream);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}
