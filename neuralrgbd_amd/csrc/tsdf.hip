// tsdf.hip — truncated-signed-distance fusion of depth maps into a dense voxel volume, and its surface points
// (neuralrgbd_amd/fusion.py: TSDFVolume, FusionVideoStream).
//
// No counterpart in the reference: it drops every depth / confidence map after export (test_utils/export_res.py).  The conventions are
// this library's own and are written out in include/nrgbd.h; a numpy restatement of the same operation sequences (tests/tsdf_ref.py)
// reproduces every stored value bit for bit.  Everything is fp32, every operation that decides or produces a stored value is one IEEE
// operation (the library is built with -ffp-contract=off; no fused multiply-add, no reciprocal, no fast-math below), there are no
// atomics, and the same inputs give the same bits in every run.
//
// tsdf_integrate_kernel<VEC>  one depth frame into the volume, one launch.  A lane owns four x-neighbours (VEC: X % 4 == 0 and both
//                             arrays 16-byte aligned) or one voxel (any width: the same bits).  The element form's loop body is one
//                             call of tsdf_integrate.hpp's tsdf_update_group, the update tsdf_reint.hip's kernel runs after its
//                             removal; the VEC form spells the same update out in float4 registers, with the colour planes stored
//                             as they are formed: on the shared group (50 / 91 VGPRs, 8 / 5 waves) the kernel gave the same bits but
//                             ran 2 to 5 % longer at 256^3, so the VEC form is the instruction stream it was.
//                             Per voxel: lattice point -> camera -> pixel -> depth / gate / weight tests -> t = min(1, (d - zc) /
//                             trunc); only then the running average is read.  A group none of whose voxels is updated is neither
//                             loaded nor stored; a group with one is loaded once (2 x 16 bytes) and stored once, the voxels that
//                             were skipped with the bits they had.
//                             Resources (kernel-resource-usage remarks, gfx950, -O3): VEC 56 VGPRs, element form 26, 8 waves per
//                             SIMD, no scratch, no LDS (the extraction kernels: 18 / 44 / 42 VGPRs, no scratch); two IEEE
//                             divisions for the projection, one for t and one for the average per updated voxel.
// tsdf_integrate_kernel<VEC, TsdfColour>  the same kernel with the colour arguments (nrgbd_tsdf_integrate_color_f32): for a voxel that
//                             is updated, the pixel of the colour image it projects to (the quotients xc / zc, yc / zc of the depth
//                             projection, the image's own intrinsics, clamped into the image) goes through the affine and, when its
//                             three values are finite, into the running average of the three colour planes with the OLD weight; the
//                             image is read only for voxels that passed every test, a group that updates nothing touches no plane, and
//                             a group whose colour changes loads and stores five planes (5 x 16 bytes per lane in the VEC form,
//                             which also needs the colour planes 16-byte aligned).  The colour arguments are an optional parameter
//                             pack: without them (Colour... empty) COLOR is false and no colour code is compiled in.
//                             Resources (kernel-resource-usage remarks, gfx950, -O3): VEC 94 VGPRs (5 waves per SIMD), element form
//                             45 (8 waves); ScratchSize 0, no LDS; three more IEEE divisions per updated voxel.  The coloured point
//                             writer: 50 VGPRs, no scratch.
// tsdf_extract_kernel<false>  surface crossings per workgroup of kExtractVoxels consecutive voxels (linear index order)
// tsdf_scan_kernel            one workgroup: exclusive prefix of those counts in index order, kScanPass records per pass with a
//                             carried total (int64), then (crossings found, points written) into the caller's int64 [2]
// tsdf_extract_kernel<true>   re-evaluates the crossings and writes point `offset of the workgroup + rank inside it` while that is
//                             below the capacity: ascending (linear voxel index, axis) order, nothing behind the written rows.
// The crossing predicate, a lane's four voxels, the point writer and the scan live in tsdf_extract.hpp: tsdf_mesh.hip (the triangle
// mesh, whose vertices are these points) runs the same device code.
#include "tsdf_integrate.hpp"    // the frame, the lane group's update, the checks: shared with tsdf_reint.hip

namespace nrgbd {

// block (64, 4): threadIdx.x walks x (groups of four voxels, or voxels), threadIdx.y rows; blockIdx.y / .z stride over rows and slices
template <bool VEC, class... Colour>
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                             const float* __restrict__ depth, const float* __restrict__ gate,
                                                             const float* __restrict__ wmap, const TsdfFrame f, const Colour... colour) {
    constexpr bool COLOR = sizeof...(Colour) != 0;
    const TsdfColour k = tsdf_colour_args(colour...);
    float* __restrict__ const color = k.color;
    const float* __restrict__ const image = k.image;
    const TsdfImage& m = k.m;
    const long at = (long)(VEC ? (f.x0 >> 2) : f.x0) + (long)(blockIdx.x * 64 + threadIdx.x);
    if (at >= (VEC ? (long)((f.x1 + 3) >> 2) : (long)f.x1)) return;
    const int unit = (int)at;
    for (int iz = f.z0 + (int)blockIdx.z; iz < f.z1; iz += (int)gridDim.z) {
        for (int iy = f.y0 + (int)(blockIdx.y * 4 + threadIdx.y); iy < f.y1; iy += (int)gridDim.y * 4) {
            const size_t base = ((size_t)iz * (size_t)f.Y + (size_t)iy) * (size_t)f.X;
            if (VEC) {                                              // tsdf_update_group<4, false, true, COLOR> spelt out: see the header
                const TsdfRow row = tsdf_row(f, iy, iz);
                float t[4], w[4], xq[4], yq[4];
                bool ok[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ix = 4 * unit + j;
                    t[j] = 0.f;
                    w[j] = 0.f;
                    xq[j] = yq[j] = 0.f;
                    ok[j] = ix >= f.x0 && ix < f.x1 && tsdf_observe<COLOR>(f, row, ix, depth, gate, wmap, t[j], w[j], xq[j], yq[j]);
                }
                if (!(ok[0] || ok[1] || ok[2] || ok[3])) continue;
                float4* pt = reinterpret_cast<float4*>(tsdf + base) + unit;
                float4* pw = reinterpret_cast<float4*>(weight + base) + unit;
                float4 T = *pt, Wt = *pw;
                if (COLOR) {                                        // with the old weights, before the average replaces them
                    float c[4][3];
                    bool fin[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        c[j][0] = c[j][1] = c[j][2] = 0.f;
                        fin[j] = ok[j] && tsdf_colour(m, image, xq[j], yq[j], c[j]);
                    }
                    if (fin[0] || fin[1] || fin[2] || fin[3]) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            float4* pc = reinterpret_cast<float4*>(color + k * m.volume + base) + unit;
                            float4 C = *pc;
                            if (fin[0]) C.x = tsdf_blend(C.x, Wt.x, c[0][k], w[0]);
                            if (fin[1]) C.y = tsdf_blend(C.y, Wt.y, c[1][k], w[1]);
                            if (fin[2]) C.z = tsdf_blend(C.z, Wt.z, c[2][k], w[2]);
                            if (fin[3]) C.w = tsdf_blend(C.w, Wt.w, c[3][k], w[3]);
                            *pc = C;
                        }
                    }
                }
                if (ok[0]) tsdf_average(T.x, Wt.x, t[0], w[0], f.w_max);
                if (ok[1]) tsdf_average(T.y, Wt.y, t[1], w[1], f.w_max);
                if (ok[2]) tsdf_average(T.z, Wt.z, t[2], w[2], f.w_max);
                if (ok[3]) tsdf_average(T.w, Wt.w, t[3], w[3], f.w_max);
                *pt = T;
                *pw = Wt;
            } else
                tsdf_update_group<1, false, true, COLOR>(tsdf, weight, color, depth, gate, wmap, image, f, f, m, 0.f, iy, iz, unit,
                                                         base + (size_t)unit);
        }
    }
}

// The launch of both entries: the form (VEC / element) chosen on the host.
template <class... Colour>
static void tsdf_integrate_launch(bool vec, const TsdfFrame& f, float* tsdf, float* weight, const float* depth, const float* gate,
                                  const float* wmap, hipStream_t st, const Colour&... colour) {
    const dim3 grid = tsdf_integrate_grid(f, vec), block(64, 4);
    if (vec)
        hipLaunchKernelGGL((tsdf_integrate_kernel<true, Colour...>), grid, block, 0, st, tsdf, weight, depth, gate, wmap, f, colour...);
    else
        hipLaunchKernelGGL((tsdf_integrate_kernel<false, Colour...>), grid, block, 0, st, tsdf, weight, depth, gate, wmap, f, colour...);
}

// ---- extraction ---------------------------------------------------------------------------------------------------------------

// Colour...: nothing, or one TsdfPointColour (the third launch of nrgbd_tsdf_extract_points_color: the points and their colours)
template <bool WRITE, class... Colour>
__global__ __launch_bounds__(256) void tsdf_extract_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsdfGrid g,
                                                           int* __restrict__ wg_count, const long long* __restrict__ wg_offset,
                                                           float* __restrict__ points, long long capacity, const Colour... colour) {
    constexpr bool COLOR = sizeof...(Colour) != 0;
    const TsdfPointColour k = tsdf_point_colour(colour...);
    __shared__ int lds[4];
    const unsigned long long first = tsdf_lane_first();
    TsdfLane L;
    tsdf_lane_crossings(tsdf, weight, g, first, L);
    if (!WRITE) {
        const int s = block_sum_256(L.mine, lds);
        if (threadIdx.x == 0) wg_count[blockIdx.x] = s;
        return;
    }
    int total;
    const long long pos = wg_offset[blockIdx.x] + block_exclusive_256<int>(L.mine, lds, total);
    tsdf_lane_write<false, COLOR>(g, L, first, pos, points, capacity, nullptr, k.color, k.colors);
}

__global__ __launch_bounds__(256) void tsdf_scan_kernel(const int* __restrict__ wg_count, long long* __restrict__ wg_offset, int nwg,
                                                        long long capacity, long long* __restrict__ counts) {
    __shared__ long long lds[4];
    tsdf_scan_records(wg_count, wg_offset, nwg, capacity, counts, lds);
}

}  // namespace nrgbd

// no counterpart in the reference: see the header of this file and include/nrgbd.h
extern "C" int nrgbd_tsdf_integrate_f32(float* tsdf, float* weight, int X, int Y, int Z, float ox, float oy, float oz, float voxel_size,
                                        const float* depth, const float* gate, float gate_thr, const float* wmap, int H, int W,
                                        const float* pose, float fx, float fy, float cx, float cy, float trunc, float d_near, float d_far,
                                        float w_max, const int* box, void* stream) {
    using namespace nrgbd;
    if (!tsdf || !weight || !depth || !pose) return NRGBD_E_NULL;
    TsdfFrame f;
    const int rc = tsdf_frame(f, X, Y, Z, ox, oy, oz, voxel_size, H, W, pose, fx, fy, cx, cy, trunc, d_near, d_far, w_max, gate_thr, box, nullptr);
    if (rc != NRGBD_OK) return rc;
    tsdf_integrate_launch(tsdf_vec_ok(X, tsdf, weight), f, tsdf, weight, depth, gate, wmap, (hipStream_t)stream);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

// no counterpart in the reference: the same launch with the frame's colour averaged into three more planes
extern "C" int nrgbd_tsdf_integrate_color_f32(float* tsdf, float* weight, float* color, int X, int Y, int Z, float ox, float oy, float oz,
                                              float voxel_size, const float* depth, const float* gate, float gate_thr, const float* wmap,
                                              int H, int W, const float* pose, float fx, float fy, float cx, float cy, float trunc,
                                              float d_near, float d_far, float w_max, const int* box, const float* image, int Hc, int Wc,
                                              float fxc, float fyc, float cxc, float cyc, const float* affine, void* stream) {
    using namespace nrgbd;
    if (!tsdf || !weight || !depth || !pose || !color || !image || !affine) return NRGBD_E_NULL;
    const TsdfImage m = tsdf_image(X, Y, Z, Hc, Wc, fxc, fyc, cxc, cyc, affine);
    TsdfFrame f;
    const int rc = tsdf_frame(f, X, Y, Z, ox, oy, oz, voxel_size, H, W, pose, fx, fy, cx, cy, trunc, d_near, d_far, w_max, gate_thr, box, &m);
    if (rc != NRGBD_OK) return rc;
    tsdf_integrate_launch(tsdf_vec_ok(X, tsdf, weight, color), f, tsdf, weight, depth, gate, wmap, (hipStream_t)stream,
                          TsdfColour{color, image, m});
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

extern "C" long nrgbd_tsdf_extract_workspace(int X, int Y, int Z) {
    const long n = nrgbd::tsdf_voxels(X, Y, Z);
    if (n < 0) return n;
    return (n + nrgbd::kExtractVoxels - 1) / nrgbd::kExtractVoxels * 16;      // an int64 offset and an int32 count per workgroup
}

namespace nrgbd {

// nrgbd_tsdf_extract_points and its coloured form: the same checks, launches, workspace and counts (color NULL: the points alone)
static int tsdf_extract_launch(const float* tsdf, const float* weight, const float* color, int X, int Y, int Z, float ox, float oy, float oz,
                               float voxel_size, float w_min, void* workspace, long workspace_bytes, float* points, float* colors,
                               long capacity, long long* counts, void* stream) {
    const long n = tsdf_voxels(X, Y, Z);
    if (n < 0) return (int)n;
    if (capacity < 0) return NRGBD_E_SHAPE;
    const long nwg = (n + kExtractVoxels - 1) / kExtractVoxels;
    if (workspace_bytes < nwg * 16) return NRGBD_E_SHAPE;
    if (!tsdf_positive(voxel_size) || w_min != w_min) return NRGBD_E_ARG;
    if (((uintptr_t)workspace | (uintptr_t)counts) & 7) return NRGBD_E_ALIGN;
    const TsdfGrid g = tsdf_grid(X, Y, Z, n, ox, oy, oz, voxel_size, w_min);
    long long* wg_offset = (long long*)workspace;
    int* wg_count = (int*)(wg_offset + nwg);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tsdf_extract_kernel<false>, dim3((unsigned)nwg), dim3(256), 0, st, tsdf, weight, g, wg_count,
                       (const long long*)wg_offset, points, (long long)capacity);
    NRGBD_CHECK_LAUNCH();
    hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(256), 0, st, (const int*)wg_count, wg_offset, (int)nwg, (long long)capacity, counts);
    NRGBD_CHECK_LAUNCH();
    if (capacity > 0) {
        if (color)
            hipLaunchKernelGGL((tsdf_extract_kernel<true, TsdfPointColour>), dim3((unsigned)nwg), dim3(256), 0, st, tsdf, weight, g, wg_count,
                               (const long long*)wg_offset, points, (long long)capacity, TsdfPointColour{color, colors});
        else
            hipLaunchKernelGGL(tsdf_extract_kernel<true>, dim3((unsigned)nwg), dim3(256), 0, st, tsdf, weight, g, wg_count,
                               (const long long*)wg_offset, points, (long long)capacity);
        NRGBD_CHECK_LAUNCH();
    }
    return NRGBD_OK;
}

}  // namespace nrgbd

extern "C" int nrgbd_tsdf_extract_points(const float* tsdf, const float* weight, int X, int Y, int Z, float ox, float oy, float oz,
                                         float voxel_size, float w_min, void* workspace, long workspace_bytes, float* points,
                                         long capacity, long long* counts, void* stream) {
    if (!tsdf || !weight || !workspace || !counts || (!points && capacity > 0)) return NRGBD_E_NULL;
    return nrgbd::tsdf_extract_launch(tsdf, weight, nullptr, X, Y, Z, ox, oy, oz, voxel_size, w_min, workspace, workspace_bytes, points,
                                      nullptr, capacity, counts, stream);
}

extern "C" int nrgbd_tsdf_extract_points_color(const float* tsdf, const float* weight, const float* color, int X, int Y, int Z, float ox,
                                               float oy, float oz, float voxel_size, float w_min, void* workspace, long workspace_bytes,
                                               float* points, float* colors, long capacity, long long* counts, void* stream) {
    if (!tsdf || !weight || !color || !workspace || !counts || ((!points || !colors) && capacity > 0)) return NRGBD_E_NULL;
    return nrgbd::tsdf_extract_launch(tsdf, weight, color, X, Y, Z, ox, oy, oz, voxel_size, w_min, workspace, workspace_bytes, points,
                                      colors, capacity, counts, stream);
}
