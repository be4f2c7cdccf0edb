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
//                             arrays 16-byte aligned) or one voxel (any width: the same bits).  Per voxel: lattice point -> camera
//                             -> pixel -> depth / gate / weight tests -> t = min(1, (d - zc) / trunc); only then the running average
//                             is read.  A group none of whose voxels is updated is neither loaded nor stored; a group with one is
//                             loaded once (2 x 16 bytes) and stored once, the voxels that were skipped with the bits they had.  The
//                             row products r01 yw, r02 zw (and rows 1, 2) do not depend on x and are formed once per lane and row:
//                             the same products, the same bits.
//                             Resources (kernel-resource-usage remarks, gfx950, -O3): VEC 56 VGPRs, element form 28, 8 waves per
//                             SIMD, no scratch, no LDS (the extraction kernels: 18 / 46 / 42 VGPRs, no scratch); two IEEE
//                             divisions for the projection, one for t and one for the average per updated voxel.
// tsdf_extract_kernel<false>  surface crossings per workgroup of kExtractVoxels consecutive voxels (linear index order)
// tsdf_scan_kernel            one workgroup: exclusive prefix of those counts in index order, kScanPass records per pass with a
//                             carried total (int64), then (crossings found, points written) into the caller's int64 [2]
// tsdf_extract_kernel<true>   re-evaluates the crossings and writes point `offset of the workgroup + rank inside it` while that is
//                             below the capacity: ascending (linear voxel index, axis) order, nothing behind the written rows.
// The crossing predicate, a lane's four voxels, the point writer and the scan live in tsdf_extract.hpp: tsdf_mesh.hip (the triangle
// mesh, whose vertices are these points) runs the same device code.
#include "tsdf_extract.hpp"      // the crossings, the lane's four voxels, the scan: shared with tsdf_mesh.hip

namespace nrgbd {

struct TsdfFrame {
    float r[12];                        // float32(extM[:3,:4]) row-major: r00 r01 r02 tx | r10 r11 r12 ty | r20 r21 r22 tz
    float ox, oy, oz, vs;
    float fx, fy, cx, cy;
    float trunc, d_near, d_far, w_max, gate_thr;
    int X, Y, H, W;
    int x0, y0, z0, x1, y1, z1;         // half-open voxel box
};

// What does not depend on x: the lattice row's contribution to the three camera coordinates.
struct TsdfRow {
    float bx, cx, by, cy, bz, cz;       // r01 yw, r02 zw | r11 yw, r12 zw | r21 yw, r22 zw
};

__device__ __forceinline__ TsdfRow tsdf_row(const TsdfFrame& f, int iy, int iz) {
    const float yw = f.oy + f.vs * (float)iy;
    const float zw = f.oz + f.vs * (float)iz;
    TsdfRow r;
    r.bx = f.r[1] * yw; r.cx = f.r[2] * zw;
    r.by = f.r[5] * yw; r.cy = f.r[6] * zw;
    r.bz = f.r[9] * yw; r.cz = f.r[10] * zw;
    return r;
}

// The chain of include/nrgbd.h up to t and w for lattice column ix of a row; false: the voxel is skipped.
__device__ __forceinline__ bool tsdf_observe(const TsdfFrame& f, const TsdfRow& row, int ix, const float* __restrict__ depth,
                                             const float* __restrict__ gate, const float* __restrict__ wmap, float& t, float& w) {
    const float xw = f.ox + f.vs * (float)ix;
    const float xc = ((f.r[0] * xw + row.bx) + row.cx) + f.r[3];
    const float yc = ((f.r[4] * xw + row.by) + row.cy) + f.r[7];
    const float zc = ((f.r[8] * xw + row.bz) + row.cz) + f.r[11];
    if (!(zc > 0.f)) return false;
    const float u = f.fx * (xc / zc) + f.cx;
    const float v = f.fy * (yc / zc) + f.cy;
    if (!(u >= 0.f && u < (float)f.W && v >= 0.f && v < (float)f.H)) return false;       // a NaN fails
    const int iu = (int)floorf(u), iv = (int)floorf(v);                                  // 0 <= iu < W, 0 <= iv < H
    const size_t p = (size_t)iv * (size_t)f.W + (size_t)iu;
    const float d = depth[p];
    if (!(fabsf(d) <= kFltMax && d > f.d_near && d <= f.d_far)) return false;
    if (gate && !(gate[p] >= f.gate_thr)) return false;
    w = wmap ? wmap[p] : 1.f;
    if (!(w <= kFltMax && w > 0.f)) return false;
    const float s = d - zc;
    if (s < -f.trunc) return false;
    t = fminf(1.f, s / f.trunc);
    return true;
}

__device__ __forceinline__ void tsdf_average(float& T, float& Wt, float t, float w, float w_max) {
    T = (T * Wt + t * w) / (Wt + w);
    Wt = fminf(Wt + w, w_max);
}

// block (64, 4): threadIdx.x walks x (groups of four voxels, or voxels), threadIdx.y rows; blockIdx.y / .z stride over rows and slices
template <bool VEC>
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                             const float* __restrict__ depth, const float* __restrict__ gate,
                                                             const float* __restrict__ wmap, const TsdfFrame f) {
    const long at = (long)(VEC ? (f.x0 >> 2) : f.x0) + (long)(blockIdx.x * 64 + threadIdx.x);
    if (at >= (VEC ? (long)((f.x1 + 3) >> 2) : (long)f.x1)) return;
    const int unit = (int)at;
    for (int iz = f.z0 + (int)blockIdx.z; iz < f.z1; iz += (int)gridDim.z) {
        for (int iy = f.y0 + (int)(blockIdx.y * 4 + threadIdx.y); iy < f.y1; iy += (int)gridDim.y * 4) {
            const TsdfRow row = tsdf_row(f, iy, iz);
            const size_t base = ((size_t)iz * (size_t)f.Y + (size_t)iy) * (size_t)f.X;
            if (VEC) {
                float t[4], w[4];
                bool ok[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ix = 4 * unit + j;
                    t[j] = 0.f;
                    w[j] = 0.f;
                    ok[j] = ix >= f.x0 && ix < f.x1 && tsdf_observe(f, row, ix, depth, gate, wmap, t[j], w[j]);
                }
                if (!(ok[0] || ok[1] || ok[2] || ok[3])) continue;
                float4* pt = reinterpret_cast<float4*>(tsdf + base) + unit;
                float4* pw = reinterpret_cast<float4*>(weight + base) + unit;
                float4 T = *pt, Wt = *pw;
                if (ok[0]) tsdf_average(T.x, Wt.x, t[0], w[0], f.w_max);
                if (ok[1]) tsdf_average(T.y, Wt.y, t[1], w[1], f.w_max);
                if (ok[2]) tsdf_average(T.z, Wt.z, t[2], w[2], f.w_max);
                if (ok[3]) tsdf_average(T.w, Wt.w, t[3], w[3], f.w_max);
                *pt = T;
                *pw = Wt;
            } else {
                float t, w;
                if (!tsdf_observe(f, row, unit, depth, gate, wmap, t, w)) continue;
                float T = tsdf[base + unit], Wt = weight[base + unit];
                tsdf_average(T, Wt, t, w, f.w_max);
                tsdf[base + unit] = T;
                weight[base + unit] = Wt;
            }
        }
    }
}

// ---- extraction ---------------------------------------------------------------------------------------------------------------

template <bool WRITE>
__global__ __launch_bounds__(256) void tsdf_extract_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsdfGrid g,
                                                           int* __restrict__ wg_count, const long long* __restrict__ wg_offset,
                                                           float* __restrict__ points, long long capacity) {
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
    tsdf_lane_write<false>(g, L, first, pos, points, capacity, nullptr);
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
    const long n = tsdf_voxels(X, Y, Z);
    if (n < 0) return (int)n;
    if (H <= 0 || W <= 0) return NRGBD_E_SHAPE;
    TsdfFrame f;
    f.x0 = f.y0 = f.z0 = 0;
    f.x1 = X; f.y1 = Y; f.z1 = Z;
    if (box) {
        f.x0 = box[0]; f.y0 = box[1]; f.z0 = box[2];
        f.x1 = box[3]; f.y1 = box[4]; f.z1 = box[5];
        if (f.x0 < 0 || f.y0 < 0 || f.z0 < 0 || f.x1 > X || f.y1 > Y || f.z1 > Z) return NRGBD_E_SHAPE;
        if (f.x0 >= f.x1 || f.y0 >= f.y1 || f.z0 >= f.z1) return NRGBD_E_SHAPE;
    }
    if (!tsdf_positive(voxel_size) || !tsdf_positive(trunc) || !tsdf_positive(w_max)) return NRGBD_E_ARG;
    if (!(d_near < d_far)) return NRGBD_E_ARG;                   // a NaN bound included
    for (int i = 0; i < 12; ++i) f.r[i] = pose[i];
    f.ox = ox; f.oy = oy; f.oz = oz; f.vs = voxel_size;
    f.fx = fx; f.fy = fy; f.cx = cx; f.cy = cy;
    f.trunc = trunc; f.d_near = d_near; f.d_far = d_far; f.w_max = w_max; f.gate_thr = gate_thr;
    f.X = X; f.Y = Y; f.H = H; f.W = W;
    const bool vec = X % 4 == 0 && (((uintptr_t)tsdf | (uintptr_t)weight) & 15) == 0;
    const int units = vec ? (f.x1 + 3) / 4 - f.x0 / 4 : f.x1 - f.x0;
    const int rows = f.y1 - f.y0, slices = f.z1 - f.z0;
    const dim3 grid((unsigned)ceil_div(units, 64), (unsigned)(ceil_div(rows, 4) < 65535 ? ceil_div(rows, 4) : 65535),
                    (unsigned)(slices < 65535 ? slices : 65535));
    if (vec)
        hipLaunchKernelGGL(tsdf_integrate_kernel<true>, grid, dim3(64, 4), 0, (hipStream_t)stream, tsdf, weight, depth, gate, wmap, f);
    else
        hipLaunchKernelGGL(tsdf_integrate_kernel<false>, grid, dim3(64, 4), 0, (hipStream_t)stream, tsdf, weight, depth, gate, wmap, f);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

extern "C" long nrgbd_tsdf_extract_workspace(int X, int Y, int Z) {
    const long n = nrgbd::tsdf_voxels(X, Y, Z);
    if (n < 0) return n;
    return (n + nrgbd::kExtractVoxels - 1) / nrgbd::kExtractVoxels * 16;      // an int64 offset and an int32 count per workgroup
}

extern "C" int nrgbd_tsdf_extract_points(const float* tsdf, const float* weight, int X, int Y, int Z, float ox, float oy, float oz,
                                         float voxel_size, float w_min, void* workspace, long workspace_bytes, float* points,
                                         long capacity, long long* counts, void* stream) {
    using namespace nrgbd;
    if (!tsdf || !weight || !workspace || !counts || (!points && capacity > 0)) return NRGBD_E_NULL;
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
        hipLaunchKernelGGL(tsdf_extract_kernel<true>, dim3((unsigned)nwg), dim3(256), 0, st, tsdf, weight, g, wg_count,
                           (const long long*)wg_offset, points, (long long)capacity);
        NRGBD_CHECK_LAUNCH();
    }
    return NRGBD_OK;
}
