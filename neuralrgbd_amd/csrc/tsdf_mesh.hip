// tsdf_mesh.hip — the fused TSDF volume as an indexed triangle mesh (neuralrgbd_amd/fusion.py: TSDFVolume.mesh).
//
// No counterpart in the reference.  The vertices are the points of nrgbd_tsdf_extract_points (tsdf_extract.hpp: the same predicate,
// quotient, operations and order, the same device code), the connectivity comes from the 256-case table of tsdf_mc_table.hpp
// (generated from a rule by tools/gen_mc_table.py).  No atomics, four launches, nothing synchronised, the same bits in every run; the
// numpy restatement is tests/tsdf_mesh_ref.py.  A workgroup owns kExtractVoxels consecutive voxels (linear index order), a lane four of
// them; the cell of a voxel is the one whose lowest corner it is.
//
// tsdf_mesh_count_kernel   crossings and triangles per workgroup
// tsdf_mesh_scan_kernel    two workgroups: the exclusive prefix of either count sequence (tsdf_scan_records), then
//                          (vertices found, written, triangles found, written) into the caller's int64 [4]
// tsdf_mesh_vertex_kernel  the points, and for EVERY voxel the row of its first crossing into first_row[voxel] (int32, workspace);
//                          <TsdfPointColour>: the vertices' colours as well (nrgbd_tsdf_extract_mesh_color; 52 VGPRs, no scratch)
// tsdf_mesh_face_kernel    per valid cell the case's triangles at `offset of the workgroup + rank inside it`; the row of the vertex on
//                          edge (voxel v, axis k) is first_row[v] + popc(crossings(v) & ((1 << k) - 1)) with the crossings of v
//                          re-evaluated by tsdf_crossings.  A lane forms the rows of a cell's sign-changing edges into its own
//                          column of an LDS array [12][256] (no register array indexed at run time) and then walks the table, which
//                          lies in LDS as well (4 KB, indexed per lane).
//
// The signs and the validity of a cell come from `columns`: for voxel i the four lattice points i + {0, X} + {0, X Y}, their sign bits
// spread to the corner numbers of cx = 0.  Cell i is column i and column i + 1 (shifted to cx = 1); a lane evaluates the five columns
// of its four cells once (at most 40 loads, 10 where the voxels themselves fail; the fifth is the next lane's first, an L1 hit).
#include "tsdf_extract.hpp"
#include "tsdf_mc_table.hpp"

namespace nrgbd {

constexpr int kColumnInvalid = 0x100;

// Column of voxel i = (ix, iy, iz), i <= g.n: bit 2 dy + 4 dz set iff T(ix, iy + dy, iz + dz) < 0; kColumnInvalid unless the four
// points exist and pass tsdf_side.  The voxel itself is tested first: where it fails (unobserved and free space: most of a volume) the
// other three points are not read.
__device__ __forceinline__ int tsdf_column(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsdfGrid& g, unsigned i,
                                           unsigned iy, unsigned iz) {
    if (!(iy + 1 < g.Y && iz + 1 < g.Z)) return kColumnInvalid;
    float T;
    if (!tsdf_side(tsdf, weight, i, g.w_min, T)) return kColumnInvalid;
    int col = T < 0.f ? 1 : 0;
#pragma unroll
    for (int p = 1; p < 4; ++p) {
        const size_t at = (size_t)i + ((p & 1) ? g.X : 0u) + ((p & 2) ? g.XY : 0u);
        if (!tsdf_side(tsdf, weight, at, g.w_min, T)) col |= kColumnInvalid;
        if (T < 0.f) col |= 1 << (2 * p);
    }
    return col;
}

// The cases of the lane's four cells, -1 where there is no valid cell.  L holds the voxels' coordinates (tsdf_lane_crossings).
__device__ __forceinline__ void tsdf_lane_cases(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsdfGrid& g,
                                                unsigned long long first, const TsdfLane& L, int (&cell)[4]) {
    int col[5];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        col[j] = first + j <= g.n ? tsdf_column(tsdf, weight, g, (unsigned)(first + j), L.iy[j], L.iz[j]) : kColumnInvalid;
    // the fifth column matters only when it lies in the row of the fourth voxel: then it has that voxel's iy, iz
    col[4] = first + 4 <= g.n && L.ix[3] + 1 < g.X && !(col[3] & kColumnInvalid) ? tsdf_column(tsdf, weight, g, (unsigned)(first + 4), L.iy[3], L.iz[3])
                                                                       : kColumnInvalid;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool exists = first + j <= g.n && L.ix[j] + 1 < g.X;          // the next linear index is this cell's cx = 1 column
        const int both = col[j] | (exists ? col[j + 1] << 1 : kColumnInvalid);
        cell[j] = (both & (kColumnInvalid | (kColumnInvalid << 1))) ? -1 : both;
    }
}

// a[j] for a run-time j without an indexed register array (which would live in scratch)
template <typename T>
__device__ __forceinline__ T pick4(const T (&a)[4], int j) {
    return j == 0 ? a[0] : j == 1 ? a[1] : j == 2 ? a[2] : a[3];
}

__global__ __launch_bounds__(256) void tsdf_mesh_count_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsdfGrid g,
                                                              int* __restrict__ vertex_count, int* __restrict__ face_count) {
    __shared__ int lds[8];
    __shared__ unsigned char n_tri[256];
    n_tri[threadIdx.x] = kMcCount[threadIdx.x];
    const unsigned long long first = tsdf_lane_first();
    TsdfLane L;
    tsdf_lane_crossings(tsdf, weight, g, first, L);
    int cell[4];
    tsdf_lane_cases(tsdf, weight, g, first, L, cell);
    __syncthreads();
    int tris = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) tris += cell[j] >= 0 ? (int)n_tri[cell[j]] : 0;
    const int v = block_sum_256(L.mine, lds);
    const int f = block_sum_256(tris, lds + 4);
    if (threadIdx.x == 0) {
        vertex_count[blockIdx.x] = v;
        face_count[blockIdx.x] = f;
    }
}

// blockIdx.x = 0: the vertices, 1: the triangles.  Both sequences, their offsets and capacities lie nwg records apart.
__global__ __launch_bounds__(256) void tsdf_mesh_scan_kernel(const int* __restrict__ wg_count, long long* __restrict__ wg_offset, int nwg,
                                                             long long vertex_capacity, long long face_capacity,
                                                             long long* __restrict__ counts) {
    __shared__ long long lds[4];
    const size_t s = blockIdx.x;
    tsdf_scan_records(wg_count + s * nwg, wg_offset + s * nwg, nwg, s ? face_capacity : vertex_capacity, counts + 2 * s, lds);
}

// Colour...: nothing, or one TsdfPointColour (nrgbd_tsdf_extract_mesh_color: the vertices' colours as well)
template <class... Colour>
__global__ __launch_bounds__(256) void tsdf_mesh_vertex_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsdfGrid g,
                                                               const long long* __restrict__ wg_offset, float* __restrict__ points,
                                                               long long capacity, int* __restrict__ first_row, const Colour... colour) {
    constexpr bool COLOR = sizeof...(Colour) != 0;
    const TsdfPointColour k = tsdf_point_colour(colour...);
    __shared__ int lds[4];
    const unsigned long long first = tsdf_lane_first();
    TsdfLane L;
    tsdf_lane_crossings(tsdf, weight, g, first, L);
    int total;
    const long long pos = wg_offset[blockIdx.x] + block_exclusive_256<int>(L.mine, lds, total);
    tsdf_lane_write<true, COLOR>(g, L, first, pos, points, capacity, first_row, k.color, k.colors);
}

__global__ __launch_bounds__(256) void tsdf_mesh_face_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsdfGrid g,
                                                             const long long* __restrict__ wg_offset, const int* __restrict__ first_row,
                                                             int* __restrict__ faces, long long capacity) {
    __shared__ int lds[4];
    __shared__ uint4 table[256];                                // kMcTriangles: 16 edge slots per case
    __shared__ unsigned char table_count[256];
    __shared__ int edge_row[12][256];                           // [edge][lane]: a lane reads and writes its own column only
    table[threadIdx.x] = reinterpret_cast<const uint4*>(kMcTriangles)[threadIdx.x];
    table_count[threadIdx.x] = kMcCount[threadIdx.x];
    const unsigned long long first = tsdf_lane_first();
    TsdfLane L;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        L.ix[j] = L.iy[j] = L.iz[j] = 0;
        if (first + j > g.n) continue;
        const unsigned i = (unsigned)(first + j);
        L.iz[j] = i / g.XY;
        const unsigned rem = i - L.iz[j] * g.XY;
        L.iy[j] = rem / g.X;
        L.ix[j] = rem - L.iy[j] * g.X;
    }
    int cell[4];
    tsdf_lane_cases(tsdf, weight, g, first, L, cell);
    __syncthreads();                                            // the table is in place
    const signed char* tri = reinterpret_cast<const signed char*>(table);
    int n_tri[4], mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        n_tri[j] = cell[j] >= 0 ? (int)table_count[cell[j]] : 0;
        mine += n_tri[j];
    }
    int total;
    long long pos = wg_offset[blockIdx.x] + block_exclusive_256<int>(mine, lds, total);
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {                               // one body for the four cells; pick4 keeps their values in registers
        const int n = pick4(n_tri, j);
        if (n == 0) continue;
        if (pos >= capacity) return;                            // rows only grow from here on
        const int c = pick4(cell, j);
        const unsigned i = (unsigned)(first + j);
        const unsigned ix = pick4(L.ix, j), iy = pick4(L.iy, j), iz = pick4(L.iz, j);
        // the seven voxels that own an edge of the cell: d = dx + 2 dy + 4 dz, all but (1, 1, 1); axis a of voxel d is an edge of the
        // cell iff the voxel's coordinate on a is 0, and is then edge 4 a + p + 2 q with (p, q) its other two coordinates
#pragma unroll
        for (int d = 0; d < 7; ++d) {
            int changing = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if (!(d & (1 << a)) && (((c >> d) ^ (c >> (d | (1 << a)))) & 1)) changing |= 1 << a;
            if (!changing) continue;
            const unsigned v = i + ((d & 1) ? 1u : 0u) + ((d & 2) ? g.X : 0u) + ((d & 4) ? g.XY : 0u);
            float q[3];
            const int mask = tsdf_crossings(tsdf, weight, g, v, ix + (d & 1), iy + ((d >> 1) & 1), iz + (d >> 2), q);
            const int row0 = first_row[v];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!(changing & (1 << a))) continue;
                const int others = a == 0 ? d >> 1 : a == 1 ? (d & 1) | ((d >> 1) & 2) : d & 3;      // p + 2 q
                edge_row[4 * a + others][threadIdx.x] = row0 + __popc(mask & ((1 << a) - 1));
            }
        }
        for (int t = 0; t < n; ++t, ++pos) {
            if (pos >= capacity) return;
            int* out = faces + 3 * pos;
#pragma unroll
            for (int m = 0; m < 3; ++m) out[m] = edge_row[tri[16 * c + 3 * t + m]][threadIdx.x];
        }
    }
}

constexpr long kMeshMaxVoxels = 0x7fffffffL / 3;               // 3 X Y Z <= 2^31 - 1: a vertex row fits an int32

static long mesh_voxels(int X, int Y, int Z) {
    const long n = tsdf_voxels(X, Y, Z);
    return n > kMeshMaxVoxels ? (long)NRGBD_E_SHAPE : n;
}

// workspace: int64 offsets [2][nwg] | int32 counts [2][nwg] | int32 first_row [n]
static long mesh_workspace_bytes(long n) {
    const long nwg = (n + kExtractVoxels - 1) / kExtractVoxels;
    return nwg * 24 + n * 4;
}

}  // namespace nrgbd

extern "C" long nrgbd_tsdf_mesh_workspace(int X, int Y, int Z) {
    const long n = nrgbd::mesh_voxels(X, Y, Z);
    if (n < 0) return n;
    return nrgbd::mesh_workspace_bytes(n);
}

namespace nrgbd {

// nrgbd_tsdf_extract_mesh and its coloured form: the same checks, launches, workspace and counts (color NULL: no colours)
static int tsdf_mesh_launch(const float* tsdf, const float* weight, const float* color, int X, int Y, int Z, float ox, float oy, float oz,
                            float voxel_size, float w_min, void* workspace, long workspace_bytes, float* vertices, float* colors,
                            long vertex_capacity, int* faces, long face_capacity, long long* counts, void* stream) {
    const long n = mesh_voxels(X, Y, Z);
    if (n < 0) return (int)n;
    if (vertex_capacity < 0 || face_capacity < 0) return NRGBD_E_SHAPE;
    if (workspace_bytes < mesh_workspace_bytes(n)) return NRGBD_E_SHAPE;
    if (!tsdf_positive(voxel_size) || w_min != w_min) return NRGBD_E_ARG;
    if (((uintptr_t)workspace | (uintptr_t)counts) & 7) return NRGBD_E_ALIGN;
    const TsdfGrid g = tsdf_grid(X, Y, Z, n, ox, oy, oz, voxel_size, w_min);
    const long nwg = (n + kExtractVoxels - 1) / kExtractVoxels;
    long long* wg_offset = (long long*)workspace;
    int* wg_count = (int*)(wg_offset + 2 * nwg);
    int* first_row = wg_count + 2 * nwg;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tsdf_mesh_count_kernel, dim3((unsigned)nwg), dim3(256), 0, st, tsdf, weight, g, wg_count, wg_count + nwg);
    NRGBD_CHECK_LAUNCH();
    hipLaunchKernelGGL(tsdf_mesh_scan_kernel, dim3(2), dim3(256), 0, st, (const int*)wg_count, wg_offset, (int)nwg, (long long)vertex_capacity,
                       (long long)face_capacity, counts);
    NRGBD_CHECK_LAUNCH();
    if (vertex_capacity > 0 || face_capacity > 0) {            // the triangles need every voxel's first row, written or not
        if (color)                                              // capacity 0: no row is below it, neither output is touched
            hipLaunchKernelGGL(tsdf_mesh_vertex_kernel<TsdfPointColour>, dim3((unsigned)nwg), dim3(256), 0, st, tsdf, weight, g,
                               (const long long*)wg_offset, vertices, (long long)vertex_capacity, first_row, TsdfPointColour{color, colors});
        else
            hipLaunchKernelGGL(tsdf_mesh_vertex_kernel<>, dim3((unsigned)nwg), dim3(256), 0, st, tsdf, weight, g, (const long long*)wg_offset,
                               vertices, (long long)vertex_capacity, first_row);
        NRGBD_CHECK_LAUNCH();
    }
    if (face_capacity > 0) {
        hipLaunchKernelGGL(tsdf_mesh_face_kernel, dim3((unsigned)nwg), dim3(256), 0, st, tsdf, weight, g, (const long long*)(wg_offset + nwg),
                           (const int*)first_row, faces, (long long)face_capacity);
        NRGBD_CHECK_LAUNCH();
    }
    return NRGBD_OK;
}

}  // namespace nrgbd

// no counterpart in the reference: see the header of this file and include/nrgbd.h
extern "C" int nrgbd_tsdf_extract_mesh(const float* tsdf, const float* weight, int X, int Y, int Z, float ox, float oy, float oz,
                                       float voxel_size, float w_min, void* workspace, long workspace_bytes, float* vertices,
                                       long vertex_capacity, int* faces, long face_capacity, long long* counts, void* stream) {
    if (!tsdf || !weight || !workspace || !counts || (!vertices && vertex_capacity > 0) || (!faces && face_capacity > 0)) return NRGBD_E_NULL;
    return nrgbd::tsdf_mesh_launch(tsdf, weight, nullptr, X, Y, Z, ox, oy, oz, voxel_size, w_min, workspace, workspace_bytes, vertices, nullptr,
                                   vertex_capacity, faces, face_capacity, counts, stream);
}

extern "C" int nrgbd_tsdf_extract_mesh_color(const float* tsdf, const float* weight, const float* color, int X, int Y, int Z, float ox,
                                             float oy, float oz, float voxel_size, float w_min, void* workspace, long workspace_bytes,
                                             float* vertices, float* colors, long vertex_capacity, int* faces, long face_capacity,
                                             long long* counts, void* stream) {
    if (!tsdf || !weight || !color || !workspace || !counts || ((!vertices || !colors) && vertex_capacity > 0) ||
        (!faces && face_capacity > 0))
        return NRGBD_E_NULL;
    return nrgbd::tsdf_mesh_launch(tsdf, weight, color, X, Y, Z, ox, oy, oz, voxel_size, w_min, workspace, workspace_bytes, vertices, colors,
                                   vertex_capacity, faces, face_capacity, counts, stream);
}
