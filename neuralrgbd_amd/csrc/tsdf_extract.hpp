// tsdf_extract.hpp — what the two extractions of a TSDF volume share: the surface points (tsdf.hip, nrgbd_tsdf_extract_points) and the
// triangle mesh (tsdf_mesh.hip, nrgbd_tsdf_extract_mesh), whose vertices ARE those points.  The crossing predicate, the quotient and
// the three operations per coordinate exist once, here, so the two write the same bits in the same order.
#pragma once
#include "common.hpp"

namespace nrgbd {

constexpr int kExtractVoxels = NRGBD_TSDF_EXTRACT_VOXELS;      // 1024: four consecutive voxels per lane
constexpr int kScanPass = NRGBD_TSDF_SCAN_PASS;                // 1024: four consecutive records per lane and pass
constexpr long kTsdfMaxVoxels = 1L << 31;
constexpr float kFltMax = 3.402823466e+38f;

struct TsdfGrid {
    float ox, oy, oz, vs, w_min;
    unsigned X, Y, Z, XY;
    unsigned n;                         // X Y Z - 1 (the count itself may be 2^31)
};

__device__ __forceinline__ bool tsdf_side(const float* __restrict__ tsdf, const float* __restrict__ weight, size_t i, float w_min, float& T) {
    T = tsdf[i];
    return weight[i] >= w_min && fabsf(T) < 1.f;                 // a NaN weight or value fails
}

// The crossings of voxel i along x, y, z: bit k of the result, q[k] = T_a / (T_a - T_b).
__device__ __forceinline__ int tsdf_crossings(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsdfGrid& g, unsigned i,
                                              unsigned ix, unsigned iy, unsigned iz, float (&q)[3]) {
    float Ta;
    if (!tsdf_side(tsdf, weight, i, g.w_min, Ta)) return 0;
    const bool inside[3] = {ix + 1 < g.X, iy + 1 < g.Y, iz + 1 < g.Z};
    const unsigned step[3] = {1u, g.X, g.XY};
    int mask = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        q[k] = 0.f;
        if (!inside[k]) continue;
        float Tb;
        if (!tsdf_side(tsdf, weight, (size_t)i + step[k], g.w_min, Tb)) continue;
        if ((Ta < 0.f) == (Tb < 0.f)) continue;
        q[k] = Ta / (Ta - Tb);
        mask |= 1 << k;
    }
    return mask;
}

__device__ __forceinline__ int block_sum_256(int v, int* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// exclusive prefix of v over the 256 lanes of the workgroup in lane order (lds: 4 ints); total: the workgroup's sum
template <typename T>
__device__ __forceinline__ T block_exclusive_256(T v, T* lds, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    T before = 0;
    for (int k = 0; k < wave; ++k) before += lds[k];
    total = ((lds[0] + lds[1]) + lds[2]) + lds[3];
    return before + inc - v;
}

// A lane's four consecutive voxels (linear index order) of its workgroup's kExtractVoxels, and their crossings.
struct TsdfLane {
    int mask[4];
    float q[4][3];
    unsigned ix[4], iy[4], iz[4];
    int mine;                           // crossings of the four voxels
};

__device__ __forceinline__ unsigned long long tsdf_lane_first() {
    return (unsigned long long)blockIdx.x * kExtractVoxels + 4ull * threadIdx.x;
}

__device__ __forceinline__ void tsdf_lane_crossings(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsdfGrid& g,
                                                    unsigned long long first, TsdfLane& L) {
    L.mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        L.mask[j] = 0;
        if (first + j > g.n) continue;
        const unsigned i = (unsigned)(first + j);
        L.iz[j] = i / g.XY;
        const unsigned rem = i - L.iz[j] * g.XY;
        L.iy[j] = rem / g.X;
        L.ix[j] = rem - L.iy[j] * g.X;
        L.mask[j] = tsdf_crossings(tsdf, weight, g, i, L.ix[j], L.iy[j], L.iz[j], L.q[j]);
        L.mine += __popc(L.mask[j]);
    }
}

// Writes the lane's crossings as points from row `pos` on while the row is below the capacity.  ROWS: also the row of every voxel's
// first crossing (whether written or not, and whether the voxel has one or not) into first_row[linear voxel index].  COLOR: also row
// `pos` of colors, per plane j of color [3][Z][Y][X]: C_j(a) + q * (C_j(b) - C_j(a)) with the q that places the point.
template <bool ROWS, bool COLOR = false>
__device__ __forceinline__ void tsdf_lane_write(const TsdfGrid& g, const TsdfLane& L, unsigned long long first, long long pos,
                                                float* __restrict__ points, long long capacity, int* __restrict__ first_row,
                                                const float* __restrict__ color = nullptr, float* __restrict__ colors = nullptr) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (ROWS && first + j <= g.n) first_row[first + j] = (int)pos;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!(L.mask[j] & (1 << k))) continue;
            if (pos < capacity) {
                const float fi[3] = {(float)L.ix[j], (float)L.iy[j], (float)L.iz[j]};
                float* out = points + 3 * pos;
                out[0] = g.ox + g.vs * (k == 0 ? fi[0] + L.q[j][0] : fi[0]);
                out[1] = g.oy + g.vs * (k == 1 ? fi[1] + L.q[j][1] : fi[1]);
                out[2] = g.oz + g.vs * (k == 2 ? fi[2] + L.q[j][2] : fi[2]);
                if (COLOR) {
                    const size_t a = (size_t)(first + j), b = a + (k == 0 ? 1u : k == 1 ? g.X : g.XY);
                    const size_t plane = (size_t)g.n + 1;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float Ca = color[c * plane + a], Cb = color[c * plane + b];
                        colors[3 * pos + c] = Ca + L.q[j][k] * (Cb - Ca);
                    }
                }
            }
            ++pos;
        }
    }
}

// The coloured writers' further kernel arguments; the colourless kernels take none (an empty pack: the kernels they were before colour).
struct TsdfPointColour {
    const float* color;                 // the volume's planes [3][Z][Y][X]
    float* colors;                      // [capacity][3]
};

__device__ __forceinline__ TsdfPointColour tsdf_point_colour() { return TsdfPointColour(); }
__device__ __forceinline__ const TsdfPointColour& tsdf_point_colour(const TsdfPointColour& k) { return k; }

// One workgroup: the exclusive prefix of nwg count records in index order, kScanPass records per pass with a carried total (int64),
// then (found, written = min(found, capacity)) into counts[0..1].
__device__ __forceinline__ void tsdf_scan_records(const int* __restrict__ wg_count, long long* __restrict__ wg_offset, int nwg,
                                                  long long capacity, long long* __restrict__ counts, long long* lds) {
    long long carry = 0;
    for (int base = 0; base < nwg; base += kScanPass) {
        const int r0 = base + 4 * (int)threadIdx.x;
        long long c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = r0 + j < nwg ? (long long)wg_count[r0 + j] : 0;
        long long total;
        long long at = carry + block_exclusive_256<long long>(((c[0] + c[1]) + c[2]) + c[3], lds, total);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (r0 + j < nwg) wg_offset[r0 + j] = at;
            at += c[j];
        }
        carry += total;
        __syncthreads();                // lds is rewritten by the next pass
    }
    if (threadIdx.x == 0) {
        counts[0] = carry;
        counts[1] = carry < capacity ? carry : capacity;
    }
}

static inline long tsdf_voxels(int X, int Y, int Z) {
    if (X <= 0 || Y <= 0 || Z <= 0) return NRGBD_E_SHAPE;
    const long xy = (long)X * Y;
    if (xy > kTsdfMaxVoxels || xy * Z > kTsdfMaxVoxels) return NRGBD_E_SHAPE;
    return xy * Z;
}

static inline bool tsdf_positive(float v) { return v > 0.f && v <= kFltMax; }

static inline TsdfGrid tsdf_grid(int X, int Y, int Z, long n, float ox, float oy, float oz, float voxel_size, float w_min) {
    TsdfGrid g;
    g.ox = ox; g.oy = oy; g.oz = oz; g.vs = voxel_size; g.w_min = w_min;
    g.X = (unsigned)X; g.Y = (unsigned)Y; g.Z = (unsigned)Z;
    g.XY = (unsigned)((long)X * Y > 0x7fffffffL ? 0x80000000u : (unsigned)((long)X * Y));
    g.n = (unsigned)(n - 1);
    return g;
}

}  // namespace nrgbd
