// wave_fold.hpp — fixed-order wave64 reductions of many values per lane, shared by depth_eval.hip and icp.hip.
#pragma once
#include "common.hpp"

namespace nrgbd {

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Wave sums of N = 16 m values per lane with m + N / 2 + N / 4 + ... shuffles instead of 6 N: at each of four steps (lane bits 5, 4, 3, 2)
// a lane keeps one half of its values and hands the other half to its partner, which keeps that one — statically indexed selects, no
// dynamic register index —, then the m values left are added over the last two lane bits.  Afterwards a[0 .. m) of every lane hold the
// wave's sums of the values fold_index(lane, i); the order of the additions is fixed.
template <typename T, int N, int H>
__device__ __forceinline__ void fold_step(T (&a)[N], bool upper, int offset) {
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const T send = upper ? a[i] : a[i + H];
        const T keep = upper ? a[i + H] : a[i];
        a[i] = keep + __shfl_xor(send, offset, 64);
    }
}
template <typename T, int N>
__device__ __forceinline__ void wave_fold_sum(T (&a)[N], int lane) {
    static_assert(N % 16 == 0, "four halving steps");
    fold_step<T, N, N / 2>(a, (lane & 32) != 0, 32);
    fold_step<T, N, N / 4>(a, (lane & 16) != 0, 16);
    fold_step<T, N, N / 8>(a, (lane & 8) != 0, 8);
    fold_step<T, N, N / 16>(a, (lane & 4) != 0, 4);
#pragma unroll
    for (int i = 0; i < N / 16; ++i) {
        a[i] += __shfl_xor(a[i], 2, 64);
        a[i] += __shfl_xor(a[i], 1, 64);
    }
}
template <int N>
__device__ __forceinline__ int fold_index(int lane, int i) {
    return i + ((lane & 32) ? N / 2 : 0) + ((lane & 16) ? N / 4 : 0) + ((lane & 8) ? N / 8 : 0) + ((lane & 4) ? N / 16 : 0);
}

}  // namespace nrgbd
