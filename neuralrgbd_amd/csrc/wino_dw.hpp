// wino_dw.hpp — what the two depth-Winograd kernels of the K-Net share (wino_dw.hip: F(2, 3) along depth, two output slices per
// tile; wino_dw4.hip: F(4, 3), four) and that can be shared without changing one instruction of either kernel:
//   geometry   strip / stash / table constants, DwTile + dw_decode<slices per tile>, the serpentine channel-block order dw_cb
//   weights    the packer conv_wino_dw_pack_kernel<POINTS> with the depth matrices DwDepth<POINTS>, and its entry dw_pack
//   host       dw_workgroups (persistent workgroups), dw_check (the launchers' shared refusals), dw_unit_ok
// From wino_pc.hpp, shared with wino_pc.hip as well: the XCD-aware split of the tile list (pc_tile_share) and the (scale, shift) table
// load (pc_load_ss_table).  NOT here, although both kernels carry them token for token: the consumers' MFMA stage,
// plane inverse transform and statistics, the producers' item map, book, activation and plane transform.  Both kernels run with the
// register file full; moved into functions of this header (arrays by reference, every scheduling barrier in place) each of them
// changed the kernels' register allocation or instruction order, and a changed stream needs a timing gate.
#pragma once
#include "wino_pc.hpp"

namespace nrgbd {

constexpr int kDwStashWave = 2 * 8 * 64 * 4;   // floats of one consumer wave's two LDS stashes: [2][8 words][64 lanes][4]
constexpr int kDwMaxCin = 512;                 // (scale, shift) tables of x and res live in LDS: 2 x 2 x Cin floats
constexpr int kDwNBuf = 2;                     // V buffers (wino_pc.hip: 3; the third one's 32 KB hold the second stash here)
// SHARED strips (round 4): wino_pc.hip's producer wave p loads the four halo rows 2p .. 2p+3 its tile row needs into a PRIVATE strip
// — 16 rows for a 10-row halo, i.e. every interior row is loaded, activated and published twice.  Here the 10 x 18 halo of a unit is
// split once over the 256 producer lanes (3 words per lane instead of 5) into a strip all four waves share, published one stage
// AHEAD: iteration i publishes stage i into strip[i & 1] and transforms stage i - 1 from strip[(i - 1) & 1] (complete since the
// stage barrier), so the only synchronisation is the barrier the stage has anyway (one more at the start).  Per stage and
// producer wave: 6 instead of 10 loads, 18 instead of 30 packed activation / combine FMAs, 9 instead of 15 strip accesses.
constexpr int kDwShRows = kPcTH + 2;                       // halo rows of a tile
constexpr int kDwShStrip = kDwShRows * kPcRawW * kCB;      // floats of one shared strip: [10 rows][20 pixels][16] = 12.8 KB
constexpr int kDwShItems = kDwShRows * 18 * 4;             // (row, column, 16-byte word) items of a unit: 720
constexpr int kDwNPF = 3;                                  // items per producer lane and unit (720 over 256 lanes)
constexpr int kDwStrips = 2 * kDwShStrip;                  // floats of the strip region

struct DwTile { int z0, y0, x0, cg, row0; };   // row0: statistics row of slice z0 (slice z0 + k: row0 + k)

// tile t of the list -> ZT output slices z0 .. z0 + ZT - 1 of an 8x16 tile, 64 output channels
template <int ZT>
__device__ __forceinline__ DwTile dw_decode(int t, const WinoPcArgs& a) {
    DwTile r;
    const int ncg = a.Cout >> 6;
    const int tiles_x = (a.W + kPcTW - 1) / kPcTW;
    const int row = t / ncg;
    r.cg = t - row * ncg;
    t = row;
    const int nz = a.N >> (ZT == 4 ? 2 : 1);
    const int zi = t % nz; t /= nz;             // depth fastest: list neighbours share all but ZT of their ZT + 2 input slices
    const int tx = t % tiles_x, ty = t / tiles_x;
    r.z0 = ZT * zi;
    r.y0 = ty * kPcTH; r.x0 = tx * kPcTW;
    r.row0 = (ty * tiles_x + tx) * a.N + r.z0;
    return r;
}

// Channel block of the i-th stage of phase p: odd phases sweep the blocks backwards (ncb-1 .. 0).  Neighbouring phases read the
// same slices (wino_dw.hip: phases 1 and 2 the same two, 0 / 1 and 2 / 3 share one): with every phase sweeping forwards a unit's
// re-read came Cin/16 stages after its first read, and the 32 workgroups of an XCD stream 1.5 MB (3 MB with a residual operand)
// per stage through their 4 MB L2 beside the 1 MB weight stream — every re-read missed (profiles/r3_pmc_wino.txt: the residual
// variant fetched ALL its reads).  Turning round at the phase boundary puts the most recently read units first.
// serp: the kernel's build knob (NRGBD_DW_SERP / NRGBD_D4_SERP; 0 in experimental A/B builds only, build.build_variant)
__device__ __forceinline__ int dw_cb(int serp, int p, int i, int ncb) { return (serp && (p & 1)) ? ncb - 1 - i : i; }

// ---------------------------------------------------------------- weights -----------------------------------------------------
// The depth transform of a kernel with POINTS transform points: Gd (U_t = sum_kd Gd[t][kd] (G g_kd G^T)) and the depth index t of
// phase p of the weight stream — wino_dw.hip runs its phases in the order of t, wino_dw4.hip in the order its fold wants.
template <int POINTS> struct DwDepth;
template <> struct DwDepth<4> {
    static constexpr double Gd[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
    static constexpr int t_of_phase[4] = {0, 1, 2, 3};
};
template <> struct DwDepth<6> {
    static constexpr double Gd[6][3] = {{16.0 / 9.0, 0.0, 0.0}, {-1.0, -0.5, -0.25}, {-1.0, 0.5, -0.25}, {1.0 / 9.0, 1.0 / 6.0, 0.25},
                                        {1.0 / 9.0, -1.0 / 6.0, 0.25}, {0.0, 0.0, 1.0}};
    static constexpr int t_of_phase[6] = {1, 2, 3, 4, 0, 5};
};

// w [Cout][Cin][3][3][3] -> U_t = sum_kd Gd[t][kd] (G g_kd G^T) (float64, rounded once) in the kernels' B-operand order, phases in
// EXECUTION order: [cg][stage = p*ncb + cb][xi][wave][lane = kq*16 + j][e], co = cg*64 + 16*wave + j, ci = cb*16 + 4*kq + e.
// transposed = 1: the data-gradient stream (w is stored [Cin][Cout][3][3][3] seen from this kernel: its ci is the stored tensor's output
// channel; taps flipped in every dimension); 2: both streams in one launch (grid.y = 2), the data gradient's behind the forward one
// (see conv_wino_pack_kernel).
template <int POINTS>
__global__ __launch_bounds__(256) void conv_wino_dw_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout,
                                                                int transposed) {
    const long total = (long)Cout * Cin * POINTS * 16;
    if (transposed == 2) {
        transposed = blockIdx.y;
        if (transposed) { const int c = Cin; Cin = Cout; Cout = c; wp += total; }
    }
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    long t = idx;
    const int e = t & 3; t >>= 2;
    const int j = t & 15; t >>= 4;
    const int kq = t & 3; t >>= 2;
    const int wave = t & 3; t >>= 2;
    const int xi = t & 15; t >>= 4;
    const int ncb = Cin / kCB;
    const int stage = (int)(t % (POINTS * ncb));
    const int cg = (int)(t / (POINTS * ncb));
    const int p = stage / ncb, cb = stage - p * ncb;
    const int co = cg * 64 + 16 * wave + j, ci = cb * kCB + 4 * kq + e;
    const double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
    const int td = DwDepth<POINTS>::t_of_phase[p];
    const int aa = xi >> 2, bb = xi & 3;
    double u = 0.0;
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) {
        const float* g = transposed ? w + (((size_t)ci * Cout + co) * 3 + (2 - kd)) * 9 : w + (((size_t)co * Cin + ci) * 3 + kd) * 9;
        double u2 = 0.0;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) u2 += G[aa][ky] * (double)g[transposed ? (2 - ky) * 3 + (2 - kx) : ky * 3 + kx] * G[bb][kx];
        u += DwDepth<POINTS>::Gd[td][kd] * u2;
    }
    wp[idx] = (float)u;
}

// ---------------------------------------------------------------- host --------------------------------------------------------
template <int POINTS>
static inline int dw_pack(const float* w, float* w_wino, int Cin, int Cout, int transposed, void* stream) {
    if (!w || !w_wino) return NRGBD_E_NULL;
    if (Cin <= 0 || Cin % kCB || Cout <= 0 || Cout % 64) return NRGBD_E_SHAPE;
    if (transposed < 0 || transposed > 2) return NRGBD_E_ARG;
    if (transposed == 2 && Cin % 64) return NRGBD_E_SHAPE;
    const long total = (long)Cout * Cin * POINTS * 16;
    hipLaunchKernelGGL(conv_wino_dw_pack_kernel<POINTS>, dim3((unsigned)((total + 255) / 256), transposed == 2 ? 2 : 1), dim3(256), 0,
                       (hipStream_t)stream, w, w_wino, Cin, Cout, transposed);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

// persistent workgroups of a launch over tiles of ZT output slices: one per CU, or one per tile where there are fewer
static inline int dw_workgroups(int ZT, int N, int H, int W, int Cout, int* out) {
    const long nt = (long)(nrgbd_conv_wino_tiles(N, H, W, 1) / ZT) * (Cout / 64);
    int dev = 0, ncu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return (int)e;
    if (ncu <= 0) return NRGBD_E_ARG;
    *out = nt < ncu ? (int)nt : ncu;
    return NRGBD_OK;
}

// what both launchers refuse about the shape (after their own null-pointer checks); rows: statistics rows, one per (8x16 tile,
// slice) as wino_pc.hip; ntiles: entries of the tile list
static inline int dw_check(int ZT, int N, int H, int W, int Cin, int Cout, int* rows, long* ntiles) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cin % kCB || Cin > kDwMaxCin || Cout <= 0 || Cout % 64) return NRGBD_E_SHAPE;
    if (N % ZT) return NRGBD_E_SHAPE;                                 // whole groups of ZT output slices
    if (H % kPcTH || W % kPcTW) return NRGBD_E_SHAPE;                 // whole 8x16 tiles only (every grid of the path; others: nrgbd_conv_wino_f32)
    if ((long)H * W * Cin >= (1L << 30)) return NRGBD_E_SHAPE;       // 32-bit BYTE offsets inside a slice (the slice is a 64-bit base)
    *rows = nrgbd_conv_wino_tiles(N, H, W, 1);
    *ntiles = (long)(*rows / ZT) * (Cout / 64);
    return NRGBD_OK;
}

// x_unit of the CLAMP forms: a power of two in (0, 1]
static inline bool dw_unit_ok(float x_unit) {
    int ex = 0;
    return x_unit > 0.f && x_unit <= 1.f && frexpf(x_unit, &ex) == 0.5f;
}

}  // namespace nrgbd
