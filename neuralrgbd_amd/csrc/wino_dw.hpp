// wino_dw.hpp — what the two depth-Winograd kernels of the K-Net share (wino_dw.hip: F(2, 3) along depth, two output slices per
// tile; wino_dw4.hip: F(4, 3), four).  One copy of every step the two kernels have in common:
//   geometry   strip / stash / table constants, DwTile + dw_decode<slices per tile>, the serpentine channel-block order dw_cb
//   weights    the packer conv_wino_dw_pack_kernel<POINTS> with the depth matrices DwDepth<POINTS>, and its entry dw_pack
//   consumers  DwLane + dw_lane, dw_prime, dw_mfma_stage<FIRST>, dw_phase<P, NP> (the stages of one depth-transform index),
//              dw_plane_inverse + dw_plane_word, dw_emit, dw_store_stats
//   producers  DwItems + dw_items, DwBook + dw_book<OWN>, dw_activate<IDENT, CLAMP>, dw_transform, the running state DwProd with
//              dw_prod_init / dw_next_tile / dw_stage_end / dw_tile_end
//   protocol   the barrier protocol both kernels follow, written once (below, above the consumer steps)
//   host       dw_workgroups, dw_check (the launchers' shared refusals), dw_unit_ok, dw_lds_bytes / dw_lds_attr, DwLaunch + dw_launch
// From wino_pc.hpp, shared with wino_pc.hip as well: the XCD-aware split of the tile list (pc_tile_share) and the (scale, shift) table
// load (pc_load_ss_table).  Still a copy: DwItems / dw_items / dw_transform are wino_pc.hip's PcItems / pc_items / pc_transform (that
// file keeps its steps in an anonymous namespace of its own).  In the .hip files: what really differs — the depth transform's issue,
// publish / combine and fold (dw2_* in wino_dw.hip, d4_* in wino_dw4.hip) — and the two kernels.
// Both kernels run with the register file full.  Every step is a __forceinline__ function with its register arrays by reference and
// every scheduling barrier, opaque asm and __syncthreads() in its place in program order; DESIGN.md 6.2 ("Shared source") has what the
// split did to the device code and the timings that gated it.
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
// variant fetched ALL its reads).  Turning round at the phase boundary puts the most recently read units first.  Measured against
// the forward-only order, then the only order (profiles/r4_wino_serpentine_ab.txt): wino_dw.hip at config B 2.298 -> 2.282 ms plain
// and 2.821 -> 2.807 ms with residual + materialise, at config H 2.256 -> 2.228 ms with residual + materialise.
__device__ __forceinline__ int dw_cb(int p, int i, int ncb) { return (p & 1) ? ncb - 1 - i : i; }

// ---- The barrier protocol of both kernels.  G = tiles of this workgroup x NS stages, counted across tiles (DwProd::gi); every wave
// executes G + 2 barriers behind the one that follows the (scale, shift) table load.  A workgroup without tiles returns before the
// first of them, the table's included: the test is uniform and follows nothing but the tile-list split.
//   Producers, iteration g = 0 .. G-1: publish stage g into strip g & 1 from register sets requested ONE stage earlier, refill each
//   set for stage g + 1 right behind its use, transform stage g - 1 from strip (g - 1) & 1 into V[(g - 1) & 1], barrier.  The
//   transform lags the publish by one iteration because the barrier between them is what completes the shared strip (four waves
//   write it, each reads all of it); iteration 0 transforms nothing and does not advance the V buffer.
//   Closing: the transform of the last published stage G - 1 and its barrier, then one more: the consumers' last stage.
//   Consumers: two opening barriers (stage 0 published | stage 0 transformed), then per stage g its MFMAs on V[g & 1] and one barrier,
//   at which the wave ARRIVES EARLY: behind transform point xi = 14, when the stage's last LDS operands (xi = 15) are in registers.
//   The producers may then overwrite V[g & 1] with stage g + 2 — two V buffers, not wino_pc.hip's three: the third one's 32 KB hold
//   the second stash — and the wave reads the first operands of stage g + 1 from V[(g + 1) & 1], complete once that barrier is
//   passed, under its own last 8 MFMAs.  The phase-end fold sits between the last barrier of a phase and the next phase's MFMAs.
//   One barrier per stage; the consumers never wait for data, the producers wait for the consumers.

// ======================================================= consumer steps =====================================================
// A consumer lane (kq, jj) of wave wv: output channel 16 wv + jj; accumulator register r of row block m = Winograd tile
// 16 m + 4 kq + r = tile row 2m + (kq >> 1), tile column 4 (kq & 1) + r.
struct DwLane {
    int kq, jj;
    int a0, a1;                // LDS offsets of the lane's A operands of the two row blocks (+ xi * 512 floats + buffer)
    unsigned lane_yoff;        // the lane's part of an output's address (loop-invariant)
    const f32x4* wbase;        // the lane's word of the wave's weight line 0 of column group 0
};
using DwAcc = f32x4[16][2];    // [xi][row block]: ONE M_t at a time; the first stage of a phase takes a zero C operand: never cleared

__device__ __forceinline__ DwLane dw_lane(const WinoPcArgs& a, int lane, int wv) {
    DwLane c;
    c.kq = lane >> 4; c.jj = lane & 15;
    c.a0 = pc_slot(0, c.jj, c.kq); c.a1 = pc_slot(0, 16 + c.jj, c.kq);
    c.wbase = reinterpret_cast<const f32x4*>(a.wp) + wv * 64 + lane;
    c.lane_yoff = (unsigned)c.jj + (unsigned)((2 * (c.kq >> 1)) * a.W + 8 * (c.kq & 1)) * (unsigned)a.Cout;
    return c;
}

// the first weight lines of the ring (7 ahead, continues across stages, phases and tiles), the two opening barriers, the first A
// operands; returns an opaque (-1, -1): a - b is fma(b, -1, a) on register pairs (same rounding; a literal would be folded into two v_sub)
__device__ __forceinline__ f32x2 dw_prime(f32x4 (&Bn)[kPcNB], f32x4 (&An)[2][2], const f32x4* wt, const float* Vb, const DwLane& c) {
#pragma unroll
    for (int b = 0; b < kPcBD; ++b) Bn[b] = wt[b * 256];
    __syncthreads();                               // the producers publish stage 0 (transformed one iteration later)
    __syncthreads();                               // producers finish stage 0
    An[0][0] = *reinterpret_cast<const f32x4*>(Vb + c.a0);
    An[0][1] = *reinterpret_cast<const f32x4*>(Vb + c.a1);
    float neg1 = -1.f;
    asm volatile("" : "+v"(neg1));
    return f32x2{neg1, neg1};
}

// one stage = 16 transform points x (2 A reads + 1 weight line + 8 MFMAs) from V buffer Vc, with the stage's barrier (Vn: the next
// stage's buffer, for its first operands; wcur / wnx: the weight lines of this stage / the next).  FIRST (first stage of a phase):
// the first k-step takes a zero C operand instead of the accumulator.
template <bool FIRST>
__device__ __forceinline__ void dw_mfma_stage(DwAcc& acc, f32x4 (&An)[2][2], f32x4 (&Bn)[kPcNB], const float* Vc, const float* Vn,
                                              const f32x4* wcur, const f32x4* wnx, const DwLane& c) {
    const int a0 = c.a0, a1 = c.a1;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) {
        const int cur = xi & 1, nxt = cur ^ 1;
        if (xi + 1 < 16) {
            An[nxt][0] = *reinterpret_cast<const f32x4*>(Vc + a0 + (xi + 1) * (kPcTiles * kCB));
            An[nxt][1] = *reinterpret_cast<const f32x4*>(Vc + a1 + (xi + 1) * (kPcTiles * kCB));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[xi][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(An[cur][0][e], Bn[xi % kPcNB][e], FIRST && e == 0 ? zero4 : acc[xi][0], 0, 0, 0);
            acc[xi][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(An[cur][1][e], Bn[xi % kPcNB][e], FIRST && e == 0 ? zero4 : acc[xi][1], 0, 0, 0);
            // the weight line of the point 7 ahead is requested HERE, in the second MFMA gap of the point, not at its top beside the two
            // LDS reads: a vector-memory instruction costs the wave ~50 issue cycles, and three memory instructions in one gap let the
            // matrix pipe run dry (tools/probes/mfma_stream_probe.hip: 78.5 -> 85.4 % busy)
            if (e == kPcWPos) Bn[(xi + kPcBD) % kPcNB] = xi + kPcBD < 16 ? wcur[(xi + kPcBD) * 256] : wnx[(xi + kPcBD - 16) * 256];
            __builtin_amdgcn_sched_barrier(0);
        }
        if (xi == 14) {
            // EARLY stage barrier (the protocol above): with two V buffers this hides the LDS latency a third buffer hides in wino_pc.hip
            __syncthreads();
            An[0][0] = *reinterpret_cast<const f32x4*>(Vn + a0);
            An[0][1] = *reinterpret_cast<const f32x4*>(Vn + a1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// phase P of NP = the Cin/16 stages of one depth-transform index, accumulating its M_t (the kernel's fold follows).  The phases of a
// tile are separate straight-line instantiations so that the accumulators stay in fixed registers.  The weight stream is packed in
// EXECUTION order: stage s = P * ncb + channel block; behind the last phase comes the next tile's stream wt_next.
template <int P, int NP>
__device__ __forceinline__ void dw_phase(DwAcc& acc, f32x4 (&An)[2][2], f32x4 (&Bn)[kPcNB], const float* Vb, int& buf, const f32x4* wt,
                                         const f32x4* wt_next, int ncb, const DwLane& c) {
    for (int cb = 0; cb < ncb; ++cb) {                  // cb: position in the phase's sweep
        const int s = P * ncb + dw_cb(P, cb, ncb);
        const float* Vc = Vb + buf * kPcV;
        const int nbuf = buf ^ 1;
        const float* Vn = Vb + nbuf * kPcV;
        const f32x4* wcur = wt + (size_t)s * (16 * 256);
        const f32x4* wnx = cb + 1 < ncb ? wt + (size_t)(P * ncb + dw_cb(P, cb + 1, ncb)) * (16 * 256)
                           : (P < NP - 1 ? wt + (size_t)((P + 1) * ncb + dw_cb(P + 1, 0, ncb)) * (16 * 256) : wt_next);
        if (cb == 0) dw_mfma_stage<true>(acc, An, Bn, Vc, Vn, wcur, wnx, c);
        else dw_mfma_stage<false>(acc, An, Bn, Vc, Vn, wcur, wnx, c);
        buf = nbuf;
    }
}

// The plane inverse transform A^T M_t A of one (row block m, register pair rp) group: tr[a][xi_x] = sum_xi_y A^T[a][xi_y] M[xi_y][xi_x] ...
__device__ __forceinline__ void dw_plane_inverse(const DwAcc& acc, int m, int rp, f32x2 n1, f32x2 (&tr)[2][4]) {
#pragma unroll
    for (int xx = 0; xx < 4; ++xx) {
        const f32x2 m0 = rp ? acc[0 + xx][m].hi : acc[0 + xx][m].lo, m1 = rp ? acc[4 + xx][m].hi : acc[4 + xx][m].lo;
        const f32x2 m2 = rp ? acc[8 + xx][m].hi : acc[8 + xx][m].lo, m3 = rp ? acc[12 + xx][m].hi : acc[12 + xx][m].lo;
        tr[0][xx] = (m0 + m1) + m2;
        tr[1][xx] = __builtin_elementwise_fma(m3, n1, __builtin_elementwise_fma(m2, n1, m1));   // (m1 - m2) - m3
    }
}
// ... and its word (m, rp, aa) = output row 2 (tile row) + aa of tiles r = 2 rp (.x, .z) and 2 rp + 1 (.y, .w), columns
// 2 (tile column) + 0 (.lo) and + 1 (.hi).  The folds keep word wi = (m * 2 + rp) * 2 + aa of a lane at stash[wi * 64].
__device__ __forceinline__ f32x4 dw_plane_word(const f32x2 (&tr)[2][4], int aa, f32x2 n1) {
    const f32x2 o0 = (tr[aa][0] + tr[aa][1]) + tr[aa][2];
    const f32x2 o1 = __builtin_elementwise_fma(tr[aa][3], n1, __builtin_elementwise_fma(tr[aa][2], n1, tr[aa][1]));
    return __builtin_shufflevector(o0, o1, 0, 1, 2, 3);
}

// a completed word of an output slice (ys: the wave's 16 channels of the tile's first pixel in that slice) goes out at once — short
// live ranges: the register file is full here — with the slice's partial statistics: the (m, rp, aa) part of the address is uniform
__device__ __forceinline__ void dw_emit(const WinoPcArgs& a, const DwLane& c, float* ys, int m, int rp, int aa, const f32x4 v, f32x2& S1, f32x2& S2) {
    float* oa = ys + ((size_t)(4 * m + aa) * a.W + (size_t)(2 * (2 * rp))) * a.Cout;       // tile r = 2 rp
    float* ob = ys + ((size_t)(4 * m + aa) * a.W + (size_t)(2 * (2 * rp + 1))) * a.Cout;   // tile r + 1
    oa[c.lane_yoff] = v.x; oa[c.lane_yoff + a.Cout] = v.z;
    ob[c.lane_yoff] = v.y; ob[c.lane_yoff + a.Cout] = v.w;
    S1 = (S1 + v.lo) + v.hi;
    S2 = __builtin_elementwise_fma(v.hi, v.hi, __builtin_elementwise_fma(v.lo, v.lo, S2));
}

// the N slices a phase completed: the wave owns its 16 channels, so reduce over the 4 lanes (kq) that share a channel; column-major
// partials [2 Cout][rows], slice q in row row0 + q.  All N reductions come first and run whether or not statistics are wanted; only
// the stores look at a.stats.  With the reductions under that test the compiler is free to sink a slice's 32 accumulations out of the
// fold into the branch, which keeps every output word alive across the fold (wino_dw4.hip: 28 -> 152 bytes of scratch).
template <int N>
__device__ __forceinline__ void dw_store_stats(const WinoPcArgs& a, const DwLane& c, int co, int row0, const f32x2 (&S1)[N], const f32x2 (&S2)[N]) {
    float s1[N], s2[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        s1[q] = S1[q].x + S1[q].y; s2[q] = S2[q].x + S2[q].y;
        s1[q] += __shfl_xor(s1[q], 16, 64); s2[q] += __shfl_xor(s2[q], 16, 64);
        s1[q] += __shfl_xor(s1[q], 32, 64); s2[q] += __shfl_xor(s2[q], 32, 64);
    }
    if (c.kq == 0 && a.stats) {
#pragma unroll
        for (int q = 0; q < N; ++q) {
            a.stats[(size_t)co * a.rows + row0 + q] = s1[q];
            a.stats[(size_t)(a.Cout + co) * a.rows + row0 + q] = s2[q];
        }
    }
}

// ======================================================= producer steps =====================================================
// A producer lane's items (as wino_pc.hip's PcItems).  Load / publish item u = 192 pw + lane + 64 u over the whole 10-row halo (every
// halo word has ONE loader) -> strip pixel pi = item >> 2 in (row, de-interleaved column) order, 16-byte word w4; row and column are
// recomputed where needed.  Transform item: (tile of the row, 16-byte word, half of the xi rows).
struct DwItems {
    int id0, w4;               // item u = id0 + 64 u; the item's 16-byte word
    int wr_off[kDwNPF];        // strip offset an item is published at
    int rdR0, rdR1, rdR2;      // strip offsets of the transform's three rows, in the order it takes them
    float sg, m1;              // sign of the third row; an opaque -1
    int vslot;                 // float offset in a V buffer of the lane's first transform point xi = 8 thalf; point xi + k: + 512 k
    __device__ __forceinline__ int item_id(int u) const { return id0 + 64 * u; }
    __device__ __forceinline__ int row(int u) const { return (item_id(u) >> 2) / 18; }
    __device__ __forceinline__ int cp(int u) const { const int pi = item_id(u) >> 2; return pi - (pi / 18) * 18; }
    __device__ __forceinline__ int col(int u) const { const int c = cp(u); return c < 9 ? 2 * c : 2 * c - 17; }   // even columns first, then odd
};

__device__ __forceinline__ DwItems dw_items(int pw, int lane) {
    DwItems p;
    p.id0 = 192 * pw + lane;
    p.w4 = lane & 3;
#pragma unroll
    for (int u = 0; u < kDwNPF; ++u) {
        const int item = p.item_id(u), e = (item - kDwShItems) >> 2;   // lanes without an item write a zero into a pad pixel (columns 18, 19)
        p.wr_off[u] = item < kDwShItems ? (p.row(u) * kPcRawW + p.cp(u)) * kCB + p.w4 * 4
                                        : ((e >> 1) * kPcRawW + 18 + (e & 1)) * kCB + p.w4 * 4;
    }
    const int tword = lane & 3, txl = ((lane >> 5) << 2) | ((lane >> 2) & 3), thalf = (lane >> 4) & 1;
    p.vslot = pc_slot(8 * thalf, pw * 8 + txl, tword);
    // the lane reads its three strip rows in a lane-dependent ORDER (R0, R1, R2) and computes ya = R0 - R1, yb = R1 + sg * R2:
    // half 0 (xi_y 0, 1): rows (0, 2, 1), sg = +1; half 1 (xi_y 2, 3): rows (2, 1, 3), sg = -1 — no per-lane selects
    const int rdc = txl * kCB + tword * 4 + 2 * pw * kPcRawW * kCB;   // the tile row's halo rows start at strip row 2 pw
    p.rdR0 = (thalf ? 2 : 0) * kPcRawW * kCB + rdc; p.rdR1 = (thalf ? 1 : 2) * kPcRawW * kCB + rdc;
    p.rdR2 = (thalf ? 3 : 1) * kPcRawW * kCB + rdc;
    p.sg = thalf ? -1.f : 1.f;
    p.m1 = -1.f;
    asm volatile("" : "+v"(p.m1));
    return p;
}

// Per-tile book of a lane's items: in-plane BYTE offset (a harmless in-tensor offset when outside), 1 inside the image / 0 outside
// (zero padding), OWN: owner bits — the materialised input is written once per pixel: every halo pixel has ONE loader, it owns the
// tile's own 8 x 16.  Two books: the refills of a tile's last stage already load the next tile's words.
struct DwBook { unsigned off[kDwNPF]; float keep[kDwNPF]; unsigned own; };

template <bool OWN>
__device__ __forceinline__ void dw_book(const WinoPcArgs& a, const DwItems& p, const DwTile& t, DwBook& b) {
    b.own = 0;
#pragma unroll
    for (int u = 0; u < kDwNPF; ++u) {
        const int hy = p.row(u), hx = p.col(u);
        const int gy = t.y0 + hy - 1, gx = t.x0 + hx - 1;
        const bool in = p.item_id(u) < kDwShItems && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        b.off[u] = 4u * (in ? (unsigned)(((size_t)gy * a.W + gx) * a.Cin + p.w4 * 4) : (unsigned)(p.w4 * 4));
        b.keep[u] = in ? 1.f : 0.f;
        if constexpr (OWN) {
            const bool mine = hy >= 1 && hy <= kPcTH;
            if (in && mine && hx >= 1 && hx <= kPcTW) b.own |= 1u << u;
        }
    }
}

// a unit's raw words -> act(x * s + t) as register pairs, breadth-first and pinned (wino_pc.hip's pc_activate_publish says why); ss: the
// channel block's (scale, shift) words of the pre-paired LDS table (pc_ss_slot).  IDENT: x as it is; CLAMP: the ReLU is the FMA's clamp.
template <bool IDENT, bool CLAMP>
__device__ __forceinline__ void dw_activate(const f32x4 (&pre)[kDwNPF], const f32x4 (&ss)[2], int x_relu, f32x2 (&lo)[kDwNPF], f32x2 (&hi)[kDwNPF]) {
    if constexpr (IDENT) {
#pragma unroll
        for (int i = 0; i < kDwNPF; ++i) { lo[i] = pre[i].lo; hi[i] = pre[i].hi; }
    } else {
        const f32x2 sc01 = ss[0].lo, sh01 = ss[0].hi, sc23 = ss[1].lo, sh23 = ss[1].hi;
        if constexpr (CLAMP) {
#pragma unroll
            for (int i = 0; i < kDwNPF; ++i) {
                lo[i] = pk_fma_clamp01(pre[i].lo, sc01, sh01);
                hi[i] = pk_fma_clamp01(pre[i].hi, sc23, sh23);
            }
        } else {
#pragma unroll
            for (int i = 0; i < kDwNPF; ++i) {
                lo[i] = __builtin_elementwise_fma(pre[i].lo, sc01, sh01);
                hi[i] = __builtin_elementwise_fma(pre[i].hi, sc23, sh23);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (x_relu) {
#pragma unroll
                for (int i = 0; i < kDwNPF; ++i) { lo[i].x = relu1(lo[i].x); lo[i].y = relu1(lo[i].y); hi[i].x = relu1(hi[i].x); hi[i].y = relu1(hi[i].y); }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// plane transform B^T d B of this lane's (tile, word): rows (2 of the 4 xi_y), then columns; strip rawT -> V buffer Vq
__device__ __forceinline__ void dw_transform(const DwItems& p, const float* rawT, float* Vq) {
    const float m1 = p.m1;
    f32x4 ya[4], yb[4];
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        const int co = ((cc & 1) * 9 + (cc >> 1)) * kCB;   // strip columns of the tile: cc = 0 at its column pixel, 1: +9 pixels, 2: +1, 3: +10
        const f32x4 R0 = *reinterpret_cast<const f32x4*>(rawT + p.rdR0 + co);
        const f32x4 R1 = *reinterpret_cast<const f32x4*>(rawT + p.rdR1 + co);
        const f32x4 R2 = *reinterpret_cast<const f32x4*>(rawT + p.rdR2 + co);
        ya[cc] = pk_fma_s(R1, m1, R0);     // R0 - R1
        yb[cc] = pk_fma_s(R2, p.sg, R1);   // R1 +- R2
    }
    float* V = Vq + p.vslot;                     // points 8 thalf + 0 .. 3 from ya, + 4 .. 7 from yb
    constexpr int kXi = kPcTiles * kCB;          // floats per transform point
    *reinterpret_cast<f32x4*>(V + 0 * kXi) = pk_fma_s(ya[2], m1, ya[0]);   // y0 - y2
    *reinterpret_cast<f32x4*>(V + 1 * kXi) = pk_add(ya[1], ya[2]);
    *reinterpret_cast<f32x4*>(V + 2 * kXi) = pk_fma_s(ya[1], m1, ya[2]);   // y2 - y1
    *reinterpret_cast<f32x4*>(V + 3 * kXi) = pk_fma_s(ya[3], m1, ya[1]);   // y1 - y3
    *reinterpret_cast<f32x4*>(V + 4 * kXi) = pk_fma_s(yb[2], m1, yb[0]);
    *reinterpret_cast<f32x4*>(V + 5 * kXi) = pk_add(yb[1], yb[2]);
    *reinterpret_cast<f32x4*>(V + 6 * kXi) = pk_fma_s(yb[1], m1, yb[2]);
    *reinterpret_cast<f32x4*>(V + 7 * kXi) = pk_fma_s(yb[3], m1, yb[1]);
}

// a producer wave's state across stages and tiles.  The book is selected per value (nx ? nxt.off[u] : cur.off[u]), not per pointer:
// a pointer select would force both books into scratch memory.
struct DwProd {
    DwItems p;
    DwTile tl, tn;             // current tile; the next one once the refills reach into it
    DwBook cur, nxt;
    float* Vb; float* rawb; const float* ssl;
    unsigned plane;            // floats of one slice
    int qbuf, gi;              // V buffer the next transform writes; stages published so far (strip parity)
    bool has_next, interior;   // another tile follows; the current tile's whole 10 x 18 halo lies inside the image: no padding mask
    __device__ __forceinline__ float* strip(int parity) const { return rawb + parity * kDwShStrip; }
};

template <int ZT, bool OWN>
__device__ __forceinline__ void dw_prod_init(const WinoPcArgs& a, DwProd& P, int pw, int lane, float* Vb, float* rawb, const float* ssl, int first) {
    P.p = dw_items(pw, lane);
    P.Vb = Vb; P.rawb = rawb; P.ssl = ssl;
    P.plane = (unsigned)((size_t)a.H * a.W * a.Cin);
    P.tl = dw_decode<ZT>(first, a); P.tn = P.tl;
    dw_book<OWN>(a, P.p, P.tl, P.cur);
    P.qbuf = 0; P.gi = 0; P.has_next = false;
}
// top of a tile (80 % of the tiles at config B are interior)
__device__ __forceinline__ void dw_tile_begin(const WinoPcArgs& a, DwProd& P, bool has_next) {
    P.has_next = has_next;
    P.interior = P.tl.y0 >= 1 && P.tl.y0 + kPcTH + 1 <= a.H && P.tl.x0 >= 1 && P.tl.x0 + kPcTW + 1 <= a.W;
}
// the book of the next tile t: needed by the refills of the current tile's last stage
template <int ZT, bool OWN>
__device__ __forceinline__ void dw_next_tile(const WinoPcArgs& a, DwProd& P, int t) {
    P.tn = dw_decode<ZT>(t, a);
    dw_book<OWN>(a, P.p, P.tn, P.nxt);
}
// behind a stage's barrier: the transform lags the publish by one stage, so the first stage does not advance the V buffer
__device__ __forceinline__ void dw_stage_end(DwProd& P) {
    if (P.gi > 0) P.qbuf ^= 1;
    ++P.gi;
}
__device__ __forceinline__ void dw_tile_end(DwProd& P) {
    P.tl = P.tn;
    P.cur = P.nxt;
}

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

// dynamic LDS of a launch: 2 x 32 KB V + 2 x 12.8 KB strips + 4 waves x 2 x 8 KB stashes + `tables` (scale, shift) tables of Cin pairs
static inline size_t dw_lds_bytes(int tables, int Cin) {
    return (size_t)(kDwNBuf * kPcV + kDwStrips + 4 * kDwStashWave + tables * 2 * Cin) * sizeof(float);
}
// the function's opt-in is set to the form's maximum (Cin = kDwMaxCin, capped by the CU's 160 KB), not to a call's size (see
// nrgbd_conv_wino_f32: hipGraph replays read it)
static inline int dw_lds_attr(int tables) {
    const size_t b = dw_lds_bytes(tables, kDwMaxCin), cap = 160 * 1024;
    return (int)(b < cap ? b : cap);
}

// one launch of one instantiation: persistent workgroups of 8 waves
struct DwLaunch { int nwg; size_t lds; int lds_attr; hipStream_t st; };
template <auto Kernel, class Args>
static inline int dw_launch(const DwLaunch& l, const Args& a) {
    const hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(Kernel), l.lds_attr);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(Kernel, dim3(l.nwg), dim3(512), l.lds, l.st, a);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

}  // namespace nrgbd
