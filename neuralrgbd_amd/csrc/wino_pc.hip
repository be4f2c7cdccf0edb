// wino_pc.hip — 3x3(x3) convolutions in the Winograd domain F(2x2, 3x3) on the fp32 matrix cores of gfx950, second generation:
// a PERSISTENT workgroup of 8 waves split into 4 consumer waves that do nothing but issue MFMAs and 4 producer waves that
// load, normalise, transform and publish the operand of the stage two steps ahead.
//
// Serves  (a) the K-Net's ten 64 -> 64 3x3x3 layers (models/basic.py:71-94): KD = 3 depth taps, each a 2-D Winograd problem;
//         (b) the 3x3 stride-1 layers of the feature CNN (models/psm_submodule.py:10-16,31-50,100-134), dilation 1 or 2:
//             KD = 1, any Cin % 16 == 0, Cout % 64 == 0 (a tile is repeated per 64-column group of outputs);
//         (c) the R-Net's 3x3 layers (EPI = 1) and its two transposed convolutions (EPI = 2: the deconv form, see pc_dc_*)
// with the same fused BatchNorm work around them as conv3d.hip / conv2d.hip: statistics of the raw output in the epilogue,
// normalise + ReLU + residual add (+ materialise) while the input is loaded.
//
// Why a second generation.  conv3d_wino.hip (generation 1) runs publish -> barrier -> transform -> barrier -> 128 MFMAs per
// stage in every wave: at 2 workgroups per CU the matrix pipe idles whenever both resident waves of a SIMD are in their
// load / transform phases or wait for the first weight line after the barrier (measured: 3.36 ms per layer at the
// 192x256x64 grid = 59 % of the Winograd-domain MFMA time).  Here the two kinds of work live in different waves:
//   consumer wave c (waves 4..7) = output channels 16c .. 16c+15 of ALL 16 transform points and all 32 tiles of the workgroup's
//       8x16-pixel tile (128 accumulator VGPRs): per stage 16 x (2 LDS reads + 1 weight line + 8 v_mfma_f32_16x16x4_f32);
//       weight lines (1 KB, packed per wave) run 7 steps ahead in an 8-deep register ring that continues across stages and
//       tiles; the first A operand of the next stage is read before the stage barrier (three V buffers make that legal);
//       the first k-step of a tile takes a zero C operand (the accumulators are never cleared).
//   producer waves (waves 0..3: the older waves win the SIMD's VALU arbitration): the 10x18 halo of one 16-channel block is
//       split over their 256 lanes (3 16-byte words each: every halo word has ONE loader): global -> registers (buffer loads,
//       TWO stages ahead, two register sets, the stage's (scale, shift) with them) -> BatchNorm / ReLU / residual, packed and
//       breadth-first -> the SHARED strip of the stage (two of them alternate); the transform B^T d B per (tile, 16-byte word,
//       half) -> V[q % 3] of producer wave p = tile row p (8 Winograd tiles) runs one iteration LATER, on the strip the stage
//       barrier has completed — no other synchronisation.
//   One s_barrier per stage; the consumers never wait for data (producers are two stages ahead), the producers wait for
//   the consumers — which is the point: the matrix pipe is the resource to keep busy.  What was measured on the way
//   (in-kernel clocks, profiles/r2_pmc_wino.txt): beside a wave that streams MFMAs a partner's VALU
//   instruction issues about once per MFMA, a dependent one misses its slot, so the producers' code is written for
//   instruction count and independence, not for FLOPs.
//   Persistent: one workgroup per CU walks its share of the tile list (XCD-aware: an XCD's workgroups sweep neighbouring
//   tiles, depth fastest, so the three slices a 3-D tile needs are shared in that XCD's L2), so a tile's epilogue and the
//   next tile's first loads overlap with the producers' run-ahead instead of being exposed at every workgroup boundary.
// LDS: 3 x 32 KB V + 2 x 12.8 KB strips = 122 KB (one workgroup per CU; 2 waves per SIMD, up to 256 VGPRs each).
//
// Measured, then removed (the switches and in-kernel timers this file carried until its split into named steps):
//   * private strips (producer wave p loads halo rows 2p .. 2p+3 into its own 4-row strip, 5 words per lane and stage, transform
//     in the same iteration behind an lgkmcnt(0)) against the shared strip (3 words per lane, transform one iteration later):
//     trunk 64 -> 64 layer 91.6 -> 87.9 us, residual + materialise 103 -> 92.9, HALF 32 -> 32 148.5 -> 140.8, HALF res + mat
//     178.1 -> 164.4 (profiles/r4_knet_producer_diet_ab.txt, 3b).  The shared strip is the only form now.
//   * producers only / consumers only (ablation bits 1 and 2 of a developer build), trunk 64 -> 64 before the shared strips:
//     full 106.1 us, consumers only 92.9, producers only 45.6 (same profile); per stage at the K-Net's config B, 10 ns ticks:
//     consumers mfma 220, barrier 19, epilogue 14; producers publish 118, transform 67, barrier 48 (profiles/r2_pmc_wino.txt).
//   * the HALF form's consumer clocks (wall_clock64 around the MFMA loop, the stage barrier and the epilogue, 32 -> 32 @
//     5 x 384 x 512): MFMA loop 65 %, barrier 18 %, epilogue 17 %: there the producers set the pace.
#include "wino_pc.hpp"

namespace nrgbd {

// MAT: the activated input is also written out (a.mat).  A template parameter because of what its stores do to the variants
// WITHOUT them (round 3, learnt on wino_dw.hip): once loads and stores of one wave can both be pending the
// compiler turns every s_waitcnt on a prefetched register into vmcnt(0), which also waits for the refill issued a moment
// earlier.  For the same reason the refills are unconditional and the (scale, shift) pairs come from an LDS copy.
// HALF: Cout = 32 (the feature CNN's half-resolution layers, psm_submodule.py:90-99,103: firstconv.1/.2 and layer1).  The four
// consumer waves split the tile as (row block m = wave >> 1: 16 of the 32 Winograd tiles) x (16-column group = wave & 1): 64
// accumulators and 64 MFMAs per stage and wave, transform points taken in PAIRS so that MFMAs on one accumulator still
// alternate with another's; the weight stream is the 64-column one with the upper 32 columns zero (waves 0 / 1 read their two
// lines of it); statistics rows are (tile, row block).  The producers are unchanged — they now set the pace (a stage's MFMAs
// take 0.85 us): 2.25x fewer multiplies than conv2d.hip's direct form of these layers.
// EPI = 1: the R-Net form (bias + LeakyReLU in the epilogue, no prologue, no statistics).  ODD: an odd stage count per tile.
// EPI = 2: the R-Net's transposed convolutions on that form: four sub-pixel phases, dead transform points skipped (pc_dc_*).
namespace {

// ======================================================= consumer steps =====================================================
// A consumer lane (kq, jj): output channel 16 cwv + jj of its column group; register r of row block m = tile 16 m + 4 kq + r.
struct PcLane {
    int kq, jj;
    int msel, cwv;             // HALF: the one row block this wave owns / the wave's 16-column group
    int a0, a1;                // LDS offsets of the lane's A operands of the two row blocks (+ xi * 512 floats + buffer)
    unsigned ldy, lane_yoff;   // pixel stride of the output; the lane's part of an output's address (loop-invariant)
};
template <bool HALF> using PcAcc = f32x4[16][HALF ? 1 : 2];   // [xi][row block]: written by the first stage of every tile (C operand = 0): never cleared

template <int DIL, int EPI, bool HALF>
__device__ __forceinline__ PcLane pc_lane(const WinoPcArgs& a, int lane, int wv) {
    PcLane c;
    c.kq = lane >> 4; c.jj = lane & 15;
    c.msel = HALF ? (wv >> 1) : 0;
    c.cwv = HALF ? (wv & 1) : wv;
    c.a0 = pc_slot(0, 16 * c.msel + c.jj, c.kq); c.a1 = pc_slot(0, 16 + c.jj, c.kq);
    c.ldy = (EPI == 1 && a.ldy) ? (unsigned)a.ldy : (unsigned)a.Cout;
    c.lane_yoff = (unsigned)c.jj + (unsigned)((DIL * 2 * (c.kq >> 1)) * a.W + 8 * (c.kq & 1) * DIL) * c.ldy;
    return c;
}

// prime: the first weight lines of the ring (before the opening barriers) ...
template <bool HALF>
__device__ __forceinline__ void pc_prime_weights(f32x4 (&Bn)[kPcNB], const f32x4* wt) {
    constexpr int BD = HALF ? 6 : kPcBD;   // weight lines in flight (HALF requests two per pair of points: an even distance)
#pragma unroll
    for (int b = 0; b < BD; ++b) Bn[b] = wt[b * 256];
}
// ... and the first four A operands (after them).  A operands run TWO transform points ahead (one point = 256 MFMA cycles < a
// loaded LDS's latency); HALF: An[pair & 3][point of the pair], two PAIRS ahead
template <bool HALF>
__device__ __forceinline__ void pc_prime_a(f32x4 (&An)[4][2], const float* Vb, const PcLane& c) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {   // HALF: points 2i, 2i + 1 of the wave's row block; else point i of both row blocks
        An[i][0] = *reinterpret_cast<const f32x4*>(Vb + c.a0 + (HALF ? 2 * i : i) * kPcTiles * kCB);
        An[i][1] = *reinterpret_cast<const f32x4*>(Vb + (HALF ? c.a0 + (2 * i + 1) * kPcTiles * kCB : c.a1 + i * kPcTiles * kCB));
    }
}

// one stage = 16 transform points x (2 A reads + 1 weight line + 8 MFMAs) from V buffer Vc (Vn: the next stage's, for its first
// operands; wcur / wnx: the weight lines of this stage / the next).  FIRST (stage 0 of a tile): the first k-step takes a zero C
// operand instead of the accumulator, which saves clearing 128 registers per tile.
template <bool HALF, bool FIRST>
__device__ __forceinline__ void pc_mfma_stage(PcAcc<HALF>& acc, f32x4 (&An)[4][2], f32x4 (&Bn)[kPcNB], const float* Vc, const float* Vn,
                                              const f32x4* wcur, const f32x4* wnx, const PcLane& c) {
    const int a0 = c.a0, a1 = c.a1;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    if constexpr (HALF) {
        // a step = the PAIR of transform points (2 xp, 2 xp + 1): 2 A reads (two pairs ahead), 8 MFMAs alternating
        // between the two accumulators, the weight lines of points 2 xp + 6 and 2 xp + 7 requested in two MFMA gaps
#pragma unroll
        for (int xp = 0; xp < 8; ++xp) {
            const int cur = xp & 3, nxt = (xp + 2) & 3;
            const float* Vs = xp + 2 < 8 ? Vc : Vn;   // pairs 0, 1 of the next stage: its buffer was completed before the previous barrier
            const int pn = (xp + 2) & 7;
            An[nxt][0] = *reinterpret_cast<const f32x4*>(Vs + a0 + (2 * pn) * (kPcTiles * kCB));
            An[nxt][1] = *reinterpret_cast<const f32x4*>(Vs + a0 + (2 * pn + 1) * (kPcTiles * kCB));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[2 * xp][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(An[cur][0][e], Bn[(2 * xp) % kPcNB][e],
                                                                      FIRST && e == 0 ? zero4 : acc[2 * xp][0], 0, 0, 0);
                acc[2 * xp + 1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(An[cur][1][e], Bn[(2 * xp + 1) % kPcNB][e],
                                                                          FIRST && e == 0 ? zero4 : acc[2 * xp + 1][0], 0, 0, 0);
                if (e == 1) Bn[(2 * xp + 6) % kPcNB] = 2 * xp + 6 < 16 ? wcur[(2 * xp + 6) * 256] : wnx[(2 * xp + 6 - 16) * 256];
                if (e == 3) Bn[(2 * xp + 7) % kPcNB] = 2 * xp + 7 < 16 ? wcur[(2 * xp + 7) * 256] : wnx[(2 * xp + 7 - 16) * 256];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else {
#pragma unroll
        for (int xi = 0; xi < 16; ++xi) {
            const int cur = xi & 3, nxt = (xi + 2) & 3;
            if (xi + 2 < 16) {
                An[nxt][0] = *reinterpret_cast<const f32x4*>(Vc + a0 + (xi + 2) * (kPcTiles * kCB));
                An[nxt][1] = *reinterpret_cast<const f32x4*>(Vc + a1 + (xi + 2) * (kPcTiles * kCB));
            } else {   // the first two operands of the next stage: its buffer was completed before the previous barrier
                An[nxt][0] = *reinterpret_cast<const f32x4*>(Vn + a0 + (xi + 2 - 16) * (kPcTiles * kCB));
                An[nxt][1] = *reinterpret_cast<const f32x4*>(Vn + a1 + (xi + 2 - 16) * (kPcTiles * kCB));
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[xi][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(An[cur][0][e], Bn[xi % kPcNB][e], FIRST && e == 0 ? zero4 : acc[xi][0], 0, 0, 0);
                acc[xi][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(An[cur][1][e], Bn[xi % kPcNB][e], FIRST && e == 0 ? zero4 : acc[xi][1], 0, 0, 0);
                // the weight line of the point 7 ahead is requested HERE, in the second MFMA gap of the point (kPcWPos = 1), not at its
                // top beside the two LDS reads: a vector-memory instruction costs the wave ~50 issue cycles, and three memory
                // instructions in one gap let the matrix pipe run dry (tools/probes/mfma_stream_probe.hip: 78.5 -> 85.4 % busy)
                if (e == kPcWPos) Bn[(xi + kPcBD) % kPcNB] = xi + kPcBD < 16 ? wcur[(xi + kPcBD) * 256] : wnx[(xi + kPcBD - 16) * 256];
                __builtin_amdgcn_sched_barrier(0);   // pin the order: the row blocks alternate (no back-to-back dependent MFMAs), the operand streams keep their distances
            }
        }
    }
}

// The epilogues: inverse transform Y = A^T M A in registers + output (+ bias, LeakyReLU when EPI = 1) + the lane's partial
// statistics (s1, s2).  Row block m, register r = tile row 2m + (kq >> 1), tile column 4 (kq & 1) + r: the (m, r, a) part of
// an output's address is uniform -> scalar base (ybase) + 32-bit lane offset stores, no per-store address arithmetic.
// Interior tile: everything on register PAIRS (tiles r, r+1 of a row block): v_pk_add_f32 / v_pk_fma_f32 halve the epilogue's VALU
// instructions; a - b is fma(b, -1, a) with an opaque -1 (same rounding; a literal would be folded into two scalar v_sub)
template <int DIL, int EPI, bool HALF>
__device__ __forceinline__ void pc_epilogue_interior(const PcAcc<HALF>& acc, const WinoPcArgs& a, const PcLane& c, float* ybase, bool cok,
                                                     float bval, float& s1, float& s2) {
    const unsigned ldy = c.ldy, lane_yoff = c.lane_yoff;
    float neg1 = -1.f;
    asm volatile("" : "+v"(neg1));
    const f32x2 n1 = {neg1, neg1};
    const f32x2 bias2 = {bval, bval};
    f32x2 S1 = {0.f, 0.f}, S2 = {0.f, 0.f};
#pragma unroll
    for (int mi = 0; mi < (HALF ? 1 : 2); ++mi) {
        const int m = HALF ? c.msel : mi;   // row block: address arithmetic uses m, the register index is mi
#pragma unroll
        for (int rp = 0; rp < 2; ++rp) {
            f32x2 tr[2][4];   // t[a][xi_x] = sum_xi_y A^T[a][xi_y] M[xi_y][xi_x]
#pragma unroll
            for (int xx = 0; xx < 4; ++xx) {
                const f32x2 m0 = rp ? acc[0 + xx][mi].hi : acc[0 + xx][mi].lo, m1 = rp ? acc[4 + xx][mi].hi : acc[4 + xx][mi].lo;
                const f32x2 m2 = rp ? acc[8 + xx][mi].hi : acc[8 + xx][mi].lo, m3 = rp ? acc[12 + xx][mi].hi : acc[12 + xx][mi].lo;
                tr[0][xx] = (m0 + m1) + m2;
                tr[1][xx] = __builtin_elementwise_fma(m3, n1, __builtin_elementwise_fma(m2, n1, m1));   // (m1 - m2) - m3
            }
#pragma unroll
            for (int aa = 0; aa < 2; ++aa) {
                f32x2 o0 = (tr[aa][0] + tr[aa][1]) + tr[aa][2];
                f32x2 o1 = __builtin_elementwise_fma(tr[aa][3], n1, __builtin_elementwise_fma(tr[aa][2], n1, tr[aa][1]));
                if constexpr (EPI == 1) {   // m_submodule.py:18-27: bias, LeakyReLU(0.01) = max(z, 0.01 z)
                    o0 = o0 + bias2; o1 = o1 + bias2;
                    if (a.out_lrelu) {
                        const f32x2 sl = {0.01f, 0.01f};
                        o0 = __builtin_elementwise_max(o0, o0 * sl); o1 = __builtin_elementwise_max(o1, o1 * sl);
                    }
                }
                float* oa = ybase + ((size_t)(DIL * (4 * m + aa)) * a.W + (size_t)(2 * (2 * rp) * DIL)) * ldy;       // tile r = 2 rp
                float* ob = ybase + ((size_t)(DIL * (4 * m + aa)) * a.W + (size_t)(2 * (2 * rp + 1) * DIL)) * ldy;   // tile r + 1
                if (cok) {
                    oa[lane_yoff] = o0.x; oa[lane_yoff + DIL * ldy] = o1.x;
                    ob[lane_yoff] = o0.y; ob[lane_yoff + DIL * ldy] = o1.y;
                }
                S1 = (S1 + o0) + o1;
                S2 = __builtin_elementwise_fma(o1, o1, __builtin_elementwise_fma(o0, o0, S2));
            }
        }
    }
    s1 = S1.x + S1.y; s2 = S2.x + S2.y;
}

// a tile that crosses the image's lower or right edge: scalar, every output bounds-checked
template <int DIL, int EPI, bool HALF>
__device__ __forceinline__ void pc_epilogue_edge(const PcAcc<HALF>& acc, const WinoPcArgs& a, const PcTile& tl, const PcLane& c, float* ybase,
                                                 bool cok, float bval, float& s1, float& s2) {
    const unsigned ldy = c.ldy, lane_yoff = c.lane_yoff;
#pragma unroll
    for (int mi = 0; mi < (HALF ? 1 : 2); ++mi) {
        const int m = HALF ? c.msel : mi;   // row block: address arithmetic uses m, the register index is mi
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float tr[2][4];
#pragma unroll
            for (int xx = 0; xx < 4; ++xx) {
                const float m0 = acc[0 + xx][mi][r], m1 = acc[4 + xx][mi][r], m2 = acc[8 + xx][mi][r], m3 = acc[12 + xx][mi][r];
                tr[0][xx] = (m0 + m1) + m2;
                tr[1][xx] = (m1 - m2) - m3;
            }
#pragma unroll
            for (int aa = 0; aa < 2; ++aa) {
                float o0 = (tr[aa][0] + tr[aa][1]) + tr[aa][2];
                float o1 = (tr[aa][1] - tr[aa][2]) - tr[aa][3];
                if constexpr (EPI == 1) {
                    o0 += bval; o1 += bval;
                    if (a.out_lrelu) { o0 = fmaxf(o0, 0.01f * o0); o1 = fmaxf(o1, 0.01f * o1); }
                }
                float* o = ybase + ((size_t)(DIL * (4 * m + aa)) * a.W + (size_t)(2 * r * DIL)) * ldy;   // uniform
                const int tile = 16 * m + 4 * c.kq + r;
                const int gy = tl.y0 + tl.py + DIL * (2 * (tile >> 3) + aa), gx = tl.x0 + tl.px + DIL * (2 * (tile & 7));
                if (gy < a.H && cok) {
                    if (gx < a.W) { o[lane_yoff] = o0; s1 += o0; s2 = __builtin_fmaf(o0, o0, s2); }
                    if (gx + DIL < a.W) { o[lane_yoff + DIL * ldy] = o1; s1 += o1; s2 = __builtin_fmaf(o1, o1, s2); }
                }
            }
        }
    }
}

// the wave owns its 16 channels: reduce over the 4 lanes (kq) that share a channel; column-major partials [2 Cout][rows]:
// nrgbd_bn_finalize_cm reads a channel's partials as one run
template <bool HALF>
__device__ __forceinline__ void pc_store_stats(const WinoPcArgs& a, const PcTile& tl, const PcLane& c, int co, float s1, float s2) {
    s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
    s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
    if (c.kq == 0) {
        const int srow = HALF ? 2 * tl.row + c.msel : tl.row;   // HALF: two waves share a channel -> a row per (tile, row block)
        a.stats[(size_t)co * a.rows + srow] = s1;
        a.stats[(size_t)(a.Cout + co) * a.rows + srow] = s2;
    }
}

// a finished tile: output + statistics
template <int DIL, int EPI, bool HALF>
__device__ __forceinline__ void pc_epilogue(const PcAcc<HALF>& acc, const WinoPcArgs& a, const PcTile& tl, const PcLane& c) {
    const int co = tl.cg * 64 + c.cwv * 16 + c.jj;
    float* ybase = a.y + (((size_t)tl.n * a.H + tl.y0 + tl.py) * a.W + tl.x0 + tl.px) * c.ldy + (EPI == 1 ? a.ycoff : 0) + tl.cg * 64 + c.cwv * 16;
    const bool cok = EPI != 1 || a.cout_valid == 0 || co < a.cout_valid;   // EPI = 1: a padded output column is not stored
    const bool inside = tl.y0 + tl.py + DIL * (kPcTH - 1) < a.H && tl.x0 + tl.px + DIL * (kPcTW - 1) < a.W;
    float s1 = 0.f, s2 = 0.f;
    float bval = 0.f;
    if constexpr (EPI == 1) bval = a.bias ? a.bias[co] : 0.f;
    if (inside) pc_epilogue_interior<DIL, EPI, HALF>(acc, a, c, ybase, cok, bval, s1, s2);
    else pc_epilogue_edge<DIL, EPI, HALF>(acc, a, tl, c, ybase, cok, bval, s1, s2);
    if (a.stats) pc_store_stats<HALF>(a, tl, c, co, s1, s2);
}

// ============================================ consumer steps of the deconv form (EPI = 2) ====================================
// ConvTranspose2d(k4, s2, p1) as four sub-pixel phases (a, b), each a 3x3 kernel that is non-zero in one 2x2 corner (phase-stacked
// along the output channels, autograd.conv_transpose2d_module): column group cg of the Cout = 256 launch = phase 2a + b.  A zero last
// (first) kernel row makes row 3 (0) of U = G g G^T zero, the same for columns: a phase has 9 live transform points of the 16, the
// 3 x 3 block xi_y = a .. a+2, xi_x = b .. b+2.  The consumers skip the weight line, the A reads and the MFMAs of the 7 dead points
// (2.25 instead of 4 multiplies per output and channel); the weight stream carries the 9 live lines per (stage, phase); the
// producers are the R-Net form's.  The phase is a template parameter of a whole tile (four straight-line bodies): a dead
// accumulator does not exist, the inverse transform takes the exact zero the unmasked evaluation computes there.
constexpr int kPcDcPts = 9;                     // live transform points per phase = weight lines per stage; also the weight ring's slots
template <int PH> __device__ constexpr int pc_dc_xi(int p) { return 4 * (p / 3 + (PH >> 1)) + p % 3 + (PH & 1); }   // p-th live point
template <int PH> __device__ constexpr bool pc_dc_live(int xi) {
    return (xi >> 2) >= (PH >> 1) && (xi >> 2) < (PH >> 1) + 3 && (xi & 3) >= (PH & 1) && (xi & 3) < (PH & 1) + 3;
}
__device__ __forceinline__ int pc_dc_first(int ph) { return (4 * (ph >> 1) + (ph & 1)) * (kPcTiles * kCB); }   // V offset of a phase's first live point

// the lane's output addressing: phase pixel (y, x) is full-resolution pixel (2y + a, 2x + b) of the [N][2H][2W][ldy] buffer, so a
// step in x is 2 ldy floats and a step in y 2 W of those; c.ldy holds the doubled stride
__device__ __forceinline__ PcLane pc_dc_lane(const WinoPcArgs& a, int lane, int wv) {
    PcLane c;
    c.kq = lane >> 4; c.jj = lane & 15;
    c.msel = 0; c.cwv = wv;
    c.a0 = pc_slot(0, c.jj, c.kq); c.a1 = pc_slot(0, 16 + c.jj, c.kq);
    c.ldy = 2u * (unsigned)a.ldy;
    c.lane_yoff = (unsigned)c.jj + (unsigned)((2 * (c.kq >> 1)) * (2 * a.W) + 8 * (c.kq & 1)) * c.ldy;
    return c;
}

// one stage = 9 live points x (2 A reads + 1 weight line + 8 MFMAs).  Rings whose length divides 9, so that a point's slots are
// the same in every stage: A operands two points ahead in 3 slots, weight lines 7 ahead in 9.  nx0: V offset of the first live
// point of the NEXT stage (the next tile's phase behind a tile's last stage); its second one is the point after it.
template <int PH, bool FIRST>
__device__ __forceinline__ void pc_dc_stage(PcAcc<false>& acc, f32x4 (&An)[3][2], f32x4 (&Bn)[kPcDcPts], const float* Vc, const float* Vn, int nx0,
                                            const f32x4* wcur, const f32x4* wnx, const PcLane& c) {
    const int a0 = c.a0, a1 = c.a1;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < kPcDcPts; ++p) {
        const int xi = pc_dc_xi<PH>(p), cur = p % 3, nxt = (p + 2) % 3;
        if (p + 2 < kPcDcPts) {
            An[nxt][0] = *reinterpret_cast<const f32x4*>(Vc + a0 + pc_dc_xi<PH>(p + 2) * (kPcTiles * kCB));
            An[nxt][1] = *reinterpret_cast<const f32x4*>(Vc + a1 + pc_dc_xi<PH>(p + 2) * (kPcTiles * kCB));
        } else {   // the first two operands of the next stage: its buffer was completed before the previous barrier
            An[nxt][0] = *reinterpret_cast<const f32x4*>(Vn + a0 + nx0 + (p + 2 - kPcDcPts) * (kPcTiles * kCB));
            An[nxt][1] = *reinterpret_cast<const f32x4*>(Vn + a1 + nx0 + (p + 2 - kPcDcPts) * (kPcTiles * kCB));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[xi][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(An[cur][0][e], Bn[p][e], FIRST && e == 0 ? zero4 : acc[xi][0], 0, 0, 0);
            acc[xi][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(An[cur][1][e], Bn[p][e], FIRST && e == 0 ? zero4 : acc[xi][1], 0, 0, 0);
            if (e == kPcWPos) Bn[(p + kPcBD) % kPcDcPts] = p + kPcBD < kPcDcPts ? wcur[(p + kPcBD) * 256] : wnx[(p + kPcBD - kPcDcPts) * 256];
            __builtin_amdgcn_sched_barrier(0);   // as in pc_mfma_stage: the row blocks alternate, the operand streams keep their distances
        }
    }
}

// the epilogues of pc_epilogue_interior / pc_epilogue_edge with a dead point's M = 0, bias + LeakyReLU as EPI = 1, the phase's
// scattered addresses, no statistics.  The additions are those of the unmasked form, zeros included (0 + x is not x for x = -0).
template <int PH>
__device__ __forceinline__ void pc_dc_epilogue_interior(const PcAcc<false>& acc, const WinoPcArgs& a, const PcLane& c, float* ybase, bool cok, float bval) {
    const unsigned ldy = c.ldy, lane_yoff = c.lane_yoff;
    const size_t W2 = 2 * (size_t)a.W;
    float neg1 = -1.f;
    asm volatile("" : "+v"(neg1));
    const f32x2 n1 = {neg1, neg1};
    const f32x2 bias2 = {bval, bval};
    const f32x2 z2 = {0.f, 0.f};
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int rp = 0; rp < 2; ++rp) {
            f32x2 tr[2][4];
#pragma unroll
            for (int xx = 0; xx < 4; ++xx) {
                const f32x2 m0 = !pc_dc_live<PH>(0 + xx) ? z2 : rp ? acc[0 + xx][m].hi : acc[0 + xx][m].lo;
                const f32x2 m1 = !pc_dc_live<PH>(4 + xx) ? z2 : rp ? acc[4 + xx][m].hi : acc[4 + xx][m].lo;
                const f32x2 m2 = !pc_dc_live<PH>(8 + xx) ? z2 : rp ? acc[8 + xx][m].hi : acc[8 + xx][m].lo;
                const f32x2 m3 = !pc_dc_live<PH>(12 + xx) ? z2 : rp ? acc[12 + xx][m].hi : acc[12 + xx][m].lo;
                tr[0][xx] = (m0 + m1) + m2;
                tr[1][xx] = __builtin_elementwise_fma(m3, n1, __builtin_elementwise_fma(m2, n1, m1));   // (m1 - m2) - m3
            }
#pragma unroll
            for (int aa = 0; aa < 2; ++aa) {
                f32x2 o0 = (tr[aa][0] + tr[aa][1]) + tr[aa][2];
                f32x2 o1 = __builtin_elementwise_fma(tr[aa][3], n1, __builtin_elementwise_fma(tr[aa][2], n1, tr[aa][1]));
                o0 = o0 + bias2; o1 = o1 + bias2;
                if (a.out_lrelu) {
                    const f32x2 sl = {0.01f, 0.01f};
                    o0 = __builtin_elementwise_max(o0, o0 * sl); o1 = __builtin_elementwise_max(o1, o1 * sl);
                }
                float* oa = ybase + ((size_t)(4 * m + aa) * W2 + (size_t)(2 * (2 * rp))) * ldy;       // tile r = 2 rp
                float* ob = ybase + ((size_t)(4 * m + aa) * W2 + (size_t)(2 * (2 * rp + 1))) * ldy;   // tile r + 1
                if (cok) {
                    oa[lane_yoff] = o0.x; oa[lane_yoff + ldy] = o1.x;
                    ob[lane_yoff] = o0.y; ob[lane_yoff + ldy] = o1.y;
                }
            }
        }
    }
}

template <int PH>
__device__ __forceinline__ void pc_dc_epilogue_edge(const PcAcc<false>& acc, const WinoPcArgs& a, const PcTile& tl, const PcLane& c, float* ybase,
                                                    bool cok, float bval) {
    const unsigned ldy = c.ldy, lane_yoff = c.lane_yoff;
    const size_t W2 = 2 * (size_t)a.W;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float tr[2][4];
#pragma unroll
            for (int xx = 0; xx < 4; ++xx) {
                const float m0 = pc_dc_live<PH>(0 + xx) ? acc[0 + xx][m][r] : 0.f, m1 = pc_dc_live<PH>(4 + xx) ? acc[4 + xx][m][r] : 0.f;
                const float m2 = pc_dc_live<PH>(8 + xx) ? acc[8 + xx][m][r] : 0.f, m3 = pc_dc_live<PH>(12 + xx) ? acc[12 + xx][m][r] : 0.f;
                tr[0][xx] = (m0 + m1) + m2;
                tr[1][xx] = (m1 - m2) - m3;
            }
#pragma unroll
            for (int aa = 0; aa < 2; ++aa) {
                float o0 = (tr[aa][0] + tr[aa][1]) + tr[aa][2];
                float o1 = (tr[aa][1] - tr[aa][2]) - tr[aa][3];
                o0 += bval; o1 += bval;
                if (a.out_lrelu) { o0 = fmaxf(o0, 0.01f * o0); o1 = fmaxf(o1, 0.01f * o1); }
                float* o = ybase + ((size_t)(4 * m + aa) * W2 + (size_t)(2 * r)) * ldy;   // uniform
                const int tile = 16 * m + 4 * c.kq + r;
                const int gy = tl.y0 + 2 * (tile >> 3) + aa, gx = tl.x0 + 2 * (tile & 7);   // phase (= input grid) coordinates
                if (gy < a.H && cok) {
                    if (gx < a.W) o[lane_yoff] = o0;
                    if (gx + 1 < a.W) o[lane_yoff + ldy] = o1;
                }
            }
        }
    }
}

// a whole tile of phase PH: its stages (each up to its barrier) and its epilogue.  nph: the next tile's phase.
template <int PH>
__device__ __forceinline__ void pc_dc_tile(const WinoPcArgs& a, const PcTile& tl, int nph, int NS, f32x4 (&An)[3][2], f32x4 (&Bn)[kPcDcPts],
                                           const float* Vb, int& buf, const f32x4* wt, const f32x4* wt_next, const PcLane& c) {
    PcAcc<false> acc;
    for (int s = 0; s < NS; ++s) {
        const float* Vc = Vb + buf * kPcV;
        const int nbuf = buf == kPcNBuf - 1 ? 0 : buf + 1;
        const float* Vn = Vb + nbuf * kPcV;
        const f32x4* wcur = wt + (size_t)s * (kPcDcPts * 256);
        const bool last = s + 1 == NS;
        const f32x4* wnx = last ? wt_next : wcur + kPcDcPts * 256;
        const int nx0 = pc_dc_first(last ? nph : PH);
        if (s == 0) pc_dc_stage<PH, true>(acc, An, Bn, Vc, Vn, nx0, wcur, wnx, c);
        else pc_dc_stage<PH, false>(acc, An, Bn, Vc, Vn, nx0, wcur, wnx, c);
        __syncthreads();
        buf = nbuf;
    }
    const int co = c.cwv * 16 + c.jj;     // every phase writes the slice's 64 columns
    float* ybase = a.y + (((size_t)tl.n * (2 * a.H) + 2 * tl.y0 + (PH >> 1)) * (2 * (size_t)a.W) + 2 * tl.x0 + (PH & 1)) * a.ldy + a.ycoff + c.cwv * 16;
    const bool cok = co < a.cout_valid;   // a padded output column is not stored
    const bool inside = tl.y0 + (kPcTH - 1) < a.H && tl.x0 + (kPcTW - 1) < a.W;
    const float bval = a.bias ? a.bias[co] : 0.f;
    if (inside) pc_dc_epilogue_interior<PH>(acc, a, c, ybase, cok, bval);
    else pc_dc_epilogue_edge<PH>(acc, a, tl, c, ybase, cok, bval);
}

// the consumer role of the deconv form: the barrier protocol of conv_wino_pc_kernel's consumers
__device__ __forceinline__ void pc_dc_consumer(const WinoPcArgs& a, const float* Vb, int NS, int first, int step, int count, int lane, int wv) {
    const PcLane c = pc_dc_lane(a, lane, wv);
    const f32x4* wbase = reinterpret_cast<const f32x4*>(a.wp) + wv * 64 + lane;
    const size_t wgroup = (size_t)NS * kPcDcPts * 256;                  // f32x4 per phase
    PcTile tl = pc_decode<1, 1>(first, a);
    const f32x4* wt = wbase + (size_t)tl.cg * wgroup;
    f32x4 Bn[kPcDcPts], An[3][2];
#pragma unroll
    for (int b = 0; b < kPcBD; ++b) Bn[b] = wt[b * 256];
    __syncthreads();
    __syncthreads();
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        An[i][0] = *reinterpret_cast<const f32x4*>(Vb + c.a0 + pc_dc_first(tl.cg) + i * kPcTiles * kCB);
        An[i][1] = *reinterpret_cast<const f32x4*>(Vb + c.a1 + pc_dc_first(tl.cg) + i * kPcTiles * kCB);
    }
    int buf = 0;
    for (int it = 0; it < count; ++it) {
        const int tnext = first + (it + 1 < count ? it + 1 : it) * step;
        const PcTile tn = pc_decode<1, 1>(tnext, a);
        const f32x4* wt_next = wbase + (size_t)tn.cg * wgroup;
        switch (__builtin_amdgcn_readfirstlane(tl.cg)) {   // uniform: the barriers inside are reached by whole waves
            case 0: pc_dc_tile<0>(a, tl, tn.cg, NS, An, Bn, Vb, buf, wt, wt_next, c); break;
            case 1: pc_dc_tile<1>(a, tl, tn.cg, NS, An, Bn, Vb, buf, wt, wt_next, c); break;
            case 2: pc_dc_tile<2>(a, tl, tn.cg, NS, An, Bn, Vb, buf, wt, wt_next, c); break;
            default: pc_dc_tile<3>(a, tl, tn.cg, NS, An, Bn, Vb, buf, wt, wt_next, c); break;
        }
        tl = tn;
        wt = wt_next;
    }
}

// ======================================================= producer steps =====================================================
// A producer lane's items.  Load / publish item u = 192 pw + lane + 64 u over the whole 10-row halo (every halo word has ONE
// loader) -> strip pixel pi = item >> 2 in (row, de-interleaved column) order, 16-byte word w4; row and column are recomputed
// where needed: a few integer operations instead of 15 live registers.  Transform item: (tile of the row, 16-byte word, half
// of the xi rows); 16 consecutive lanes = 4 tiles x 4 words: conflict-free strip reads (the four tiles' columns are consecutive
// strip pixels) and V writes.
struct PcItems {
    int id0, w4;               // item u = id0 + 64 u; the item's 16-byte word
    int wr_off[kPcNPF];        // strip offset an item is published at
    int rdR0, rdR1, rdR2;      // strip offsets of the transform's three rows, in the order it takes them
    float sg, m1;              // sign of the third row; an opaque -1
    int vslot;                 // float offset in a V buffer of the lane's first transform point xi = 8 thalf; point xi + k: + 512 k
    __device__ __forceinline__ int item_id(int u) const { return id0 + 64 * u; }
    __device__ __forceinline__ int row(int u) const { return (item_id(u) >> 2) / 18; }
    __device__ __forceinline__ int cp(int u) const { const int pi = item_id(u) >> 2; return pi - (pi / 18) * 18; }
    __device__ __forceinline__ int col(int u) const { const int c = cp(u); return c < 9 ? 2 * c : 2 * c - 17; }   // even columns first, then odd
};

__device__ __forceinline__ PcItems pc_items(int pw, int lane) {
    PcItems p;
    p.id0 = 192 * pw + lane;
    p.w4 = lane & 3;
    // the 48 items beyond the halo's 720 (768 = 3 x 256) go to pad pixels of the strip (columns 18, 19 of the 20-pixel row
    // pitch, written as zero) so that the publish loop has no per-lane branch
#pragma unroll
    for (int u = 0; u < kPcNPF; ++u) {
        const int item = p.item_id(u), e = (item - kPcShItems) >> 2;
        p.wr_off[u] = item < kPcShItems ? (p.row(u) * kPcRawW + p.cp(u)) * kCB + p.w4 * 4
                                        : ((e >> 1) * kPcRawW + 18 + (e & 1)) * kCB + p.w4 * 4;
    }
    const int tword = lane & 3, thalf = (lane >> 4) & 1, txl = ((lane >> 5) << 2) | ((lane >> 2) & 3);
    p.vslot = pc_slot(8 * thalf, pw * 8 + txl, tword);
    // Row transform without per-lane selects: the lane reads its three strip rows in a lane-dependent ORDER (R0, R1, R2) and
    // computes ya = R0 - R1, yb = R1 + sg * R2:
    //   half 0 (xi_y 0, 1): R = strip rows (0, 2, 1), sg = +1 ->  d0 - d2,  d2 + d1
    //   half 1 (xi_y 2, 3): R = strip rows (2, 1, 3), sg = -1 ->  d2 - d1,  d1 - d3
    // (strip columns of tile txl: cc = 0 at column pixel txl, cc = 1: +9 pixels, cc = 2: +1, cc = 3: +10)
    const int rdc = txl * kCB + tword * 4 + 2 * pw * kPcRawW * kCB;   // the tile row's halo rows start at strip row 2 pw
    p.rdR0 = (thalf ? 2 : 0) * kPcRawW * kCB + rdc; p.rdR1 = (thalf ? 1 : 2) * kPcRawW * kCB + rdc;
    p.rdR2 = (thalf ? 3 : 1) * kPcRawW * kCB + rdc;
    p.sg = thalf ? -1.f : 1.f;
    p.m1 = -1.f;                            // opaque to the optimiser: fma(a, -1, c) would otherwise be folded into four scalar
    asm volatile("" : "+v"(p.m1));          // v_sub_f32; as a register operand it stays one v_pk_fma_f32 per pair (same rounding)
    return p;
}

// Per-tile book of a lane's items: in-plane BYTE offset (a harmless in-tensor offset when outside), 1 inside the image / 0
// outside (zero padding), owner bits (materialise target).  Two books: the raw words run TWO stages ahead of their use, so the
// last two stages of a tile already load the next tile's words.
struct PcBook { unsigned off[kPcNPF]; float keep[kPcNPF]; unsigned own; };

template <int KD, int DIL>
__device__ __forceinline__ void pc_book(const WinoPcArgs& a, const PcItems& p, const PcTile& t, PcBook& b) {
    b.own = 0;
#pragma unroll
    for (int u = 0; u < kPcNPF; ++u) {
        const int hy = p.row(u), hx = p.col(u);
        const int gy = t.y0 + t.py + DIL * (hy - 1), gx = t.x0 + t.px + DIL * (hx - 1);
        const bool in = p.item_id(u) < kPcShItems && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        const unsigned n2 = KD == 3 ? 0u : (unsigned)t.n;
        b.off[u] = 4u * (in ? (unsigned)((((size_t)n2 * a.H + gy) * a.W + gx) * a.Cin + p.w4 * 4) : (unsigned)(p.w4 * 4));
        b.keep[u] = in ? 1.f : 0.f;
        const bool mine = hy >= 1 && hy <= kPcTH;   // the one loader of a pixel of the tile's own 8 x 16
        if (in && mine && hx >= 1 && hx <= kPcTW) b.own |= 1u << u;
    }
}

// One register set per stage parity: raw words (+ residual words) and the (scale, shift) of the stage's 4 channels.
// A set is refilled for stage s+2 right after stage s has published it, so a load has two stage periods to land:
// with a single set the chain load -> publish -> next load made the producers' period = memory latency + publish
// (measured 2.8 us against the consumers' 2.0 us of MFMAs), i.e. the matrix pipe waited for the producers.
template <bool RES> struct PcRegs { f32x4 pre[kPcNPF]; f32x4 prer[RES ? kPcNPF : 1]; f32x4 ss[2]; f32x4 rs[2]; };

// a producer wave's state across stages and tiles
struct PcProd {
    PcItems p;
    PcTile tl, tn;             // current tile; the next one once the refills reach into it
    PcBook cur, nxt;
    float* Vb; float* rawb; const float* ssl;
    unsigned plane;            // floats of one slice
    int qbuf, gi;              // V buffer the next transform writes; stages published so far (strip parity)
    bool has_next, interior;   // another tile follows; the current tile's whole halo lies inside the image
};

// raw words of stage s -> registers; nx: the stage belongs to the NEXT tile (book nxt, tile tn).  The book is selected per
// value, not per pointer: a pointer select would force both books into scratch memory.
template <int KD, bool RES, int EPI>
__device__ __forceinline__ void pc_issue(const WinoPcArgs& a, const PcProd& P, bool nx, int s, PcRegs<RES>& r) {
    const int cb = s / KD, kd = s - cb * KD, w4 = P.p.w4;
    r.ss[0] = r.ss[1] = r.rs[0] = r.rs[1] = f32x4{1.f, 1.f, 0.f, 0.f};
    if constexpr (EPI == 0) {
        r.ss[0] = *reinterpret_cast<const f32x4*>(P.ssl + 2 * (cb * kCB + w4 * 4));
        r.ss[1] = *reinterpret_cast<const f32x4*>(P.ssl + 2 * (cb * kCB + w4 * 4) + 4);
        if constexpr (RES) {
            r.rs[0] = *reinterpret_cast<const f32x4*>(P.ssl + 2 * a.Cin + 2 * (cb * kCB + w4 * 4));
            r.rs[1] = *reinterpret_cast<const f32x4*>(P.ssl + 2 * a.Cin + 2 * (cb * kCB + w4 * 4) + 4);
        }
    }
    const int tz = nx ? P.tn.n : P.tl.n;
    const int z = KD == 3 ? min(max(tz + kd - 1, 0), a.N - 1) : 0;   // clamped: an outside slice is zeroed when published
    // uniform 64-bit base + per-lane 32-bit byte offset: the global_load saddr form, no per-lane 64-bit address math
    const size_t base = ((size_t)z * P.plane + (size_t)(cb * kCB)) * sizeof(float);
    const __amdgpu_buffer_rsrc_t xb = pc_rsrc(reinterpret_cast<const char*>(a.x) + base);
    const __amdgpu_buffer_rsrc_t rb = pc_rsrc(reinterpret_cast<const char*>(RES ? a.res : a.x) + base);
#pragma unroll
    for (int u = 0; u < kPcNPF; ++u) {
        const unsigned o = nx ? P.nxt.off[u] : P.cur.off[u];
        r.pre[u] = pc_bload(xb, o);
        if constexpr (RES) r.prer[u] = pc_bload(rb, o);
    }
}

// (1) normalise / activate the prefetched words of set r and publish them to the strip `raw` (+ materialise).
// Straight-line, packed, no per-lane branches or selects: as a chain of exec-masked blocks this phase took 0.74 us alone and
// 2.0 us beside the consumers' MFMA stream — longer than the MFMAs it has to stay ahead of.  Breadth-first over the items — all
// FMAs, then all ReLUs, then all masks, then the stores — and pinned in that order: beside the consumer's MFMA stream a VALU
// instruction that has to wait for its predecessor's result loses the issue port to the next MFMA (32 cycles), an
// independent one issues back to back.  INTERIOR: every item of every lane inside the image: no padding mask (the strip's
// pad pixels are never read by the transform).
template <int KD, bool RES, int EPI, bool MAT, bool INTERIOR>
__device__ __forceinline__ void pc_activate_publish(const WinoPcArgs& a, const PcProd& P, const PcRegs<RES>& r, float* raw, int cb, int kd, int z) {
    // (scale, shift) pairs of channels (0,1) and (2,3); identity = (1, 0); the LDS table is stored pre-paired (pc_ss_slot)
    const f32x2 sc01 = r.ss[0].lo, sh01 = r.ss[0].hi, sc23 = r.ss[1].lo, sh23 = r.ss[1].hi;
    const f32x2 rc01 = r.rs[0].lo, rh01 = r.rs[0].hi, rc23 = r.rs[1].lo, rh23 = r.rs[1].hi;
    const bool wmat = MAT && (KD != 3 || kd == 1) && P.tl.cg == 0;
    constexpr int NU = kPcNPF;
    f32x2 lo[NU], hi[NU];
    if constexpr (EPI >= 1) {   // the R-Net forms have no prologue: no identity FMAs (x * 1 + 0 is not folded: -0)
#pragma unroll
        for (int i = 0; i < NU; ++i) { lo[i] = r.pre[i].lo; hi[i] = r.pre[i].hi; }
    } else {
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            lo[i] = __builtin_elementwise_fma(r.pre[i].lo, sc01, sh01);
            hi[i] = __builtin_elementwise_fma(r.pre[i].hi, sc23, sh23);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (EPI == 0 && a.x_relu) {
#pragma unroll
        for (int i = 0; i < NU; ++i) { lo[i].x = relu1(lo[i].x); lo[i].y = relu1(lo[i].y); hi[i].x = relu1(hi[i].x); hi[i].y = relu1(hi[i].y); }
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (RES) {
        f32x2 ql[NU], qh[NU];
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            ql[i] = __builtin_elementwise_fma(r.prer[i].lo, rc01, rh01);
            qh[i] = __builtin_elementwise_fma(r.prer[i].hi, rc23, rh23);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (a.res_relu) {
#pragma unroll
            for (int i = 0; i < NU; ++i) { ql[i].x = relu1(ql[i].x); ql[i].y = relu1(ql[i].y); qh[i].x = relu1(qh[i].x); qh[i].y = relu1(qh[i].y); }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NU; ++i) { lo[i] = lo[i] + ql[i]; hi[i] = hi[i] + qh[i]; }
        __builtin_amdgcn_sched_barrier(0);
    }
    // zero padding applies to the ACTIVATED tensor: out-of-image lanes (their loads read a harmless in-tensor word) are multiplied by 0
    if constexpr (!INTERIOR) {
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const f32x2 kk = {P.cur.keep[i], P.cur.keep[i]};
            lo[i] = lo[i] * kk; hi[i] = hi[i] * kk;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const f32x4 v = __builtin_shufflevector(lo[u], hi[u], 0, 1, 2, 3);
        // the activated input is written once: by the wave that owns the pixel, at the centre tap
        if (MAT && wmat) {
            if ((P.cur.own >> u) & 1u)
                *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(a.mat) + ((size_t)(KD == 3 ? z : 0) * P.plane + (size_t)(cb * kCB)) * sizeof(float) + P.cur.off[u]) = v;
        }
        *reinterpret_cast<f32x4*>(raw + P.p.wr_off[u]) = v;
    }
}

// (3) input transform B^T d B of this lane's (tile, word): rows (2 of the 4 xi_y), then columns; strip rawT -> V buffer Vq
__device__ __forceinline__ void pc_transform(const PcItems& p, const float* rawT, float* Vq) {
    const float m1 = p.m1;
    f32x4 ya[4], yb[4];
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        const int co = ((cc & 1) * 9 + (cc >> 1)) * kCB;
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

// one stage, up to its barrier: (1) publish set r (stage s of the current tile) into strip gi & 1, (2) refill the set for stage
// s+2 (of this tile, or stage s+2-NS of the next one), (3) transform the strip published one stage ago into V[qbuf]
template <int KD, bool RES, int EPI, bool MAT>
__device__ __forceinline__ void pc_stage(const WinoPcArgs& a, const PcProd& P, int NS, int s, PcRegs<RES>& r) {
    const int cb = s / KD, kd = s - cb * KD;
    const int z = KD == 3 ? P.tl.n + kd - 1 : P.tl.n;
    const bool zin = KD != 3 || (z >= 0 && z < a.N);
    float* raw = P.rawb + (P.gi & 1) * kPcShStrip;
    const float* rawT = P.rawb + ((P.gi & 1) ^ 1) * kPcShStrip;
    if (!zin) {   // a depth tap outside the volume: the whole slice is zero padding
#pragma unroll
        for (int u = 0; u < kPcNPF; ++u) *reinterpret_cast<f32x4*>(raw + P.p.wr_off[u]) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
        asm volatile("" : "+v"(r.ss[0]), "+v"(r.ss[1]));   // the pairs are re-paired HERE, not behind their loads
        if constexpr (RES) asm volatile("" : "+v"(r.rs[0]), "+v"(r.rs[1]));
        if (P.interior) pc_activate_publish<KD, RES, EPI, MAT, true>(a, P, r, raw, cb, kd, z);
        else pc_activate_publish<KD, RES, EPI, MAT, false>(a, P, r, raw, cb, kd, z);
    }
    // UNCONDITIONAL (the last two stages of the last tile re-read this tile's first two: harmless, never used)
    const bool nx = s + 2 >= NS;
    pc_issue<KD, RES, EPI>(a, P, nx && P.has_next, nx ? s + 2 - NS : s + 2, r);
    if (P.gi > 0) pc_transform(P.p, rawT, P.Vb + P.qbuf * kPcV);
}
// ... and behind its barrier: the transform lags the publish by one stage, so the first stage does not advance the V buffer
__device__ __forceinline__ void pc_stage_end(PcProd& P) {
    if (P.gi > 0) P.qbuf = P.qbuf == kPcNBuf - 1 ? 0 : P.qbuf + 1;
    ++P.gi;
}

}  // namespace

// ---- The barrier protocol.  G = tiles of this workgroup x NS stages, counted across tiles (P.gi); every wave executes G + 3
// barriers (+ 1 behind the (scale, shift) table load when EPI = 0).  A workgroup without tiles returns before the first one: the
// test is uniform and follows nothing but the tile-list split.
//   Producers, iteration g = 0 .. G-1: publish stage g into strip g & 1 from a register set loaded TWO stages earlier, refill
//   that set for stage g + 2, transform stage g - 1 into V[(g - 1) % 3], barrier.  The transform runs one iteration after the
//   publish because the barrier between them is what completes the shared strip (four waves write it, each reads all of it).
//   Closing: the transform of the last published stage G - 1 and its barrier, then two more: the consumers' last two stages.
//   Consumers: three opening barriers (stage 0 published | stage 0 transformed | stage 1 transformed), then per stage g its
//   MFMAs on V[g % 3] and one barrier.  Meanwhile the producers transform stage g + 2 into V[(g + 2) % 3] — they run two
//   stages ahead — and the consumers read the first operands of stage g + 1 from V[(g + 1) % 3], completed before the
//   previous barrier: three V buffers make both legal.
//   One barrier per stage; the consumers never wait for data, the producers wait for the consumers.
template <int KD, int DIL, bool RES, bool ODD = false, int EPI = 0, bool MAT = false, bool HALF = false>
__global__ __launch_bounds__(512) void conv_wino_pc_kernel(const WinoPcArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Vb = lds;                           // [3][16 xi][32 tiles][16]
    float* rawb = lds + kPcNBuf * kPcV;        // [2 strips][10 rows][20 pixels][16]
    float* ssl = rawb + kPcStrips;             // [Cin][2] (scale, shift) of x, then [Cin][2] of res (identity where null)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wv = wave & 3;                   // index within the role
    const int NS = (a.Cin / kCB) * KD;         // stages per tile

    int first, step, end;
    pc_tile_share(a.ntiles, first, step, end);
    if (first >= end) return;                  // uniform: no wave of this workgroup ever reaches a barrier
    const int count = (end - first + step - 1) / step;
    if constexpr (EPI == 0) {
        pc_load_ss_table<true>(ssl, a.Cin, a.x_ss, RES ? a.res_ss : nullptr, 1.f);
        __syncthreads();
    }

    // Producers are waves 0-3: VALU issue on a SIMD is arbitrated by age, and the producers' (few) VALU instructions have to
    // get through beside the consumer's continuous MFMA stream (measured: 3.58 -> 3.38 ms per layer from this alone)
    if constexpr (EPI == 2) {   // the deconv form has its own consumers (pc_dc_consumer); the producers below are the R-Net form's
        if (wave >= 4) { pc_dc_consumer(a, Vb, NS, first, step, count, lane, wv); return; }
    }
    if (wave >= 4) {
        // =========================================== consumer: 16 output channels x 16 xi x 32 tiles ====================
        const PcLane c = pc_lane<DIL, EPI, HALF>(a, lane, wv);
        PcAcc<HALF> acc;
        const f32x4* wbase = reinterpret_cast<const f32x4*>(a.wp) + c.cwv * 64 + lane;
        const size_t wgroup = (size_t)NS * 16 * 256;                        // f32x4 per 64-column output group
        PcTile tl = pc_decode<KD, DIL>(first, a);
        const f32x4* wt = wbase + (size_t)tl.cg * wgroup;
        f32x4 Bn[kPcNB], An[4][2];             // weight ring (7 lines ahead, continues across stages and tiles); A operands
        pc_prime_weights<HALF>(Bn, wt);
        __syncthreads();                       // the producers publish stage 0 (transformed one iteration later)
        __syncthreads();                       // producers finish stage 0
        __syncthreads();                       // ... and stage 1
        pc_prime_a<HALF>(An, Vb, c);
        int buf = 0;
        for (int it = 0; it < count; ++it) {
            const int tnext = first + (it + 1 < count ? it + 1 : it) * step;
            const PcTile tn = pc_decode<KD, DIL>(tnext, a);
            const f32x4* wt_next = wbase + (size_t)tn.cg * wgroup;
            for (int s = 0; s < NS; ++s) {
                const float* Vc = Vb + buf * kPcV;
                const int nbuf = buf == kPcNBuf - 1 ? 0 : buf + 1;
                const float* Vn = Vb + nbuf * kPcV;
                const f32x4* wcur = wt + (size_t)s * (16 * 256);
                const f32x4* wnx = s + 1 < NS ? wcur + 16 * 256 : wt_next;
                if (s == 0) pc_mfma_stage<HALF, true>(acc, An, Bn, Vc, Vn, wcur, wnx, c);
                else pc_mfma_stage<HALF, false>(acc, An, Bn, Vc, Vn, wcur, wnx, c);
                __syncthreads();
                buf = nbuf;
            }
            pc_epilogue<DIL, EPI, HALF>(acc, a, tl, c);
            tl = tn;
            wt = wt_next;
        }
    } else {
        // =========================================== producer: tile row wv (8 Winograd tiles) ===========================
        PcProd P;
        P.p = pc_items(wv, lane);
        P.Vb = Vb; P.rawb = rawb; P.ssl = ssl;
        P.plane = (unsigned)((size_t)a.H * a.W * a.Cin);
        P.tl = pc_decode<KD, DIL>(first, a); P.tn = P.tl;
        pc_book<KD, DIL>(a, P.p, P.tl, P.cur);
        PcRegs<RES> set0, set1;
        pc_issue<KD, RES, EPI>(a, P, false, 0, set0);
        pc_issue<KD, RES, EPI>(a, P, false, 1, set1);   // NS >= 2 (checked by the launcher)
        P.qbuf = 0; P.gi = 0;
        for (int it = 0; it < count; ++it) {
            P.has_next = it + 1 < count;
            P.interior = P.tl.y0 + P.tl.py - DIL >= 0 && P.tl.y0 + P.tl.py + DIL * kPcTH < a.H && P.tl.x0 + P.tl.px - DIL >= 0 && P.tl.x0 + P.tl.px + DIL * kPcTW < a.W;
            if constexpr (!ODD) {   // stages in pairs: the register set of a stage is static
                for (int s = 0; s < NS; s += 2) {
                    // the book of the next tile is needed from the first refill that reaches into it (stage NS-2 refills stage 0)
                    if (s + 2 == NS && P.has_next) { P.tn = pc_decode<KD, DIL>(first + (it + 1) * step, a); pc_book<KD, DIL>(a, P.p, P.tn, P.nxt); }
                    pc_stage<KD, RES, EPI, MAT>(a, P, NS, s, set0);
                    __syncthreads();
                    pc_stage_end(P);
                    pc_stage<KD, RES, EPI, MAT>(a, P, NS, s + 1, set1);
                    __syncthreads();
                    pc_stage_end(P);
                }
            } else {                // odd stage count (16 input channels x 3 depth taps): set = parity of the running stage count
                for (int s = 0; s < NS; ++s) {
                    if (s + 2 == NS && P.has_next) { P.tn = pc_decode<KD, DIL>(first + (it + 1) * step, a); pc_book<KD, DIL>(a, P.p, P.tn, P.nxt); }
                    if (((unsigned)it * (unsigned)NS + (unsigned)s) & 1u) { pc_stage<KD, RES, EPI, MAT>(a, P, NS, s, set1); __syncthreads(); }
                    else { pc_stage<KD, RES, EPI, MAT>(a, P, NS, s, set0); __syncthreads(); }
                    pc_stage_end(P);
                }
            }
            P.tl = P.tn;
            P.cur = P.nxt;
        }
        pc_transform(P.p, rawb + ((P.gi & 1) ^ 1) * kPcShStrip, Vb + P.qbuf * kPcV);   // the last published stage
        __syncthreads();
        __syncthreads();                       // the consumers' last two stages
        __syncthreads();
    }
}

// Column-major partials [2C][rows] -> BatchNorm (scale, shift) [C][2] + running statistics: workgroup c reads channel c's two
// runs of `rows` floats coalesced (the row-major finaliser walks a 4-byte column of a [rows][2C] matrix: 64 us per K-Net layer
// at 24,576 rows; this one 6 us), fixed-order fp64 tree.
__global__ __launch_bounds__(1024) void bn_finalize_cm_kernel(const float* __restrict__ stats, int rows, int C, double count,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              float eps, float momentum, float* __restrict__ running_mean,
                                                              float* __restrict__ running_var, float* __restrict__ ss, unsigned int* __restrict__ collapse_count, long long* __restrict__ batches_tracked) {
    __shared__ double sh[2][1024];
    const int c = blockIdx.x, tid = threadIdx.x;
    const float* p1 = stats + (size_t)c * rows;
    const float* p2 = stats + (size_t)(C + c) * rows;
    // a thread's share is a few dozen strided floats (K-Net at config B: rows = 12,288 -> 12 per run): all of them are requested
    // before the first is added (round 6: the one-at-a-time loop cost a DRAM latency per element, 15.4 us per K-Net layer at
    // config B); the order of the fp64 additions per thread is unchanged (g ascending), so are the bits
    double s1 = 0.0, s2 = 0.0;
    int g = tid;
    for (; g + 7 * 1024 < rows; g += 8 * 1024) {
        float u[8], v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { u[k] = p1[g + k * 1024]; v[k] = p2[g + k * 1024]; }
#pragma unroll
        for (int k = 0; k < 8; ++k) { s1 += (double)u[k]; s2 += (double)v[k]; }
    }
    for (; g < rows; g += 1024) { s1 += (double)p1[g]; s2 += (double)p2[g]; }
    sh[0][tid] = s1; sh[1][tid] = s2;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) { sh[0][tid] += sh[0][tid + o]; sh[1][tid] += sh[1][tid + o]; }
        __syncthreads();
    }
    if (tid == 0) bn_finalize_channel(sh[0][0], sh[1][0], count, gamma[c], beta[c], eps, momentum, running_mean, running_var, ss, c, collapse_count);
    if (tid == 0 && c == 0 && batches_tracked) *batches_tracked += 1;      // nn.BatchNorm's num_batches_tracked side effect (one launch less per layer)
}

// w [Cout][Cin][KD][3][3] -> U = G g G^T (float64, rounded once) in the kernel's B-operand order
// [cg][stage = cb*KD + kd][xi][wave][lane = kq*16 + j][e], co = cg*64 + 16*wave + j, ci = cb*16 + 4*kq + e
// transposed == 2 (grid.y = 2): BOTH streams of a layer [Cout][Cin] in one launch — y = 0 the forward one at wp, y = 1 the data-gradient
// one (roles of Cin / Cout swapped, taps flipped) right behind it (training packs both every iteration: the weights just changed)
__global__ __launch_bounds__(256) void conv_wino_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout, int KD,
                                                             int transposed) {
    const long total = (long)Cout * Cin * KD * 16;
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
    const int kd = (int)(t % KD); t /= KD;
    const int ncb = Cin / kCB;
    const int cb = (int)(t % ncb);
    const int cg = (int)(t / ncb);
    const int co = cg * 64 + 16 * wave + j, ci = cb * kCB + 4 * kq + e;
    // transposed: the stored tensor is [Cin][Cout][KD][3][3] (this kernel's ci is ITS output channel), taps flipped in every dimension
    const float* g = transposed ? w + (((size_t)ci * Cout + co) * KD + (KD - 1 - kd)) * 9 : w + (((size_t)co * Cin + ci) * KD + kd) * 9;
    const double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
    const int a = xi >> 2, b = xi & 3;
    double u = 0.0;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) u += G[a][ky] * (double)g[transposed ? (2 - ky) * 3 + (2 - kx) : ky * 3 + kx] * G[b][kx];
    wp[idx] = (float)u;
}

// The deconv form's stream: the lines of the 9 live points of every (phase, stage) of the unmasked 256-column stream, copied
// [4 phases][stage][9][4 waves][64 lanes][4] (the dropped lines are the transforms of zero kernel rows / columns: exact zeros)
__global__ __launch_bounds__(256) void conv_wino_deconv_pack_kernel(const f32x4* __restrict__ wp, f32x4* __restrict__ wm, int NS) {
    const long total = 4L * NS * kPcDcPts * 256;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int in = (int)(idx & 255);
    long t = idx >> 8;
    const int p = (int)(t % kPcDcPts); t /= kPcDcPts;
    const int s = (int)(t % NS);
    const int ph = (int)(t / NS);
    const int xi = 4 * (p / 3 + (ph >> 1)) + p % 3 + (ph & 1);
    wm[idx] = wp[(((long)ph * NS + s) * 16 + xi) * 256 + in];
}

// ---- host side of conv_wino_pc_kernel, shared by nrgbd_conv_wino_f32 and nrgbd_conv_wino_rnet_ex_f32 ----
// persistent workgroups: one per CU, or one per tile where the list is shorter
static int pc_workgroups(long ntiles, int* nwg) {
    int dev = 0, ncu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return (int)e;
    if (ncu <= 0) return NRGBD_E_ARG;
    *nwg = ntiles < ncu ? (int)ntiles : ncu;
    return NRGBD_OK;
}

struct PcLaunch { int nwg; size_t lds; int lds_attr; hipStream_t stream; };   // lds: this call's dynamic LDS; lds_attr: the function's opt-in

// one instantiation: > 64 KB of dynamic LDS needs the opt-in, once per function and device (common.hpp set_max_dynamic_lds)
template <int KD, int DIL, bool RES, bool ODD = false, int EPI = 0, bool MAT = false, bool HALF = false>
static hipError_t pc_launch(const PcLaunch& L, const WinoPcArgs& a) {
    const hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(&conv_wino_pc_kernel<KD, DIL, RES, ODD, EPI, MAT, HALF>), L.lds_attr);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((conv_wino_pc_kernel<KD, DIL, RES, ODD, EPI, MAT, HALF>), dim3(L.nwg), dim3(512), L.lds, L.stream, a);
    return hipSuccess;
}

// the four (residual, materialise) forms of one <KD, DIL, HALF> (even stage count, EPI = 0)
template <int KD, int DIL, bool HALF>
static hipError_t pc_launch_forms(const void* res, const void* mat, const PcLaunch& L, const WinoPcArgs& a) {
    if (res && mat) return pc_launch<KD, DIL, true, false, 0, true, HALF>(L, a);
    if (res) return pc_launch<KD, DIL, true, false, 0, false, HALF>(L, a);
    if (mat) return pc_launch<KD, DIL, false, false, 0, true, HALF>(L, a);
    return pc_launch<KD, DIL, false, false, 0, false, HALF>(L, a);
}

}  // namespace nrgbd

extern "C" int nrgbd_conv_wino_pack(const float* w, float* w_wino, int Cin, int Cout, int kd, int transposed, void* stream) {
    using namespace nrgbd;
    if (!w || !w_wino) return NRGBD_E_NULL;
    if (Cin <= 0 || Cin % kCB || Cout <= 0 || Cout % 64 || (kd != 1 && kd != 3)) return NRGBD_E_SHAPE;
    if (transposed < 0 || transposed > 2) return NRGBD_E_ARG;
    if (transposed == 2 && Cin % 64) return NRGBD_E_SHAPE;           // both streams: each channel count is a Cout once
    const long total = (long)Cout * Cin * kd * 16;
    hipLaunchKernelGGL(conv_wino_pack_kernel, dim3((unsigned)((total + 255) / 256), transposed == 2 ? 2 : 1), dim3(256), 0, (hipStream_t)stream,
                       w, w_wino, Cin, Cout, kd, transposed);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

extern "C" int nrgbd_bn_finalize_cm(const float* stats, int rows, int C, long count, const float* gamma, const float* beta,
                                    float eps, float momentum, float* running_mean, float* running_var, float* scale_shift, unsigned int* collapse_count, long long* batches_tracked,
                                    void* stream) {
    using namespace nrgbd;
    if (!stats || !gamma || !beta || !scale_shift) return NRGBD_E_NULL;
    if (rows <= 0 || count <= 0 || C <= 0) return NRGBD_E_SHAPE;
    if ((running_mean == nullptr) != (running_var == nullptr)) return NRGBD_E_NULL;
    hipLaunchKernelGGL(bn_finalize_cm_kernel, dim3(C), dim3(1024), 0, (hipStream_t)stream, stats, rows, C, (double)count, gamma,
                       beta, eps, momentum, running_mean, running_var, scale_shift, collapse_count, batches_tracked);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

extern "C" int nrgbd_conv_wino_tiles(int N, int H, int W, int dilation) {
    using namespace nrgbd;
    if (N <= 0 || H <= 0 || W <= 0 || (dilation != 1 && dilation != 2)) return NRGBD_E_SHAPE;
    return N * ceil_div(H, kPcTH * dilation) * ceil_div(W, kPcTW * dilation) * dilation * dilation;
}

extern "C" int nrgbd_conv_wino_f32(const float* x, const float* x_ss, int x_relu, const float* res, const float* res_ss,
                                   int res_relu, float* materialized, const float* w_wino, float* y, float* stats, int N,
                                   int H, int W, int Cin, int Cout, int kd, int dilation, void* stream) {
    using namespace nrgbd;
    if (!x || !w_wino || !y) return NRGBD_E_NULL;
    const bool half = Cout == 32;               // the HALF form: 2-D, dilation 1 only
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cin % kCB || Cin > 2048 || Cout <= 0 || (Cout % 64 && !half)) return NRGBD_E_SHAPE;
    if ((kd != 1 && kd != 3) || (dilation != 1 && dilation != 2) || (kd == 3 && dilation != 1)) return NRGBD_E_ARG;
    if (half && (kd != 1 || dilation != 1)) return NRGBD_E_SHAPE;
    if ((Cin / kCB) * kd < 2) return NRGBD_E_SHAPE;      // two stages are always in flight (two register sets)
    // 32-bit BYTE offsets in the loader: inside one slice when kd = 3 (the slice is a 64-bit base), inside the tensor otherwise
    if ((long)(kd == 3 ? 1 : N) * H * W * Cin >= (1L << 30)) return NRGBD_E_SHAPE;
    const int rows = nrgbd_conv_wino_tiles(N, H, W, dilation);
    const long nt = (long)rows * (half ? 1 : Cout / 64);
    if (nt >= (1L << 30)) return NRGBD_E_SHAPE;
    WinoPcArgs a{x, x_ss, res, res_ss, materialized, w_wino, y, stats, x_relu, res_relu, N, H, W, Cin, Cout, (int)nt, half ? 2 * rows : rows,
                 nullptr, 0, 0, 0, 0};
    int nwg = 0;
    const int rc = pc_workgroups(nt, &nwg);
    if (rc != NRGBD_OK) return rc;
    const size_t lds = (size_t)(kPcNBuf * kPcV + kPcStrips + 4 * Cin) * sizeof(float);   // 96 KB V + 25.6 KB strips (2 x 12.8) + (scale, shift) tables
    // The opt-in for > 64 KB of dynamic LDS is a property of the FUNCTION, and a launch recorded in a hipGraph is replayed under whatever
    // value the function carries at that moment: it is therefore always set to the form's maximum (Cin = 2048), never to this call's size —
    // a later eager call with fewer channels would otherwise shrink it under a captured launch with more (round 6: a training graph
    // replayed after an eager iteration ran with part of its (scale, shift) tables cut off)
    const int lds_attr = (int)((size_t)(kPcNBuf * kPcV + kPcStrips + 4 * 2048) * sizeof(float));
    const bool odd = (((Cin / kCB) * kd) & 1) != 0;
    if (odd && (kd != 3 || res || materialized)) return NRGBD_E_SHAPE;   // an odd stage count is instantiated for the K-Net's first layer only
    const PcLaunch L{nwg, lds, lds_attr, (hipStream_t)stream};
    hipError_t e;
    if (half) e = pc_launch_forms<1, 1, true>(res, materialized, L, a);
    else if (kd == 3 && odd) e = pc_launch<3, 1, false, true>(L, a);
    else if (kd == 3) e = pc_launch_forms<3, 1, false>(res, materialized, L, a);
    else if (dilation == 1) e = pc_launch_forms<1, 1, false>(res, materialized, L, a);
    else e = pc_launch_forms<1, 2, false>(res, materialized, L, a);
    if (e != hipSuccess) return (int)e;
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

// R-Net form (models/m_submodule.py:18-27 conv2d_leakyRelu at widths with Cin % 16 == 0 (>= 32), Cout % 64 == 0: Refine.py:51-56 conv0,
// conv0_1): 3x3 convolution + bias + LeakyReLU(0.01) in the Winograd domain, no prologue, no statistics
extern "C" int nrgbd_conv_wino_rnet_ex_f32(const float* x, const float* w_wino, const float* bias, int out_lrelu, float* y, int N,
                                           int H, int W, int Cin, int Cout, int ldy, int ycoff, int cout_valid, void* stream) {
    using namespace nrgbd;
    if (!x || !w_wino || !y) return NRGBD_E_NULL;
    const bool half = Cout == 32;               // the HALF form: a 32-column slice (e.g. the 3 columns a 67-wide layer has beyond 64)
    if (N <= 0 || H <= 0 || W <= 0 || Cin < 32 || Cin % kCB || Cout <= 0 || (Cout % 64 && !half)) return NRGBD_E_SHAPE;   // >= 2 stages
    if ((long)N * H * W * Cin >= (1L << 30)) return NRGBD_E_SHAPE;
    if (cout_valid < 0 || cout_valid > Cout || ycoff < 0 || (ldy != 0 && ldy < ycoff + (cout_valid ? cout_valid : Cout))) return NRGBD_E_ARG;
    if ((long)N * H * W * (ldy ? ldy : Cout) >= (1L << 32)) return NRGBD_E_SHAPE;   // 32-bit lane offsets into a tile's rows only, but keep it sane
    const int rows = nrgbd_conv_wino_tiles(N, H, W, 1);
    const long nt = (long)rows * (half ? 1 : Cout / 64);
    if (nt >= (1L << 30)) return NRGBD_E_SHAPE;
    WinoPcArgs a{x, nullptr, nullptr, nullptr, nullptr, w_wino, y, nullptr, 0, 0, N, H, W, Cin, Cout, (int)nt, half ? 2 * rows : rows,
                 bias, out_lrelu, ldy, ycoff, cout_valid};
    int nwg = 0;
    const int rc = pc_workgroups(nt, &nwg);
    if (rc != NRGBD_OK) return rc;
    const size_t lds = (size_t)(kPcNBuf * kPcV + kPcStrips) * sizeof(float);   // no (scale, shift) tables: the size does not depend on the call
    const PcLaunch L{nwg, lds, (int)lds, (hipStream_t)stream};
    // an odd stage count (the R-Net's 67 -> 80 and 131 -> 144 channel pixels): the register set of a stage = parity of the running count
    const bool odd = ((Cin / kCB) & 1) != 0;
    hipError_t e;
    if (odd && half) e = pc_launch<1, 1, false, true, 1, false, true>(L, a);
    else if (odd) e = pc_launch<1, 1, false, true, 1, false, false>(L, a);
    else if (half) e = pc_launch<1, 1, false, false, 1, false, true>(L, a);
    else e = pc_launch<1, 1, false, false, 1, false, false>(L, a);
    if (e != hipSuccess) return (int)e;
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

// Deconv form: ConvTranspose2d(k4, s2, p1) + bias + LeakyReLU of one 64-column output slice, all four sub-pixel phases in one launch
extern "C" int nrgbd_conv_wino_rnet_deconv_pack(const float* w_wino, float* w_masked, int Cin, void* stream) {
    using namespace nrgbd;
    if (!w_wino || !w_masked) return NRGBD_E_NULL;
    if (Cin <= 0 || Cin % kCB) return NRGBD_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(w_wino) | reinterpret_cast<uintptr_t>(w_masked)) & 15) return NRGBD_E_ALIGN;
    const int NS = Cin / kCB;
    const long total = 4L * NS * kPcDcPts * 256;
    hipLaunchKernelGGL(conv_wino_deconv_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const f32x4*>(w_wino), reinterpret_cast<f32x4*>(w_masked), NS);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

extern "C" int nrgbd_conv_wino_rnet_deconv_f32(const float* x, const float* w_masked, const float* bias, int out_lrelu, float* y, int N,
                                               int H, int W, int Cin, int Cout, int ldy, int ycoff, int cout_valid, void* stream) {
    using namespace nrgbd;
    if (!x || !w_masked || !y) return NRGBD_E_NULL;
    if (N <= 0 || H <= 0 || W <= 0 || Cin < 32 || Cin % kCB || ((Cin / kCB) & 1) || Cout != 64) return NRGBD_E_SHAPE;   // an even stage count >= 2
    if ((long)N * H * W * Cin >= (1L << 30)) return NRGBD_E_SHAPE;
    if (ldy == 0) ldy = Cout;
    if (cout_valid == 0) cout_valid = Cout;
    if (cout_valid < 0 || cout_valid > Cout || ycoff < 0 || ldy < ycoff + cout_valid) return NRGBD_E_ARG;
    if (4L * N * H * W * ldy >= (1L << 31)) return NRGBD_E_SHAPE;        // 32-bit lane offsets inside a tile's rows of y [N][2H][2W][ldy]
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w_masked)) & 15) return NRGBD_E_ALIGN;   // 16-byte loads
    if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(bias)) & 3) return NRGBD_E_ALIGN;
    const int rows = nrgbd_conv_wino_tiles(N, H, W, 1);
    const long nt = (long)rows * 4;                                     // a tile per sub-pixel phase: the kernel's four column groups
    if (nt >= (1L << 30)) return NRGBD_E_SHAPE;
    WinoPcArgs a{x, nullptr, nullptr, nullptr, nullptr, w_masked, y, nullptr, 0, 0, N, H, W, Cin, 4 * Cout, (int)nt, rows,
                 bias, out_lrelu, ldy, ycoff, cout_valid};
    int nwg = 0;
    const int rc = pc_workgroups(nt, &nwg);
    if (rc != NRGBD_OK) return rc;
    const size_t lds = (size_t)(kPcNBuf * kPcV + kPcStrips) * sizeof(float);
    const PcLaunch L{nwg, lds, (int)lds, (hipStream_t)stream};
    const hipError_t e = pc_launch<1, 1, false, false, 2, false, false>(L, a);
    if (e != hipSuccess) return (int)e;
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

extern "C" int nrgbd_conv_wino_rnet_f32(const float* x, const float* w_wino, const float* bias, int out_lrelu, float* y, int N,
                                        int H, int W, int Cin, int Cout, void* stream) {
    return nrgbd_conv_wino_rnet_ex_f32(x, w_wino, bias, out_lrelu, y, N, H, W, Cin, Cout, 0, 0, 0, stream);
}
