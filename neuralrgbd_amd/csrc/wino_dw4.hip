// wino_dw4.hip — the K-Net's 64 -> 64 3x3x3 convolutions (models/basic.py:71-94) with F(4, 3) ALONG THE DEPTH AXIS on top of the
// in-plane F(2x2, 3x3): 6 transform points per FOUR output slices = 6 multiplies per output voxel (wino_dw.hip's F(2, 3): 8; direct: 27).
//
// Why (profiles/r6_wino_d4_probe.txt).  wino_dw.hip runs at 0.67 of the fp32 matrix peak with the matrix pipe and the
// producers' issue slots as co-limits; the lever left is fewer multiplies.  F(4x4, 3x3) in the plane was rejected on numerics in round 5
// (3.9x further from float64 than the direct convolution).  F(4, 3) along depth ONLY applies the ill-conditioned transform once, and with
// the interpolation points (0, +-1/2, +-3/2, inf) the whole K-Net sits 1.24x as far from float64 as the direct convolution (today's form:
// 0.92x; acceptance 1.25x; oracle/wino_d4_eval.py).
//
//   input    d_j = act(x[z0 - 1 + j]),  j = 0..5                       (z0 = first of the four output slices of a tile)
//   depth    D_t = sum_j Bd[t][j] d_j,  Bd = [ 9/16 0 -5/2 0 1 0 | 0 -9/8 -9/4 1/2 1 0 | 0 9/8 -9/4 -1/2 1 0 | 0 -3/8 -1/4 3/2 1 0 |
//                                               0 3/8 -1/4 -3/2 1 0 | 0 9/16 0 -5/2 0 1 ]            (3 or 4 slices per D_t)
//   plane    V_t = B^T D_t B per 4x4 patch                                                    (as wino_pc.hip / wino_dw.hip)
//   weights  U_t = sum_kd Gd[t][kd] (G g_kd G^T),  Gd = [16/9 0 0 | -1 -1/2 -1/4 | -1 1/2 -1/4 | 1/9 1/6 1/4 | 1/9 -1/6 1/4 | 0 0 1]
//   product  M_t = sum_ci V_t U_t                                                             (the MFMAs: 6 x Cin/16 stages per tile)
//   output   y[z0]   = M0 + (M1 + M2) + (M3 + M4)          y[z0+1] = 1/2 (M1 - M2) + 3/2 (M3 - M4)
//            y[z0+2] = 1/4 (M1 + M2) + 9/4 (M3 + M4)       y[z0+3] = 1/8 (M1 - M2) + 27/8 (M3 - M4) + M5
//
// Same persistent producer / consumer organisation, tile geometry, LDS images, shared strips and early stage barrier as wino_dw.hip (read
// its header first).  What differs:
//   * a tile is 8x16 pixels x FOUR depth slices; phases run in the order t = 1, 2, 3, 4, 0, 5 so that the fold needs few live values:
//       after M1: A = M1 | after M2: A = S12 = M1 + M2, B = D12 = M1 - M2 | after M3: C = M3 | after M4: S34 = C + M4, D34 = C - M4,
//       slices z0+1 and z0+2 are COMPLETE and stored, A = S12 + S34, B = D12 / 8 + 27/8 D34 | after M0: slice z0 = A + M0 |
//       after M5: slice z0+3 = B + M5.
//     A and B are the two 32 KB LDS stashes wino_dw.hip has; C — live for one phase only — does not fit the LDS (it would be the third of
//     three: 185 KB) and goes through a per-workgroup 32 KB scratch in global memory that the wave itself wrote (8 stores + 8 loads of 1 KB
//     per tile: 0.5 % of the tile's issue slots; the 8 MB of all workgroups stay in the L2s).
//   * producers: a stage combines 3 or 4 slices with rational coefficients.  The unit of prefetch stays one (slice, channel block) in one of
//     four register sets (the fourth empty for t = 0 and t = 5), all requested one stage ahead; the stage's combination sum_k c_k act(x_k)
//     is formed in registers and the strip written once (wino_dw.hip publishes unit A and read-modify-writes the strip for unit B).
//   * PAIRED PHASES (Cin <= 64, i.e. every K-Net layer).  For t = 1..4 the four units are the same slices j = 4, 1, 2, 3; only the
//     coefficients differ.  A stage of t = 1 (t = 3) therefore runs a second FMA chain with the coefficients of t = 2 (t = 4) on the
//     units it has just activated — same slot order, same first-slot rule, same outside-slice test: the bits are those of the stage
//     that loaded them afresh — and keeps its three words per lane in registers (one set per channel block, up to four in flight:
//     48 VGPRs).  The stage of t = 2 (t = 4) loads and activates nothing: kept words, plane mask, strip.  Unit loads per tile and
//     channel block: 4+0+4+0+3+3 = 14 instead of 22.  Prefetch: the last stage of a loading phase requests nothing, and the stages
//     of the restoring phase request the sets of the next loading stage spread over themselves (d4_restore).
//     Measured on one MI355X, 64 -> 64 at 64x192x256, parent and this file alternated (profiles/dw4_pair_reuse.txt): the producers'
//     vector-memory reads fall by exactly 8/22 (16.17 M -> 13.81 M instructions per launch with the consumers'), beyond-L2 fetch by
//     11-12 %; the pairing alone 1.781 -> 1.736 ms IDENT, 1.752 -> 1.731 ms CLAMP; with the two select-to-branch changes below
//     (d4_mask, the first slot) 1.721 ms and 1.713 ms: -3.4 % and -2.2 %.
//   * only the two forms the K-Net uses behind its materialise passes: IDENT (x as it is) and CLAMP (relu(x * s + t) as a clamped FMA).
// Work per four output slices: 24 stages (wino_dw: 32), 16 of them loading; producer units 56 (wino_dw: 64), MFMAs 0.75x.
//
// In wino_dw.hpp, shared with wino_dw.hip: the constants, DwTile + dw_decode<4>, the serpentine order dw_cb, the barrier protocol, the
// consumers' steps (dw_lane, dw_prime, dw_phase / dw_mfma_stage, dw_plane_inverse, dw_emit, dw_store_stats), the producers' (dw_items,
// dw_book, dw_activate, dw_transform, DwProd), the weight packer (dw_pack<6>) and the host helpers.  Here: the F(4, 3) depth transform
// — the coefficient tables d4_*, d4_issue, d4_combine, d4_restore, d4_stage, d4_fold — the kernel and its launcher.
#include "wino_dw.hpp"

namespace nrgbd {

constexpr int kD4ScratchWave = 8 * 64 * 4;                 // floats of one consumer wave's global scratch (stash C)

// depth-transform index of phase p (execution order) and the unit slots of index t: (input slice j = 0..5 relative to z0 - 1, coefficient)
__device__ __forceinline__ int d4_t(int p) { return p < 4 ? p + 1 : (p == 4 ? 0 : 5); }
__device__ __forceinline__ int d4_nslot(int t) { return (t == 0 || t == 5) ? 3 : 4; }
__device__ __forceinline__ int d4_j(int t, int k) {
    if (t == 0) return k == 0 ? 4 : (k == 1 ? 0 : 2);
    if (t == 5) return k == 0 ? 5 : (k == 1 ? 1 : 3);
    return k == 0 ? 4 : k;                         // t = 1..4: slices 4 (coefficient 1), 1, 2, 3
}
__device__ __forceinline__ float d4_c(int t, int k) {
    if (k == 0) return 1.f;
    if (t == 0 || t == 5) return k == 1 ? 0.5625f : -2.5f;
    const float s = (t & 1) ? -1.f : 1.f;          // t = 1, 3: the odd part enters with a minus sign
    if (t <= 2) return k == 1 ? s * 1.125f : (k == 2 ? -2.25f : -s * 0.5f);
    return k == 1 ? s * 0.375f : (k == 2 ? -0.25f : -s * 1.5f);
}

struct WinoD4Args {
    WinoPcArgs b;       // x, x_ss, wp, y, stats, N, H, W, Cin, Cout, ntiles, rows, x_unit (res / mat / bias unused)
    float* scratch;     // [workgroups][4 consumer waves][8][64][4] floats: stash C
};

// ======================================================= consumer: the fold =================================================
// A consumer wave's three stashes: A and B in LDS (this lane's word i at A[i * 64]); C: the wave's 8 KB of the global scratch
// through a buffer descriptor (uniform base in SGPRs + the lane's 32-bit byte offset: no 64-bit per-lane pointer kept alive across
// the tile loop — the register file has none to spare)
struct D4Stash { f32x4* A; f32x4* B; __amdgpu_buffer_rsrc_t C; int laneC; };

// End of the phase at position P (depth-transform index t = 1, 2, 3, 4, 0, 5): plane inverse transform of M_t (A^T . A: 32 values
// per lane) and the depth fold of the file header; P = 3 completes slices z0 + 1 and z0 + 2, P = 4 slice z0, P = 5 slice z0 + 3.
template <int P>
__device__ __forceinline__ void d4_fold(const DwAcc& acc, const WinoPcArgs& a, const DwLane& c, const DwTile& tl, int wv, const D4Stash& st, f32x2 n1) {
    constexpr int NEMIT = P == 3 ? 2 : (P >= 4 ? 1 : 0);           // slices completed by this phase
    constexpr int ZS0 = P == 3 ? 1 : (P == 4 ? 0 : 3);              // the (first) one
    f32x2 S1[NEMIT ? NEMIT : 1] = {}, S2[NEMIT ? NEMIT : 1] = {};
    float* ybase = a.y + (((size_t)tl.z0 * a.H + tl.y0) * a.W + tl.x0) * a.Cout + tl.cg * 64 + wv * 16;
    const size_t zstride = (size_t)a.H * a.W * a.Cout;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int rp = 0; rp < 2; ++rp) {
            f32x2 tr[2][4];
            dw_plane_inverse(acc, m, rp, n1, tr);
#pragma unroll
            for (int aa = 0; aa < 2; ++aa) {
                const int wi = (m * 2 + rp) * 2 + aa;
                const f32x4 o = dw_plane_word(tr, aa, n1);
                if constexpr (P == 0) {                    // M1
                    st.A[wi * 64] = o;
                } else if constexpr (P == 1) {             // M2: S12, D12
                    const f32x4 m1v = st.A[wi * 64];
                    st.A[wi * 64] = m1v + o;
                    st.B[wi * 64] = m1v - o;
                } else if constexpr (P == 2) {             // M3 -> the global scratch (read back one phase later by this lane)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4_t, o), st.C, st.laneC, wi * 1024, 0);
                } else if constexpr (P == 3) {             // M4: S34, D34; slices z0+1, z0+2 complete
                    const f32x4 m3v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(st.C, st.laneC, wi * 1024, 0));
                    {
                        const f32x4 d34 = m3v - o, d12 = st.B[wi * 64];
                        st.B[wi * 64] = 0.125f * d12 + 3.375f * d34;                                            // + M5 -> y[z0+3]
                        dw_emit(a, c, ybase + 1 * zstride, m, rp, aa, 0.5f * d12 + 1.5f * d34, S1[0], S2[0]);   // y[z0+1]
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    {
                        const f32x4 s34 = m3v + o, s12 = st.A[wi * 64];
                        st.A[wi * 64] = s12 + s34;                                                              // + M0 -> y[z0]
                        dw_emit(a, c, ybase + 2 * zstride, m, rp, aa, 0.25f * s12 + 2.25f * s34, S1[1], S2[1]); // y[z0+2]
                    }
                    __builtin_amdgcn_sched_barrier(0);
                } else if constexpr (P == 4) {             // M0
                    dw_emit(a, c, ybase, m, rp, aa, st.A[wi * 64] + o, S1[0], S2[0]);
                } else {                                   // M5
                    dw_emit(a, c, ybase + 3 * zstride, m, rp, aa, st.B[wi * 64] + o, S1[0], S2[0]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);      // one (m, rp) group at a time (register pressure, wino_dw.hip)
        }
    }
    if constexpr (NEMIT >= 1) dw_store_stats(a, c, tl.cg * 64 + wv * 16 + c.jj, tl.row0 + ZS0, S1, S2);
}

// ======================================================= producer steps =====================================================
struct D4Regs { f32x4 pre[kDwNPF]; };
// the combination of depth index t + 1 a stage of t = 1 or t = 3 formed beside its own: a lane's three words of one channel block
struct D4Keep { f32x2 lo[kDwNPF], hi[kDwNPF]; };

// one more unit into the running combination(s): + c u (and, PAIR, + cp u into the kept one)
template <bool PAIR>
__device__ __forceinline__ void d4_chain(const f32x2 (&ul)[kDwNPF], const f32x2 (&uh)[kDwNPF], float c, float cp, f32x2 (&lo)[kDwNPF],
                                         f32x2 (&hi)[kDwNPF], D4Keep& kp) {
    const f32x2 c2 = {c, c};
#pragma unroll
    for (int i = 0; i < kDwNPF; ++i) { lo[i] = __builtin_elementwise_fma(ul[i], c2, lo[i]); hi[i] = __builtin_elementwise_fma(uh[i], c2, hi[i]); }
    if constexpr (PAIR) {
        const f32x2 p2 = {cp, cp};
#pragma unroll
        for (int i = 0; i < kDwNPF; ++i) { kp.lo[i] = __builtin_elementwise_fma(ul[i], p2, kp.lo[i]); kp.hi[i] = __builtin_elementwise_fma(uh[i], p2, kp.hi[i]); }
    }
}

// the zero padding of the plane: one multiply of the combined words, in tiles that touch the plane's edge only (80 % are interior).
// A branch (the empty asm keeps it one): as selects, 6 multiplies and 12 selects in every stage of every tile.
__device__ __forceinline__ void d4_mask(const DwProd& P, f32x2 (&lo)[kDwNPF], f32x2 (&hi)[kDwNPF]) {
    if (!P.interior) {
        asm volatile("");
#pragma unroll
        for (int i = 0; i < kDwNPF; ++i) {
            const f32x2 kk = {P.cur.keep[i], P.cur.keep[i]};
            lo[i] = lo[i] * kk; hi[i] = hi[i] * kk;
        }
    }
}

// raw words of one unit = (slice z0 - 1 + j, channel block cb) -> registers; nx: of the NEXT tile (book nxt, tile tn)
__device__ __forceinline__ void d4_issue(const WinoPcArgs& a, const DwProd& P, bool nx, int j, int cb, D4Regs& r) {
    const int tz = (nx ? P.tn.z0 : P.tl.z0) - 1 + j;
    const int z = __builtin_amdgcn_readfirstlane(min(max(tz, 0), a.N - 1));    // clamped: an outside slice is not used when published
    const size_t base = ((size_t)z * P.plane + (size_t)(__builtin_amdgcn_readfirstlane(cb) * kCB)) * sizeof(float);
    const __amdgpu_buffer_rsrc_t xb = pc_rsrc(reinterpret_cast<const char*>(a.x) + base);
#pragma unroll
    for (int u = 0; u < kDwNPF; ++u) r.pre[u] = pc_bload(xb, nx ? P.nxt.off[u] : P.cur.off[u]);
}

// One stage up to its transform: stage s of the current tile = position cbi of the phase at position p.  The stage's depth
// combination D_t = sum_k c_k act(x[z_k]) is formed IN REGISTERS (all four unit sets were requested a stage ago) and the strip gi & 1
// written once: wino_dw.hip's publish-then-combine through the strip (a read-modify-write of the LDS words per further unit) would
// cost 9 more LDS reads and 6-9 more writes per lane and stage here.  A slice outside the volume enters with coefficient 0 (its
// clamped load is finite); the zero padding of the plane is one multiply of the combined words.
// Unit by unit: wait for ITS words only, fold them into the running combination, request the same slot of stage s + 1 right away —
// one register set per unit slot, a whole stage for the load to land (two sets alternating inside the stage left one unit of work
// between request and use).  The refills stay spread over the stage: twelve loads in one burst cost ~600 issue cycles in a row, and
// one wait for all four sets exposes the slowest — measured +3 % against this order.
// PAIR (phases t = 1 and t = 3 when the kept sets are in use): t + 1 names the SAME four slices with other coefficients, so every
// activated unit feeds a second FMA chain — same slot order, same "first slot copied or zero" rule, same outside-slice test as the
// stage of t + 1 would apply, hence the same bits — whose three words per lane wait in `kp` for d4_restore.  The last stage of such
// a phase requests nothing: its successor loads nothing, and d4_restore requests the sets of the next loading stage.
template <bool IDENT, bool CLAMP, bool PAIR>
__device__ __forceinline__ void d4_combine(const WinoPcArgs& a, const DwProd& P, int NS, int ncb, int s, int p, int cbi, D4Regs& set0, D4Regs& set1,
                                           D4Regs& set2, D4Regs& set3, D4Keep& kp) {
    float* raw = P.strip(P.gi & 1);
    const int t = d4_t(p), cb = PAIR ? cbi : dw_cb(p, cbi, ncb), nsl = d4_nslot(t);      // PAIR: p is even, a forward sweep
    // stage s + 1: (position, channel block, depth index), possibly of the next tile; PAIR: the next block of this phase, if any
    const bool nx = !PAIR && s + 1 >= NS;
    const bool refill = !PAIR || cbi + 1 < ncb;
    const int cbn = cbi + 1 == ncb ? 0 : cbi + 1, pn = nx ? 0 : (cbi + 1 == ncb ? p + 1 : p);
    const int tnx = PAIR ? t : d4_t(pn), cbne = PAIR ? cbi + 1 : dw_cb(pn, cbn, ncb);
    f32x4 ssw[2] = {{1.f, 1.f, 0.f, 0.f}, {1.f, 1.f, 0.f, 0.f}};     // (scale, shift) pairs of the stage's channel block (pre-paired table)
    if constexpr (!IDENT) {
        ssw[0] = *reinterpret_cast<const f32x4*>(P.ssl + 2 * (cb * kCB + P.p.w4 * 4));
        ssw[1] = *reinterpret_cast<const f32x4*>(P.ssl + 2 * (cb * kCB + P.p.w4 * 4) + 4);
    }
    const int nsn = d4_nslot(tnx);
    float c[4], cp[4];                                       // cp: the partner's (t + 1) coefficients, PAIR only
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int z = P.tl.z0 - 1 + d4_j(t, k < nsl ? k : 0);
        const bool in = k < nsl && z >= 0 && z < a.N;
        c[k] = in ? d4_c(t, k) : 0.f;
        cp[k] = PAIR && in ? d4_c(t + 1, k) : 0.f;
    }
    f32x2 lo[kDwNPF], hi[kDwNPF], ul[kDwNPF], uh[kDwNPF];
    // the first slot's coefficient is 1 (every row of Bd has one): its unit IS the running combination — unless its slice is outside
    // the volume (t = 5 of the last depth tile), then 0.  A branch (the empty asm keeps it one): as a select it is 12 moves to zero
    // and 12 moves back in every stage.
    dw_activate<IDENT, CLAMP>(set0.pre, ssw, a.x_relu, lo, hi);
    if (c[0] == 0.f) {
        asm volatile("");
#pragma unroll
        for (int i = 0; i < kDwNPF; ++i) { lo[i] = f32x2{0.f, 0.f}; hi[i] = f32x2{0.f, 0.f}; }
    }
    if constexpr (PAIR) {                                    // the partner's first slot is the same slice with the same coefficient
#pragma unroll
        for (int i = 0; i < kDwNPF; ++i) { kp.lo[i] = lo[i]; kp.hi[i] = hi[i]; }
    }
    if (refill) d4_issue(a, P, nx && P.has_next, d4_j(tnx, 0), cbne, set0);
    dw_activate<IDENT, CLAMP>(set1.pre, ssw, a.x_relu, ul, uh);
    d4_chain<PAIR>(ul, uh, c[1], cp[1], lo, hi, kp);
    if (refill) d4_issue(a, P, nx && P.has_next, d4_j(tnx, 1), cbne, set1);
    dw_activate<IDENT, CLAMP>(set2.pre, ssw, a.x_relu, ul, uh);
    d4_chain<PAIR>(ul, uh, c[2], cp[2], lo, hi, kp);
    if (refill) d4_issue(a, P, nx && P.has_next, d4_j(tnx, 2), cbne, set2);
    if (nsl > 3) {
        dw_activate<IDENT, CLAMP>(set3.pre, ssw, a.x_relu, ul, uh);
        d4_chain<PAIR>(ul, uh, c[3], cp[3], lo, hi, kp);
    }
    if (refill && nsn > 3) d4_issue(a, P, nx && P.has_next, d4_j(tnx, 3), cbne, set3);
    d4_mask(P, lo, hi);
#pragma unroll
    for (int i = 0; i < kDwNPF; ++i) *reinterpret_cast<f32x4*>(raw + P.p.wr_off[i]) = __builtin_shufflevector(lo[i], hi[i], 0, 1, 2, 3);
}

// A stage of t = 2 or t = 4 (position p = 1 or 3) when the kept sets are in use: no load, no activation, no combination — the
// words its partner stage left in `kp`, the plane-padding mask, the strip.  The register sets are idle through such a phase, so
// its stages request, spread over themselves, the units of the NEXT LOADING stage — the first of phase p + 1, same tile: slot k
// goes out in the stage at position 4 cbi / ncb <= k < 4 (cbi + 1) / ncb (one per stage at four channel blocks, two at two, all
// four at one), each between two strip writes.  Nothing reads a set between the partner phase's last stage and that stage.
__device__ __forceinline__ void d4_restore(const WinoPcArgs& a, const DwProd& P, int ncb, int p, int cbi, const D4Keep& kp, D4Regs& set0,
                                           D4Regs& set1, D4Regs& set2, D4Regs& set3) {
    float* raw = P.strip(P.gi & 1);
    const int tnx = d4_t(p + 1), cbne = 0, nsn = d4_nslot(tnx);          // p + 1 is even: its sweep starts at block 0
    const int k0 = 4 * cbi / ncb, k1 = 4 * (cbi + 1) / ncb;
    f32x2 lo[kDwNPF], hi[kDwNPF];
#pragma unroll
    for (int i = 0; i < kDwNPF; ++i) { lo[i] = kp.lo[i]; hi[i] = kp.hi[i]; }
    d4_mask(P, lo, hi);
    if (k0 <= 0 && 0 < k1) d4_issue(a, P, false, d4_j(tnx, 0), cbne, set0);
    *reinterpret_cast<f32x4*>(raw + P.p.wr_off[0]) = __builtin_shufflevector(lo[0], hi[0], 0, 1, 2, 3);
    if (k0 <= 1 && 1 < k1) d4_issue(a, P, false, d4_j(tnx, 1), cbne, set1);
    *reinterpret_cast<f32x4*>(raw + P.p.wr_off[1]) = __builtin_shufflevector(lo[1], hi[1], 0, 1, 2, 3);
    if (k0 <= 2 && 2 < k1) d4_issue(a, P, false, d4_j(tnx, 2), cbne, set2);
    *reinterpret_cast<f32x4*>(raw + P.p.wr_off[2]) = __builtin_shufflevector(lo[2], hi[2], 0, 1, 2, 3);
    if (k0 <= 3 && 3 < k1 && nsn > 3) d4_issue(a, P, false, d4_j(tnx, 3), cbne, set3);
}

// The kept set of a stage's channel block is picked by a uniform branch, one marker (an empty asm statement) per set: the four
// branches stay branches on registers of their own.  Merged by the compiler they become a dynamically indexed array, which lives in
// scratch memory; as selects they cost 36 instructions a stage.  (The two phases written out stage by stage in straight-line code
// — every set named at compile time — spilled: 156 to 436 bytes of scratch.)
template <int SET>
__device__ __forceinline__ void d4_keep(D4Keep& k, const D4Keep& v) {
#pragma unroll
    for (int i = 0; i < kDwNPF; ++i) {
        asm volatile("v_mov_b64 %0, %1 ; keep set %2" : "+v"(k.lo[i]) : "v"(v.lo[i]), "n"(SET));
        asm volatile("v_mov_b64 %0, %1 ; keep set %2" : "+v"(k.hi[i]) : "v"(v.hi[i]), "n"(SET));
    }
}
template <int SET>
__device__ __forceinline__ void d4_restore_set(const WinoPcArgs& a, const DwProd& P, int ncb, int p, int cbi, const D4Keep& k, D4Regs& set0,
                                               D4Regs& set1, D4Regs& set2, D4Regs& set3) {
    asm volatile("; kept set %0" ::"n"(SET));
    d4_restore(a, P, ncb, p, cbi, k, set0, set1, set2, set3);
    asm volatile("; kept set %0 written" ::"n"(SET));
}

// the tile's stage (p, cbi); pair: the kept sets are in use
template <bool IDENT, bool CLAMP>
__device__ __forceinline__ void d4_stage(const WinoPcArgs& a, const DwProd& P, bool pair, int NS, int ncb, int s, int p, int cbi, D4Regs& set0,
                                         D4Regs& set1, D4Regs& set2, D4Regs& set3, D4Keep& k0, D4Keep& k1, D4Keep& k2, D4Keep& k3) {
    const int cb = dw_cb(p, cbi, ncb);
    D4Keep kp;
    if (!pair || p >= 4) {
        d4_combine<IDENT, CLAMP, false>(a, P, NS, ncb, s, p, cbi, set0, set1, set2, set3, kp);
    } else if (!(p & 1)) {
        d4_combine<IDENT, CLAMP, true>(a, P, NS, ncb, s, p, cbi, set0, set1, set2, set3, kp);
        if (cb == 0) d4_keep<0>(k0, kp);
        else if (cb == 1) d4_keep<1>(k1, kp);
        else if (cb == 2) d4_keep<2>(k2, kp);
        else d4_keep<3>(k3, kp);
    } else {
        if (cb == 0) d4_restore_set<0>(a, P, ncb, p, cbi, k0, set0, set1, set2, set3);
        else if (cb == 1) d4_restore_set<1>(a, P, ncb, p, cbi, k1, set0, set1, set2, set3);
        else if (cb == 2) d4_restore_set<2>(a, P, ncb, p, cbi, k2, set0, set1, set2, set3);
        else d4_restore_set<3>(a, P, ncb, p, cbi, k3, set0, set1, set2, set3);
    }
}

template <bool IDENT, bool CLAMP>
__global__ __launch_bounds__(512) void conv_wino_dw4_kernel(const WinoD4Args aa) {
    const WinoPcArgs& a = aa.b;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Vb = lds;                                   // [2][16 xi][32 tiles][16]
    float* rawb = lds + kDwNBuf * kPcV;                // [2][10 rows][20 pixels][16] shared strips
    float* stashb = rawb + kDwStrips;                  // [4 consumer waves][2 stashes][8][64][4]
    float* ssl = stashb + 4 * kDwStashWave;            // [Cin][2] (scale, shift) of x, pre-paired

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wv = wave & 3;                           // index within the role
    const int ncb = a.Cin / kCB;
    const int NS = 6 * ncb;                            // stages per tile (four output slices)

    int first, step, end;
    pc_tile_share(a.ntiles, first, step, end);
    if (first >= end) return;                  // uniform: no wave of this workgroup ever reaches a barrier
    const int count = (end - first + step - 1) / step;
    pc_load_ss_table<false>(ssl, a.Cin, a.x_ss, nullptr, CLAMP ? a.x_unit : 1.f);
    __syncthreads();

    if (wave >= 4) {
        // =========================================== consumer: 16 output channels x 16 xi x 32 tiles, one M_t at a time ========
        const DwLane c = dw_lane(a, lane, wv);
        DwAcc acc;
        const size_t wgroup = (size_t)NS * 16 * 256;                        // f32x4 per 64-column output group
        D4Stash st;
        st.A = reinterpret_cast<f32x4*>(stashb + wv * kDwStashWave) + lane;
        st.B = st.A + 8 * 64;
        st.C = pc_rsrc(reinterpret_cast<const char*>(aa.scratch) + ((size_t)blockIdx.x * 4 + wv) * kD4ScratchWave * sizeof(float));
        st.laneC = lane * 16;
        DwTile tl = dw_decode<4>(first, a);
        const f32x4* wt = c.wbase + (size_t)tl.cg * wgroup;
        f32x4 Bn[kPcNB], An[2][2];
        const f32x2 n1 = dw_prime(Bn, An, wt, Vb, c);                       // the two opening barriers
        int buf = 0;
        for (int it = 0; it < count; ++it) {
            const int tnext = first + (it + 1 < count ? it + 1 : it) * step;
            const DwTile tn = dw_decode<4>(tnext, a);
            const f32x4* wt_next = c.wbase + (size_t)tn.cg * wgroup;
            dw_phase<0, 6>(acc, An, Bn, Vb, buf, wt, wt_next, ncb, c);      // a barrier per stage inside
            d4_fold<0>(acc, a, c, tl, wv, st, n1);
            dw_phase<1, 6>(acc, An, Bn, Vb, buf, wt, wt_next, ncb, c);
            d4_fold<1>(acc, a, c, tl, wv, st, n1);
            dw_phase<2, 6>(acc, An, Bn, Vb, buf, wt, wt_next, ncb, c);
            d4_fold<2>(acc, a, c, tl, wv, st, n1);
            dw_phase<3, 6>(acc, An, Bn, Vb, buf, wt, wt_next, ncb, c);
            d4_fold<3>(acc, a, c, tl, wv, st, n1);                          // slices z0 + 1, z0 + 2 complete
            dw_phase<4, 6>(acc, An, Bn, Vb, buf, wt, wt_next, ncb, c);
            d4_fold<4>(acc, a, c, tl, wv, st, n1);                          // slice z0
            dw_phase<5, 6>(acc, An, Bn, Vb, buf, wt, wt_next, ncb, c);
            d4_fold<5>(acc, a, c, tl, wv, st, n1);                          // slice z0 + 3
            tl = tn;
            wt = wt_next;
        }
    } else {
        // =========================================== producer: tile row wv (8 Winograd tiles) ===========================
        DwProd P;
        dw_prod_init<4, false>(a, P, wv, lane, Vb, rawb, ssl, first);
        D4Regs set0, set1, set2, set3;     // one register set per unit slot of a stage (the fourth empty for t = 0 and t = 5)
        {
            const int t0 = d4_t(0), cb0 = dw_cb(0, 0, ncb);
            d4_issue(a, P, false, d4_j(t0, 0), cb0, set0);
            d4_issue(a, P, false, d4_j(t0, 1), cb0, set1);
            d4_issue(a, P, false, d4_j(t0, 2), cb0, set2);
            d4_issue(a, P, false, d4_j(t0, 3 < d4_nslot(t0) ? 3 : 0), cb0, set3);
        }
        // up to four channel blocks (Cin <= 64: every K-Net layer) pair t = 1 with 2 and t = 3 with 4; a wider input loads every
        // phase's units afresh, as t = 0 and t = 5 always do
        const bool pair = ncb <= 4;
        D4Keep k0 = {}, k1 = {}, k2 = {}, k3 = {};     // one kept combination per channel block in flight (t = 1 -> 2, t = 3 -> 4)
        for (int it = 0; it < count; ++it) {
            dw_tile_begin(a, P, it + 1 < count);
            int cbi = 0, p = 0;
            for (int s = 0; s < NS; ++s) {
                if (s == NS - 1 && P.has_next) dw_next_tile<4, false>(a, P, first + (it + 1) * step);
                d4_stage<IDENT, CLAMP>(a, P, pair, NS, ncb, s, p, cbi, set0, set1, set2, set3, k0, k1, k2, k3);
                if (P.gi > 0) dw_transform(P.p, P.strip((P.gi & 1) ^ 1), Vb + P.qbuf * kPcV);   // the stage published one iteration ago
                __syncthreads();
                dw_stage_end(P);
                if (++cbi == ncb) { cbi = 0; ++p; }
            }
            dw_tile_end(P);
        }
        dw_transform(P.p, P.strip((P.gi & 1) ^ 1), Vb + P.qbuf * kPcV);     // the last published stage
        __syncthreads();
        __syncthreads();                       // the consumers' last stage
    }
}

}  // namespace nrgbd

// the weight stream's phases are in EXECUTION order: stage = p*ncb + cb, t = d4_t(p) (DwDepth<6>::t_of_phase)
extern "C" int nrgbd_conv_wino_dw4_pack(const float* w, float* w_wino, int Cin, int Cout, int transposed, void* stream) {
    return nrgbd::dw_pack<6>(w, w_wino, Cin, Cout, transposed, stream);
}

extern "C" int nrgbd_conv_wino_dw4_workspace(int N, int H, int W, int Cout, size_t* bytes) {
    if (!bytes) return NRGBD_E_NULL;
    if (N <= 0 || (N & 3) || H <= 0 || W <= 0 || Cout <= 0 || Cout % 64) return NRGBD_E_SHAPE;
    int n = 0;
    const int rc = nrgbd::dw_workgroups(4, N, H, W, Cout, &n);
    if (rc != NRGBD_OK) return rc;
    *bytes = (size_t)n * 4 * nrgbd::kD4ScratchWave * sizeof(float);
    return NRGBD_OK;
}

extern "C" int nrgbd_conv_wino_dw4_f32(const float* x, const float* x_ss, int x_relu, float x_unit, const float* w_wino, float* y,
                                       float* stats, void* workspace, size_t workspace_bytes, int N, int H, int W, int Cin, int Cout,
                                       void* stream) {
    using namespace nrgbd;
    if (!x || !w_wino || !y || !workspace) return NRGBD_E_NULL;
    int rows = 0, nwg = 0;           // statistics rows; persistent workgroups
    long nt = 0;
    int rc = dw_check(4, N, H, W, Cin, Cout, &rows, &nt);
    if (rc != NRGBD_OK) return rc;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return NRGBD_E_ALIGN;
    const bool clamp = x_unit != 0.f;
    if (clamp && (!x_ss || !x_relu || !dw_unit_ok(x_unit))) return NRGBD_E_ARG;
    if (nt >= (1L << 31)) return NRGBD_E_SHAPE;
    rc = dw_workgroups(4, N, H, W, Cout, &nwg);
    if (rc != NRGBD_OK) return rc;
    if (workspace_bytes < (size_t)nwg * 4 * kD4ScratchWave * sizeof(float)) return NRGBD_E_NULL;
    WinoD4Args aa{};
    aa.b = WinoPcArgs{x, x_ss, nullptr, nullptr, nullptr, w_wino, y, stats, x_relu, 0, N, H, W, Cin, Cout, (int)nt, rows,
                      nullptr, 0, 0, 0, 0, x_unit};
    aa.scratch = static_cast<float*>(workspace);
    const DwLaunch l{nwg, dw_lds_bytes(1, Cin), dw_lds_attr(1), (hipStream_t)stream};
    if (clamp) return dw_launch<conv_wino_dw4_kernel<false, true>>(l, aa);
    if (!x_ss && !x_relu) return dw_launch<conv_wino_dw4_kernel<true, false>>(l, aa);
    return dw_launch<conv_wino_dw4_kernel<false, false>>(l, aa);
}
