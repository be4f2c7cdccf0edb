// wino_dw.hip — the K-Net's 3x3x3 convolutions (models/basic.py:71-94) in the Winograd domain in ALL THREE dimensions:
// F(2x2, 3x3) in the image plane (as wino_pc.hip) and F(2, 3) along the depth axis on top of it.
//
// Why.  wino_pc.hip treats the three depth taps of a 3x3x3 layer as three independent 2-D Winograd problems: 16 multiplies per
// 2x2 outputs and depth tap, 3 taps -> 12 multiplies per output voxel (direct: 27).  At config B its ten 64 -> 64 layers are
// 61 % of the frame and run at 66 % of the fp32 matrix peak with the matrix pipe as the critical resource — the only lever left
// is fewer multiplies.  F(2, 3) along depth produces TWO output slices from FOUR transformed slices: 4 x 16 multiplies per
// 2x2x2 outputs = 8 per output voxel, 1.5x fewer MFMAs, still exact-algorithm fp32 (only the rounding order differs; measured
// against float64: mean error 1.3x the 2-D form's, tests/test_gpu_knet.py).
//
//   input   d_j = act(x[z0 - 1 + j]),  j = 0..3                      (z0 = first of the two output slices of a tile)
//   depth   D_0 = d_0 - d_2,  D_1 = d_1 + d_2,  D_2 = d_2 - d_1,  D_3 = d_1 - d_3          (B^T of F(2,3))
//   plane   V_t = B^T D_t B per 4x4 patch                                                   (as wino_pc.hip)
//   weights U_t = sum_kd Gd[t][kd] (G g_kd G^T),  Gd = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]  (packed on the device, float64)
//   product M_t = sum_ci V_t U_t                                                            (the MFMAs: 4 x Cin/16 stages)
//   output  y[z0] = A^T (M_0 + M_1 + M_2) A,   y[z0 + 1] = A^T (M_1 - M_2 - M_3) A
//
// Same persistent producer / consumer organisation, tile geometry, LDS images and weight-stream layout as wino_pc.hip (read its
// header first); what differs:
//   * a tile is 8x16 pixels x TWO depth slices; its stage list is t-major: stage s = t * (Cin/16) + cb, so that the consumers'
//     128 accumulator registers hold ONE M_t at a time;
//   * consumers: at the end of phase t (its last channel block) the accumulators are inverse-transformed in the plane (A^T . A:
//     32 values per lane) and folded into the two output slices, which accumulate in two 32 KB LDS stashes (the register file
//     is full: 128 accumulators + weight ring + operands); phase 2 completes and stores slice z0, phase 3 slice z0+1, each
//     with its BatchNorm partial statistics;
//   * producers: a stage needs the depth combination of TWO slices.  The unit of prefetch stays one (slice, channel block):
//     unit A is normalised / activated and published to the stage's strip exactly as in wino_pc.hip, unit B is activated and
//     COMBINED with what the strip holds (A +- B: a lane reads back its own words; a wave's LDS operations execute in order),
//     and the strip is transformed one iteration later (shared strips, below).  Each unit has its own register set, refilled
//     for the NEXT stage right after it was published.
// Work per pair of output slices: 16 stages (wino_pc: 24); producer publishes 32 (24); plane transforms 16 (24).
// LDS: 2 x 32 KB V + 2 x 12.8 KB strips + 2 x 32 KB stash = 154 KB; 8 waves, up to 256 VGPRs each.  (Two V buffers instead of
// wino_pc's three — the third one's 32 KB hold the second stash.  A consumer therefore cannot read the first operand of the
// next stage before the stage barrier; instead it ARRIVES at the barrier early, as soon as its last LDS operand of the stage is
// in registers, and reads the next stage's first operand under its own last 8 MFMAs.)
//
// In wino_dw.hpp, shared with wino_dw4.hip: the constants, DwTile + dw_decode<2>, the serpentine order dw_cb, the barrier protocol, the
// consumers' steps (dw_lane, dw_prime, dw_phase / dw_mfma_stage, dw_plane_inverse, dw_emit, dw_store_stats), the producers' (dw_items,
// dw_book, dw_activate, dw_transform, DwProd), the weight packer (dw_pack<4>) and the host helpers.  Here: the F(2, 3) depth transform
// — dw2_issue, dw2_publish, dw2_stage, dw2_fold — the kernel and its launcher.
//
// Measured, then removed (the ablation bits of a developer build this file carried until its split into named steps — 1 no MFMAs,
// 2 no producer work, 4 no transform, 8 / 16 no publish of unit A / B, 32 no refills, 64 no fold; results invalid, timing only):
// at config B, in the first version of this kernel, the producers alone took 1.4 ms per layer, the consumers alone 2.0 ms, both
// together 2.8 ms: the two roles hardly overlapped (docs/design_notes_r1-r3.md lists what was found with that and changed).
#include "wino_dw.hpp"

namespace nrgbd {

// slices combined by stage phase t: V_t = d[zA] + sign * d[zB]
__device__ __forceinline__ int dw_zA(int t) { return t == 0 ? -1 : (t == 2 ? 1 : 0); }   // relative to z0: -1, 0, 1, 0
__device__ __forceinline__ int dw_zB(int t) { return t == 2 ? 0 : (t == 3 ? 2 : 1); }    //                  1, 1, 0, 2

// RES: a second operand (res) is added after activation.  MAT: the activated input is also written out (a.mat).  MAT is a
// template parameter because of what its stores do to the OTHER variants: with loads and stores of one wave both pending the
// compiler cannot rely on in-order completion and turns every s_waitcnt on a prefetched register into vmcnt(0) — which also
// waits for the refill issued a few instructions earlier, i.e. exposes a full memory latency per stage.
// RSID: the residual operand comes with identity (scale, shift) and no ReLU (the K-Net's four residual layers: a materialised
// skip tensor) — its normalisation FMAs are dropped.
// IDENT: x needs no (scale, shift) and no ReLU (an input some earlier pass materialised: the K-Net's residual layers behind
// nrgbd_nhwc_act, every layer of the training path) — the producers' 10 packed FMAs per unit are dropped (instantiated for the
// plain form only).
// CLAMP: x = relu(x * s + t) with the ReLU taken by the FMA's own [0, 1] clamp: the (scale, shift) pairs are multiplied by
// a.x_unit = 2^-k on their way to LDS (k chosen by the caller so that no activated value can reach 2^k: |BatchNorm(y)| <=
// |gamma| sqrt(n) + |beta| for batch statistics over n values) and the weight stream carries 2^k.  Scaling by a power of two
// commutes with every rounding of the path, so the output bits are those of the plain form; the producers lose the 20
// v_max_f32 per unit (instantiated for the plain form only).
template <bool RES_, bool MAT_, bool RSID_, bool IDENT_, bool CLAMP_>
struct Dw2Form { static constexpr bool RES = RES_, MAT = MAT_, RSID = RSID_, IDENT = IDENT_, CLAMP = CLAMP_; };

// ======================================================= consumer: the fold =================================================
// End of phase T: plane inverse transform of M_T (A^T . A: 32 values per lane) and the depth fold
//   y[z0]     = M_0 + M_1 + M_2      (LDS stash 0; complete after phase 2)
//   y[z0 + 1] = M_1 - M_2 - M_3      (LDS stash 1; complete after phase 3)
// (in registers the 32 running values of a slice do not fit beside 128 accumulators + weight ring + operands: the compiler spilled
//  them to scratch INSIDE the MFMA blocks, i.e. into the in-order queue of the weight loads).  stash0: slice z0, this lane's word i at
// stash0[i * 64]; slice z0 + 1: 8 words further.  T >= 2 completes a slice: stores + statistics.
template <int T>
__device__ __forceinline__ void dw2_fold(const DwAcc& acc, const WinoPcArgs& a, const DwLane& c, const DwTile& tl, int wv, f32x4* stash0, f32x2 n1) {
    constexpr bool EMIT = T >= 2;
    f32x4* stash1 = stash0 + 8 * 64;
    const int zs = tl.z0 + (T == 3 ? 1 : 0);
    float* ys = a.y + (((size_t)zs * a.H + tl.y0) * a.W + tl.x0) * a.Cout + tl.cg * 64 + wv * 16;
    f32x2 S1[1] = {}, S2[1] = {};
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
                if constexpr (T == 0) {
                    stash0[wi * 64] = o;
                } else if constexpr (T == 1) {
                    stash0[wi * 64] = stash0[wi * 64] + o;
                    stash1[wi * 64] = o;
                } else if constexpr (T == 2) {
                    const f32x4 b = stash1[wi * 64];
                    stash1[wi * 64] = b - o;
                    dw_emit(a, c, ys, m, rp, aa, stash0[wi * 64] + o, S1[0], S2[0]);
                } else {
                    dw_emit(a, c, ys, m, rp, aa, stash1[wi * 64] - o, S1[0], S2[0]);
                }
            }
            // one (m, rp) group at a time: left to itself the scheduler interleaves all four groups and the 8 stash
            // words, and the register file (128 accumulators + ring + operands live here) overflows into scratch
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (EMIT) dw_store_stats(a, c, tl.cg * 64 + wv * 16 + c.jj, tl.row0 + (T == 3 ? 1 : 0), S1, S2);
}

// ======================================================= producer steps =====================================================
// One register set per unit of a stage (A, B): raw words (+ residual words) and the (scale, shift) words of the unit's 4 channels
template <bool RES> struct Dw2Regs { f32x4 pre[kDwNPF]; f32x4 prer[RES ? kDwNPF : 1]; f32x4 ss[2]; f32x4 rs[2]; };

// raw words of one unit = (slice zA or zB of phase t, channel block cb) -> registers; nx: of the NEXT tile (book nxt, tile tn)
template <class F>
__device__ __forceinline__ void dw2_issue(const WinoPcArgs& a, const DwProd& P, bool nx, int t, int cb, bool unitB, Dw2Regs<F::RES>& r) {
    const int w4 = P.p.w4;
    r.rs[0] = r.rs[1] = f32x4{1.f, 1.f, 0.f, 0.f};
    if constexpr (!F::IDENT) {
        r.ss[0] = *reinterpret_cast<const f32x4*>(P.ssl + 2 * (cb * kCB + w4 * 4));
        r.ss[1] = *reinterpret_cast<const f32x4*>(P.ssl + 2 * (cb * kCB + w4 * 4) + 4);
    }
    if constexpr (F::RES && !F::RSID) {
        r.rs[0] = *reinterpret_cast<const f32x4*>(P.ssl + 2 * a.Cin + 2 * (cb * kCB + w4 * 4));
        r.rs[1] = *reinterpret_cast<const f32x4*>(P.ssl + 2 * a.Cin + 2 * (cb * kCB + w4 * 4) + 4);
    }
    const int tz = (nx ? P.tn.z0 : P.tl.z0) + (unitB ? dw_zB(t) : dw_zA(t));
    // (z, cb) are wave-uniform; saying so keeps the base in SGPRs and the loads in their saddr form (uniform 64-bit base +
    // 32-bit lane offset) — otherwise every load of the stage loop pays a v_lshl_add_u64
    const int z = __builtin_amdgcn_readfirstlane(min(max(tz, 0), a.N - 1));    // clamped: an outside slice is not used when published
    const size_t base = ((size_t)z * P.plane + (size_t)(__builtin_amdgcn_readfirstlane(cb) * kCB)) * sizeof(float);
    const __amdgpu_buffer_rsrc_t xb = pc_rsrc(reinterpret_cast<const char*>(a.x) + base);
    const __amdgpu_buffer_rsrc_t rb = pc_rsrc(reinterpret_cast<const char*>(F::RES ? a.res : a.x) + base);
#pragma unroll
    for (int u = 0; u < kDwNPF; ++u) {
        const unsigned o = nx ? P.nxt.off[u] : P.cur.off[u];
        r.pre[u] = pc_bload(xb, o);
        if constexpr (F::RES) r.prer[u] = pc_bload(rb, o);
    }
}

// normalise / activate one unit (slice z, channel block cb) and publish it to the strip `raw`: COMBINE = false: strip = v; true:
// strip = strip + sgn * v.  INTERIOR: every item of every lane inside the image: no padding mask.  wmat: this unit is materialised.
template <class F, bool COMBINE, bool INTERIOR>
__device__ __forceinline__ void dw2_publish(const WinoPcArgs& a, const DwProd& P, Dw2Regs<F::RES>& r, float* raw, int z, int cb, bool wmat, float sgn) {
    constexpr int NU = kDwNPF;
    // the (scale, shift) words are re-paired for the packed FMAs HERE and not where they were loaded: without this the
    // compiler hoists the eight moves to right behind the loads, i.e. waits for the prefetch the moment it is issued
    if constexpr (!F::IDENT) asm volatile("" : "+v"(r.ss[0]), "+v"(r.ss[1]));
    if constexpr (F::RES && !F::RSID) asm volatile("" : "+v"(r.rs[0]), "+v"(r.rs[1]));
    const f32x2 rc01 = r.rs[0].lo, rh01 = r.rs[0].hi, rc23 = r.rs[1].lo, rh23 = r.rs[1].hi;   // the LDS table is stored pre-paired (pc_ss_slot)
    const f32x2 sg2 = {sgn, sgn};
    f32x2 lo[NU], hi[NU];
    f32x4 old[COMBINE ? NU : 1];
    if constexpr (COMBINE) {
        // the strip words unit A left: this lane wrote them itself (in-order LDS, no barrier); the memory clobber
        // keeps the compiler from forwarding the stored registers across the refill instead (20 live VGPRs)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int i = 0; i < NU; ++i) old[i] = *reinterpret_cast<const f32x4*>(raw + P.p.wr_off[i]);
    }
    dw_activate<F::IDENT, F::CLAMP>(r.pre, r.ss, a.x_relu, lo, hi);
    if constexpr (F::RES && F::RSID) {
#pragma unroll
        for (int i = 0; i < NU; ++i) { lo[i] = lo[i] + r.prer[i].lo; hi[i] = hi[i] + r.prer[i].hi; }
        __builtin_amdgcn_sched_barrier(0);
    } else if constexpr (F::RES) {
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
        f32x4 v = __builtin_shufflevector(lo[u], hi[u], 0, 1, 2, 3);
        if (F::MAT && wmat) {   // the activated input is written once per slice: by the wave that owns the pixel, in phase 1
            if ((P.cur.own >> u) & 1u)
                *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(a.mat) + ((size_t)z * P.plane + (size_t)(cb * kCB)) * sizeof(float) + P.cur.off[u]) = v;
        }
        if constexpr (COMBINE) {
            const f32x2 cl = __builtin_elementwise_fma(lo[u], sg2, old[u].lo), ch = __builtin_elementwise_fma(hi[u], sg2, old[u].hi);
            v = __builtin_shufflevector(cl, ch, 0, 1, 2, 3);
        }
        *reinterpret_cast<f32x4*>(raw + P.p.wr_off[u]) = v;
    }
}

// one stage up to its transform: stage s of the current tile = position cb of phase t.  (1) unit A -> strip gi & 1, its set refilled
// for stage s + 1 (of this tile or stage 0 of the next), (2) unit B combined into the strip, its set refilled.  A set is refilled right
// after it was published (longest time to land), and the refills are UNCONDITIONAL (the last stage of the last tile re-reads this
// tile's stage 0: harmless, never used).
template <class F>
__device__ __forceinline__ void dw2_stage(const WinoPcArgs& a, const DwProd& P, int NS, int ncb, int s, int t, int cb, Dw2Regs<F::RES>& setA,
                                          Dw2Regs<F::RES>& setB) {
    float* raw = P.strip(P.gi & 1);
    const int zA = P.tl.z0 + dw_zA(t), zB = P.tl.z0 + dw_zB(t);
    const bool zinA = zA >= 0, zinB = zB < a.N;          // zA <= z0 + 1 < N and zB >= z0 >= 0 always hold
    const bool wmat = F::MAT && t == 1 && P.tl.cg == 0;  // phase 1 publishes slices z0 (unit A) and z0 + 1 (unit B)
    const bool nx = s + 1 >= NS;
    const int cbn = cb + 1 == ncb ? 0 : cb + 1, tnx = nx ? 0 : (cb + 1 == ncb ? t + 1 : t);   // (t, position) of stage s + 1
    const int cbe = dw_cb(t, cb, ncb), cbne = dw_cb(tnx, cbn, ncb);                           // their channel blocks
    if constexpr (F::MAT) {
        // With materialise stores in the queue the compiler cannot count it (loads and stores of one wave pending =
        // "may complete out of order" = every wait becomes vmcnt(0)), and the wait for set B would also wait for the
        // refill of set A issued just before it.  So BOTH sets are waited for here, at the one point of the stage where
        // nothing else is in flight, and passed through an opaque asm: later uses no longer depend on the loads.
#pragma unroll
        for (int u = 0; u < kDwNPF; ++u) {
            asm volatile("" : "+v"(setA.pre[u]), "+v"(setB.pre[u]));
            if constexpr (F::RES) asm volatile("" : "+v"(setA.prer[u]), "+v"(setB.prer[u]));
        }
        asm volatile("" : "+v"(setA.ss[0]), "+v"(setA.ss[1]), "+v"(setB.ss[0]), "+v"(setB.ss[1]));
        if constexpr (F::RES && !F::RSID) asm volatile("" : "+v"(setA.rs[0]), "+v"(setA.rs[1]), "+v"(setB.rs[0]), "+v"(setB.rs[1]));
    }
    if (!zinA) {          // a slice outside the volume: the whole unit is zero padding
#pragma unroll
        for (int u = 0; u < kDwNPF; ++u) *reinterpret_cast<f32x4*>(raw + P.p.wr_off[u]) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
        if (P.interior) dw2_publish<F, false, true>(a, P, setA, raw, zA, cbe, wmat, 1.f);
        else dw2_publish<F, false, false>(a, P, setA, raw, zA, cbe, wmat, 1.f);
    }
    dw2_issue<F>(a, P, nx && P.has_next, tnx, cbne, false, setA);
    if (zinB) {           // V_t = d[zA] + sign d[zB], sign = +1 in phase 1 only
        if (P.interior) dw2_publish<F, true, true>(a, P, setB, raw, zB, cbe, wmat, t == 1 ? 1.f : -1.f);
        else dw2_publish<F, true, false>(a, P, setB, raw, zB, cbe, wmat, t == 1 ? 1.f : -1.f);
    }
    dw2_issue<F>(a, P, nx && P.has_next, tnx, cbne, true, setB);
}

template <bool RES, bool MAT, bool RSID, bool IDENT = false, bool CLAMP = false>
__global__ __launch_bounds__(512) void conv_wino_dw_kernel(const WinoPcArgs a) {
    using F = Dw2Form<RES, MAT, RSID, IDENT, CLAMP>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Vb = lds;                                   // [2][16 xi][32 tiles][16]
    float* rawb = lds + kDwNBuf * kPcV;                // the two shared strips: [2][10 rows][20 pixels][16]
    float* stashb = rawb + kDwStrips;                  // [4 consumer waves][2 slices][8][64][4]
    float* ssl = stashb + 4 * kDwStashWave;            // [Cin][2] (scale, shift) of x, then [Cin][2] of res

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wv = wave & 3;                           // index within the role
    const int ncb = a.Cin / kCB;
    const int NS = 4 * ncb;                            // stages per tile (pair of slices), t-major

    int first, step, end;
    pc_tile_share(a.ntiles, first, step, end);
    if (first >= end) return;                  // uniform: no wave of this workgroup ever reaches a barrier
    const int count = (end - first + step - 1) / step;
    // The per-channel (scale, shift) pairs go to LDS once (identity where the pointer is null).  Loading a stage's pairs from
    // global memory with its raw words puts them FIRST in the refill's queue, and the compiler moves them into their home
    // registers immediately: an s_waitcnt right behind the loads, i.e. one exposed L2 round trip per unit.
    pc_load_ss_table<true>(ssl, a.Cin, a.x_ss, RES ? a.res_ss : nullptr, CLAMP ? a.x_unit : 1.f);
    __syncthreads();

    if (wave >= 4) {
        // =========================================== consumer: 16 output channels x 16 xi x 32 tiles, one M_t at a time ========
        const DwLane c = dw_lane(a, lane, wv);
        DwAcc acc;
        const size_t wgroup = (size_t)NS * 16 * 256;                        // f32x4 per 64-column output group
        f32x4* stash0 = reinterpret_cast<f32x4*>(stashb + wv * kDwStashWave) + lane;
        DwTile tl = dw_decode<2>(first, a);
        const f32x4* wt = c.wbase + (size_t)tl.cg * wgroup;
        f32x4 Bn[kPcNB], An[2][2];
        const f32x2 n1 = dw_prime(Bn, An, wt, Vb, c);                       // the two opening barriers
        int buf = 0;
        for (int it = 0; it < count; ++it) {
            const int tnext = first + (it + 1 < count ? it + 1 : it) * step;
            const DwTile tn = dw_decode<2>(tnext, a);
            const f32x4* wt_next = c.wbase + (size_t)tn.cg * wgroup;
            dw_phase<0, 4>(acc, An, Bn, Vb, buf, wt, wt_next, ncb, c);      // a barrier per stage inside
            dw2_fold<0>(acc, a, c, tl, wv, stash0, n1);
            dw_phase<1, 4>(acc, An, Bn, Vb, buf, wt, wt_next, ncb, c);
            dw2_fold<1>(acc, a, c, tl, wv, stash0, n1);
            dw_phase<2, 4>(acc, An, Bn, Vb, buf, wt, wt_next, ncb, c);
            dw2_fold<2>(acc, a, c, tl, wv, stash0, n1);                     // slice z0 complete
            dw_phase<3, 4>(acc, An, Bn, Vb, buf, wt, wt_next, ncb, c);
            dw2_fold<3>(acc, a, c, tl, wv, stash0, n1);                     // slice z0 + 1
            tl = tn;
            wt = wt_next;
        }
    } else {
        // =========================================== producer: tile row wv (8 Winograd tiles) ===========================
        DwProd P;
        dw_prod_init<2, MAT>(a, P, wv, lane, Vb, rawb, ssl, first);
        Dw2Regs<RES> setA, setB;
        dw2_issue<F>(a, P, false, 0, 0, false, setA);
        dw2_issue<F>(a, P, false, 0, 0, true, setB);
        for (int it = 0; it < count; ++it) {
            dw_tile_begin(a, P, it + 1 < count);
            int cb = 0, t = 0;
            for (int s = 0; s < NS; ++s) {
                if (s == NS - 1 && P.has_next) dw_next_tile<2, MAT>(a, P, first + (it + 1) * step);
                dw2_stage<F>(a, P, NS, ncb, s, t, cb, setA, setB);
                if (P.gi > 0) dw_transform(P.p, P.strip((P.gi & 1) ^ 1), Vb + P.qbuf * kPcV);   // the stage published one iteration ago
                __syncthreads();
                dw_stage_end(P);
                if (++cb == ncb) { cb = 0; ++t; }
            }
            dw_tile_end(P);
        }
        dw_transform(P.p, P.strip((P.gi & 1) ^ 1), Vb + P.qbuf * kPcV);     // the last published stage
        __syncthreads();
        __syncthreads();                       // the consumers' last stage
    }
}

}  // namespace nrgbd

extern "C" int nrgbd_conv_wino_dw_pack(const float* w, float* w_wino, int Cin, int Cout, int transposed, void* stream) {
    return nrgbd::dw_pack<4>(w, w_wino, Cin, Cout, transposed, stream);
}

extern "C" int nrgbd_conv_wino_dw_workgroups(int N, int H, int W, int Cout) {
    if (N <= 0 || (N & 1) || H <= 0 || W <= 0 || Cout <= 0 || Cout % 64) return NRGBD_E_SHAPE;
    int n = 0;
    const int rc = nrgbd::dw_workgroups(2, N, H, W, Cout, &n);
    return rc == NRGBD_OK ? n : (rc < 0 ? rc : NRGBD_E_ARG);
}

static int conv_wino_dw_launch(const float* x, const float* x_ss, int x_relu, const float* res, const float* res_ss,
                               int res_relu, float* materialized, const float* w_wino, float* y, float* stats, int N,
                               int H, int W, int Cin, int Cout, void* stream, float x_unit = 0.f) {
    using namespace nrgbd;
    if (!x || !w_wino || !y) return NRGBD_E_NULL;
    int rows = 0, nwg = 0;           // statistics rows; persistent workgroups: one per CU
    long nt = 0;
    int rc = dw_check(2, N, H, W, Cin, Cout, &rows, &nt);
    if (rc != NRGBD_OK) return rc;
    if (nt >= (1L << 31)) return NRGBD_E_SHAPE;
    WinoPcArgs a{x, x_ss, res, res_ss, materialized, w_wino, y, stats, x_relu, res_relu, N, H, W, Cin, Cout, (int)nt, rows,
                 nullptr, 0, 0, 0, 0, x_unit};
    rc = dw_workgroups(2, N, H, W, Cout, &nwg);
    if (rc != NRGBD_OK) return rc;
    const DwLaunch l{nwg, dw_lds_bytes(2, Cin), dw_lds_attr(2), (hipStream_t)stream};   // 64 + 25.6 + 64 KB + tables; opt-in: 160 KB
    const bool rsid = res && !res_ss && !res_relu;
    if (x_unit != 0.f) return dw_launch<conv_wino_dw_kernel<false, false, false, false, true>>(l, a);   // CLAMP (nrgbd_conv_wino_dw_unit_f32 checked its preconditions)
    if (res && rsid) return materialized ? dw_launch<conv_wino_dw_kernel<true, true, true>>(l, a) : dw_launch<conv_wino_dw_kernel<true, false, true>>(l, a);
    if (res) return materialized ? dw_launch<conv_wino_dw_kernel<true, true, false>>(l, a) : dw_launch<conv_wino_dw_kernel<true, false, false>>(l, a);
    if (materialized) return dw_launch<conv_wino_dw_kernel<false, true, false>>(l, a);
    if (!x_ss && !x_relu) return dw_launch<conv_wino_dw_kernel<false, false, false, true>>(l, a);       // IDENT: nothing to apply to x
    return dw_launch<conv_wino_dw_kernel<false, false, false>>(l, a);
}

extern "C" int nrgbd_conv_wino_dw_f32(const float* x, const float* x_ss, int x_relu, const float* res, const float* res_ss,
                                      int res_relu, float* materialized, const float* w_wino, float* y, float* stats, int N,
                                      int H, int W, int Cin, int Cout, void* stream) {
    return conv_wino_dw_launch(x, x_ss, x_relu, res, res_ss, res_relu, materialized, w_wino, y, stats, N, H, W, Cin, Cout, stream);
}

// The plain form with relu(x * s + t) as a clamped FMA (the CLAMP instantiation): x_unit = 2^-k, the weight stream packed from
// 2^k * w; see include/nrgbd.h.
extern "C" int nrgbd_conv_wino_dw_unit_f32(const float* x, const float* x_ss, float x_unit, const float* w_wino, float* y, float* stats,
                                           int N, int H, int W, int Cin, int Cout, void* stream) {
    if (!x_ss) return NRGBD_E_NULL;
    if (!nrgbd::dw_unit_ok(x_unit)) return NRGBD_E_ARG;
    return conv_wino_dw_launch(x, x_ss, 1, nullptr, nullptr, 0, nullptr, w_wino, y, stats, N, H, W, Cin, Cout, stream, x_unit);
}
