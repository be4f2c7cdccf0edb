// costvol_quad.hip — generation 3 of the fused plane-sweep cost volume: FOUR LANES PER (pixel, candidate).
//
// Why (profiles/r1_pmc_summary.txt): generation 2 gives every lane one reference pixel and keeps its
// 68-channel texel in 68 VGPRs; with the staging batch and the tap pipeline that is 246 VGPRs = 2 waves per SIMD, its
// ds_read_b128 taps conflict on 25 % of the LDS cycles (16 lanes of a service group read 16 unrelated texels), and a
// workgroup alternates stage -> barrier -> math -> barrier with nothing to overlap them.  Here the 64 feature channels of a
// texel are split over the 4 lanes of a quad:
//
//   quad   = one reference pixel (8x8-pixel tile = 64 quads = 256 threads), walking the depth candidates;
//   lane j = feature words {j, 4+j, 8+j, 12+j} of that pixel (16 VGPRs of reference instead of 68), visited in an order
//            rotated by the quad's index: at step s quad i reads quarter (s + i) & 3 of its tap texel, so the four quads that
//            one ds_read_b128 service group holds ({0-3,12-15,20-27}, ... = quads {0,3,5,6}, {1,2,4,7}) always read FOUR
//            DIFFERENT 64-byte quarters => different banks whatever the four texels are: conflict-free BY CONSTRUCTION (LDS
//            texel stride 256 B), not by the luck of the homography being close to a translation;
//   the 4-tap interpolation of a lane's 16 channels needs no data from other lanes; the channel sum of (s - r)^2 is finished
//   with two DPP quad-permute adds (the wavefront-shuffle reduction);
//   the sampling coordinates (2 IEEE divisions each for x and y: the expensive scalar part) are computed ONCE per
//   (pixel, candidate): lane j of the quad does candidate 4g+j, then the record (4 weights + patch address) is broadcast
//   inside the quad with DPP quad_perm [i,i,i,i] while the four lanes evaluate candidate 4g+i together;
//   the RGB word (channels 64..66) of candidate 4g+j is done by lane j alone from a separate 16-B plane of the patch.
//
// Source texels reach the LDS by global_load_lds (no VGPR round trip): a wave instruction drops 4 texels x 256 B in lane
// order, which IS the patch layout.  The patch is the union footprint of a run of 2/4/8 candidates for one view, with a
// one-texel apron that may lie outside the image (filled from the clamped coordinate; its weight is zero), so the four taps
// of a pixel are {A, A+256, A+pitch, A+pitch+256}: one broadcast address per candidate instead of four clamped ones.
// Candidates whose footprint does not fit even as a pair (nearest planes: large, fast-moving footprints) are evaluated
// straight from L1/L2 with the same quad layout — a quad's taps are 64-byte contiguous runs, which the texture path serves at
// 4 lanes/clk (the generation-1 gather paid 1 lane/clk) — so they need neither a patch nor a barrier.
// 165 VGPRs => 3 workgroups (12 waves) per CU; one workgroup owns ALL candidates of its tile (when the grid fills the chip),
// so log_softmax over depth is taken in the same launch (models/basic.py:299-300).
//
// Arithmetic per tap / channel is the same as generations 1-2 (common.hpp helpers, same operation sequence for the
// coordinates); only the order of the channel sum differs (16 channels per lane, then the quad), like any other reduction order.
//
// The kernel below is the algorithm above as a sequence of named steps (anonymous namespace, all __forceinline__):
//   quad_tile_of_block  workgroup -> (tile, candidate chunk), XCD-aware
//   quad_prologue            the thread's constants (QuadCtx): LDS carve-up, pixel, its 16 + 4 reference channels
//   for every pass of 32 candidates, for every view:
//     quad_boxes        footprint of the tile on every candidate plane of the pass
//     for every run:    quad_priority_by_progress, quad_pick_run (longest run whose united footprint fits the patch),
//                       quad_stage<INTERIOR> (patch fill), quad_group_cost -> quad_group<STAGED, NI> per group of 4 candidates
//   quad_flush_pass     the pass's costs leave the LDS accumulators
//   quad_softmax<KMAX>  log-softmax over depth when the workgroup owns all candidates
//
// Tried and rejected (config B, us per launch of the same chip; each was a developer bit of NRGBD_ABLATE or a build knob until the
// kernel was split into steps; the bits 16 / 32 / 64 mean nothing now):
//   * every other workgroup walks its candidates far -> near, to de-phase the staging-bound (near planes) and math-bound (far
//     planes) parts of co-resident workgroups (bit 16): 288 with, 277 without (profiles/r2_pmc_summary.txt) — the workgroups
//     are not phase-locked;
//   * staging a single candidate whose footprint fits (bit 32): 300 vs 287 — a patch fill + two barriers for 64 (pixel,
//     candidate) pairs cost more than their 16 global loads;
//   * handing out a band's tiles in plain instead of scrambled order (bit 64): 280 vs 277, within run-to-run noise — per-CU
//     load imbalance is not what limits the kernel; nor do two mirrored half-bands per XCD help (round 5: 236 vs 234, the
//     workgroups' durations spread 1.9x inside every XCD, profiles/r5_costvol_limits.txt);
//   * wave priority (NRGBD_CV_PRIO): none (0) 229.8 / 230.2 against by progress (1, kept) 210.7 / 212.1; per view only
//     (2: 3 - view) 229 — the leader runs away (profiles/r5_costvol_limits.txt §2b).
#include "costvol.hpp"

// developer builds: phase clocks of a workgroup as seen by its thread 0 (a.trace, tools/cv_trace.py); compiled out of the product
#ifdef NRGBD_DEV
#define CVT_DECL long long cvt_[24] = {0}; long long cvt_t0_ = 0; const bool cvt_on_ = a.trace != nullptr && threadIdx.x == 0; \
    if (cvt_on_) { cvt_[0] = wall_clock64(); cvt_[2] = -clock64(); }
#define CVT_BEGIN() do { if (cvt_on_) cvt_t0_ = clock64(); } while (0)
#define CVT_END(slot) do { if (cvt_on_) cvt_[slot] += clock64() - cvt_t0_; } while (0)
#define CVT_COUNT(slot, n) do { if (cvt_on_) cvt_[slot] += (n); } while (0)
#define CVT_FLUSH() do { if (cvt_on_) { cvt_[1] = wall_clock64(); cvt_[2] += clock64(); \
    unsigned hw_; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_)); cvt_[17] = hw_; \
    unsigned xcc_; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_)); cvt_[18] = xcc_; \
    for (int q_ = 0; q_ < 24; ++q_) a.trace[(size_t)blockIdx.x * 24 + q_] = cvt_[q_]; } } while (0)
#else
#define CVT_DECL
#define CVT_BEGIN() do {} while (0)
#define CVT_END(slot) do {} while (0)
#define CVT_COUNT(slot, n) do {} while (0)
#define CVT_FLUSH() do {} while (0)
#endif

namespace nrgbd {

namespace {

constexpr int kQT = 8;            // tile edge
constexpr int kQRun = 32;         // candidates per staged run at most (groups of 4): two 16-lane DPP rows of footprint boxes
// texels of the patch (x 272 B): 156 texels = 42 KB, + 8.4 KB of cost accumulators [64 pixels][32 + 1 candidates], + boxes and candidates = 52.2 KB
// -> 3 workgroups per CU.  Round 5: the views' partial costs of a PASS (32 candidates of the workgroup, all views) meet in these LDS accumulators
// and leave them once; until then a candidate's cost was read-modify-written in global memory once per view (188-texel patch): WRITE_SIZE 53 -> 18.5 MB
// per launch, 236 -> 233.5 us at config B, 50.5 -> 49.1 at S, 226 -> 223 at H (same chip).  (Round 3's generation 4 did the same for all D
// candidates at once next to a 128-texel patch of LOOSE boxes: 415 vs 281 us — it was the patch size, not the accumulators.)
constexpr int kQPatch3 = 156;
constexpr int kQPatchR = (kQPatch3 + 63) / 64 * 64;   // RGB plane: a wave instruction fills 64 slots
constexpr int kQPass = 32;        // candidates per pass (= the longest run)
constexpr int kQAccPitch = kQPass + 1;
constexpr int kQFeatBytes = 256;  // feature plane: 16 words of 16 B per texel

template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}
// quad_perm controls: broadcast lane I of every quad; butterfly partners
template <int I> constexpr int kBcast = I * 0x55;
constexpr int kXor1 = 0xB1;  // [1,0,3,2]
constexpr int kXor2 = 0x4E;  // [2,3,0,1]

// one 16-byte word of the 4 taps against the reference word: accumulate dist(sample - ref) of its 4 channels
template <int DIST>
__device__ __forceinline__ void word_acc(const f32x4 A, const f32x4 B, const f32x4 C, const f32x4 D, const f32x4 rr,
                                         const f32x2 wnw, const f32x2 wne, const f32x2 wsw, const f32x2 wse, f32x2& pa,
                                         f32x2& pb) {
    // sample - ref with the reference word as the initial value of the tap chain (one rounding order among many; saves the
    // separate subtraction: 10 instead of 12 packed operations per word)
    f32x2 lo = __builtin_elementwise_fma(A.xy, wnw, -rr.xy), hi = __builtin_elementwise_fma(A.zw, wnw, -rr.zw);
    lo = __builtin_elementwise_fma(B.xy, wne, lo); hi = __builtin_elementwise_fma(B.zw, wne, hi);
    lo = __builtin_elementwise_fma(C.xy, wsw, lo); hi = __builtin_elementwise_fma(C.zw, wsw, hi);
    lo = __builtin_elementwise_fma(D.xy, wse, lo); hi = __builtin_elementwise_fma(D.zw, wse, hi);
    if constexpr (DIST == NRGBD_DIST_L2) {
        pa = __builtin_elementwise_fma(lo, lo, pa);
        pb = __builtin_elementwise_fma(hi, hi, pb);
    } else {
        pa = pa + __builtin_elementwise_abs(lo);
        pb = pb + __builtin_elementwise_abs(hi);
    }
}

// the RGB word (channels 64.. : `tail` of them count) of one candidate, all four taps by one lane
template <int DIST>
__device__ __forceinline__ float rgb_word(const f32x4 A, const f32x4 B, const f32x4 C, const f32x4 D, const f32x4 rr,
                                          const TapW& t, int tail) {
    float s[4];
    s[0] = __builtin_fmaf(D.x, t.se, __builtin_fmaf(C.x, t.sw, __builtin_fmaf(B.x, t.ne, A.x * t.nw))) - rr.x;
    s[1] = __builtin_fmaf(D.y, t.se, __builtin_fmaf(C.y, t.sw, __builtin_fmaf(B.y, t.ne, A.y * t.nw))) - rr.y;
    s[2] = __builtin_fmaf(D.z, t.se, __builtin_fmaf(C.z, t.sw, __builtin_fmaf(B.z, t.ne, A.z * t.nw))) - rr.z;
    s[3] = __builtin_fmaf(D.w, t.se, __builtin_fmaf(C.w, t.sw, __builtin_fmaf(B.w, t.ne, A.w * t.nw))) - rr.w;
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float term = (DIST == NRGBD_DIST_L2) ? s[e] * s[e] : fabsf(s[e]);
        acc = acc + ((e < tail) ? term : 0.f);
    }
    return acc;
}

// What the steps below need of the thread and its workgroup; fixed before the first pass.
struct QuadCtx {
    int tid, lane, wave;          // wave: scalar
    int quad, j;                  // the quad = reference pixel of the tile (0..63), and the lane's place in it
    int tx, ty;                   // the tile
    int tx0, tx1, ty0, ty1;       // its corner pixels, clipped to the image
    size_t hw, p;                 // pixels of an image; the quad's reference pixel (clamped into the image)
    float wf, hf;
    int tail;                     // valid channels of the RGB word
    int cofs[4];                  // per-lane word order: step s -> byte offset of word ((s + quad) & 3) * 4 + j inside a texel's feature plane
    f32x4 rr[4];                  // the reference words in that order
    f32x4 rgbref;
    char* ldsF;                   // [kQPatch3][256 B] feature plane of the patch; the softmax's scratch once the patch is dead
    char* ldsR;                   // [kQPatchR][16 B] RGB plane
    int4* boxes;                  // [kQPass] footprint of the tile per candidate of the pass (this view)
    float* dcand;                 // [D] depth candidates
    float* ldsA;                  // [64 pixels][kQAccPitch] partial costs of the pass, summed over the views
};

// The run of candidates that is evaluated next: n of them starting at `lo`; staged = from a patch that holds the box [xlo, xhi] x [ylo, yhi]
struct QuadRun {
    int n;
    bool staged;
    int xlo, xhi, ylo, yhi, cols;
};

// ---- workgroup -> (tile, candidate chunk) ----
// XCD k (= blockIdx % 8) owns a contiguous eighth of the TILE list so that the source rows a band of tiles samples stay in ONE
// 4 MB L2; with several chunks per tile the XCD's workgroups are ordered chunk-major — every tile's NEAREST chunk first: those
// are the expensive ones (short runs, unstaged groups: 2-3x the time of a far chunk, profiles/r5_costvol_diag_before.txt), and
// the hardware hands out workgroups in index order as slots free up, so the cheap far chunks fill in behind the slow near ones
// (longest-processing-time-first) instead of a slow chunk starting last.
__device__ __forceinline__ void quad_tile_of_block(const CostvolArgs& a, int& tile, int& chunk) {
    const int ntiles = gridDim.x / a.nchunk;
    tile = blockIdx.x / a.nchunk;
    chunk = blockIdx.x - tile * a.nchunk;
    if ((ntiles & 7) == 0) {
        const int per = ntiles >> 3;             // tiles of one XCD = its band of the tile list
        const int uu = blockIdx.x >> 3;
        chunk = uu / per;
        int u = uu - chunk * per;
        // Inside the band the tiles are handed out in a scrambled order: the workgroups that share a CU (consecutive or 32 apart
        // in an XCD's dispatch order) then come from tiles ~5 columns / a row + 11 columns apart instead of neighbours.  A tile's
        // cost (how many near-plane runs go to global memory) varies smoothly over the image, so neighbours on one CU could make
        // slow CUs and fast CUs.  (Worth nothing measurable — file header, "tried and rejected" — but it is what the timings of
        // rounds 4-6 were taken with.)
        if ((per & 31) == 0) {
            const int r = u >> 5, c = u & 31;
            u = (r << 5) | ((c * 5 + r * 11) & 31);
        }
        tile = (blockIdx.x & 7) * per + u;
    } else if ((gridDim.x & 7) == 0) {
        // a tile count that does not split into eight bands (config H: 300 tiles x 4 chunks): the XCD owns a contiguous eighth of
        // the (tile, chunk) list instead, tile-major — its chunks of one tile sample the same source rows from ONE L2 (without
        // this the four chunks of a tile ran on four XCDs: FETCH_SIZE 50 -> 105 MB per launch at config H)
        const int per = (int)gridDim.x >> 3;
        const int id = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
        tile = id / a.nchunk;
        chunk = id - tile * a.nchunk;
    }
}

// ---- prologue: the thread's constants (LDS carve-up, its pixel, its share of the reference texel) and the workgroup's copy of
// the depth candidates ----
template <int TAIL>
__device__ __forceinline__ QuadCtx quad_prologue(const CostvolArgs& a, char* smem, int tile) {
    QuadCtx t;
    t.ldsF = smem;
    t.ldsR = smem + kQPatch3 * kQFeatBytes;
    t.boxes = reinterpret_cast<int4*>(t.ldsR + kQPatchR * 16);
    t.dcand = reinterpret_cast<float*>(t.boxes + kQPass);
    t.ldsA = t.dcand + ((a.D + 3) & ~3);
    t.tid = threadIdx.x; t.lane = t.tid & 63; t.wave = __builtin_amdgcn_readfirstlane(t.tid >> 6);
    t.quad = t.tid >> 2; t.j = t.tid & 3;
    const int tiles_x = (a.w + kQT - 1) / kQT;
    t.tx = tile % tiles_x; t.ty = tile / tiles_x;
    const int x = t.tx * kQT + (t.quad & 7), y = t.ty * kQT + (t.quad >> 3);
    const int xc = min(x, a.w - 1), yc = min(y, a.h - 1);
    t.hw = (size_t)a.h * a.w;
    t.p = (size_t)yc * a.w + xc;
    t.wf = (float)a.w; t.hf = (float)a.h;
    t.tail = TAIL >= 0 ? TAIL : a.C - 64;
    for (int k = t.tid; k < a.D; k += 256) t.dcand[k] = a.d_candi[k];
    const int i3 = t.quad & 3;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        t.cofs[s] = (((s + i3) & 3) * 4 + t.j) * 16;
        t.rr[s] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(a.ref + t.p * a.Cp) + t.cofs[s]);
    }
    t.rgbref = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (TAIL != 0) t.rgbref = *reinterpret_cast<const f32x4*>(a.ref + t.p * a.Cp + 64);
    t.tx0 = t.tx * kQT; t.tx1 = min(t.tx * kQT + kQT - 1, a.w - 1);
    t.ty0 = t.ty * kQT; t.ty1 = min(t.ty * kQT + kQT - 1, a.h - 1);
    return t;
}

// ---- footprint of the tile on the candidate planes kb .. ke - 1 of one view -> t.boxes ----
// thread = (candidate, tile corner); the sampling positions of the 4 corner pixels bound the taps of the whole tile (a homography
// maps the convex tile onto a convex quadrilateral as long as the plane stays in front of the source camera: `bad` otherwise).
// Box = the texels their bounding box touches, inside [-1, w] x [-1, h] (apron), at least 2 x 2
template <bool ALIGN>
__device__ __forceinline__ void quad_boxes(const CostvolArgs& a, const QuadCtx& t, const float* KRv, const float* Ktv, int kb, int ke) {
    for (int c0 = kb; c0 < ke; c0 += 64) {
        const int c = c0 + (t.tid >> 2), cr = t.tid & 3;
        float fxlo = 0.f, fxhi = 0.f, fylo = 0.f, fyhi = 0.f;
        int bad = 0;
        if (c < ke) {
            const int pxc = (cr & 1) ? t.tx1 : t.tx0, pyc = (cr & 2) ? t.ty1 : t.ty0;
            const size_t pc = (size_t)pyc * a.w + pxc;
            const SweepTerm sc = make_sweep_term(KRv, Ktv, a.rays[pc], a.rays[t.hw + pc], a.rays[2 * t.hw + pc]);
            const float dc = t.dcand[c];
            const float den = (sc.t1z + sc.t2z * dc) + 1e-10f;
            float ix, iy;
            sweep_sample_pos_fast<ALIGN>(sc, dc, a.cx, a.cy, a.rcx, a.rcy, t.wf, t.hf, ix, iy);
            bad = ((den > 0.f) && (fabsf(ix) < 1e8f) && (fabsf(iy) < 1e8f)) ? 0 : 1;
            fxlo = fxhi = ix; fylo = fyhi = iy;
        }
        fxlo = fminf(fxlo, dpp_f<kXor1>(fxlo)); fxhi = fmaxf(fxhi, dpp_f<kXor1>(fxhi));
        fylo = fminf(fylo, dpp_f<kXor1>(fylo)); fyhi = fmaxf(fyhi, dpp_f<kXor1>(fyhi));
        bad |= dpp_i<kXor1>(bad);
        fxlo = fminf(fxlo, dpp_f<kXor2>(fxlo)); fxhi = fmaxf(fxhi, dpp_f<kXor2>(fxhi));
        fylo = fminf(fylo, dpp_f<kXor2>(fylo)); fyhi = fmaxf(fyhi, dpp_f<kXor2>(fyhi));
        bad |= dpp_i<kXor2>(bad);
        if (c < ke && cr == 0) {
            int4 b;
            // TIGHT box (round 5): a pixel's taps are texels floor(i) and floor(i) + 1; over the tile floor(i) ranges over
            // [floor(min), floor(max)] of the corner positions (convexity), so the box is [floor(min), floor(max) + 1] — with
            // 1/64 texel of guard for the fp32 evaluation of interior pixels against the corners' (their positions agree
            // with exact arithmetic to ~1e-4 texel).  Rounds 2-4 carried one more texel on every side: an 8x8 tile at unit
            // scale filled 11 x 11 = 121 texels per candidate instead of 9 x 9 = 81, and a patch held 2/3 of the candidates.
            const float mnx = fmaxf(fxlo, -4.f) - 0.015625f, mxx = fminf(fxhi, t.wf + 4.f) + 0.015625f;
            const float mny = fmaxf(fylo, -4.f) - 0.015625f, mxy = fminf(fyhi, t.hf + 4.f) + 0.015625f;
            b.x = min(max((int)floorf(mnx), -1), a.w - 1);
            b.y = min(max((int)floorf(mxx) + 1, b.x + 1), a.w);
            b.z = min(max((int)floorf(mny), -1), a.h - 1);
            b.w = min(max((int)floorf(mxy) + 1, b.z + 1), a.h);
            if (bad) { b.x = -(1 << 20); b.y = 1 << 20; b.z = -(1 << 20); b.w = 1 << 20; }   // unbounded: never fits
            t.boxes[c - kb] = b;                               // boxes[] is indexed relative to the pass
        }
    }
}

// ---- WAVE PRIORITY BY PROGRESS (round 5) ----
// The launch is one round of 3 workgroups per CU (768 tiles = 256 x 3 at config B) and a SIMD arbitrates its three waves by age:
// the workgroup dispatched first wins every contended issue slot, so the three finished at 350 / 420 / 480 k clocks whatever their
// tiles (the per-tile cost map has a period of exactly one dispatch round, profiles/r5_costvol_limits.txt) and the last one ran
// its final quarter alone on the CU, with nothing to hide its LDS latency behind.  s_setprio beats age: a workgroup's priority is
// 3 minus the quarter of its own (view, candidate) list it has finished, so whoever is ahead yields and the three stay within a
// quarter of each other.  230 -> 211 us.
__device__ __forceinline__ void quad_priority_by_progress(int done, int total, int& prio_q) {
    const int q = (4 * done) / total;
    if (q != prio_q) {
        prio_q = q;
        if (q <= 0) __builtin_amdgcn_s_setprio(3); else if (q == 1) __builtin_amdgcn_s_setprio(2);
        else if (q == 2) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
    }
}

// ---- longest run of the next candidates lo .. (up to 32, below ke) whose united footprint fits the patch ----
// Lane l < 32 of every wave holds the l-th next candidate, inclusive prefix union along the two 16-lane DPP rows (the second row
// joins the first row's total), every lane tests ITS prefix, and the run length is the number of leading lanes that fit — any
// length, not only 16 / 8 / 4 / 2 (round 5: one ballot instead of five rounds of four v_readlane + scalar compares; the
// selection took 8 % of a workgroup's time, profiles/r5_costvol_diag_before.txt).  Fewer than two that fit (a single candidate
// is never staged: file header, "tried and rejected"): one group of up to 4 straight from global memory.
__device__ __forceinline__ QuadRun quad_pick_run(const CostvolArgs& a, const QuadCtx& t, int lo, int kb, int ke) {
    const int nmax = min(kQRun, ke - lo);
    int4 bx = make_int4(1 << 30, -(1 << 30), 1 << 30, -(1 << 30));
    if (t.lane < nmax) bx = t.boxes[lo + t.lane - kb];
#define NRGBD_ROW_SHR_UNION(SH)                                                                                   \
    bx.x = min(bx.x, __builtin_amdgcn_update_dpp(1 << 30, bx.x, 0x110 + SH, 0xf, 0xf, false));              \
    bx.y = max(bx.y, __builtin_amdgcn_update_dpp(-(1 << 30), bx.y, 0x110 + SH, 0xf, 0xf, false));           \
    bx.z = min(bx.z, __builtin_amdgcn_update_dpp(1 << 30, bx.z, 0x110 + SH, 0xf, 0xf, false));              \
    bx.w = max(bx.w, __builtin_amdgcn_update_dpp(-(1 << 30), bx.w, 0x110 + SH, 0xf, 0xf, false));
    NRGBD_ROW_SHR_UNION(1) NRGBD_ROW_SHR_UNION(2) NRGBD_ROW_SHR_UNION(4) NRGBD_ROW_SHR_UNION(8)
#undef NRGBD_ROW_SHR_UNION
    if (nmax > 16) {                                   // block-uniform
        const int r0x = __builtin_amdgcn_readlane(bx.x, 15), r0y = __builtin_amdgcn_readlane(bx.y, 15);
        const int r0z = __builtin_amdgcn_readlane(bx.z, 15), r0w = __builtin_amdgcn_readlane(bx.w, 15);
        if (t.lane >= 16) { bx.x = min(bx.x, r0x); bx.y = max(bx.y, r0y); bx.z = min(bx.z, r0z); bx.w = max(bx.w, r0w); }
    }
    const int bwd = bx.y - bx.x + 1, bht = bx.w - bx.z + 1;      // 2^21 for an unbounded box: test the sides before the product
    const bool fit = t.lane < nmax && bwd <= kQPatch3 && bht <= kQPatch3 && bwd * bht <= kQPatch3;
    // prefix unions only grow, so the lanes that fit are a prefix of the wave: its length is the run
    QuadRun r;
    r.n = (int)__builtin_ctzll(~__ballot(fit));
    r.xlo = 0; r.xhi = 1; r.ylo = 0; r.yhi = 1;
    if (r.n >= 1) {
        r.xlo = __builtin_amdgcn_readlane(bx.x, r.n - 1); r.xhi = __builtin_amdgcn_readlane(bx.y, r.n - 1);
        r.ylo = __builtin_amdgcn_readlane(bx.z, r.n - 1); r.yhi = __builtin_amdgcn_readlane(bx.w, r.n - 1);
    }
    r.staged = r.n >= 2 && !NRGBD_DBG(a, 1);
    if (!r.staged) r.n = min(4, nmax);                 // one group straight from global memory
    r.cols = r.xhi - r.xlo + 1;
    return r;
}

// ---- one plane of the patch, L2 -> LDS without touching VGPRs ----
// A wave instruction drops PER texels in lane order = patch order: 4 x 256 B of the feature plane or 64 x 16 B of the RGB plane
// (1 KB either way); `inbyte` is the lane's byte inside the source texel.  A patch wholly inside the image (INTERIOR, the common
// case) needs no coordinate clamps: texel (qx, qy) of the patch is at base + qy * row pitch + qx * texel pitch.
template <bool INTERIOR, int PER>
__device__ __forceinline__ void quad_stage_plane(const CostvolArgs& a, const QuadCtx& t, const char* svb, const QuadRun& r, int area,
                                                 float inv_cols, int inbyte, char* dst) {
    const int cpb = a.Cp * 4, rowb = a.w * cpb;
    const unsigned base = (unsigned)((r.ylo * a.w + r.xlo) * cpb);
    for (int it = t.wave; it * PER < area; it += 4) {
        const int q = min(it * PER + t.lane / (64 / PER), area - 1);
        const int qy = (int)(((float)q + 0.5f) * inv_cols), qx = q - __mul24(qy, r.cols);
        unsigned off;                                          // 24-bit multiplies: full rate (a row pitch < 16 MB)
        if constexpr (INTERIOR) {
            off = base + (unsigned)(__mul24(qy, rowb) + __mul24(qx, cpb) + inbyte);
        } else {
            const int gx = min(max(r.xlo + qx, 0), a.w - 1), gy = min(max(r.ylo + qy, 0), a.h - 1);
            off = (unsigned)(__mul24(gy, rowb) + __mul24(gx, cpb) + inbyte);
        }
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(svb + off),
                                         (__attribute__((address_space(3))) void*)(dst + it * 1024), 16, 0, 0);
    }
}

// ---- stage the patch of a run: feature plane, then the RGB plane ----
template <bool INTERIOR, bool EXTRA>
__device__ __forceinline__ void quad_stage(const CostvolArgs& a, const QuadCtx& t, const float* sv, const QuadRun& r) {
    const int area = r.cols * (r.yhi - r.ylo + 1);
    const float inv_cols = 1.0f / (float)r.cols;       // q / cols = (int)((q + 0.5) * inv_cols): exact for q, cols <= 192
    const char* svb = reinterpret_cast<const char*>(sv);
    quad_stage_plane<INTERIOR, 4>(a, t, svb, r, area, inv_cols, (t.lane & 15) * 16, t.ldsF);
    if constexpr (EXTRA) quad_stage_plane<INTERIOR, 64>(a, t, svb, r, area, inv_cols, kQFeatBytes, t.ldsR);
}

// ---- one group of NI <= 4 candidates (lane j owns candidate k0 + j) for one view: the lane's cost of ITS candidate ----
// STAGED: taps from the LDS patch of run r; otherwise straight from global memory.  The NI x 4 (candidate, step) tap fetches run
// as one software pipeline, PD steps ahead of the math (LDS: 1, global memory: 2).
template <int DIST, int TAIL, bool ALIGN, bool STAGED, int NI>
__device__ __forceinline__ float quad_group(const CostvolArgs& a, const QuadCtx& t, const float* sv, const SweepTerm& st, int k0,
                                            int ncand, const QuadRun& r, bool& escaped) {
    constexpr bool EXTRA = TAIL != 0;
    constexpr int PD = STAGED ? 1 : 2;
    const int kc = min(k0 + t.j, k0 + ncand - 1);          // lanes beyond the group repeat its last candidate
    float ix, iy;
    sweep_sample_pos_fast<ALIGN>(st, t.dcand[kc], a.cx, a.cy, a.rcx, a.rcy, t.wf, t.hf, ix, iy);
    const TapW tw = tap_weights(ix, iy, t.wf, t.hf);
    // tap addresses: STAGED one patch address (apron => the 3 other taps are +256, +pitch, +pitch+256);
    // global: four clamped texel offsets
    int adr[4];
    if constexpr (STAGED) {
        const float xcl = fminf(fmaxf(tw.x0f, (float)r.xlo), (float)(r.xhi - 1));           // NaN -> xlo
        const float ycl = fminf(fmaxf(tw.y0f, (float)r.ylo), (float)(r.yhi - 1));
        const int xi = (int)xcl - r.xlo, yi = (int)ycl - r.ylo;
        adr[0] = __mul24(yi, r.cols) + xi;                // texel index in the patch
        // A tap with a non-zero weight that the clamp moved has LEFT the box the tile's corners predicted.  The box is exact for
        // the pinhole ray table of the reference (warping/View.py:16-62: rays affine in (x, y), z = 1 — a homography maps the convex
        // tile into the convex hull of its corners' images) and carries 1/64 texel of guard; another table (unit-norm or
        // distortion-corrected rays: the C ABI takes any) can bend a tile's image out of it.  Legitimate clamps — a box clipped to
        // the image's one-texel apron — only ever move taps whose weights are all zero.  The caller re-evaluates the group from
        // global memory when any lane of the wave reports an escape: 2 compares per (pixel, candidate).
        escaped = tw.any() && ((xcl != tw.x0f) || (ycl != tw.y0f));
        adr[1] = adr[2] = adr[3] = 0;
    } else {
        const int xa = (int)fminf(fmaxf(tw.x0f, 0.f), t.wf - 1.f), xb = (int)fminf(fmaxf(tw.x0f + 1.f, 0.f), t.wf - 1.f);
        const int ya = (int)fminf(fmaxf(tw.y0f, 0.f), t.hf - 1.f), yb = (int)fminf(fmaxf(tw.y0f + 1.f, 0.f), t.hf - 1.f);
        const int cpb = a.Cp * 4;
        const int ra = __mul24(ya, a.w), rb = __mul24(yb, a.w);          // 24-bit multiplies (full rate): h * w < 2^24, checked by the launcher
        adr[0] = __mul24(ra + xa, cpb); adr[1] = __mul24(ra + xb, cpb);
        adr[2] = __mul24(rb + xa, cpb); adr[3] = __mul24(rb + xb, cpb);
    }
    const int pitchB = r.cols * kQFeatBytes;
    const char* gsv = reinterpret_cast<const char*>(sv);

    // broadcast tap addresses of the NI candidates (item I = the candidate lane I of the quad prepared)
    int ib[NI][STAGED ? 1 : 4];
    static_for<NI>([&](auto ic) {
        constexpr int I = decltype(ic)::value;
        if constexpr (STAGED) {
            ib[I][0] = dpp_i<kBcast<I>>(adr[0]) * kQFeatBytes;
        } else {
#pragma unroll
            for (int tp = 0; tp < 4; ++tp) ib[I][tp] = dpp_i<kBcast<I>>(adr[tp]);
        }
    });
    f32x4 buf[PD + 1][4];
    auto issue = [&](auto sc) {
        constexpr int S = decltype(sc)::value;
        constexpr int I = S >> 2, s4 = S & 3, slot = S % (PD + 1);
        if constexpr (STAGED) {
            const char* t0 = t.ldsF + ib[I][0] + t.cofs[s4];
            const char* t1 = t0 + pitchB;
            buf[slot][0] = *reinterpret_cast<const f32x4*>(t0);
            buf[slot][1] = *reinterpret_cast<const f32x4*>(t0 + kQFeatBytes);
            buf[slot][2] = *reinterpret_cast<const f32x4*>(t1);
            buf[slot][3] = *reinterpret_cast<const f32x4*>(t1 + kQFeatBytes);
        } else {
#pragma unroll
            for (int tp = 0; tp < 4; ++tp)
                buf[slot][tp] = *reinterpret_cast<const f32x4*>(gsv + (unsigned)(ib[I][tp] + t.cofs[s4]));
        }
    };
    static_for<(PD < NI * 4 ? PD : NI * 4)>([&](auto sc) { issue(sc); });

    // RGB word of this lane's own candidate (its four taps by this lane alone), overlapped with the first fetches
    float rgbpart = 0.f;
    if constexpr (EXTRA) {
        f32x4 A, B, C, Dd;
        if constexpr (STAGED) {
            const char* r0 = t.ldsR + adr[0] * 16;
            const char* r1 = r0 + r.cols * 16;
            A = *reinterpret_cast<const f32x4*>(r0); B = *reinterpret_cast<const f32x4*>(r0 + 16);
            C = *reinterpret_cast<const f32x4*>(r1); Dd = *reinterpret_cast<const f32x4*>(r1 + 16);
        } else {
            const char* g = gsv + kQFeatBytes;
            A = *reinterpret_cast<const f32x4*>(g + (unsigned)adr[0]); B = *reinterpret_cast<const f32x4*>(g + (unsigned)adr[1]);
            C = *reinterpret_cast<const f32x4*>(g + (unsigned)adr[2]); Dd = *reinterpret_cast<const f32x4*>(g + (unsigned)adr[3]);
        }
        rgbpart = rgb_word<DIST>(A, B, C, Dd, t.rgbref, tw, t.tail);
    }

    float keep = 0.f;
    f32x2 wnw, wne, wsw, wse, pa, pb;
    static_for<NI * 4>([&](auto sc) {
        constexpr int S = decltype(sc)::value;
        constexpr int I = S >> 2, s4 = S & 3, slot = S % (PD + 1);
        if constexpr (S + PD < NI * 4) issue(std::integral_constant<int, S + PD>{});
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (s4 == 0) {
            const float bnw = dpp_f<kBcast<I>>(tw.nw), bne = dpp_f<kBcast<I>>(tw.ne);
            const float bsw = dpp_f<kBcast<I>>(tw.sw), bse = dpp_f<kBcast<I>>(tw.se);
            wnw = f32x2{bnw, bnw}; wne = f32x2{bne, bne}; wsw = f32x2{bsw, bsw}; wse = f32x2{bse, bse};
            pa = f32x2{0.f, 0.f}; pb = f32x2{0.f, 0.f};
        }
        word_acc<DIST>(buf[slot][0], buf[slot][1], buf[slot][2], buf[slot][3], t.rr[s4], wnw, wne, wsw, wse, pa, pb);
        if constexpr (s4 == 3) {
            const f32x2 pc = pa + pb;
            float part = pc.x + pc.y;
            part = part + dpp_f<kXor1>(part);              // quad reduction: all four lanes end with the channel sum
            part = part + dpp_f<kXor2>(part);
            keep = (t.j == I) ? part : keep;
        }
        __builtin_amdgcn_sched_barrier(0);
    });
    return keep + rgbpart;
}

// ---- a group of nc candidates of run r: from the patch when the run is staged, and once more from global memory when a tap of
// any lane of the wave escaped the patch's box (`redone`) ----
template <int DIST, int TAIL, bool ALIGN>
__device__ __forceinline__ float quad_group_cost(const CostvolArgs& a, const QuadCtx& t, const float* sv, const SweepTerm& st,
                                                 int k0, int nc, const QuadRun& r, bool& redone) {
    float acc = 0.f;
    bool esc = false, from_lds = r.staged;
#pragma unroll 1
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (!from_lds) { acc = quad_group<DIST, TAIL, ALIGN, false, 4>(a, t, sv, st, k0, nc, r, esc); break; }
        if (nc == 1) acc = quad_group<DIST, TAIL, ALIGN, true, 1>(a, t, sv, st, k0, 1, r, esc);
        else if (nc == 2) acc = quad_group<DIST, TAIL, ALIGN, true, 2>(a, t, sv, st, k0, 2, r, esc);
        else if (nc == 3) acc = quad_group<DIST, TAIL, ALIGN, true, 3>(a, t, sv, st, k0, 3, r, esc);
        else acc = quad_group<DIST, TAIL, ALIGN, true, 4>(a, t, sv, st, k0, 4, r, esc);
        if (__ballot(esc) == 0) break;          // wave-uniform: the 16 quads of a wave redo the group together
        redone = true;
        from_lds = false;                       // a tap escaped the footprint box: this group straight from global memory
    }
    return acc;
}

// ---- the pass kb .. ke - 1 is complete: its costs leave the LDS once (no read-modify-write per view: -3 reads and -3 writes of
// D x hw floats) ----
__device__ __forceinline__ void quad_flush_pass(const CostvolArgs& a, const QuadCtx& t, float* out, int kb, int ke) {
    for (int idx = t.tid; idx < 64 * (ke - kb); idx += 256) {
        const int kk = idx >> 6, q = idx & 63;
        const int xq = t.tx * kQT + (q & 7), yq = t.ty * kQT + (q >> 3);
        if (xq < a.w && yq < a.h) out[(size_t)(kb + kk) * t.hw + (size_t)yq * a.w + xq] = t.ldsA[q * kQAccPitch + kk];
    }
}

// ---- log_softmax(-cost) over the D candidates of the tile's pixels (models/basic.py:299-300) ----
// thread = (pixel, quarter of the candidates): KMAX candidates per thread — 16 for D <= 64 (the path's configs S / B / K; the
// D <= 128 instantiation spent half of its unrolled iterations on candidates that do not exist), 32 for D <= 128 (config H when
// unchunked).  The costs were written by other lanes of THIS workgroup: the caller has made the stores visible (L2), they are
// read past the L1.
template <int KMAX>
__device__ __forceinline__ void quad_softmax(const CostvolArgs& a, const QuadCtx& t, const float* out) {
    float* red = reinterpret_cast<float*>(t.ldsF);     // the patch is dead by now
    const int pp = t.tid & 63, part = t.tid >> 6;
    const int x2 = t.tx * kQT + (pp & 7), y2 = t.ty * kQT + (pp >> 3);
    const bool in2 = (x2 < a.w) && (y2 < a.h);
    const size_t p2 = (size_t)min(y2, a.h - 1) * a.w + min(x2, a.w - 1);
    float col[KMAX];
    float m = -INFINITY;
#pragma unroll
    for (int u = 0; u < KMAX; ++u) {
        const int k = part + 4 * u;
        col[u] = (k < a.D) ? -__builtin_nontemporal_load(out + (size_t)k * t.hw + p2) : -INFINITY;
        m = fmaxf(m, col[u]);
    }
    red[part * 64 + pp] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[pp], red[64 + pp]), fmaxf(red[128 + pp], red[192 + pp]));
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < KMAX; ++u)
        if (part + 4 * u < a.D) s += expf(col[u] - m);
    red[256 + part * 64 + pp] = s;
    __syncthreads();
    s = (red[256 + pp] + red[256 + 64 + pp]) + (red[256 + 128 + pp] + red[256 + 192 + pp]);
    const float ls = logf(s);
    if (in2) {
#pragma unroll
        for (int u = 0; u < KMAX; ++u) {
            const int k = part + 4 * u;
            if (k < a.D) a.out_logp[(size_t)k * t.hw + p2] = (col[u] - m) - ls;
        }
    }
}

}  // namespace

// TAIL: valid channels of the texel's 17th word (Cp = 68: channels 64..66 = pooled RGB => 3; -1 = a.C - 64 at run time);
// 0 = no 17th word (Cp = 64).  ALIGN: grid_sample's align_corners.
//
// Loop order: passes of kQPass candidates > views > runs > groups of 4.  Views OUTSIDE the runs: all workgroups of an XCD (one
// band of tiles) sweep the same source view at about the same time, so the band's footprint in ONE view (~2 MB) is what has to
// live in the 4 MB L2 — with the views inside the candidate loop it would be all V of them (~9 MB) and every patch fill would go
// to the fabric.  The price is that a candidate's cost has to be accumulated across views: in the LDS accumulators of the pass
// (t.ldsA), by the lane that owns the candidate in each view; they leave for global memory once at the end of the pass.
template <int DIST, int TAIL, bool ALIGN>
__global__ __launch_bounds__(256, 3) void costvol_quad(const CostvolArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    CVT_DECL
    int tile, chunk;
    quad_tile_of_block(a, tile, chunk);
    const QuadCtx t = quad_prologue<TAIL>(a, smem, tile);
    const int kb_all = chunk * a.kchunk, ke_all = min(a.D, kb_all + a.kchunk);   // this workgroup's candidates
    const float rx = a.rays[t.p], ry = a.rays[t.hw + t.p], rz = a.rays[2 * t.hw + t.p];
    float* out = a.out_cost ? a.out_cost : a.out_logp;

    int prio_q = -1;
    for (int kb = kb_all; kb < ke_all; kb += kQPass) {
        const int ke = min(ke_all, kb + kQPass);
        for (int v = 0; v < a.V; ++v) {
            const float* KRv = a.KR + 9 * v;
            const float* Ktv = a.Kt + 3 * v;
            const float* sv = a.src + (size_t)v * t.hw * a.Cp;
            const SweepTerm st = make_sweep_term(KRv, Ktv, rx, ry, rz);
            CVT_BEGIN();
            __syncthreads();                                   // the previous view's boxes / the prologue's dcand
            quad_boxes<ALIGN>(a, t, KRv, Ktv, kb, ke);
            __syncthreads();
            CVT_END(3);
            for (int lo = kb, n; lo < ke; lo += n) {
                quad_priority_by_progress(a.V * (kb - kb_all) + v * (ke - kb) + (lo - kb), a.V * (ke_all - kb_all), prio_q);
                CVT_BEGIN();
                const QuadRun r = quad_pick_run(a, t, lo, kb, ke);
                n = r.n;
                CVT_END(4);
                if (r.staged) { CVT_COUNT(n >= 16 ? 10 : n >= 8 ? 11 : n >= 4 ? 12 : 13, 1); CVT_COUNT(15, n); CVT_COUNT(19, (long long)r.cols * (r.yhi - r.ylo + 1)); } else CVT_COUNT(14, 1);

                if (r.staged) {
                    CVT_BEGIN();
                    __syncthreads();                           // the previous patch has been read by every wave
                    CVT_END(16);
                    CVT_BEGIN();
                    if (r.xlo >= 0 && r.ylo >= 0 && r.xhi <= a.w - 1 && r.yhi <= a.h - 1)   // block-uniform
                        quad_stage<true, TAIL != 0>(a, t, sv, r);
                    else
                        quad_stage<false, TAIL != 0>(a, t, sv, r);
                    CVT_END(5);
                    CVT_BEGIN();
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                    CVT_END(6);
                }
                CVT_BEGIN();
                if (!NRGBD_DBG(a, 2)) {
#pragma unroll 1
                    for (int g = 0; g < (n + 3) >> 2; ++g) {
                        const int k0 = lo + 4 * g, nc = min(4, n - 4 * g);
                        float* o = t.ldsA + t.quad * kQAccPitch + (min(k0 + t.j, ke - 1) - kb);   // this lane's candidate of the group; a quad is inside one wave: in-order LDS
                        const float prev = (v > 0) ? *o : 0.f;
                        bool redone = false;
                        const float acc = quad_group_cost<DIST, TAIL, ALIGN>(a, t, sv, st, k0, nc, r, redone);
                        if (redone) CVT_COUNT(20, 1);
                        if (t.j < nc) *o = prev + div_by_const(acc, a.sigma, a.rsigma);               // homography.py:325 (/ sigma), views in order
                    }
                }
                if (r.staged) CVT_END(7); else CVT_END(8);
            }
        }
        __syncthreads();
        quad_flush_pass(a, t, out, kb, ke);
        __syncthreads();                                       // the accumulators are free for the next pass
    }

    if (!a.fuse_softmax) { CVT_FLUSH(); return; }
    CVT_BEGIN();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     // the costs were written by other lanes of this workgroup
    __syncthreads();
    if (a.D <= 64) quad_softmax<16>(a, t, out); else quad_softmax<32>(a, t, out);
    CVT_END(9);
    CVT_FLUSH();
}

bool costvol_quad_supported(const CostvolArgs& a) {
    const bool extra = a.Cp == 68 && a.C > 64;
    const bool plain = a.Cp == 64 && a.C == 64;
    // 32-bit byte offsets into a view; the LDS image (patch + 20 B per candidate + accumulators) has to fit a workgroup's share
    // ... and a row pitch below 8 MB and fewer than 2^23 pixels: the address arithmetic uses __mul24, a SIGNED 24-bit multiply whose
    // operands must stay below 2^23 (a pitch in [8, 16) MB would be sign-extended to a negative offset)
    return (extra || plain) && (long)a.h * a.w * a.Cp * 4 < (1L << 31) && (long)a.w * a.Cp * 4 < (1L << 23) && (long)a.h * a.w < (1L << 23) && a.D <= NRGBD_MAX_D;
}

// Returns NRGBD_OK and sets *did_softmax when the launch also produced out_logp.
int launch_costvol_quad(const CostvolArgs& args, hipStream_t stream, bool* did_softmax) {
    CostvolArgs a = args;
    const int tiles = ceil_div(a.w, kQT) * ceil_div(a.h, kQT);
    // one workgroup per tile owns all D candidates when that fills the chip (3 workgroups per CU); smaller grids split the
    // candidates into chunks (>= 8 each) so that every CU has work, and leave the log-softmax to its own launch
    int nchunk = 1;
    while (tiles * nchunk < 3 * 256 && ceil_div(a.D, nchunk * 2) >= 8) nchunk *= 2;
    if (const int forced = dev_env_int("NRGBD_QUAD_CHUNKS")) nchunk = forced;   // developer builds only
    a.nchunk = nchunk;
    a.kchunk = ceil_div(a.D, nchunk);
    a.fuse_softmax = (nchunk == 1 && a.out_logp != nullptr && a.D <= 128) ? 1 : 0;
    *did_softmax = a.fuse_softmax != 0;
    const int patch = kQPatch3;
    const size_t lds = (size_t)patch * kQFeatBytes + (size_t)((patch + 63) / 64 * 64) * 16 + (size_t)kQPass * sizeof(int4) +
                       (size_t)((a.D + 3) & ~3) * sizeof(float) + (size_t)64 * kQAccPitch * sizeof(float);
    const dim3 grid(tiles * nchunk);
    const int tail = a.Cp == 68 ? (a.C - 64 == 3 ? 3 : -1) : 0;
    const bool al = a.align != 0;
    hipError_t e = hipSuccess;
#define NRGBD_QUAD_CFG(DIST, TL, AL)                                                                                           \
    do {                                                                                                                       \
        if (lds > 64 * 1024) {                                                                                                 \
            e = set_max_dynamic_lds(reinterpret_cast<const void*>(&costvol_quad<DIST, TL, AL>),                   \
                                    (int)lds);                                     \
            if (e != hipSuccess) return (int)e;                                                                                \
        }                                                                                                                      \
        hipLaunchKernelGGL((costvol_quad<DIST, TL, AL>), grid, dim3(256), lds, stream, a);                        \
    } while (0)
#define NRGBD_QUAD_DISPATCH(DIST)                                                                   \
    if (tail == 3) { if (al) NRGBD_QUAD_CFG(DIST, 3, true); else NRGBD_QUAD_CFG(DIST, 3, false); }        \
    else if (tail == 0) { if (al) NRGBD_QUAD_CFG(DIST, 0, true); else NRGBD_QUAD_CFG(DIST, 0, false); }   \
    else { if (al) NRGBD_QUAD_CFG(DIST, -1, true); else NRGBD_QUAD_CFG(DIST, -1, false); }
    if (a.dist == NRGBD_DIST_L2) { NRGBD_QUAD_DISPATCH(NRGBD_DIST_L2) } else { NRGBD_QUAD_DISPATCH(NRGBD_DIST_L1) }
#undef NRGBD_QUAD_DISPATCH
#undef NRGBD_QUAD_CFG
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

}  // namespace nrgbd
