// icp.hip — frame-to-model tracking: a depth frame registered against the fused TSDF volume's ray cast (tsdf_raycast.hip) by
// point-to-plane ICP with projective data association (neuralrgbd_amd/tracking.py: FrameTracker; fusion.py: TSDFVolume.track,
// FusionVideoStream(track=True)).
//
// No counterpart in the reference, which takes its poses from an external odometry.  The operation sequence per pixel and per solve
// is written out in include/nrgbd.h and restated in numpy by tests/icp_ref.py: fp32 per pixel, double from the promoted values on,
// one IEEE operation per operation of the header (the library is built with -ffp-contract=off), no atomics, no library function.
// One Gauss-Newton iteration is two launches on the caller's stream; nothing is read back between iterations.
//
// icp_terms_kernel   one visited pixel per lane and grid-stride step: association, residual, and the lane's 28 double sums (the
//                    upper triangle of A = sum w J J^T, g = sum w J r, E = sum w r r) with statically indexed predicated adds, a
//                    count; then the workgroup's record in a fixed order — the folded wave64 shuffle tree depth_eval.hip uses
//                    (wave_fold.hpp: wave_fold_sum, here for 32 values), then the 4 wave sums through LDS in wave order —
//                    written with plain vector stores.  The pixels of a lane depend on (Hs, Ws) alone, so the same inputs give the same bits.
//                    Streams the frame's depth (and gate) and gathers from the two model maps; launch- and latency-bound at the
//                    sizes of a tracker's pyramid, not by bytes.  template <bool PHOTO>: false is nrgbd_icp_terms_f32, bit for bit what
//                    it was; true (nrgbd_icp_terms_photo_f32) adds, for a pixel that kept its geometric pair, one intensity residual
//                    against the model's rendered colour (tsdf_raycast.hip, rgb) to the same 28 sums: the 16 neighbour gathers and
//                    the 3 frame reads are requested together under the pair's predicate, before the first is used.
// icp_update_kernel  one workgroup.  step 0: the state from the caller's initial motion.  step >= 1: the records are staged in LDS
//                    (coalesced loads, all in flight: read one after the other from memory the 256 records of a large map cost
//                    96 us per step, over half of a track), a lane per value adds them in index order; lane 0 tests, factorises
//                    A = L D L^T, solves, forms the rotation of the step from fixed Taylor polynomials and composes it onto the
//                    state, in double; the fp32 copy the next icp_terms reads is rounded once.
#include <type_traits>

#include "common.hpp"
#include "wave_fold.hpp"

namespace nrgbd {

constexpr int kIcpMaxWg = NRGBD_ICP_MAX_WG;
constexpr int kIcpSums = 28;                                   // 21 (A, i <= j, row-major) + 6 (g) + 1 (E)
constexpr int kIcpRecord = NRGBD_ICP_RECORD_BYTES / 8;         // 30 words: the sums, the int64 count, one word of padding (PHOTO: the
                                                               // int64 count of photometric pairs)
constexpr float kIcpFltMax = 3.402823466e+38f;
constexpr int kIcpMaxSide = 1 << 15;

struct IcpState {                                              // NRGBD_ICP_STATE_BYTES
    double T[12];                                              // the motion frame camera -> model camera, [3][4] row-major
    float Tf[12];                                              // the same, rounded once
    int flag, iterations;
};
static_assert(sizeof(IcpState) == NRGBD_ICP_STATE_BYTES, "the state's layout is part of the interface");

struct IcpTermsArgs {
    const float* depth; const float* gate; const float* mdepth; const float* mnormal; const IcpState* state;
    double* partial; float* resid;
    int H, W, Hs, Ws, sub, Hm, Wm;
    float gate_thr, d_near, d_far, fx, fy, cx, cy, fxm, fym, cxm, cym, dist_thr, huber;
};

struct IcpPhotoArgs {                                          // what the photometric term adds
    const float* image; const float* mrgb; float* resid_photo;
    float aff_a[3], aff_b[3], photo_weight, photo_huber;
};
struct IcpNoPhotoArgs {};
template <bool PHOTO> using IcpPhotoArgsOf = typename std::conditional<PHOTO, IcpPhotoArgs, IcpNoPhotoArgs>::type;

__device__ __forceinline__ float icp_luma(float c0, float c1, float c2) { return (0.299f * c0 + 0.587f * c1) + 0.114f * c2; }

template <bool PHOTO>
__global__ __launch_bounds__(256) void icp_terms_kernel(const IcpTermsArgs a, const IcpPhotoArgsOf<PHOTO> ph) {
    constexpr int NF = 32;                                     // the 28 sums padded to the fold's width
    __shared__ double w_sum[4][NF];
    __shared__ int w_cnt[4];
    [[maybe_unused]] __shared__ int w_pcnt[4];
    const float qnan = __builtin_nanf("");
    const long stride = (long)gridDim.x * 256;
    const long first = (long)blockIdx.x * 256 + threadIdx.x;
    float* resid_photo = nullptr;
    if constexpr (PHOTO) resid_photo = ph.resid_photo;
    if (a.resid || resid_photo) {                              // the pixels no lane visits: a quiet NaN
        const long n = (long)a.H * a.W;
        const int half = a.sub / 2;
        for (long p = first; p < n; p += stride) {
            const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);
            const bool visited = y % a.sub == half && x % a.sub == half && y / a.sub < a.Hs && x / a.sub < a.Ws;
            if (!visited) {
                if (a.resid) a.resid[p] = qnan;
                if (resid_photo) resid_photo[p] = qnan;
            }
        }
    }
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = a.state->Tf[i];
    const float thr2 = a.dist_thr * a.dist_thr;
    const size_t mplane = (size_t)a.Hm * (size_t)a.Wm;
    double acc[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) acc[i] = 0.0;
    int cnt = 0;
    [[maybe_unused]] int pcnt = 0;
    const long ns = (long)a.Hs * a.Ws;
    for (long p = first; p < ns; p += stride) {
        const int j = (int)(p / a.Ws), i = (int)(p - (long)j * a.Ws);
        const int y = a.sub * j + a.sub / 2, x = a.sub * i + a.sub / 2;
        const size_t at = (size_t)y * (size_t)a.W + (size_t)x;
        const float d = a.depth[at];
        bool ok = d > a.d_near && d <= a.d_far && d <= kIcpFltMax;                  // a NaN fails
        if (ok && a.gate) ok = a.gate[at] >= a.gate_thr;
        float J[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float r = 0.f, w = 0.f;
        [[maybe_unused]] float pq[3] = {0.f, 0.f, 1.f}, puv[2] = {0.f, 0.f}, pdm = 0.f;      // PHOTO: the pair's q, (u, v) and dm
        if (ok) {
            const float xn = (((float)x + 0.5f) - a.cx) / a.fx;
            const float yn = (((float)y + 0.5f) - a.cy) / a.fy;
            const float px = xn * d, py = yn * d, pz = d;
            const float qx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
            const float qy = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
            const float qz = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
            ok = qz > 0.f;
            if (ok) {
                const float u = a.fxm * (qx / qz) + a.cxm;
                const float v = a.fym * (qy / qz) + a.cym;
                if constexpr (PHOTO) {
                    pq[0] = qx; pq[1] = qy; pq[2] = qz; puv[0] = u; puv[1] = v;
                }
                ok = u >= 0.f && u < (float)a.Wm && v >= 0.f && v < (float)a.Hm;      // a NaN fails
                if (ok) {
                    const int iu = (int)floorf(u), iv = (int)floorf(v);
                    const size_t am = (size_t)iv * (size_t)a.Wm + (size_t)iu;
                    const float dm = a.mdepth[am];
                    if constexpr (PHOTO) pdm = dm;
                    const float nx = a.mnormal[am], ny = a.mnormal[mplane + am], nz = a.mnormal[2 * mplane + am];
                    const bool zero = nx == 0.f && ny == 0.f && nz == 0.f;
                    const bool finite = fabsf(nx) <= kIcpFltMax && fabsf(ny) <= kIcpFltMax && fabsf(nz) <= kIcpFltMax;
                    ok = dm > 0.f && !zero && finite;
                    if (ok) {
                        const float mx = ((((float)iu + 0.5f) - a.cxm) / a.fxm) * dm;
                        const float my = ((((float)iv + 0.5f) - a.cym) / a.fym) * dm;
                        const float ex = qx - mx, ey = qy - my, ez = qz - dm;
                        ok = (ex * ex + ey * ey) + ez * ez <= thr2;                   // a NaN fails
                        r = (nx * ex + ny * ey) + nz * ez;
                        J[0] = nx; J[1] = ny; J[2] = nz;
                        J[3] = qy * nz - qz * ny;
                        J[4] = qz * nx - qx * nz;
                        J[5] = qx * ny - qy * nx;
                        const float ar = fabsf(r);
                        w = ar <= a.huber ? 1.f : a.huber / ar;
                    }
                }
            }
        }
        if (a.resid) a.resid[at] = ok ? r : qnan;
        if (ok) {
            const double wd = (double)w, rd = (double)r;
            int k = 0;
#pragma unroll
            for (int i0 = 0; i0 < 6; ++i0) {
#pragma unroll
                for (int j0 = i0; j0 < 6; ++j0) acc[k++] += wd * ((double)J[i0] * (double)J[j0]);
            }
#pragma unroll
            for (int i0 = 0; i0 < 6; ++i0) acc[21 + i0] += wd * ((double)J[i0] * rd);
            acc[27] += wd * (rd * rd);
            cnt += 1;
        }
        if constexpr (PHOTO) {                                     // the intensity residual of a pixel that kept its pair
            const float qx = pq[0], qy = pq[1], qz = pq[2], dm = pdm;
            const float xq = qx / qz, yq = qy / qz;                // the quotients u and v were formed from
            const float ub = puv[0] - 0.5f, vb = puv[1] - 0.5f;
            const float x0 = floorf(ub), y0 = floorf(vb);
            bool pok = ok && x0 >= 0.f && x0 + 1.f <= (float)(a.Wm - 1) && y0 >= 0.f && y0 + 1.f <= (float)(a.Hm - 1);
            float Ji[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            float ri = 0.f, wi = 0.f;
            if (pok) {
                const size_t fplane = (size_t)a.H * (size_t)a.W;
                const size_t a00 = (size_t)(int)y0 * (size_t)a.Wm + (size_t)(int)x0, a01 = a00 + (size_t)a.Wm;
                // the 19 reads, all requested before the first is used
                const float f0 = ph.image[at], f1 = ph.image[fplane + at], f2 = ph.image[2 * fplane + at];
                const float d00 = a.mdepth[a00], d10 = a.mdepth[a00 + 1], d01 = a.mdepth[a01], d11 = a.mdepth[a01 + 1];
                const float r00 = ph.mrgb[a00], r10 = ph.mrgb[a00 + 1], r01 = ph.mrgb[a01], r11 = ph.mrgb[a01 + 1];
                const float g00 = ph.mrgb[mplane + a00], g10 = ph.mrgb[mplane + a00 + 1];
                const float g01 = ph.mrgb[mplane + a01], g11 = ph.mrgb[mplane + a01 + 1];
                const float b00 = ph.mrgb[2 * mplane + a00], b10 = ph.mrgb[2 * mplane + a00 + 1];
                const float b01 = ph.mrgb[2 * mplane + a01], b11 = ph.mrgb[2 * mplane + a01 + 1];
                const float Lf = icp_luma(f0 * ph.aff_a[0] + ph.aff_b[0], f1 * ph.aff_a[1] + ph.aff_b[1], f2 * ph.aff_a[2] + ph.aff_b[2]);
                const float L00 = icp_luma(r00, g00, b00), L10 = icp_luma(r10, g10, b10);
                const float L01 = icp_luma(r01, g01, b01), L11 = icp_luma(r11, g11, b11);
                const bool seen = d00 > 0.f && d10 > 0.f && d01 > 0.f && d11 > 0.f && fabsf(d00 - dm) <= a.dist_thr &&
                                  fabsf(d10 - dm) <= a.dist_thr && fabsf(d01 - dm) <= a.dist_thr && fabsf(d11 - dm) <= a.dist_thr;   // a NaN fails
                const bool finite = fabsf(Lf) <= kIcpFltMax && fabsf(L00) <= kIcpFltMax && fabsf(L10) <= kIcpFltMax &&
                                    fabsf(L01) <= kIcpFltMax && fabsf(L11) <= kIcpFltMax;
                pok = seen && finite;
                const float fu = ub - x0, fv = vb - y0;
                const float gu0 = L10 - L00, gu1 = L11 - L01;
                const float Im = (1.f - fv) * (L00 + fu * gu0) + fv * (L01 + fu * gu1);
                const float gu = (1.f - fv) * gu0 + fv * gu1;
                const float gv = (1.f - fu) * (L01 - L00) + fu * (L11 - L10);
                ri = Im - Lf;
                const float ax = (gu * a.fxm) / qz, ay = (gv * a.fym) / qz;
                const float az = -(ax * xq + ay * yq);
                Ji[0] = ax; Ji[1] = ay; Ji[2] = az;
                Ji[3] = qy * az - qz * ay;
                Ji[4] = qz * ax - qx * az;
                Ji[5] = qx * ay - qy * ax;
                const float ar = fabsf(ri);
                wi = ar <= ph.photo_huber ? ph.photo_weight : ph.photo_weight * (ph.photo_huber / ar);
            }
            if (resid_photo) resid_photo[at] = pok ? ri : qnan;
            if (pok) {
                const double wd = (double)wi, rd = (double)ri;
                int k = 0;
#pragma unroll
                for (int i0 = 0; i0 < 6; ++i0) {
#pragma unroll
                    for (int j0 = i0; j0 < 6; ++j0) acc[k++] += wd * ((double)Ji[i0] * (double)Ji[j0]);
                }
#pragma unroll
                for (int i0 = 0; i0 < 6; ++i0) acc[21 + i0] += wd * ((double)Ji[i0] * rd);
                acc[27] += wd * (rd * rd);
                pcnt += 1;
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    wave_fold_sum<double, NF>(acc, lane);
    if ((lane & 3) == 0) {
#pragma unroll
        for (int i = 0; i < NF / 16; ++i) w_sum[wave][fold_index<NF>(lane, i)] = acc[i];
    }
    cnt = wave_sum(cnt);
    if (lane == 0) w_cnt[wave] = cnt;
    if constexpr (PHOTO) {
        pcnt = wave_sum(pcnt);
        if (lane == 0) w_pcnt[wave] = pcnt;
    }
    __syncthreads();
    const int v = threadIdx.x;
    double* rec = a.partial + (size_t)blockIdx.x * kIcpRecord;
    if (v < kIcpSums)
        rec[v] = ((w_sum[0][v] + w_sum[1][v]) + w_sum[2][v]) + w_sum[3][v];
    else if (v == kIcpSums)
        ((long long*)rec)[v] = (((long long)w_cnt[0] + w_cnt[1]) + w_cnt[2]) + w_cnt[3];
    else if (v == kIcpSums + 1) {
        if (PHOTO)
            ((long long*)rec)[v] = (((long long)w_pcnt[0] + w_pcnt[1]) + w_pcnt[2]) + w_pcnt[3];
        else
            rec[v] = 0.0;                                      // the padding word
    }
}

struct IcpUpdateArgs {
    IcpState* state; const double* partial; double* log;
    double init[12];
    double min_pivot;
    long long min_pairs;
    int step, nwg;
};

// sin(x) / x and (1 - cos(x)) / x^2 as polynomials of degree 8 in t = x^2, Horner: coefficient k is (-1)^k / (2k + 1)! and
// (-1)^k / (2k + 2)! (the factorials up to 18! are exact in double; one IEEE division each, folded at compile time)
__device__ __forceinline__ void icp_sinc_cosc(double t, double& sa, double& cb) {
    const double ca[9] = {1.0, -1.0 / 6.0, 1.0 / 120.0, -1.0 / 5040.0, 1.0 / 362880.0, -1.0 / 39916800.0, 1.0 / 6227020800.0,
                          -1.0 / 1307674368000.0, 1.0 / 355687428096000.0};
    const double cc[9] = {1.0 / 2.0, -1.0 / 24.0, 1.0 / 720.0, -1.0 / 40320.0, 1.0 / 3628800.0, -1.0 / 479001600.0,
                          1.0 / 87178291200.0, -1.0 / 20922789888000.0, 1.0 / 6402373705728000.0};
    sa = ca[8];
    cb = cc[8];
#pragma unroll
    for (int k = 7; k >= 0; --k) {
        sa = sa * t + ca[k];
        cb = cb * t + cc[k];
    }
}

__device__ __forceinline__ bool icp_finite(double x) { return fabs(x) <= 1.7976931348623157e+308; }      // a NaN fails

// value v of the nwg staged records added in index order, ((rec_0 + rec_1) + rec_2) + ...: sixteen LDS reads in flight, then their
// additions in order (a record past the end is not added: s + 0.0 would turn a -0.0 into +0.0)
template <typename T, typename Load>
__device__ __forceinline__ T icp_add_records(const double* stage, int nwg, int v, Load load) {
    T s = load(stage[v]);
    for (int b0 = 1; b0 < nwg; b0 += 16) {
        T x[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = load(stage[(size_t)min(b0 + k, nwg - 1) * kIcpRecord + v]);
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (b0 + k < nwg) s += x[k];
    }
    return s;
}

__global__ __launch_bounds__(256) void icp_update_kernel(const IcpUpdateArgs a) {
    __shared__ double stage[kIcpMaxWg * kIcpRecord];            // the records, staged with coalesced loads: 60 KB
    __shared__ double S[kIcpSums];
    __shared__ long long count_s;
    const int t = threadIdx.x;
    if (a.step == 0) {
        if (t < 12) {
            a.state->T[t] = a.init[t];
            a.state->Tf[t] = (float)a.init[t];
        } else if (t == 12) {
            a.state->flag = 0;
        } else if (t == 13) {
            a.state->iterations = 0;
        }
        return;
    }
    for (int i = t; i < a.nwg * kIcpRecord; i += 256) stage[i] = a.partial[i];
    __syncthreads();
    if (t < kIcpSums)
        S[t] = icp_add_records<double>(stage, a.nwg, t, [](double x) { return x; });
    else if (t == 64)                                           // another wave: the count's adds run beside the sums'
        count_s = icp_add_records<long long>(stage, a.nwg, kIcpSums, [](double x) { return __double_as_longlong(x); });
    __syncthreads();
    if (t != 0) return;
    const long long count = count_s;
    double* row = a.log + 4 * (size_t)(a.step - 1);
    int flag = a.state->flag;
    double xi2 = 0.0;
    if (flag == 0) {
        bool finite = true;
#pragma unroll
        for (int i = 0; i < kIcpSums; ++i) finite = finite && icp_finite(S[i]);
        if (count < a.min_pairs)
            flag = NRGBD_ICP_FEW;
        else if (!finite)
            flag = NRGBD_ICP_NONFINITE;
    }
    if (flag == 0) {
        double A[6][6];
        {
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int j = i; j < 6; ++j) {
                    A[i][j] = S[k];
                    A[j][i] = S[k];
                    ++k;
                }
            }
        }
        double amax = A[0][0];
#pragma unroll
        for (int i = 1; i < 6; ++i) amax = fmax(amax, A[i][i]);
        const double floor_ = a.min_pivot * amax;
        double L[6][6], D[6];
        bool good = true;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double dj = A[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) dj = dj - (L[j][k] * L[j][k]) * D[k];
            good = good && dj > floor_;                        // a NaN fails
            D[j] = dj;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double s = A[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) s = s - (L[i][k] * L[j][k]) * D[k];
                L[i][j] = s / dj;
            }
        }
        if (!good) {
            flag = NRGBD_ICP_DEGENERATE;
        } else {
            double x[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double s = -S[21 + i];
#pragma unroll
                for (int k = 0; k < i; ++k) s = s - L[i][k] * x[k];
                x[i] = s;
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) x[i] = x[i] / D[i];
#pragma unroll
            for (int i = 5; i >= 0; --i) {
                double s = x[i];
#pragma unroll
                for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
                x[i] = s;
            }
            xi2 = ((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5];
            const double wx = x[3], wy = x[4], wz = x[5];
            const double xx = wx * wx, yy = wy * wy, zz = wz * wz;
            const double th2 = (xx + yy) + zz;
            if (!(th2 <= NRGBD_ICP_MAX_THETA2)) {              // a NaN included
                flag = NRGBD_ICP_LARGE;
            } else {
                double sa, cb;
                icp_sinc_cosc(th2, sa, cb);
                const double xy = wx * wy, xz = wx * wz, yz = wy * wz;
                double R[3][3];
                R[0][0] = 1.0 - cb * (yy + zz);
                R[0][1] = cb * xy - sa * wz;
                R[0][2] = cb * xz + sa * wy;
                R[1][0] = cb * xy + sa * wz;
                R[1][1] = 1.0 - cb * (xx + zz);
                R[1][2] = cb * yz - sa * wx;
                R[2][0] = cb * xz - sa * wy;
                R[2][1] = cb * yz + sa * wx;
                R[2][2] = 1.0 - cb * (xx + yy);
                double T[12], N[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) T[i] = a.state->T[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) N[4 * i + j] = (R[i][0] * T[j] + R[i][1] * T[4 + j]) + R[i][2] * T[8 + j];
                    N[4 * i + 3] = N[4 * i + 3] + x[i];
                }
#pragma unroll
                for (int i = 0; i < 12; ++i) {
                    a.state->T[i] = N[i];
                    a.state->Tf[i] = (float)N[i];
                }
                a.state->iterations = a.state->iterations + 1;
            }
        }
    }
    a.state->flag = flag;
    row[0] = (double)count;
    row[1] = S[27];
    row[2] = xi2;
    row[3] = (double)flag;
}

static bool icp_pos(float x) { return x > 0.f && x <= kIcpFltMax; }
static bool icp_fin(float x) { return x >= -kIcpFltMax && x <= kIcpFltMax; }

static int icp_workgroups(int Hs, int Ws) {
    if (Hs <= 0 || Ws <= 0 || Hs > kIcpMaxSide || Ws > kIcpMaxSide) return NRGBD_E_SHAPE;
    const int n = ceil_div((long)Hs * Ws, 256);
    return n < kIcpMaxWg ? n : kIcpMaxWg;
}

}  // namespace nrgbd

// no counterpart in the reference: see the header of this file and include/nrgbd.h
extern "C" int nrgbd_icp_workgroups(int Hs, int Ws) { return nrgbd::icp_workgroups(Hs, Ws); }

extern "C" long nrgbd_icp_workspace(int Hs, int Ws) {
    const int nwg = nrgbd::icp_workgroups(Hs, Ws);
    return nwg < 0 ? (long)nwg : (long)nwg * NRGBD_ICP_RECORD_BYTES;
}

namespace nrgbd {

// the checks and the launch of both nrgbd_icp_terms entries; ph: the photometric arguments (image, mrgb, resid_photo, the affine and
// the two parameters already in place) or NULL
template <bool PHOTO>
static int icp_terms(const float* depth, const float* gate, float gate_thr, int H, int W, float d_near, float d_far, float fx, float fy,
                     float cx, float cy, int sub, const float* mdepth, const float* mnormal, int Hm, int Wm, float fxm, float fym,
                     float cxm, float cym, const void* state, float dist_thr, float huber, void* partial, long partial_bytes,
                     float* resid, const float* image, const float* aff_a, const float* aff_b, const float* mrgb, float photo_weight,
                     float photo_huber, float* resid_photo, void* stream) {
    if (!depth || !mdepth || !mnormal || !state || !partial) return NRGBD_E_NULL;
    if (PHOTO && (!image || !mrgb || !aff_a || !aff_b)) return NRGBD_E_NULL;
    if (H <= 0 || W <= 0 || Hm <= 0 || Wm <= 0 || sub < 1) return NRGBD_E_SHAPE;
    if (H > kIcpMaxSide || W > kIcpMaxSide || Hm > kIcpMaxSide || Wm > kIcpMaxSide) return NRGBD_E_SHAPE;
    const int Hs = H / sub, Ws = W / sub;
    if (Hs == 0 || Ws == 0) return NRGBD_E_SHAPE;
    const int nwg = icp_workgroups(Hs, Ws);
    if (nwg < 0) return nwg;
    if (partial_bytes < (long)nwg * NRGBD_ICP_RECORD_BYTES) return NRGBD_E_SHAPE;
    if (!icp_pos(fx) || !icp_pos(fy) || !icp_pos(fxm) || !icp_pos(fym)) return NRGBD_E_ARG;
    if (!icp_fin(cx) || !icp_fin(cy) || !icp_fin(cxm) || !icp_fin(cym)) return NRGBD_E_ARG;
    if (!icp_pos(dist_thr) || !icp_pos(huber)) return NRGBD_E_ARG;
    if (!(d_near < d_far)) return NRGBD_E_ARG;                  // a NaN bound included
    if (gate && gate_thr != gate_thr) return NRGBD_E_ARG;
    if (PHOTO) {
        if (!icp_pos(photo_weight) || !icp_pos(photo_huber)) return NRGBD_E_ARG;
        for (int k = 0; k < 3; ++k)
            if (!icp_fin(aff_a[k]) || !icp_fin(aff_b[k])) return NRGBD_E_ARG;
    }
    if (((uintptr_t)state & 7) || ((uintptr_t)partial & 7)) return NRGBD_E_ALIGN;
    IcpTermsArgs a;
    a.depth = depth; a.gate = gate; a.mdepth = mdepth; a.mnormal = mnormal; a.state = (const IcpState*)state;
    a.partial = (double*)partial; a.resid = resid;
    a.H = H; a.W = W; a.Hs = Hs; a.Ws = Ws; a.sub = sub; a.Hm = Hm; a.Wm = Wm;
    a.gate_thr = gate_thr; a.d_near = d_near; a.d_far = d_far; a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    a.fxm = fxm; a.fym = fym; a.cxm = cxm; a.cym = cym; a.dist_thr = dist_thr; a.huber = huber;
    IcpPhotoArgsOf<PHOTO> ph;
    if constexpr (PHOTO) {
        ph.image = image; ph.mrgb = mrgb; ph.resid_photo = resid_photo;
        for (int k = 0; k < 3; ++k) {
            ph.aff_a[k] = aff_a[k];
            ph.aff_b[k] = aff_b[k];
        }
        ph.photo_weight = photo_weight; ph.photo_huber = photo_huber;
    }
    hipLaunchKernelGGL(icp_terms_kernel<PHOTO>, dim3(nwg), dim3(256), 0, (hipStream_t)stream, a, ph);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}

}  // namespace nrgbd

extern "C" int nrgbd_icp_terms_f32(const float* depth, const float* gate, float gate_thr, int H, int W, float d_near, float d_far,
                                   float fx, float fy, float cx, float cy, int sub, const float* mdepth, const float* mnormal, int Hm,
                                   int Wm, float fxm, float fym, float cxm, float cym, const void* state, float dist_thr, float huber,
                                   void* partial, long partial_bytes, float* resid, void* stream) {
    return nrgbd::icp_terms<false>(depth, gate, gate_thr, H, W, d_near, d_far, fx, fy, cx, cy, sub, mdepth, mnormal, Hm, Wm, fxm, fym, cxm,
                                   cym, state, dist_thr, huber, partial, partial_bytes, resid, nullptr, nullptr, nullptr, nullptr, 0.f,
                                   0.f, nullptr, stream);
}

extern "C" int nrgbd_icp_terms_photo_f32(const float* depth, const float* gate, float gate_thr, int H, int W, float d_near, float d_far,
                                         float fx, float fy, float cx, float cy, int sub, const float* mdepth, const float* mnormal,
                                         int Hm, int Wm, float fxm, float fym, float cxm, float cym, const void* state, float dist_thr,
                                         float huber, void* partial, long partial_bytes, float* resid, const float* image,
                                         const float* aff_a, const float* aff_b, const float* mrgb, float photo_weight,
                                         float photo_huber, float* resid_photo, void* stream) {
    return nrgbd::icp_terms<true>(depth, gate, gate_thr, H, W, d_near, d_far, fx, fy, cx, cy, sub, mdepth, mnormal, Hm, Wm, fxm, fym, cxm,
                                  cym, state, dist_thr, huber, partial, partial_bytes, resid, image, aff_a, aff_b, mrgb, photo_weight,
                                  photo_huber, resid_photo, stream);
}

extern "C" int nrgbd_icp_update(void* state, const double* init, int step, const void* partial, int nwg, long long min_pairs,
                                double min_pivot, double* log, void* stream) {
    using namespace nrgbd;
    if (!state || (step > 0 && (!partial || !log))) return NRGBD_E_NULL;
    if (step < 0 || (step > 0 && (nwg < 1 || nwg > kIcpMaxWg))) return NRGBD_E_SHAPE;
    IcpUpdateArgs a;
    for (int i = 0; i < 12; ++i) a.init[i] = init ? init[i] : ((i % 5 == 0) ? 1.0 : 0.0);
    if (step == 0) {
        for (int i = 0; i < 12; ++i)
            if (!(a.init[i] >= -1.7976931348623157e+308 && a.init[i] <= 1.7976931348623157e+308)) return NRGBD_E_ARG;
    } else {
        if (!(min_pivot > 0.0 && min_pivot <= 1.7976931348623157e+308) || min_pairs < 6) return NRGBD_E_ARG;
    }
    if (((uintptr_t)state & 7) || (step > 0 && (((uintptr_t)partial & 7) || ((uintptr_t)log & 7)))) return NRGBD_E_ALIGN;
    a.state = (IcpState*)state; a.partial = (const double*)partial; a.log = log;
    a.min_pivot = min_pivot; a.min_pairs = min_pairs; a.step = step; a.nwg = nwg;
    hipLaunchKernelGGL(icp_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    NRGBD_CHECK_LAUNCH();
    return NRGBD_OK;
}
