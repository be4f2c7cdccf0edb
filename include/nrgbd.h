/*
 * nrgbd.h — C-ABI of libnrgbd_hip.so: the MI355X (gfx950) plane-sweep depth path.
 *
 * This is the drop-in boundary for the hot path of NVlabs/neuralrgbd
 * (homography warp -> D-candidate cost volume -> D-Net -> K-Net DPV predict/update).
 * The reference has no FFI of its own: its seam is the Python operator surface of
 * code/warping/homography.py and the ATen ops composed under code/models/.  Each entry
 * point below names the reference interface (file:line, relative to /root/reference)
 * that it replaces.  The Python host (neuralrgbd_amd/) binds these with ctypes and keeps
 * the reference signatures; INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless stated otherwise;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); kernels are
 *     launched on the CURRENT device, are re-entrant and keep no global mutable state;
 *   - inputs are never written; outputs are fully overwritten;
 *   - return value: 0 = success, <0 = NRGBD_E_* argument error, >0 = hipError_t;
 *   - no host synchronisation, no allocation: every call is hipGraph-capturable.
 *
 * Layouts
 *   NCHW  [N][C][h][w]   what torch convolutions produce / consume
 *   NHWC  [N][h][w][Cp]  "texel" layout used by the sampling kernels; Cp = C rounded up to
 *                        a multiple of 4 so that one texel is a whole number of 16-byte
 *                        words (67 -> 68 channels = 272 B, conflict-free for ds_read_b128)
 */
#ifndef NRGBD_H
#define NRGBD_H

#ifdef __cplusplus
extern "C" {
#endif

#define NRGBD_OK             0
#define NRGBD_E_NULL        -1   /* a required pointer is NULL                      */
#define NRGBD_E_SHAPE       -2   /* a dimension is <=0 or exceeds a kernel limit    */
#define NRGBD_E_ALIGN       -3   /* Cp not a multiple of 4 / pointer not 16-B aligned */
#define NRGBD_E_ARG         -4   /* an enum / flag argument is out of range         */

#define NRGBD_DIST_L2        0   /* homography.py:81-83  img_dis_L2_pard */
#define NRGBD_DIST_L1        1   /* homography.py:85-87  img_dis_L1_pard */

#define NRGBD_MAX_D        256   /* depth candidates per volume */
#define NRGBD_MAX_V         16   /* source views per window     */

/* Library / build identification ("nrgbd_hip <interface version> (gfx950, CDNA4)"), and error text for a return code.
 * The interface version changes whenever an entry point changes its signature or disappears: bind against the version you
 * were built for.  0.4 (round 4): nrgbd_costvol_bwd takes (workspace, workspace_bytes) before `stream` (since round 3: query
 * nrgbd_costvol_bwd_workspace first); nrgbd_conv3d_wino_* and nrgbd_conv_wino_dw_bn_f32 are gone; nrgbd_upsample_bilinear_ac
 * is new.  0.5 (round 6): the three BatchNorm finalisers take (collapse_count, batches_tracked) before `stream`; nrgbd_pack_nhwc takes
 * rgb4, nrgbd_conv2d_taps_f32 takes in_stride; nrgbd_avgpool_cl, nrgbd_scatter_channels and nrgbd_conv2d_few_f32 are new.
 * 0.6: the local bundle adjustment entries nrgbd_lba_pyramid, nrgbd_lba_workgroups, nrgbd_lba_grad and nrgbd_lba_update are new;
 * no existing entry changed.  0.7: nrgbd_bn_small_stats (the SPP branches' BatchNorm statistics) is new; no existing entry changed.
 * 0.8: nrgbd_dpv_keyframe_maps (the LBA driver's depth / confidence maps in one launch) is new; no existing entry changed.
 * 0.9: nrgbd_costvol_bwd_det and nrgbd_costvol_bwd_det_workspace (the bit-reproducible cost-volume backward) are new; no existing
 * entry changed.  0.10: nrgbd_warp_volume_cl (the K-Net input volume for temporal windows of 3, 5 and 7 frames, padded to whole
 * 16-channel blocks) is new, and nrgbd_conv3d_wgrad_f32 also takes Cin = 32; no existing entry changed.  0.10 also gained
 * nrgbd_depth_regress_rows and nrgbd_export_depth_u16_rows (the two reductions on a channels-last volume) and C = 256 in
 * nrgbd_logsoftmax_rows / _rows_bwd (the R-Net with candidate up-sampling); no existing entry changed, the version string stays.
 * 0.10 further gained global-norm gradient clipping — nrgbd_grad_norm_workspace, nrgbd_grad_norm, nrgbd_scale_tensors and
 * nrgbd_adam_step_clipped; no existing entry changed its signature or disappeared, so by the rule above the version string stays.
 * The same holds for nrgbd_frame_ingest_u8 and nrgbd_window_gather (the video stream's frame ingest and window assembly), and for
 * nrgbd_depth_ingest_u16 (the training stream's depth-label ingest).  0.10 also gained the on-device depth evaluation —
 * nrgbd_depth_eval_workgroups, nrgbd_depth_eval_workspace and nrgbd_depth_eval; no existing entry changed, the version string stays.
 * The same holds for nrgbd_dgf_refine_f32 (the guided-filter refinement net), and for the TSDF fusion entries
 * nrgbd_tsdf_integrate_f32, nrgbd_tsdf_extract_workspace and nrgbd_tsdf_extract_points, and for nrgbd_tsdf_raycast_f32 (the fused
 * volume rendered to depth and normals), and for nrgbd_tsdf_mesh_workspace and nrgbd_tsdf_extract_mesh (the fused volume as an
 * indexed triangle mesh), and for the colour entries nrgbd_tsdf_integrate_color_f32, nrgbd_tsdf_extract_points_color,
 * nrgbd_tsdf_extract_mesh_color and nrgbd_tsdf_raycast_color_f32 (the frames' colour fused into the volume), and for the tracking
 * entries nrgbd_icp_workgroups, nrgbd_icp_workspace, nrgbd_icp_terms_f32 and nrgbd_icp_update (a depth frame registered against the
 * fused volume), and for nrgbd_icp_terms_photo_f32 (the same with a photometric term against the volume's rendered colour), and for
 * nrgbd_tsdf_reintegrate_f32 and nrgbd_tsdf_reintegrate_color_f32 (a fused frame taken out of the volume and put back at a corrected
 * pose), and for nrgbd_depth_consistency_f32 (a depth map cross-checked against other views' maps before it is fused), and for nrgbd_tsdf_shift_f32
 * (the TSDF volume moved by whole voxels so that it follows the camera, with the leaving part handed out), and for
 * nrgbd_tsdf_blocks_gather_f32 and nrgbd_tsdf_blocks_scatter_f32 (8^3 voxel blocks paged out of the moving volume and back in). */
#define NRGBD_INTERFACE_VERSION "0.10"
const char* nrgbd_version(void);
const char* nrgbd_strerror(int code);

/*
 * nrgbd_homography_terms — the per-view constants of the plane sweep.
 * Replaces: warping/homography.py:315-317 (term1 = IntM.matmul(t_v); left factor IntM.matmul(R_v) of term2), also
 * :250-253 / :203-206 of the K-Net warps.  Summation order = the reference's CPU execution (fma chain for K R_v,
 * (p1 + p2) + p0 for K t_v) so that sampling coordinates agree with it bit for bit.
 *   K  [3][3]                 intrinsics at grid resolution
 *   R  element (v,i,j) at R[v*r_view_stride + i*r_row_stride + j]   (e.g. poses[:, :3, :3]: 16, 4)
 *   t  element (v,i)   at t[v*t_view_stride + i*t_elem_stride]      (e.g. poses[:, :3, 3]:  16, 4)
 *   KR [V][9], Kt [V][3]      outputs
 */
int nrgbd_homography_terms(const float* K, const float* R, long r_view_stride, long r_row_stride,
                           const float* t, long t_view_stride, long t_elem_stride, float* KR, float* Kt,
                           int V, void* stream);

/*
 * nrgbd_pose_inverse — inverse of the 4x4 rigid motions the PREDICT step resamples through.
 * Replaces: test_utils/test_KVNet.py:50,52 (`Src_CamPoses[ibatch, t_win_r].inverse()` / `cam_pose_next.inverse()`), the
 * argument `rel_extM` of warping/homography.py:654 resample_vol_cuda.  The reference leaves the operation order to the
 * host LAPACK; here it is fixed: Gauss-Jordan with partial pivoting on [A | I] in fp64 (every product / difference /
 * quotient rounded once), result rounded to fp32 (<= 0.5 ulp + double rounding from exact); the CPU oracle executes the
 * same sequence bit for bit.  General 4x4 (no rigidity assumed, like `.inverse()`).
 *   T      n matrices, matrix m at T + m*matrix_stride, row-major 4x4 (matrix_stride >= 16)
 *   T_inv  [n][16]
 *   singular_count   optional device int, incremented once per matrix with a zero pivot column (its output is NaN:
 *                    the reference raises on the host; a device entry point cannot, and never syncs)
 */
int nrgbd_pose_inverse(const float* T, long matrix_stride, float* T_inv, int* singular_count, int n, void* stream);

/*
 * nrgbd_pack_nhwc — feature packing for the sampling kernels.
 * Replaces: models/basic.py:254-263 (F.avg_pool2d of the RGB frames + torch.cat onto the
 * CNN features) and the implicit NCHW layout handed to homography.py:293.
 *   feat [N][Cf][h][w]            CNN features (NCHW), or [N][h][w][Cf] when feat_channels_last != 0
 *   rgb  [N][3][h*pool][w*pool]   full-resolution frames, or NULL (then only a transpose)
 *   out  [N][h][w][Cp]            out[..,c] = feat[c] (c<Cf); mean of the pool x pool RGB
 *                                 window (c = Cf..Cf+2, rgb != NULL); 0 for padding
 *   rgb4 [N][h][w][4] or NULL     channels Cf .. Cf+3 of every texel once more as a compact plane (what models/KVNET.py:147-158
 *                                 warps for the K-Net: `F.avg_pool2d(img, 4)`); needs Cp >= Cf + 4
 * Requires Cp % 4 == 0 and Cp >= Cf (+3 if rgb).
 */
int nrgbd_pack_nhwc(const float* feat, const float* rgb, float* out,
                    int N, int Cf, int h, int w, int pool, int Cp, int feat_channels_last, float* rgb4, void* stream);

/*
 * nrgbd_costvol_fwd — fused homography warp + bilinear sample + cost accumulate
 * (+ optional log-softmax over the depth axis).
 * Replaces: warping/homography.py:293-331 est_swp_volume_v4, :421-448
 * _back_warp_homo_parallel (F.grid_sample bilinear / zeros), :81-87 img_dis_L2/L1_pard,
 * and models/basic.py:299-300 (log_softmax(-costV, dim=1)) when out_logp != NULL.
 *   ref_nhwc [h][w][Cp], src_nhwc [V][h][w][Cp]   packed features (channels >= C ignored)
 *   KR [V][9]   row-major K·R_v          (the matmul of homography.py:317, left factor)
 *   Kt [V][3]   K·t_v                    (homography.py:315, term1)
 *   rays [3][h*w]                        cam_intrinsic['unit_ray_array_2D']
 *   d_candi [D]                          candidate depths (fp32 cast of the float64 array)
 *   cx, cy                               cam_intrinsic['intrinsic_M'][0,2], [1,2]
 *   sigma                                costV_sigma
 *   dist                                 NRGBD_DIST_L2 | NRGBD_DIST_L1
 *   align_corners                        0 = torch>=1.3 default (what the reference runs
 *                                        today), 1 = legacy grid_sample behaviour
 *   out_cost [D][h][w] or NULL, out_logp [D][h][w] or NULL (at least one non-NULL)
 * Views are accumulated in the order v = 0..V-1: cost += sum_c(.)/sigma.
 */
int nrgbd_costvol_fwd(const float* ref_nhwc, const float* src_nhwc,
                      const float* KR, const float* Kt, const float* rays,
                      const float* d_candi, float cx, float cy, float sigma,
                      int dist, int align_corners,
                      float* out_cost, float* out_logp,
                      int V, int C, int Cp, int D, int h, int w, void* stream);

/* The same operation with the kernel generation chosen by the caller (tests and A/B measurements):
 * 0 = automatic (what nrgbd_costvol_fwd does), 1 = direct gather (any shape), 2 = LDS-staged, lane = pixel (Cp/4 in
 * {1,2,3,4,8,9,16,17}), 3 = quad: 4 lanes per (pixel, candidate) (Cp = 68 with C > 64, or Cp = C = 64; V <= 8; a view below 2 GB with a
 * row pitch below 8 MB and h * w < 2^23: signed 24-bit address multiplies; what 0 picks for those shapes).
 * A generation that does not support the shape returns NRGBD_E_SHAPE; nothing is substituted silently.
 * `rays`: generations 1 and 3 accept ANY ray table.  Generation 3 stages the source texels a tile can touch from the images of the
 * tile's four corner pixels — exact for the reference's pinhole table (warping/View.py:16-62: rays affine in (x, y), z = 1) — and
 * re-evaluates from global memory every (16 pixels x 4 candidates) group in which a tap falls outside that prediction, so a
 * unit-norm or distortion-corrected table costs time, never correctness (tests/test_gpu_ops.py: non-affine rays vs the C oracle).
 * Generation 2 (not selected for the path's 64(+3)-channel texels) relies on the corner prediction with one texel of slack and
 * REQUIRES the pinhole table; pass generation 1 for any other table with its channel counts. */
int nrgbd_costvol_fwd_gen(const float* ref_nhwc, const float* src_nhwc,
                      const float* KR, const float* Kt, const float* rays,
                      const float* d_candi, float cx, float cy, float sigma,
                      int dist, int align_corners,
                      float* out_cost, float* out_logp,
                      int V, int C, int Cp, int D, int h, int w, int generation, void* stream);

/*
 * nrgbd_costvol_bwd — backward of nrgbd_costvol_fwd with respect to the packed features (training).
 * Replaces: what autograd records for warping/homography.py:293-331 (grid_sample backward scatter-add,
 * broadcast subtract, channel sum).  Same geometry arguments as the forward.
 *   g_cost [D][h][w]  gradient of the loss w.r.t. out_cost
 *   g_ref  [h][w][Cp], g_src [V][h][w][Cp]   overwritten
 *   workspace         device scratch of at least nrgbd_costvol_bwd_workspace() bytes, 16-byte aligned (per-slice
 *                     partial sums of the LDS scatter kernel); may be NULL when that size is 0 (grids whose
 *                     16*h*w bytes exceed the LDS budget use global atomics instead).
 * NRGBD_E_NULL / NRGBD_E_SHAPE when a needed workspace is missing / too small.  NRGBD_E_SHAPE also for h * w > INT_MAX / 4
 * (texels are indexed with int; the same limit as nrgbd_costvol_bwd_det, and from the workspace query too).
 */
int nrgbd_costvol_bwd_workspace(int V, int Cp, int D, int h, int w, size_t* bytes);
int nrgbd_costvol_bwd(const float* ref_nhwc, const float* src_nhwc,
                      const float* KR, const float* Kt, const float* rays,
                      const float* d_candi, float cx, float cy, float sigma,
                      int dist, int align_corners, const float* g_cost,
                      float* g_ref, float* g_src,
                      int V, int C, int Cp, int D, int h, int w,
                      void* workspace, size_t workspace_bytes, void* stream);

/*
 * nrgbd_costvol_bwd_det — nrgbd_costvol_bwd with bit-reproducible results (opt-in; csrc/costvol_bwd_det.hip).  Same arguments and
 * return codes.  g_ref is summed per pixel in (view, candidate) order; g_src is summed in fixed point (integer atomics: the sum
 * does not depend on the order of arrival) and rounded once to fp32.  For the same inputs both outputs are the same bits on every
 * run, on any stream, whatever the buffers held before, and on any device (no launch parameter comes from the CU count).  One
 * path for every grid; every output element is written, the lanes C .. Cp-1 are exactly 0.  Every element is within the rounding
 * bound that holds for nrgbd_costvol_bwd (any summation order).  A g_src element that receives a non-finite term is NaN.
 *   workspace   always required: nrgbd_costvol_bwd_det_workspace() bytes (12 per element of g_src), 16-byte aligned; cleared by the
 *               call itself.  NRGBD_E_SHAPE also for h * w * D > 2^29 (the fixed-point sums need the headroom).
 */
int nrgbd_costvol_bwd_det_workspace(int V, int Cp, int D, int h, int w, size_t* bytes);
int nrgbd_costvol_bwd_det(const float* ref_nhwc, const float* src_nhwc,
                          const float* KR, const float* Kt, const float* rays,
                          const float* d_candi, float cx, float cy, float sigma,
                          int dist, int align_corners, const float* g_cost,
                          float* g_ref, float* g_src,
                          int V, int C, int Cp, int D, int h, int w,
                          void* workspace, size_t workspace_bytes, void* stream);

/*
 * nrgbd_bn_cl_fwd / nrgbd_bn_cl_bwd — train-mode BatchNorm (batch statistics, biased variance) with its ReLU and residual add,
 * forward and backward, on channels-last activations viewed as x [rows][C] (training path, BASELINE config 4).
 * Replaces what autograd records for models/psm_submodule.py:10-16,31-50 (convbn / BasicBlock: nn.BatchNorm2d, ReLU, `out += x`)
 * and models/basic.py:53-68,71-94 (convbn_3d / KV_NET_BASIC: nn.BatchNorm3d, ReLU, residual adds) under
 * train_utils/train_KVNet.py:152 (loss.backward()).
 *   y = act(x*scale + shift) + res        res may be NULL; relu 0/1
 *   coef [4][C]   scale = gamma*invstd, shift = beta - mean*scale, mean, invstd   (forward writes, backward reads)
 *   running_mean / running_var: both NULL, or updated in place with `momentum` (unbiased variance), as nn.BatchNorm does
 *   backward: gx [rows][C], g_gamma [C], g_beta [C]; the gradient of `res` is gy itself; coef2 [2][C] is scratch
 *   partial: scratch of nrgbd_bn_cl_workgroups(rows, C) x 2*C floats (per-workgroup partial sums, added in index order in double)
 * C % 4 == 0 and 256 % (C/4) == 0 (NRGBD_E_SHAPE otherwise).
 */
int nrgbd_bn_cl_workgroups(long rows, int C);
int nrgbd_bn_cl_fwd(const float* x, const float* res, const float* gamma, const float* beta, float eps, float momentum,
                    float* running_mean, float* running_var, int relu, float* y, float* coef, float* partial,
                    long rows, int C, void* stream);
int nrgbd_bn_cl_bwd(const float* x, const float* gy, const float* coef, int relu, float* gx, float* g_gamma,
                    float* g_beta, float* coef2, float* partial, long rows, int C, void* stream);

/*
 * nrgbd_warp_volume — plane-sweep warp of low-channel maps with the samples kept, plus
 * the K-Net input-volume assembly.
 * Replaces: warping/homography.py:234-280 warp_img_feats_v3 / :183-232 warp_img_feats_mgpu
 * (C=3, output transposed to [C][D][h][w]) and models/KVNET.py:163-166 (torch.cat of the
 * warped sources, the reference RGB repeated over D, and BV_cur - BV_predict).
 *   src: V maps of Cs channels addressed as src + v*sv + c*sc + y*sy + x*sx (elements),
 *        so both planar [V][Cs][h][w] and NHWC slices are accepted
 *   ref: one map of Cs channels with strides rc, ry, rx, or NULL
 *   bv_cur, bv_pred [D][h][w] or NULL (both or neither)
 *   out [V*Cs (+Cs if ref) (+1 if bv_cur)][D][h][w]:
 *        channel v*Cs+c   = warped source v, channel c, at depth k
 *        next Cs channels = ref[c] repeated over D
 *        last channel     = bv_cur - bv_pred
 *   channels_last: 0 = out [Ch][D][h][w] (the torch layout of KVNET.py:166),
 *                  1 = out [D][h][w][Ch] (the layout nrgbd_conv3d_3x3x3_f32 consumes)
 */
int nrgbd_warp_volume(const float* src, long sv, long sc, long sy, long sx,
                      const float* ref, long rc, long ry, long rx,
                      const float* KR, const float* Kt, const float* rays,
                      const float* d_candi, float cx, float cy, int align_corners,
                      const float* bv_cur, const float* bv_pred,
                      float* out, int V, int Cs, int D, int h, int w, int channels_last,
                      void* stream);

/*
 * nrgbd_warp_volume_cl — the K-Net input volume of any temporal window, channels-last and zero-padded to Cp channels.
 * Replaces: models/KVNET.py:147-166 (the warp of the 1/4-resolution source images to the reference view for every candidate and
 * the torch.cat of :163-166) for t_win_r = 1, 2, 3 (V = 2, 4, 6 source views; the reference's --t_win).
 *   arguments as nrgbd_warp_volume; ref, bv_cur and bv_pred are required
 *   out [D][h][w][Cp]: channels 0 .. C-1 (C = V*Cs + Cs + 1) in the order of nrgbd_warp_volume — the sources in order, the
 *        reference, bv_cur - bv_pred at channel C-1 —, channels C .. Cp-1 exactly 0.  Cp % 4 == 0, Cp >= C (NRGBD_E_SHAPE otherwise).
 * The first K-Net layer runs at Cp = 16 ceil(C / 16) with zero weights in the padding (16 / 16 / 32 for V = 2 / 4 / 6).  At that Cp,
 * with Cs = 3, V in {2, 4, 6}, channel strides of 1 and 16-byte aligned texels and output, one lane assembles a voxel from 16-byte
 * loads and stores; any other call takes the general kernel.  The bits do not depend on which kernel ran.
 */
int nrgbd_warp_volume_cl(const float* src, long sv, long sc, long sy, long sx,
                         const float* ref, long rc, long ry, long rx,
                         const float* KR, const float* Kt, const float* rays,
                         const float* d_candi, float cx, float cy, int align_corners,
                         const float* bv_cur, const float* bv_pred,
                         float* out, int V, int Cs, int Cp, int D, int h, int w, void* stream);

/*
 * nrgbd_dpv_resample — PREDICT step: rigid 3-D resample of the DPV into the next frame.
 * Replaces: warping/homography.py:654-723 resample_vol_cuda (d_candi_new=None),
 * :873-887 _set_vol_border and the .clamp(max=0,min=-1000) of
 * test_utils/test_KVNet.py:54-59.  The [1,D,h,w,3] point grid the reference builds on the
 * host and copies to the device every frame (homography.py:673-682) is generated in-kernel.
 *   dpv [D][h][w]     log-probability volume
 *   T [16]            row-major 4x4 rel_extM (DEVICE pointer: no host read, no sync)
 *   rays [3][h*w]     unit_ray_array_2D (fp32 of cam_intrinsic['unit_ray_array'])
 *   d_candi [D]
 *   tan_hh, tan_hv    tan(radians(hfov)/2), tan(radians(vfov)/2)
 *   z_half, z_radius  (z_max+z_min)/2, (z_max-z_min)/2 of fp32(d_candi)  (:689-693)
 *   pad_value         border value written on the 6 faces (log(1/D))
 *   do_clamp          clamp the result to [clamp_lo, clamp_hi]
 *   out [D][h][w]
 */
int nrgbd_dpv_resample(const float* dpv, const float* T, const float* rays,
                       const float* d_candi, float tan_hh, float tan_hv,
                       float z_half, float z_radius, float pad_value,
                       int do_clamp, float clamp_lo, float clamp_hi,
                       float* out, int D, int h, int w, void* stream);

/*
 * nrgbd_dpv_resample_to — the same resample onto a DIFFERENT set of candidate depths.
 * Replaces: warping/homography.py:654-723 resample_vol_cuda(..., d_candi_new=...) as called by the local bundle
 * adjustment driver (test_KVNet_LBA.py:414-417): the sample points are d_candi_new[k] * ray (:675-682), the depth axis is
 * normalised with z_half / z_radius of the SOURCE candidates (:686-687: float64 numpy min/max, cast to fp32 when it
 * meets the fp32 tensor), the output has D_out = len(d_candi_new) planes.
 *   dpv [D_src][h][w], d_candi_out [D_out], out [D_out][h][w]; other arguments as nrgbd_dpv_resample.
 */
int nrgbd_dpv_resample_to(const float* dpv, const float* T, const float* rays,
                          const float* d_candi_out, float tan_hh, float tan_hv,
                          float z_half, float z_radius, float pad_value,
                          int do_clamp, float clamp_lo, float clamp_hi,
                          float* out, int D_src, int D_out, int h, int w, void* stream);

/*
 * nrgbd_dpv_keyframe_maps — the four [h][w] maps the local bundle adjustment reads, from a log-DPV in one launch, without
 * the resampled volume.
 * Replaces, per frame of the LBA driver: test_KVNet_LBA.py:414-419 (resample_vol_cuda(..., d_candi_new=d_candi) and its
 * .clamp), :420 / :422 (mutils/misc.py:532-548 depth_val_regression of BVs_measure and of the resampled volume), :421 / :423
 * (torch.max over the candidates) and :455 / :495 (torch.exp(conf) ** 2).
 *   dmap_kf[p]  = sum_k expf(v_k[p]) * d_candi_out[k] in candidate order k = 0 .. D_out-1, v_k = the value
 *                 nrgbd_dpv_resample_to writes at plane k (same arithmetic, same bits), clamp included;
 *   conf_kf[p]  = c * c, c = exp(max_k v_k[p]) correctly rounded (as nrgbd_export_depth_u16's confidence);
 *   dmap_ref / conf_ref: the same two reductions of dpv itself with d_candi_src [D_src].
 * Either pair may be NULL (both pointers, or one of them): it is not computed.  The driver needs the reference pair only in
 * the first window after a start or a refresh.  d_candi_src is required only with the reference pair; T, rays and
 * d_candi_out only with the keyframe pair.  Other arguments and error codes as nrgbd_dpv_resample_to.  No allocation, no
 * host synchronisation: safe to capture into a hipGraph.
 */
int nrgbd_dpv_keyframe_maps(const float* dpv, const float* T, const float* rays,
                            const float* d_candi_out, const float* d_candi_src,
                            float tan_hh, float tan_hv, float z_half, float z_radius, float pad_value,
                            int do_clamp, float clamp_lo, float clamp_hi,
                            float* dmap_kf, float* conf_kf, float* dmap_ref, float* conf_ref,
                            int D_src, int D_out, int h, int w, void* stream);

/*
 * nrgbd_logsoftmax_d — log-softmax over the depth axis of scale*a (+ b).
 * Replaces: models/basic.py:299-300 (scale=-1, b=NULL) and the UPDATE step
 * models/KVNET.py:172-173 (scale=1, a = K-Net gain, b = BV_predict).
 *   a, b, out [D][n]   (n = h*w; b may be NULL; out may alias a)
 */
int nrgbd_logsoftmax_d(const float* a, const float* b, float scale, float* out,
                       int D, long n, void* stream);

/*
 * nrgbd_depth_regress — expected depth and confidence of a log-DPV.
 * Replaces: mutils/misc.py:532-548 depth_val_regression (BV_log=True; a Python loop over
 * D) and the max_d of test_utils/export_res.py:58-59.
 *   logp [D][n]; d_candi [D]; depth [n] or NULL; conf [n] or NULL (max_k logp)
 *   A column that holds a NaN has depth NaN AND conf NaN (torch.max keeps a NaN; the first NaN of the column is returned).
 */
int nrgbd_depth_regress(const float* logp, const float* d_candi,
                        float* depth, float* conf, int D, long n, void* stream);

/*
 * nrgbd_export_depth_u16 — export epilogue of a (refined) log-DPV in one pass.
 * Replaces: test_utils/export_res.py:43-75 export_res_img — a D-slice tensor of depth values, torch.sum(exp(BV) * vol),
 * torch.max, two host round trips and `(map * scale).astype(np.uint16)` on the CPU.
 *   logp [D][n]; d_candi [D]
 *   depth [n] or NULL   sum_k exp(logp_k) d_k          conf [n] or NULL   exp(max_k logp_k)
 *   depth_u16, conf_u16 [n] or NULL   (map * scale) truncated toward zero (numpy astype), clamped to [0, 65535]
 *   A column that holds a NaN has depth NaN and conf NaN, as nrgbd_depth_regress; a NaN map value is written as 0 in the uint16 maps.
 */
int nrgbd_export_depth_u16(const float* logp, const float* d_candi, float depth_scale, float conf_scale,
                           float* depth, float* conf, unsigned short* depth_u16, unsigned short* conf_u16,
                           int D, long n, void* stream);

/*
 * nrgbd_depth_regress_rows / nrgbd_export_depth_u16_rows — the two entries above on a CHANNELS-LAST volume logp [n][D]: the
 * refined DPV as the R-Net's last layer writes it (models/Refine.py:104; with candidate up-sampling, Refine.py:44-49, D is four
 * times the candidates of the low-resolution volume: 0.8 GB per volume at 768x1024 with 256), regressed (mutils/misc.py:532-548)
 * or exported without a transposing copy.  Arguments as the planar entries; the results are the SAME BITS as theirs on the
 * transposed copy (one accumulator per pixel, acc = acc + exp(v_k) d_k for k = 0 .. D-1 from 0.f; expf / the correctly rounded
 * exponential respectively).  D % 4 == 0, D <= 1024 (else NRGBD_E_SHAPE); logp 16-byte aligned (else NRGBD_E_ALIGN).
 */
int nrgbd_depth_regress_rows(const float* logp, const float* d_candi,
                             float* depth, float* conf, int D, long n, void* stream);
int nrgbd_export_depth_u16_rows(const float* logp, const float* d_candi, float depth_scale, float conf_scale,
                                float* depth, float* conf, unsigned short* depth_u16, unsigned short* conf_u16,
                                int D, long n, void* stream);

/*
 * nrgbd_warp_depth_fwd / _bwd — photometric warp through a per-pixel depth map and its gradient w.r.t. the poses.
 * Replaces: warping/homography.py:479-528 back_warp_th_Rt_msrc (N views) and :530-575 back_warp_th_Rt (N = 1), and the
 * autograd graph ICP/opt_pose_numerical.py:245-294 differentiates (local bundle adjustment refines R_n, t_n).
 *   src [N][C][H][W]; dmap [H][W]; K [3][3]; R [N][3][3]; t [N][3] (reference -> source n); rays [3][HW]
 *   out [N][C][H][W]          out[n,c,p] = bilinear(src[n,c], K (R_n dmap[p] ray_p + t_n) / z), zeros padding
 *   g_out [N][C][H][W]        upstream gradient
 *   partial [N][nrgbd_warp_depth_bwd_workgroups(H, W)][12]   scratch (fixed-order reduction: reproducible)
 *   g_R [N][3][3], g_t [N][3] d sum(out * g_out) / d(R_n, t_n)
 */
int nrgbd_warp_depth_fwd(const float* src, const float* dmap, const float* K, const float* R, const float* t,
                         const float* rays, float* out, int N, int C, int H, int W, void* stream);
int nrgbd_warp_depth_bwd_workgroups(int H, int W);
int nrgbd_warp_depth_bwd(const float* src, const float* dmap, const float* K, const float* R, const float* t,
                         const float* rays, const float* g_out, float* partial, float* g_R, float* g_t,
                         int N, int C, int H, int W, void* stream);

/*
 * Local bundle adjustment (pose refinement): the Adam loop of ICP/opt_pose_numerical.py:28-170 (_opt_pose_warping, one view)
 * and :172-303 (_opt_pose_warping_parallel, N views jointly), called by local_BA_direct (:358-417) / _parallel (:306-355).
 * One iteration = nrgbd_lba_grad + nrgbd_lba_update; nothing is read back or uploaded between iterations.
 *
 * nrgbd_lba_pyramid — every level of mutils/misc.py:139 downsample_img (F.avg_pool2d(x, k), floor sizes, each level pooled from
 * the full-resolution input; k = 1 copies) of `nplanes` planes [H][W] (for the LBA: ref 3, sources 3 N, depth, confidence) in one
 * launch.  Replaces opt_pose_numerical.py:320-322, :338 / :387-389, :400.
 *   planes: HOST array of nplanes device pointers (nplanes <= 5 + 3 NRGBD_MAX_V); ks [nlevels] host (nlevels <= NRGBD_LBA_MAX_LEVELS)
 *   out: level l at element offset nplanes * sum_{j<l} (H/k_j)(W/k_j), laid out [nplanes][H/k_l][W/k_l]
 *
 * nrgbd_lba_grad — one fused pass for the loss and its gradient at the current poses (replaces :245-294 / :99-160: quaternion
 * chain aside, back_warp_th_Rt(_msrc), the mask, nn.L1Loss and what autograd runs for them).  Per (view n, pixel p, channel c):
 * warped w = bilinear(src[n,c], K (R_n dmap[p] ray_p + t_n)) (= nrgbd_warp_depth_fwd); where w != 0: r = w conf[p] - ref[c,p] conf[p].
 *   ref [3][H][W]; src [N][3][H][W]; dmap, conf [H][W]; K [3][3]; rays [3][HW]; state [N][NRGBD_LBA_STATE] (R_n, t_n read)
 *   partial [N][nrgbd_lba_workgroups(H, W)][13]: per workgroup sum_p sign(r) conf d(w)/d(R_n) [9], d/d(t_n) [3], and sum |r| [1]
 *   nrgbd_lba_workgroups(H, W) = min(ceil(HW / 256), 256): a fixed cap, larger images are covered by a grid-stride loop.
 *
 * nrgbd_lba_update — one workgroup.  step == 0: state[n] <- init[n] = (uq_n [3], t_n [3]), Adam moments 0, R_n = quaternion2Rotation(
 * unitQ_to_quat(uq_n)) (mutils/misc.py:295, :459) in the reference's fp32 order.  step >= 1: fixed-order double reduction of the
 * partials, normaliser 3 H W (x N when joint: the mean of nn.L1Loss), loss -> loss_log[log_slot] (joint) or
 * loss_log[n * log_stride + log_slot], chain rule to d/d uq, then the Adam step number `step` (torch.optim.Adam, betas .9/.999,
 * eps 1e-8, learning rate lr; the arithmetic of nrgbd_adam_step) of t_n when opt_t, of uq_n when opt_R (then R_n is rebuilt).
 *   state [N][NRGBD_LBA_STATE] floats: uq [0,3) t [3,6) R [6,15) Adam m_t [15,18) v_t [18,21) m_uq [21,24) v_uq [24,27)
 */
#define NRGBD_LBA_STATE      32
#define NRGBD_LBA_MAX_LEVELS  8
int nrgbd_lba_pyramid(const float* const* planes, int nplanes, int H, int W, const int* ks, int nlevels, float* out,
                      void* stream);
int nrgbd_lba_workgroups(int H, int W);
int nrgbd_lba_grad(const float* ref, const float* src, const float* dmap, const float* conf, const float* K, const float* rays,
                   const float* state, float* partial, int N, int H, int W, void* stream);
int nrgbd_lba_update(const float* partial, int nwg, const float* init, float* state, float* loss_log, int log_stride,
                     int log_slot, int N, int H, int W, int joint, int step, double lr, int opt_R, int opt_t, void* stream);

/*
 * K-Net: 3x3x3 convolution (stride 1, padding 1, no bias) on the fp32 matrix cores, with the
 * BatchNorm3d / ReLU / residual work of the reference fused around it.
 * Replaces, per layer of models/basic.py:71-94,113-132 (KV_NET_BASIC): nn.Conv3d + nn.BatchNorm3d
 * (psm_submodule.py:19-23, batch statistics) + nn.ReLU + the residual adds of :127-131.
 *
 * Activations are channels-last [D][H][W][C].  A layer reads its input as
 *       in = act(x * s + t)  [+ act(res * s' + t')]           (s,t per channel; act = ReLU or identity)
 * i.e. the normalise/affine/ReLU/add of the PREVIOUS layers is applied on the fly while the input
 * tile is loaded; `materialized` (optional) receives `in` for use as a later residual.  The raw
 * convolution output is written to y together with per-workgroup partial sums for the batch statistics:
 *   stats [nrgbd_conv3d_workgroups(D,H,W)][128]   (sum of y per channel, then sum of y^2 per channel)
 * nrgbd_bn3d_finalize reduces them (in double) to scale_shift [64][2] = (gamma*invstd, beta - mean*gamma*invstd)
 * and applies the train-mode running-statistics update (momentum, unbiased variance).
 *   x_ss / res_ss [Cin][2] or NULL (identity); x_relu / res_relu 0|1; res, materialized, stats may be NULL
 *   w_packed: nrgbd_conv3d_pack_weights(w [64][Cin][3][3][3]) -> [27*Cin*64] floats
 *   Cin in {16, 64}; Cout = 64.
 * nrgbd_conv3d_3x3x3_cout1_f32 is the last layer (Conv3d(64,1), basic.py:92-94):
 *   w_tap_major [27][64] = w[0][c][tap] transposed; y [D][H][W].
 */
int nrgbd_conv3d_workgroups(int D, int H, int W);
int nrgbd_conv3d_pack_weights(const float* w, float* w_packed, int Cin, void* stream);
int nrgbd_conv3d_3x3x3_f32(const float* x, const float* x_ss, int x_relu,
                           const float* res, const float* res_ss, int res_relu,
                           float* materialized, const float* w_packed, float* y, float* stats,
                           int D, int H, int W, int Cin, int Cout, void* stream);
int nrgbd_conv3d_3x3x3_cout1_f32(const float* x, const float* x_ss, int x_relu,
                                 const float* res, const float* res_ss, int res_relu,
                                 const float* w_tap_major, float* y,
                                 int D, int H, int W, int Cin, void* stream);
/*
 * nrgbd_conv3d_cout1_{dgrad,wgrad}_f32 — the two gradients of that last layer (training; what autograd computes for
 * nn.Conv3d(64, 1, 3, padding 1) of models/basic.py:92-94 in train_utils/train_KVNet.py:103-171).  One output channel makes every
 * direction a 27-tap stencil per voxel (memory bound); until interface 0.5 the layer ran zero-padded to 64 outputs on the 64 -> 64 kernels.
 *   gy [D][H][W] (gradient of the layer's output), x / gx [D][H][W][64] channels-last, w_tap_major [27][64] as for the forward,
 *   dw [64][27] = torch's [1][64][3][3][3] (overwritten); workspace: nrgbd_conv3d_cout1_wgrad_workspace() bytes, 16-byte aligned.
 *   gx[v][ci] = sum_tap gy[v - off(tap)] w[ci][tap];  dw[ci][tap] = sum_v gy[v - off(tap)] x[v][ci];  fixed summation orders.
 * nrgbd_conv3d_cout1_bwd_workgroups: the grid of the weight-gradient (dgrad = 0) or data-gradient (dgrad != 0) launch, host only: one
 * workgroup per 8 x 16 tile of a slice up to 512 / 2,048, beyond that the workgroups walk the tile list; < 0: a shape error.
 */
int nrgbd_conv3d_cout1_bwd_workgroups(int D, int H, int W, int dgrad);
int nrgbd_conv3d_cout1_dgrad_f32(const float* gy, const float* w_tap_major, float* gx, int D, int H, int W, void* stream);
int nrgbd_conv3d_cout1_wgrad_workspace(int D, int H, int W, size_t* bytes);
int nrgbd_conv3d_cout1_wgrad_f32(const float* x, const float* gy, float* dw, void* workspace, size_t workspace_bytes, int D, int H, int W,
                                 void* stream);
/*
 * nrgbd_conv3d_wgrad_f32 — weight gradient of the 3x3x3 convolution (training):
 *   dW[co][ci][kd][kh][kw] = sum_voxels gy[v][co] * x[v + tap][ci]      (x zero outside the volume)
 * Replaces what autograd/MIOpen compute for nn.Conv3d.weight.grad in models/basic.py:71-94.
 *   x [D][H][W][Cin] (Cin = 16, 32 or 64), gy [D][H][W][64] channels-last; dw [64][Cin][3][3][3] (torch layout, overwritten);
 *   partial: scratch of nrgbd_conv3d_wgrad_workgroups() * 27 * 64 * Cin floats.
 * The data gradient needs no new kernel: it is nrgbd_conv3d_3x3x3_f32 applied to gy with the weights
 * transposed (cin <-> cout) and flipped in all three tap axes.
 * nrgbd_conv3d_wgrad_ranges: the tile ranges of the launch (host only) — the grid is (ranges, quadrants) whatever the volume, and a
 * range walks its share of the 2 x 4 x 16-voxel tiles.
 */
int nrgbd_conv3d_wgrad_workgroups(void);
int nrgbd_conv3d_wgrad_ranges(void);
int nrgbd_conv3d_wgrad_f32(const float* x, const float* gy, float* partial, float* dw,
                           int D, int H, int W, int Cin, void* stream);
int nrgbd_bn3d_finalize(const float* stats, int num_workgroups, long count,
                        const float* gamma, const float* beta, float eps, float momentum,
                        float* running_mean, float* running_var, float* scale_shift, unsigned int* collapse_count, long long* batches_tracked, void* stream);

/*
 * 2-D feature CNN helpers (NCHW, HW % 4 == 0, 16-B aligned planes).
 * nrgbd_bn2d_train_act — train-mode BatchNorm2d (batch statistics over N*H*W, biased variance) fused with
 * its activation and the residual add: y = act(gamma*(x-mean)/sqrt(var+eps) + beta) (+ residual).
 * Replaces: psm_submodule.py:10-16 (convbn's nn.BatchNorm2d, always batch statistics: SURVEY §0.2),
 * the nn.ReLU(inplace=True) after it (:37,:94-96) and `out += x` of BasicBlock (:47).
 *   act: 0 none, 1 ReLU; residual NULL or [N][C][HW]; y may alias x;
 *   partial: scratch of nrgbd_bn2d_partial_floats(C) floats; mean_var [C][2] or NULL (batch mean, biased var:
 *   input of the running-statistics update of the shortcut norms, psm_submodule.py:131).
 * nrgbd_avgpool8 — 8x8/stride-8 average pooling (the finest SPP window, psm_submodule.py:115; the 16/32/64
 * windows of :103-111 are pooled from its output).  x [NC][H][W] -> y [NC][H/8][W/8].
 */
int nrgbd_bn2d_partial_floats(int C);
int nrgbd_bn2d_train_act(const float* x, const float* gamma, const float* beta, float eps, int act,
                         const float* residual, float* y, float* partial, float* mean_var,
                         int N, int C, long HW, void* stream);
int nrgbd_avgpool8(const float* x, float* y, int NC, int H, int W, void* stream);
/*
 * nrgbd_avgpool_cl — k x k / stride-k average pooling of a CHANNELS-LAST map: x [N][H][W][C] -> y [N][H/k][W/k][C] (floor: a ragged
 * border is dropped, as F.avg_pool2d does).  Replaces: the four nn.AvgPool2d of models/psm_submodule.py:100-117 on the inference
 * path (window 8 on the deep map, then 2 / 4 / 8 on its result: equal windows, the mean of means is the mean).  C % 4 == 0.
 * nrgbd_scatter_channels — dst[r][pixel][coff + c] = src[c * stride_c + y * stride_y + x * stride_x] for r < n_rep images of pixel
 * stride ldy, `rep_stride` floats apart: the image features models/Refine.py:88-98 concatenates behind the candidate channels
 * (`torch.cat((dpv, feat), dim=1)`), written straight into the R-Net's channels-last concat buffers for every sample of the batch.
 */
int nrgbd_avgpool_cl(const float* x, float* y, int N, int H, int W, int C, int k, void* stream);
/*
 * nrgbd_conv2d_few_f32 — 3x3 convolution (stride 1, pad 1) + bias + optional LeakyReLU(0.01) with 1..4 OUTPUT channels, on the vector
 * ALUs.  Replaces: the three output columns beyond the 64-column groups of models/Refine.py:64-66 conv2 (conv2d_leakyRelu(D + 3, D + 3):
 * 67 = 64 + 3, 131 = 128 + 3 outputs), which otherwise cost a whole extra pass of the matrix-core kernel over the full-resolution buffer.
 *   x [N][H][W][ldx] channels-last, channels 0 .. Cin-1 read (Cin % 16 == 0 <= ldx, ldx % 4 == 0: padding channels carry zero weights)
 *   w_packed [Cin/16][9 taps = ky*3 + kx][Cout][16]  = w[co][16*block + lane][ky][kx]     (host mirror: nets.DPVUpsampleNet._rnet_packed)
 *   y [N][H][W][ldy]: output column co at y[pixel * ldy + ycoff + co]; the rest of the pixel is left alone
 * Summation per output: bias, then (block, tap, channel) ascending — one fp32 FMA chain.
 */
int nrgbd_conv2d_few_f32(const float* x, int ldx, const float* w_packed, const float* bias, int out_lrelu, float* y, int ldy,
                         int ycoff, int N, int H, int W, int Cin, int Cout, void* stream);
int nrgbd_scatter_channels(const float* src, long stride_c, long stride_y, long stride_x, int C, int H, int W, float* dst,
                           int ldy, int coff, int n_rep, long rep_stride, void* stream);
/*
 * nrgbd_bias_act_nchw — x = leaky_relu(x + bias[c], slope) in place on [N][C][HW] (HW % 4 == 0): the bias + LeakyReLU
 * tail of the R-Net's conv2d_leakyRelu / conv2dTranspose_leakyRelu blocks (models/m_submodule.py:18-27,36-45) in one
 * pass after a bias-free vendor convolution; slope = 1 is the plain bias add of Refine.py:71.
 */
int nrgbd_bias_act_nchw(float* x, const float* bias, float slope, int N, int C, long HW, void* stream);

/*
 * nrgbd_conv_wino_f32 — generation 2 of the Winograd-domain convolution (csrc/wino_pc.hip): a persistent 8-wave workgroup per
 * CU, 4 consumer waves that only issue MFMAs and 4 producer waves that load / normalise / transform the operand two stages
 * ahead.  One entry for
 *   kd = 3: the K-Net's 3x3x3 layers (models/basic.py:71-94), x [N = depth][H][W][Cin], dilation 1;
 *   kd = 1: the 3x3 stride-1 layers of the feature CNN (models/psm_submodule.py:10-16,31-50,100-134), x [N images][H][W][Cin],
 *           padding = dilation in {1, 2}.
 * Cin % 16 == 0, Cout % 64 == 0; same fused prologue (x_ss / x_relu / res / res_ss / res_relu / materialized) and statistics
 * epilogue as nrgbd_conv3d_3x3x3_f32 / nrgbd_conv2d_3x3_f32.
 * Cout = 32 (kd = 1, dilation 1: the trunk's half-resolution 32 -> 32 layers, psm_submodule.py:90-103): the kernel's HALF form —
 *   w_wino is the 64-column stream of the layer's weights with the upper 32 columns zero, stats has TWO rows per tile
 *   ([2*32][2 * nrgbd_conv_wino_tiles]: one per (tile, 16-tile row block)); nrgbd_conv_wino_rnet_ex_f32 takes Cout = 32 the same way.
 *   w_wino: [Cout/64][stage = cb*kd + depth tap][16 transform points][4 waves][64 lanes][4] floats, U = G g G^T over (ky, kx)
 *           (host mirror: neuralrgbd_amd/ops.py::conv_wino_pack)
 *   stats  [2*Cout][nrgbd_conv_wino_tiles(N,H,W,dilation)] (COLUMN-major: a channel's per-tile partial sums, then its partial
 *           sums of squares, each one contiguous run) for nrgbd_bn_finalize_cm, or NULL
 * nrgbd_bn_finalize_cm — the BatchNorm finaliser (same contract as nrgbd_bn_finalize: models/basic.py:13-51 BatchNorm2d/3d with
 *   batch statistics, running-statistics side effect) for column-major partials [2C][rows]
 */
int nrgbd_conv_wino_tiles(int N, int H, int W, int dilation);
/* R-Net form of the same kernel (models/m_submodule.py:18-27 conv2d_leakyRelu where Cin % 16 == 0 (>= 32; an odd number of 16-channel stages has its own instantiation) and Cout % 64 == 0:
 * Refine.py:51-56 conv0 / conv0_1): y = leaky_relu(conv3x3(x) + bias, 0.01 if out_lrelu), x [N][H][W][Cin] -> y [N][H][W][Cout] */
int nrgbd_conv_wino_rnet_f32(const float* x, const float* w_wino, const float* bias, int out_lrelu, float* y,
                             int N, int H, int W, int Cin, int Cout, void* stream);
/* The same with the R-Net's generalised output addressing (as nrgbd_conv2d_rnet_f32): output column c of a pixel goes to
 * y[pixel * ldy + ycoff + c] for c < cout_valid (ldy = 0: Cout, cout_valid = 0: Cout) — the half- and full-resolution layers
 * (Refine.py:57-70: 96 -> 96 and 67 -> 67 / 64, widths padded to Cin % 16 == 0, Cout % 64 == 0 with zero weights) write into
 * 96-wide concat buffers whose padding channels stay zero. */
int nrgbd_conv_wino_rnet_ex_f32(const float* x, const float* w_wino, const float* bias, int out_lrelu, float* y,
                                int N, int H, int W, int Cin, int Cout, int ldy, int ycoff, int cout_valid, void* stream);
/* Deconv form of the same kernel: nn.ConvTranspose2d(kernel 4, stride 2, padding 1) + bias + LeakyReLU (m_submodule.py:36-45;
 * Refine.py:57,64 trans_conv0 / trans_conv1) of ONE 64-column output slice, x [N][H][W][Cin] -> y [N][2H][2W][ldy].  The four sub-pixel
 * phases (a, b) are 3x3 kernels that are non-zero in a 2x2 corner, stacked phase-major along the output channels (256 columns, phase
 * 2a + b = column group): of the 16 transform points of U = G g G^T a phase has 9 non-zero ones (xi_y = a .. a+2, xi_x = b .. b+2);
 * the kernel skips the other 7 (2.25 multiplies per output and input channel) and stores phase pixel (y, x) at pixel (2y + a, 2x + b),
 * columns ycoff .. ycoff + cout_valid - 1 (ldy = 0: 64, cout_valid = 0: 64).  Bit-equal to nrgbd_conv_wino_rnet_ex_f32 on the stacked
 * weights followed by the pixel shuffle (finite inputs).
 *   w_masked: [4 phases][stage = Cin/16][9 live points][4 waves][64 lanes][4] floats: nrgbd_conv_wino_rnet_deconv_pack copies them out of
 *             the 256-column stream w_wino that nrgbd_conv_wino_pack makes of the stacked weights [256][Cin][3][3]
 *   errors    NRGBD_E_NULL: x, w_masked or y NULL;  NRGBD_E_SHAPE: a dimension <= 0, Cin < 32, Cin % 32 != 0 (an even number of
 *             16-channel stages), Cout != 64, N H W Cin >= 2^30, 4 N H W ldy >= 2^31;  NRGBD_E_ARG: cout_valid outside 0 .. 64,
 *             ycoff < 0, ldy < ycoff + cout_valid;  NRGBD_E_ALIGN: x or w_masked not 16-byte aligned, y or bias not 4-byte aligned.
 *             Checked in this order, before anything is launched. */
int nrgbd_conv_wino_rnet_deconv_f32(const float* x, const float* w_masked, const float* bias, int out_lrelu, float* y,
                                    int N, int H, int W, int Cin, int Cout, int ldy, int ycoff, int cout_valid, void* stream);
int nrgbd_conv_wino_rnet_deconv_pack(const float* w_wino, float* w_masked, int Cin, void* stream);
/* w [Cout][Cin][kd][3][3] (torch layout) -> w_wino [Cout*Cin*kd*16] floats in the order described above (on the device).
 * transposed = 1: the DATA-GRADIENT weights of w [Cin][Cout][kd][3][3] (roles of the channel axes swapped, every tap flipped),
 * i.e. what the same kernel needs to turn dL/dy into dL/dx — without materialising w.transpose(0,1).flip(...) first.
 * transposed = 2: BOTH streams of the layer w [Cout][Cin][kd][3][3] in one launch (training re-packs them every iteration):
 * the forward stream at w_wino, the data-gradient stream right behind it (w_wino holds 2 * Cout*Cin*kd*16 floats; Cin % 64 too). */
int nrgbd_conv_wino_pack(const float* w, float* w_wino, int Cin, int Cout, int kd, int transposed, void* stream);
int nrgbd_bn_finalize_cm(const float* stats, int rows, int C, long count, const float* gamma, const float* beta, float eps,
                         float momentum, float* running_mean, float* running_var, float* scale_shift, unsigned int* collapse_count,
                         long long* batches_tracked, void* stream);
int nrgbd_conv_wino_f32(const float* x, const float* x_ss, int x_relu, const float* res, const float* res_ss,
                        int res_relu, float* materialized, const float* w_wino, float* y, float* stats,
                        int N, int H, int W, int Cin, int Cout, int kd, int dilation, void* stream);

/*
 * nrgbd_conv_wino_dw_f32 — generation 3 of the K-Net's 3x3x3 layers (csrc/wino_dw.hip; models/basic.py:71-94): Winograd in all
 * three dimensions, F(2x2, 3x3) in the plane and F(2, 3) along the depth axis: 8 fp32 multiplies per output voxel (generation
 * 2: 12, direct: 27), exact-algorithm fp32.  Same contract as nrgbd_conv_wino_f32 with kd = 3 (x [N = depth][H][W][Cin], fused
 * prologue, column-major statistics [2*Cout][nrgbd_conv_wino_tiles(N,H,W,1)] for nrgbd_bn_finalize_cm), restricted to N even
 * and whole 8x16 tiles (H % 8 == 0, W % 16 == 0: every grid of the path); other shapes return NRGBD_E_SHAPE and belong to
 * nrgbd_conv_wino_f32 — nothing is substituted silently.
 *   w_wino: [Cout/64][stage = t*(Cin/16) + cb][16 transform points][4 waves][64 lanes][4] floats,
 *           U_t = sum_kd Gd[t][kd] (G g_kd G^T), Gd = G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]  (nrgbd_conv_wino_dw_pack;
 *           transposed as in nrgbd_conv_wino_pack)
 */
int nrgbd_conv_wino_dw_pack(const float* w, float* w_wino, int Cin, int Cout, int transposed, void* stream);
int nrgbd_conv_wino_dw_f32(const float* x, const float* x_ss, int x_relu, const float* res, const float* res_ss,
                           int res_relu, float* materialized, const float* w_wino, float* y, float* stats,
                           int N, int H, int W, int Cin, int Cout, void* stream);
int nrgbd_conv_wino_dw_workgroups(int N, int H, int W, int Cout);
/*
 * nrgbd_conv_wino_dw4_* — the same 3x3x3 convolution (models/basic.py:71-94: the K-Net's ten 64 -> 64 layers) with F(4, 3) along the
 * depth axis (interpolation points 0, +-1/2, +-3/2, inf) on top of the in-plane F(2x2, 3x3): 6 multiplies per output voxel instead of 8;
 * N % 4 == 0 (quadruples of output slices), whole 8x16 tiles.  Numerically 1.24x as far from float64 as the direct convolution on the
 * whole K-Net (oracle/wino_d4_eval.py; nrgbd_conv_wino_dw_f32: 0.92x).  Input forms: x as it is (x_ss NULL, x_relu 0), act(x * s + t),
 * or — x_unit = 2^-k > 0, x_ss given, x_relu 1 — relu(x * s + t) as a clamped FMA with w_wino packed from 2^k * w (see
 * nrgbd_conv_wino_dw_unit_f32).  `workspace`: nrgbd_conv_wino_dw4_workspace() bytes of device scratch, 16-byte aligned, private to the
 * launch (one third of the depth fold's live values per workgroup goes through it: they do not fit the LDS).
 *   w_wino: [Cout/64][stage = p * Cin/16 + cb][16 points][4 waves][64 lanes][4], phases p in execution order t = 1, 2, 3, 4, 0, 5
 *   stats  [2*Cout][nrgbd_conv_wino_tiles(N,H,W,1)] column-major partials for nrgbd_bn_finalize_cm, or NULL
 *   pack: transposed = 1 packs the data-gradient stream (w read as [Cin][Cout][3][3][3], taps flipped), 2 both streams in one launch
 *         (forward, then data gradient; Cin % 64 == 0) — as nrgbd_conv_wino_dw_pack
 */
int nrgbd_conv_wino_dw4_pack(const float* w, float* w_wino, int Cin, int Cout, int transposed, void* stream);
int nrgbd_conv_wino_dw4_workspace(int N, int H, int W, int Cout, size_t* bytes);
int nrgbd_conv_wino_dw4_f32(const float* x, const float* x_ss, int x_relu, float x_unit, const float* w_wino, float* y, float* stats,
                            void* workspace, size_t workspace_bytes, int N, int H, int W, int Cin, int Cout, void* stream);
/*
 * nrgbd_conv_wino_dw_unit_f32 — nrgbd_conv_wino_dw_f32's plain form for an input relu(x * scale + shift) (no residual, no
 * materialise) with the ReLU taken by the producers' FMA itself (its [0, 1] clamp) instead of one v_max_f32 per element:
 *   x_unit = 2^-k: the kernel multiplies (scale, shift) by it; the caller guarantees |x * scale + shift| < 2^k everywhere (for a
 *   BatchNorm with batch statistics over n values: |gamma| sqrt(n) + |beta| bounds it, whatever the data) and packs the weight
 *   stream from 2^k * w.  Powers of two commute with every rounding on the way, so y and stats have the bits of the plain form.
 * Same layer as nrgbd_conv_wino_dw_f32 (models/basic.py:53-68,71-94: conv3d + BatchNorm3d + ReLU feeding the next conv3d).
 */
int nrgbd_conv_wino_dw_unit_f32(const float* x, const float* x_ss, float x_unit, const float* w_wino, float* y, float* stats,
                                int N, int H, int W, int Cin, int Cout, void* stream);

/*
 * R-Net (DPV up-sampler) on the same matrix-core kernel.  Replaces, per layer of models/Refine.py:51-107:
 *   m_submodule.conv2d_leakyRelu (nn.Conv2d 3x3 + bias + LeakyReLU 0.01, :18-27)      mode 0
 *   m_submodule.conv2dTranspose_leakyRelu (nn.ConvTranspose2d k4 s2 p1 + bias + LeakyReLU, :37-45)
 *                                             as four sub-pixel 2x2-tap launches (pa, pb in {0,1})   mode 1
 *   conv2_2 + F.log_softmax(dim=1) (:99-105)                                          mode 2
 *   the four phases of a transposed convolution in ONE launch (blockIdx.y = phase; w_packed = the four phases' packed
 *   weights back to back in the order (pa, pb) = (0,0), (0,1), (1,0), (1,1); pa / pb ignored)          mode 3
 *   the torch.cat of :88,93,98: a layer writes its cout_valid channels at channel offset ycoff of a wider
 *   channels-last pixel (pixel stride ldy floats), i.e. straight into the next layer's concat buffer.
 * x [N][H][W][Cin] channels-last, Cin % 16 == 0 (zero-padded channels carry zero weights);
 * w_packed: nrgbd_conv_pack_weights of w [Cout][Cin][taps], taps = 9 (modes 0, 2) or 4 (mode 1: the phase's 2x2 taps in
 *   row-major order of the input neighbourhood {y-1+pa, y+pa} x {x-1+pb, x+pb}); Cout in {64, 96, 128} (mode 0), 64 (mode 1),
 *   {64, 128} (mode 2); wider layers are launched as several output-column slices (ycoff);
 * bias [Cout] (padded) or NULL.  mode 0: y[pix*ldy + ycoff + c], c < cout_valid.  mode 1: the same at output pixel
 *   (2y+pa, 2x+pb) of a [N][2H][2W] tensor.  mode 2: y = planar [N][Cout][H][W] log-probabilities (ldy.. ignored).
 * nrgbd_rnet_pack: out [P][D+Cf] = (exp(dpv_log [D][P]), feat) — the R-Net's first concat with torch.exp fused
 *   (models/KVNET.py:128,176 + Refine.py:88); feat is [P][Cf] (feat_planar = 0) or [Cf][P].
 */
int nrgbd_conv2d_rnet_f32(const float* x, const float* w_packed, const float* bias, int out_lrelu, float* y,
                          int ldy, int ycoff, int cout_valid, int mode, int pa, int pb,
                          int N, int H, int W, int Cin, int Cout, void* stream);
int nrgbd_rnet_pack(const float* dpv_log, const float* feat, int feat_planar, float* out, int D, int Cf, long P,
                    void* stream);

/*
 * Feature CNN (and R-Net form): 3x3 convolution, stride 1, padding = dilation, on the fp32 matrix cores with the
 * BatchNorm2d / ReLU / residual work fused around it — the 2-D sibling of nrgbd_conv3d_3x3x3_f32.
 * Replaces, per trunk layer of models/psm_submodule.py:90-167 (feature_extraction; convbn :10-16, BasicBlock :31-50):
 * nn.Conv2d(bias=False) + nn.BatchNorm2d (batch statistics) + nn.ReLU + `out += x`; with (bias, out_lrelu) it is the
 * conv2d_leakyRelu of models/m_submodule.py:18-27 used by the R-Net (Refine.py:36-71).
 *
 * Activations are channels-last [N][H][W][C].  A layer reads its input as
 *       in = act(x * s + t)  [+ act(res * s' + t')]          (s,t per channel; act = ReLU or identity)
 * `materialized` (optional) receives `in`.  y = conv(in) (+ bias, LeakyReLU 0.01 if out_lrelu) and
 *   stats [nrgbd_conv2d_workgroups(N,H,W)][2*Cout] = per-workgroup sum of y, then sum of y^2, per channel.
 *   w_packed: nrgbd_conv_pack_weights(w [Cout][Cin][3][3], taps = 9) -> [9*Cin*Cout] floats
 *   Cin % 16 == 0; (Cout, dilation) in {(32,1), (64,1), (96,1), (128,1), (128,2)}; N*H*W*Cin < 2^32.
 * nrgbd_bn_finalize: partials [num_workgroups][2*C] -> scale_shift [C][2] = (gamma*invstd, beta - mean*gamma*invstd),
 *   reduced in double; running_mean / running_var (both or neither) get the train-mode update.
 *   VARIANCE COLLAPSE (all three finalisers, i.e. wherever the statistics are unshifted fp32 partials of a long reduction: the
 *   feature-CNN trunk, its 1x1 shortcuts and the K-Net; NOT the SPP branches, which use nrgbd_bn_small_stats): the variance is
 *   E[y^2] - mean^2 over fp32 per-tile partials; a channel whose computed
 *   variance is below 1e-5 mean^2 (std / |mean| < 3.2e-3: no correct digit left; the reference's two-pass statistics would still
 *   normalise it) gets scale = shift = NaN AND is counted into *collapse_count (device word, may be NULL; atomicAdd of 1 per
 *   channel) — the kernels' ReLU maps NaN to 0, so the NaN alone could vanish again; the host mirror raises on a non-zero word.
 *   batches_tracked (device int64, may be NULL): nn.BatchNorm's `num_batches_tracked += 1` side effect, done by the finaliser.
 * nrgbd_nhwc_stats: the same partials for a channels-last tensor produced elsewhere (the stride-2 / 1x1 layers that
 *   stay on the vendor library): x [P][C], stats [nrgbd_nhwc_stats_workgroups(P)][2*C]; C in {32, 64, 128}.
 * nrgbd_nhwc_act: y[p*ldy + c] = act(x*s+t) [+ act(res*s'+t')] — the loader's prologue as a stand-alone pass, for
 *   consumers that are not the conv kernel (pooling, the SPP concat of psm_submodule.py:160-163, the 1x1 head).
 * nrgbd_nhwc_act_lean: the same pass, the same bits, in a shape that shares a CU with a matrix-bound convolution of another
 *   stream: wg_per_cu (1 .. 8, else NRGBD_E_ARG) workgroups of one wave per SIMD per CU walk the tensor with a grid stride, 32
 *   registers per lane, 16 * C bytes of LDS.  wg_per_cu = 1 beside a convolution, more when the pass runs alone.  C a power of two
 *   in 4 .. 1024, P <= 2^30, ldy <= 2^22 (NRGBD_E_SHAPE otherwise); x, res and y 16-byte aligned (NRGBD_E_ALIGN).
 */
/*
 * nrgbd_conv2d_taps_f32 — the trunk's remaining convolution forms on the same kernel (round 2: no vendor convolution is left in
 * the feature CNN), with the prologue (x_ss, x_relu) and the statistics epilogue of nrgbd_conv2d_3x3_f32:
 *   taps = 1: 1x1 convolution (psm_submodule.py:40-43,63-66 shortcut of layer2 / layer3, :103-117 SPP branch convs, :122 head);
 *             w_packed = nrgbd_conv_pack_weights(w [Cout][Cin][1], taps = 1); Cout in {32, 64, 128}; in_stride = s > 1: the
 *             convolution's own stride — x is [N][H*s][W*s][Cin], output pixel (y, x) reads input pixel (y*s, x*s) (no gather pass)
 *   taps = 4: the 2x2 window {y-1, y} x {x-1, x} — a stride-2, pad-1 3x3 convolution (psm_submodule.py:90 firstconv, :120
 *             layer2's first conv) on the space-to-depth image of its input (nrgbd_space_to_depth2), weights re-indexed by the
 *             host mirror (neuralrgbd_amd/ops.py::conv_s2_pack); Cout in {32, 64}
 * nrgbd_space_to_depth2: y [N][H/2][W/2][Cp] with y[.][(py*2+px)*C + c] = x[2y+py][2x+px][c], channels >= 4C zero;
 *   x is [N][C][H][W] (nchw = 1: the input image) or [N][H][W][C]; H, W even, Cp >= 4C.
 */
int nrgbd_conv2d_taps_f32(const float* x, const float* x_ss, int x_relu, const float* w_packed, float* y, float* stats,
                          int N, int H, int W, int Cin, int Cout, int taps, int in_stride, void* stream);
int nrgbd_space_to_depth2(const float* x, int nchw, float* y, int N, int C, int H, int W, int Cp, void* stream);
/*
 * nrgbd_conv2d_wgrad_f32 — weight gradient of a 3x3 stride-1 convolution (padding = dilation in {1, 2}) on channels-last
 * activations, on the fp32 matrix cores (training: train_utils/train_KVNet.py:103-153 back-propagating through
 * models/psm_submodule.py:10-16,31-50 and models/Refine.py:51-107):
 *   dw [Cout][Cin][3][3] = sum over (n, y, x) of gy[n][y][x][co] * x[n][y+(ky-1)d][x+(kx-1)d][ci]
 * x [N][H][W][Cin], gy [N][H][W][Cout]; Cin % 16 == 0, Cout % 16 == 0.
 * partial: workspace of ceil(Cout/64) * ceil(Cin/64) * nrgbd_conv2d_wgrad_workgroups(N,H,W,Cin,Cout) * 9*64*64 floats (per-workgroup
 * partial sums, reduced in a fixed order: bitwise reproducible).  The data gradient of the same convolution is the forward
 * kernel on gy with the transposed, flipped weights.
 */
int nrgbd_conv2d_wgrad_workgroups(int N, int H, int W, int Cin, int Cout);
int nrgbd_conv2d_wgrad_f32(const float* x, const float* gy, float* partial, float* dw, int N, int H, int W, int Cin, int Cout,
                           int dilation, void* stream);
int nrgbd_conv2d_workgroups(int N, int H, int W);
int nrgbd_conv_pack_weights(const float* w, float* w_packed, int Cin, int Cout, int taps, void* stream);
int nrgbd_conv2d_3x3_f32(const float* x, const float* x_ss, int x_relu,
                         const float* res, const float* res_ss, int res_relu,
                         float* materialized, const float* w_packed, const float* bias, int out_lrelu,
                         float* y, float* stats, int N, int H, int W, int Cin, int Cout, int dilation,
                         void* stream);
int nrgbd_bn_finalize(const float* stats, int num_workgroups, int C, long count,
                      const float* gamma, const float* beta, float eps, float momentum,
                      float* running_mean, float* running_var, float* scale_shift, unsigned int* collapse_count, long long* batches_tracked, void* stream);
/*
 * nrgbd_spp_concat — the tail of the feature CNN's spatial-pyramid pooling in one channels-last pass.
 * Replaces: models/psm_submodule.py:149-161 — for the four branches nn.ReLU after convbn (:100-117 branch1..4), F.upsample(
 * bilinear, align_corners=True) (:153-158), and the torch.cat of (output_raw, output_skip, branch4, branch3, branch2, branch1)
 * (:160).  out[pixel] = [ quarter (Cq) | deep (Cd) | up(relu(bz0 * s + t)) | up(.. bz1) | up(.. bz2) | up(.. bz3) ].
 *   quarter [N][h][w][Cq], deep [N][h][w][Cd]; branch i: raw 1x1-conv output bz_i [N][bh_i][bw_i][Cb] and the (scale, shift)
 *   [Cb][2] of its BatchNorm (nrgbd_bn_small_stats); out [N][h][w][Cq + Cd + 4 Cb]; all channel counts % 4 == 0,
 *   Cq + Cd + 4 Cb <= 512 (a workgroup = four pixels' 16-byte words: 320 channels in models/psm_submodule.py), h, N <= 65535.
 * Interpolation arithmetic = ATen upsample_bilinear2d (fp32 scale (in-1)/(out-1), lambda clamped to [0,1]).
 */
/*
 * nrgbd_bn_small_stats — BatchNorm batch statistics of up to four SMALL channels-last maps in one launch: the SPP branches of the
 * feature CNN (models/psm_submodule.py:100-117 convbn behind AvgPool2d((64,64)) .. ((8,8)); the reference never leaves train
 * mode, so their BatchNorm2d normalises with the statistics of the V + 1 frames: 5 values per channel at the 64-window of a
 * 256x384 image).  Segment i: x[i] [rows[i]][C] contiguous (the raw 1x1-conv output of nrgbd_conv2d_taps_f32, no statistics
 * epilogue needed) -> scale_shift[i] [C][2] = (gamma*invstd, beta - mean*gamma*invstd), the operand of nrgbd_spp_concat.
 *   Mean and variance are sums in double over the values themselves, shifted by the channel's row-0 value k (sum (y - k),
 *   sum (y - k)^2): ~50 correct bits
 *   relative even when the five frames of a static camera agree to a few ulps, where E[y^2] - mean^2 has no digit left.  So
 *   there is no collapse guard and no status word: an exactly constant channel normalises to beta, as in the reference.
 *   running_mean / running_var (arrays of nseg pointers or NULL; per segment both or neither): the train-mode update with
 *   momentum[i] and the unbiased variance; batches_tracked (NULL or nseg pointers, each may be NULL): `+= 1`.
 *   nseg in 1..4, 1 <= C <= 1024, rows[i] >= 1.  The pointer arrays are host memory read during the call (capture-safe).
 */
int nrgbd_bn_small_stats(int nseg, const float* const* x, const long* rows, int C, const float* const* gamma, const float* const* beta,
                     const float* eps, const float* momentum, float* const* running_mean, float* const* running_var,
                     long long* const* batches_tracked, float* const* scale_shift, void* stream);
int nrgbd_spp_concat(const float* quarter, int Cq, const float* deep, int Cd,
                     const float* bz0, const float* bss0, int bh0, int bw0, const float* bz1, const float* bss1, int bh1, int bw1,
                     const float* bz2, const float* bss2, int bh2, int bw2, const float* bz3, const float* bss3, int bh3, int bw3,
                     int Cb, float* out, int N, int h, int w, void* stream);
/*
 * nrgbd_logsoftmax_rows — log_softmax over the channels of channels-last rows x [rows][C] (y may be x), C in {64, 128, 256}.
 * Replaces: F.log_softmax(conv2_2_out, dim=1) of models/Refine.py:104 once the last R-Net convolution runs on the Winograd kernel
 * (nrgbd_conv_wino_rnet_ex_f32), whose pixels are channels-last; the refined DPV is then an [N, D, H, W] VIEW of that memory.
 * C = 256: the up-sampled volume of a 64-candidate net (Refine.py:44-49), one wave per row.
 */
int nrgbd_logsoftmax_rows(const float* x, float* y, long rows, int C, void* stream);
/*
 * nrgbd_logsoftmax_d_bwd / nrgbd_logsoftmax_rows_bwd — backward of nrgbd_logsoftmax_d / nrgbd_logsoftmax_rows (training path):
 * with out = log_softmax(z), g_z = g - exp(out) * sum_k g (the _d form returns scale * g_z = the gradient of its operand a;
 * scale = 1 gives the gradient of b).  Replaces: autograd through torch.log_softmax at models/basic.py:299-300,
 * models/KVNET.py:172-173 and models/Refine.py:104 (ATen's SpatialSoftMaxBackward).
 *   _d:    logp, g, gz [D][n];   _rows: y, g, gx [rows][C], C in {64, 128, 256}
 */
int nrgbd_logsoftmax_d_bwd(const float* logp, const float* g, float scale, float* gz, int D, long n, void* stream);
int nrgbd_logsoftmax_rows_bwd(const float* y, const float* g, float* gx, long rows, int C, void* stream);
/*
 * nrgbd_nll_fwd / nrgbd_nll_bwd — F.nll_loss(logp [1, D, h, w], target [1, h, w], ignore_index) with mean reduction and its
 * backward.  Replaces: the four loss terms of train_utils/train_KVNet.py:103-120 (ignore_index = 0: pixels without ground truth).
 *   logp: planar [D][n] (channels_last = 0) or channels-last [n][D] (= 1: the refined DPV as the R-Net writes it); target [n] int64.
 *   fwd:  partial [nrgbd_nll_workgroups(n)][2] scratch; out[0] = mean over the counted pixels (NaN when there is none, as ATen),
 *         out[1] = their number.  A target outside [0, D) is not counted (ATen asserts).  Fixed summation order.
 *   bwd:  g_out [1] (device), stat = fwd's out; g_logp in logp's layout, every element written (zeros off the target).
 */
int nrgbd_nll_workgroups(long n);
int nrgbd_nll_fwd(const float* logp, const long long* target, long ignore_index, int D, long n, int channels_last,
                  float* partial, float* out, void* stream);
int nrgbd_nll_bwd(const long long* target, long ignore_index, const float* g_out, const float* stat, float* g_logp, int D,
                  long n, int channels_last, void* stream);
/*
 * nrgbd_adam_step — torch.optim.Adam's update (no amsgrad) of a LIST of fp32 tensors, 48 tensors per launch with their pointers passed
 * by value (nothing is uploaded: the launches can be captured into a hipGraph).  Replaces: optimizer_KV.step() of
 * train_utils/train_KVNet.py:153 for the optim.Adam of train_KVNet.py:228-232 (ATen: ~50 _foreach_ launches per step).
 *   params / grads / exp_avg / exp_avg_sq / steps: HOST arrays of `ntensors` DEVICE pointers; numel: host array of element counts.
 *   steps[i] points to tensor i's step counter (a device float: completed steps), read as t = *steps[i] + 1 and then incremented.
 *   Arithmetic = torch.optim.adam._single_tensor_adam, fp32, scalar factors formed in double:
 *     g' = (maximize ? -g : g) + weight_decay * p;  m += (g' - m)(1 - beta1);  v = v beta2 + (1 - beta2) g'^2;
 *     p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 */
int nrgbd_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                    float* const* steps, const long* numel, int ntensors, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int maximize, void* stream);
/*
 * nrgbd_grad_norm — the global L2 norm of a LIST of fp32 tensors and the clipping coefficient for it, on the tensor-list idiom of
 * nrgbd_adam_step (48 pointers per launch by value; nothing is allocated or uploaded, no atomics, no host synchronisation: capturable
 * into a hipGraph, and the same bits in every run, on every stream and at every grid size).  Replaces: the first half of
 * torch.nn.utils.clip_grad_norm_(model_KVnet.parameters(), grad_clip_max) of train_utils/train_KVNet.py:143-145,180-181 (ATen:
 * _foreach_norm over ~460 tensors, a stack and a norm).
 *   grads: HOST array of `ntensors` DEVICE pointers; numel: host array of element counts (each in (0, 2^30]).
 *   workspace: nrgbd_grad_norm_workspace(numel, ntensors) bytes on the device (a negative code for a bad list): one fp32 partial per
 *   2,048-element chunk of every tensor, at the chunk's index in list order.
 *   Summation order: in a chunk, thread t of 256 adds the squares of elements t, t + 256, ..., t + 1792 in that order, a wave64
 *   xor-shuffle tree (offsets 32, 16, ..., 1) adds the 64 lanes, ((w0 + w1) + w2) + w3 adds the four waves — all fp32, 17 roundings on
 *   the longest path.  One workgroup then adds all partials in double (thread t: partials t, t + 256, ... in order; the same tree).
 *   clip [4] (device): clip[0] = total_norm = (float)sqrt(sum);  clip[1] = coef = (float)min(1.0, max_norm / ((double)total_norm + 1e-6))
 *   (clip_grad_norm_'s clip_coef clamped to 1; a NaN stays a NaN);  clip[2] = 1.0f if total_norm is inf or NaN, else 0.0f;  clip[3] = 0.
 *   nonfinite_steps (device float, may be NULL): += 1.0f when clip[2] is set — once per call.
 *   max_norm = +inf gives coef = 1 (the norm alone); max_norm <= 0 or NaN: NRGBD_E_SHAPE.  A workspace that is too small:
 *   NRGBD_E_SHAPE; a NULL pointer: NRGBD_E_NULL.  Every argument is checked before the first launch.
 * nrgbd_scale_tensors — t[i] *= clip[1] in place over a tensor list (one rounded fp32 multiply per element = torch.mul): the second
 * half of clip_grad_norm_ (ATen: _foreach_mul_), for an optimizer other than nrgbd_adam_step_clipped.
 * nrgbd_adam_step_clipped — nrgbd_adam_step on g * clip[1] (the product is formed as the gradient is read: the same bits as
 * nrgbd_scale_tensors followed by nrgbd_adam_step, and the gradients in memory stay as they are; maximize and weight_decay apply to
 * the scaled gradient, as in torch).  skip_nonfinite = 1: when clip[2] is set the launch writes nothing — parameters, both moments and
 * the step counters stay as they were.  skip_nonfinite = 0: the arithmetic goes through as in torch (coef is 0 or NaN: inf * 0 = NaN
 * reaches the parameters).
 */
long nrgbd_grad_norm_workspace(const long* numel, int ntensors);
int nrgbd_grad_norm(const float* const* grads, const long* numel, int ntensors, double max_norm, void* workspace,
                    size_t workspace_bytes, float* clip, float* nonfinite_steps, void* stream);
int nrgbd_scale_tensors(float* const* tensors, const long* numel, int ntensors, const float* clip, void* stream);
int nrgbd_adam_step_clipped(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                            float* const* steps, const long* numel, int ntensors, double lr, double beta1, double beta2, double eps,
                            double weight_decay, int maximize, const float* clip, int skip_nonfinite, void* stream);
/*
 * nrgbd_bias_lrelu_cl_fwd / _bwd — y = leaky_relu(x + bias[c], slope) on channels-last rows [rows][C] and its backward
 * (training path of the R-Net).  Replaces: the bias add + nn.LeakyReLU of m_submodule.conv2d_leakyRelu /
 * conv2dTranspose_leakyRelu (models/m_submodule.py:18-27,36-45; slope = 1: the bias of Refine.py:71) and, in backward, ATen's
 * leaky_relu_backward + the bias gradient's sum.  backward: gx = gy * (y > 0 ? 1 : slope) (y = the forward's OUTPUT),
 * g_bias[c] = sum over rows of gx; partial = scratch of nrgbd_bias_lrelu_cl_workgroups(rows, C) x C floats (added in index
 * order, in double).  C % 4 == 0, C <= 1024.
 */
int nrgbd_bias_lrelu_cl_workgroups(long rows, int C);
int nrgbd_bias_lrelu_cl_fwd(const float* x, const float* bias, float slope, float* y, long rows, int C, void* stream);
int nrgbd_bias_lrelu_cl_bwd(const float* y, const float* gy, float slope, float* gx, float* g_bias, float* partial,
                            long rows, int C, void* stream);
/*
 * nrgbd_upsample_bilinear_ac — bilinear up-sampling with align_corners = True of a channels-last map and its exact adjoint
 * (training path of the SPP branches).
 * Replaces: F.upsample(mode='bilinear') of models/psm_submodule.py:153-158 and its autograd backward (ATen
 * upsample_bilinear2d_backward: an atomic scatter).  backward = 0: x [N][bh][bw][C] -> y [N][H][W][C];
 * backward = 1: x = gradient of the output [N][H][W][C] -> y = gradient of the input [N][bh][bw][C], every input element summed
 * by one thread in a fixed order with the forward's own fp32 weights.  C % 4 == 0.
 */
int nrgbd_upsample_bilinear_ac(const float* x, float* y, int N, int bh, int bw, int H, int W, int C, int backward,
                               void* stream);
/*
 * nrgbd_frame_ingest_u8 — one uint8 camera frame -> the normalised fp32 planar image [3][Hout][Wout] of the network, written into a
 * caller-given slot (a frame ring: neuralrgbd_amd/video.py).  Replaces: the loaders' image preparation — PIL.Image.NEAREST resize
 * to the network size, ToTensor, Normalize (mdataloader/scanNet.py:368-369,429-430; utils/preprocess.py:14-35) — and the upload of its
 * fp32 result (12 bytes per pixel against 3).
 *   src     DEVICE uint8.  layout 0 = HWC interleaved: channel c of pixel (y, x) at src[y * pitch + 3 x + c], pitch >= 3 Win bytes
 *           (padded camera rows are fine);  layout 1 = CHW planar: src[(c * Hin + y) * pitch + x], pitch >= Win.
 *   dst     [3][Hout][Wout] fp32, 16-byte aligned; only these 3 Hout Wout elements are written (Wout need not be a multiple of 4).
 *   value   ((float)u / 255.0f - mean_c) / std_c, two IEEE fp32 divisions in this order: ToTensor then Normalize, bit for bit.
 *   resize  when (Hin, Win) != (Hout, Wout): nearest at pixel centres, in integers — sy = ((2 y + 1) Hin) / (2 Hout),
 *           sx = ((2 x + 1) Win) / (2 Wout): PIL.Image.resize(..., NEAREST).
 *   errors  NRGBD_E_NULL: src / dst;  NRGBD_E_SHAPE: a dimension <= 0 or > 16384, a pitch below the row;  NRGBD_E_ARG: layout not
 *           0 / 1, a std that is 0 or not finite (or a mean that is not finite);  NRGBD_E_ALIGN: dst not 16-byte aligned.
 * nrgbd_window_gather — the temporal window out of the frame ring in one launch: a plain copy, bit-equal to torch.stack of the slots.
 * Replaces: split_frame_list + the list of source images of test_KVNet.py:195,213 (ATen: torch.cat / per-tensor copy_).
 *   ring    [R] images of [3][H][W] fp32, image s at ring + s * slot_stride (slot_stride >= 3 H W elements)
 *   slots   idx[0 .. V - 1] = the ring slots of the sources in window order, idx[V] = the slot of the reference; 1 <= V <= 6
 *   src     [V][3][H][W], ref [3][H][W]: every element written.  16 bytes per lane when 3 H W and slot_stride are multiples of 4 and
 *           the three pointers are 16-byte aligned, one element per lane otherwise.
 *   errors  NRGBD_E_NULL;  NRGBD_E_SHAPE: V outside 1 .. 6, a slot outside [0, R), R / H / W <= 0 or H / W > 16384, a short slot_stride.
 */
#define NRGBD_GATHER_MAX_V   6
typedef struct { int idx[NRGBD_GATHER_MAX_V + 1]; } nrgbd_window_slots;
int nrgbd_frame_ingest_u8(const unsigned char* src, int Hin, int Win, long pitch, int layout, float mean0, float mean1, float mean2,
                          float std0, float std1, float std2, float* dst, int Hout, int Wout, void* stream);
int nrgbd_window_gather(const float* ring, int R, long slot_stride, nrgbd_window_slots slots, int V, float* src, float* ref,
                        int H, int W, void* stream);
/*
 * nrgbd_depth_ingest_u16 — one uint16 ground-truth depth frame -> the labels and the metric maps of a training step, one launch.
 * Replaces: the loaders' depth preparation (mdataloader/scanNet.py:372-422: PIL NEAREST resizes of the frame and of its hole mask,
 * `.float() * .001`, the digitising of mdataloader/misc.py:13-36 = np.digitize against float64 candidates, the clamp to
 * [0, n - 1]) and the upload of its int64 results.  Every output is the loaders' result bit for bit.
 *   depth        device, [Hin] rows of Win uint16 (raw units, ScanNet: millimetres), row r at depth + r * pitch (elements);
 *                0 = a hole (`raw < 0.01`, scanNet.py:373)
 *   rows_full [H], cols_full [W]   device int32: source row / column of every row / column of the image-size maps (scanNet.py:378)
 *   rows_q [h], cols_q [w]         the same for the direct resize to the plane-sweep grid (scanNet.py:388)
 *   mask_rows_q [h], mask_cols_q [w]   source row / column of the grid-size hole mask: the image-size table composed with the
 *                image -> grid table, because the reference resizes the mask twice (scanNet.py:374-375,389)
 *                The tables are the caller's because PIL's NEAREST accumulates a double per output index — idx = (int)xo, xo += s from
 *                xo = 0.5 s, s = (double)n_in / n_out — and no integer formula gives that for every pair of sizes.  An entry outside
 *                the frame is clamped to it (never read out of bounds).
 *   depth_scale  metres per raw unit (.001), finite and > 0; metres = (float)u * depth_scale, one fp32 product
 *   thr_q [n_q], thr_full [n_full]   HOST int32, read before the call returns: non-decreasing thresholds in [0, 65536] with
 *                label(u) = min(#{k : thr[k] <= u}, n - 1), thr[k] = the smallest u whose metres, as a double, are >= d_candi[k]
 *                (65536: none) — np.digitize followed by the loaders' clamp, in integers.  1 <= n <= NRGBD_DEPTH_MAX_THRESHOLDS.
 *                n_full is D, or 4 D for `dmap_up4_imgsize_digit` (scanNet.py:419-421).
 *   labels_q [h][w] int64 (`dmap`), labels_full [H][W] int64 (`dmap_imgsize_digit` / `dmap_up4_imgsize_digit`),
 *   dmap_raw [h][w] fp32, dmap_imgsize [H][W] fp32 (masked metres): each may be NULL (not computed), not all four.
 *                16 bytes per lane and store where a map's width is a multiple of 4 and its base 16-byte aligned, element stores
 *                otherwise.  A grid pixel under a hole of the twice-resized mask is 0.0 / label(0).
 *   errors       NRGBD_E_ARG: a NULL input or table, all four outputs NULL, a size <= 0 or > 16384, pitch < Win, n outside
 *                1 .. 512, thresholds that decrease or leave [0, 65536], a depth_scale that is not finite and positive.
 */
#define NRGBD_DEPTH_MAX_THRESHOLDS 512
int nrgbd_depth_ingest_u16(const unsigned short* depth, int Hin, int Win, long pitch, const int* rows_full, const int* cols_full,
                           const int* rows_q, const int* cols_q, const int* mask_rows_q, const int* mask_cols_q, float depth_scale,
                           const int* thr_q, int n_q, const int* thr_full, int n_full, long long* labels_q, long long* labels_full,
                           float* dmap_raw, float* dmap_imgsize, int H, int W, int h, int w, void* stream);
int nrgbd_nhwc_stats_workgroups(long P);
int nrgbd_nhwc_stats(const float* x, long P, int C, float* stats, void* stream);
int nrgbd_nhwc_act(const float* x, const float* x_ss, int x_relu, const float* res, const float* res_ss,
                   int res_relu, float* y, long P, int C, int ldy, void* stream);
int nrgbd_nhwc_act_lean(const float* x, const float* x_ss, int x_relu, const float* res, const float* res_ss,
                        int res_relu, float* y, long P, int C, int ldy, int wg_per_cu, void* stream);
/*
 * On-device depth evaluation (depth_eval.hip; neuralrgbd_amd/evaluate.py): the error metrics of a depth map against ground truth
 * as sums and counts that stay on the device, per confidence set.  Replaces: the host evaluation of test_utils/export_res.py:108-116
 * (the maps downloaded, `dmap_ref > 0` as the mask, `np.abs(dmap_ref - dmap) * mask` in numpy) and the offline scoring behind it.
 *
 * nrgbd_depth_eval_workgroups — export_res.py:108-116: the partial records the first launch of nrgbd_depth_eval writes for n
 *   pixels (a function of n alone, non-decreasing in n); NRGBD_E_SHAPE for n <= 0 or n > 2^40.
 * nrgbd_depth_eval_workspace — export_res.py:108-116: the bytes nrgbd_depth_eval needs for n pixels and J confidence sets
 *   (non-decreasing in both); NRGBD_E_SHAPE for a bad n or J outside 1 .. NRGBD_DEPTH_EVAL_MAX_SETS.
 * nrgbd_depth_eval — export_res.py:108-116: one map against its ground truth, two launches, no synchronisation, no atomics; the same
 *   inputs give the same bits in every run.
 *   depth, logconf, gt   device fp32 [n]: the expected depth and max_k logp as nrgbd_depth_regress / _rows write them, and the ground
 *                truth in metres, 0 = a hole.  With d, m, g the three values of a pixel:
 *                  gt-valid  g > 0 && g >= gt_min && g <= gt_max (a NaN g is not valid)
 *                  bad       gt-valid and not (d > 0, d finite, m not NaN): counted in the header, enters no metric
 *                  set j     the pixels with m >= log_thr[j], fp32 against fp32
 *   log_thr      HOST fp32 [J], read and checked at the call: strictly ascending, log_thr[0] = -inf (set 0 holds every pixel)
 *   terms        in double from the promoted fp32 values, in this operation sequence: e = d - g; a = fabs(e); t0 = a; t1 = a / g;
 *                t2 = (e * e) / g; t3 = e * e; q = d / g; l = log(q); t4 = l * l; t5 = l; r = max(q, g / d); the delta counts are
 *                r < 1.25, r < 1.5625, r < 1.953125
 *   frame_sums   float64 [J][6] = the sums of t0 .. t5 over set j;  frame_counts int64 [J][4] = n, delta1, delta2, delta3 of set j;
 *   frame_header int64 [4] = 1, gt-valid pixels, bad pixels, 0: this call's record, every element written
 *   total_*      the same three records, total = total + frame (the caller zeroes them); all three given or all three NULL
 *   err_map      fp32 [n] or NULL: fabsf(g - d) where g > 0, else 0.f — export_res.py:113-116 on fp32 maps, independent of the
 *                range and of the confidence
 *   workspace    8-byte aligned, at least nrgbd_depth_eval_workspace(n, J) bytes; rewritten by every call
 *   errors       NRGBD_E_NULL: a NULL required pointer, or only some of total_*;  NRGBD_E_SHAPE: a bad n or J, a workspace that is
 *                too small;  NRGBD_E_ARG: log_thr[0] != -inf, a NaN threshold, thresholds not ascending, gt_min <= gt_max not true
 *                (a NaN bound included);  NRGBD_E_ALIGN: the workspace.  Every argument is checked before the first launch.
 */
#define NRGBD_DEPTH_EVAL_MAX_SETS 8
int nrgbd_depth_eval_workgroups(long n);
long nrgbd_depth_eval_workspace(long n, int J);
int nrgbd_depth_eval(const float* depth, const float* logconf, const float* gt, long n, float gt_min, float gt_max,
                     const float* log_thr, int J, void* workspace, long workspace_bytes, double* frame_sums,
                     long long* frame_counts, long long* frame_header, double* total_sums, long long* total_counts,
                     long long* total_header, float* err_map, void* stream);
/*
 * nrgbd_dgf_refine_f32 — the guided-filter refinement net of KVNET(refineNet_name='DGF') in one launch (dgf.hip;
 * neuralrgbd_amd/nets.py: DGFRefineNet).  Replaces models/Refine.py:620-641 (RefineNet_DGF.forward), models/GF/guided_filter.py:54-97
 * and models/GF/box_filter.py: bilinear up-sampling of the regressed low-resolution depth (align_corners = True), the per-pixel
 * 3 -> 64 -> 1 network on the image as the guide, and a radius-1 guided filter.  The function is the reference's; the arithmetic is
 * the centred form (direct sums over the clipped 3 x 3 window, var = sum (x - mx)^2 / N), because the reference's own fp32 form
 * (differences of cumsums, E[x^2] - E[x]^2) cancels: its fp32 bits are not reproduced, its float64 values are (README, "DGF").
 *   depth_lr   device fp32 [n][h][w], n in {1, 2} targets that share one guide
 *   img        device fp32 [3][H][W], planar and contiguous; H = s h and W = s w for one integer s >= 2; H, W in 4 .. 16384
 *   w1 [64][3], b1 [64], w2 [64], b2 [1]   the two 1 x 1 convolutions of RefineNet_DGF.feature_ext, read in place
 *   eps        the filter's regulariser (the reference: 1e-8)
 *   out        device fp32 [n][H][W], every element written; any alignment (16-byte stores where the address allows, element stores
 *              otherwise: the same bits)
 * Per pixel, in fp32 and in this order (every division an IEEE division): y = the bilinear sample with integer coordinates
 * (num = i (h - 1), i0 = num / (H - 1), lam = float(num % (H - 1)) / float(H - 1), i1 = min(i0 + 1, h - 1); the same along columns;
 * y = (1 - lr) ((1 - lc) d00 + lc d01) + lr ((1 - lc) d10 + lc d11));  x = b2 + sum_k w2[k] max(0, b1[k] + w1[k][0] r + w1[k][1] g +
 * w1[k][2] b), k ascending, fused multiply-adds;  over the 3 x 3 window clipped to the image (N = 4, 6 or 9 pixels, row-major sums):
 * mx = sum x / N, my = sum y / N, var = sum (x - mx)^2 / N, cov = sum (x - mx)(y - my) / N, A = cov / (var + eps), b = my - A mx;
 * out = (sum A / N) x + (sum b / N).  A target's bits do not depend on n.  No atomics, no workspace: capturable, the same bits in
 * every run.
 *   errors     NRGBD_E_NULL: a NULL pointer;  NRGBD_E_SHAPE: an extent <= 0 or above 16384, H, W not one common integer multiple
 *              s >= 2 of h, w, H <= 3 or W <= 3 (guided_filter.py:74);  NRGBD_E_ARG: n outside {1, 2}, eps negative or NaN.
 *              Every argument is checked before anything touches the device.
 */
#define NRGBD_DGF_TILE_Y 16
#define NRGBD_DGF_TILE_X 64
int nrgbd_dgf_refine_f32(const float* depth_lr, int n, int h, int w, const float* img, int H, int W,
                         const float* w1, const float* b1, const float* w2, const float* b2, float eps,
                         float* out, void* stream);
/*
 * TSDF fusion (tsdf.hip; neuralrgbd_amd/fusion.py: TSDFVolume, FusionVideoStream): the depth maps of a trajectory accumulated in
 * the world frame as a dense truncated-signed-distance volume on the device, and the volume's surface as points and as a triangle
 * mesh.  None of the entries has a counterpart in the reference, which drops every map after export; the conventions are the ones written here.
 * Everything is fp32, every operation below is ONE IEEE fp32 operation in the order written (no fused multiply-add, no reciprocal),
 * there are no atomics, and the same inputs give the same bits in every run.
 *
 * The volume: two planar device arrays tsdf [Z][Y][X] and weight [Z][Y][X], X fastest; lattice point (ix, iy, iz) lies at the world
 * position origin + voxel_size (ix, iy, iz); a fresh volume is tsdf = 0, weight = 0.
 *
 * nrgbd_tsdf_integrate_f32 — no counterpart in the reference: one depth frame into the volume, one launch, capturable.
 *   depth        device fp32 [H][W]: z-depth in metres (rays have z = 1, the convention of unit_ray_array)
 *   gate         device fp32 [H][W] or NULL: a pixel counts where gate >= gate_thr (a NaN fails); e.g. max_k logp against log c
 *   wmap         device fp32 [H][W] or NULL (= 1): the weight of a pixel's observation
 *   pose         HOST fp32 [12], read at the call: float32(extM[:3,:4]) row-major, world -> camera (r00 r01 r02 tx | r10 ...)
 *   fx fy cx cy  the pinhole intrinsics at the depth map's size; pixel x covers [x, x + 1) (centres at + 0.5)
 *   box          HOST int [6] = x0, y0, z0, x1, y1, z1, a half-open voxel box, read at the call, or NULL = the whole grid
 *   per voxel of the box, with T, Wt its two stored values:
 *     xw = ox + vs * (float)ix                              (likewise yw, zw)
 *     xc = ((r00 * xw + r01 * yw) + r02 * zw) + tx          (likewise yc, zc with rows 1 and 2)
 *     skip unless zc > 0
 *     u = fx * (xc / zc) + cx;  v = fy * (yc / zc) + cy
 *     skip unless u >= 0 && u < (float)W && v >= 0 && v < (float)H       (a NaN fails)
 *     iu = (int)floorf(u);  iv = (int)floorf(v);  d = depth[iv][iu];  skip unless d is finite, d > d_near, d <= d_far
 *     skip unless gate[iv][iu] >= gate_thr  (when given);   w = wmap ? wmap[iv][iu] : 1;  skip unless w is finite and w > 0
 *     s = d - zc;  skip if s < -trunc;  t = fminf(1, s / trunc)
 *     T' = (T * Wt + t * w) / (Wt + w);  W' = fminf(Wt + w, w_max)
 *   A skipped voxel keeps its bits.  Four x-neighbours per lane with 16-byte loads and stores when X % 4 == 0 and both arrays are
 *   16-byte aligned, one voxel per lane otherwise: the same bits.
 *   errors       NRGBD_E_NULL: tsdf, weight, depth or pose NULL;  NRGBD_E_SHAPE: a dimension <= 0, X Y Z > 2^31, a box that leaves
 *                the grid or is empty;  NRGBD_E_ARG: voxel_size, trunc or w_max <= 0 or not finite, d_near < d_far not true (a NaN
 *                bound included).  Checked in this order, before anything touches the device.
 * nrgbd_tsdf_extract_workspace — no counterpart in the reference: the bytes nrgbd_tsdf_extract_points needs for an X Y Z grid
 *   (16 per NRGBD_TSDF_EXTRACT_VOXELS voxels; needs no GPU); NRGBD_E_SHAPE as above.
 * nrgbd_tsdf_extract_points — no counterpart in the reference: the volume's zero crossings as points, three launches (per-workgroup
 *   counts; a one-workgroup exclusive scan in index order, NRGBD_TSDF_SCAN_PASS records per pass; re-evaluate and write at offset +
 *   rank), no atomics.  Between a = (ix, iy, iz) and b = a + e_k (k = x, y, z; b inside the grid) there is a crossing iff
 *     W_a >= w_min && W_b >= w_min  &&  fabsf(T_a) < 1 && fabsf(T_b) < 1  &&  (T_a < 0) != (T_b < 0)        (a NaN fails)
 *   at q = T_a / (T_a - T_b): coordinate k of the point is o_k + vs * ((float)i_k + q), the other two are o + vs * (float)i.
 *   points       device fp32 [capacity][3]: the first min(found, capacity) crossings in ascending (linear voxel index, axis) order;
 *                nothing behind them is written.  May be NULL when capacity is 0 (the third launch is left out).
 *   counts       device int64 [2] = crossings found, points written
 *   workspace    8-byte aligned, at least nrgbd_tsdf_extract_workspace(X, Y, Z) bytes; rewritten by every call
 *   errors       NRGBD_E_NULL: a NULL pointer (points only when capacity > 0);  NRGBD_E_SHAPE: the grid as above, capacity < 0, a
 *                workspace that is too small;  NRGBD_E_ARG: voxel_size <= 0 or not finite, a NaN w_min;  NRGBD_E_ALIGN: workspace or
 *                counts.  Checked in this order, before anything touches the device.
 * nrgbd_tsdf_raycast_f32 — no counterpart in the reference: the volume seen from a camera, one ray per pixel marched to the first
 *   zero crossing of the trilinear interpolant; one launch, capturable, no atomics, no workspace; the volume is only read.
 *   pose         HOST fp32 [12], read at the call: float32(extM[:3,:4]) row-major, world -> camera, as integrate takes it
 *   centre       HOST fp32 [3], read at the call: the camera centre -R^T t in the world, formed in float64 on the host from the
 *                float32 pose and rounded once
 *   fx fy cx cy  the pinhole intrinsics at H x W; pixel x covers [x, x + 1)
 *   d_near d_far the ray parameter (= z-depth: rays have z = 1) is searched in [d_near, d_far]
 *   w_min        a sample counts where all eight corners of its cell have weight >= w_min
 *   step         the distance between two samples along the ray, a world length in metres
 *   depth        device fp32 [H][W], always written: z-depth of the crossing; 0 = no surface
 *   normal       device fp32 [3][H][W] or NULL: the unit surface normal in the CAMERA frame (it points towards free space, at the
 *                camera: its z is negative on a surface seen from the front); (0, 0, 0) where there is none
 *   per pixel (py, px), with N = (X, Y, Z), o the origin, vs the voxel size, r the pose, a and k running over the axes x, y, z:
 *     xn = (((float)px + 0.5) - cx) / fx;  yn = (((float)py + 0.5) - cy) / fy
 *     d_k = (r0k * xn + r1k * yn) + r2k                       (the ray's world direction: column k of R)
 *     len = sqrtf((dx * dx + dy * dy) + dz * dz);  dzs = step / len
 *     go_k = (centre_k - o_k) / vs;  gd_k = d_k / vs           (voxel coordinates: the sample at ray parameter z is go + z gd)
 *     z0 = d_near, z1 = d_far; then for k = x, y, z in turn (the slab of the interpolation domain [0, N_k - 1]):
 *       gd_k != 0: ta = (0 - go_k) / gd_k;  tb = ((float)(N_k - 1) - go_k) / gd_k;
 *                  z0 = fmaxf(z0, fminf(ta, tb));  z1 = fminf(z1, fmaxf(ta, tb))
 *       gd_k == 0: a miss unless 0 <= go_k <= (float)(N_k - 1)
 *     a miss unless z0 <= z1 (a NaN fails);  a miss when any N_k < 2 (no cell)
 *     for k = 0, 1, ... while zk = z0 + (float)k * dzs <= z1 and k < NRGBD_TSDF_RAYCAST_MAX_STEPS (reaching it is a miss):
 *       p_a = go_a + zk * gd_a;  the sample is INVALID unless 0 <= p_a <= (float)(N_a - 1) on every axis (a NaN fails)
 *       i_a = min((int)floorf(p_a), N_a - 2);  f_a = p_a - (float)i_a
 *       VALID iff the weights of the eight corners i + {0,1}^3 are all >= w_min (a NaN fails)
 *       T = lerp(lerp(lerp(T000, T100, fx), lerp(T010, T110, fx), fy), lerp(lerp(T001, T101, fx), lerp(T011, T111, fx), fy), fz)
 *           with lerp(a, b, f) = a + f * (b - a) and Txyz the corner i + (x, y, z)
 *       a hit iff the previous sample (k - 1) was VALID with T_prev > 0 and this one is VALID with T <= 0:
 *           q = T_prev / (T_prev - T);  depth = z_prev + dzs * q;  the march stops
 *     normal, at a hit: p_a = go_a + depth * gd_a; (0, 0, 0) unless 0 <= p_a <= (float)(N_a - 1) on every axis and, with i, f as
 *       above, the eight weights are all >= w_min; then the gradient of the trilinear interpolant,
 *       gx = lerp(lerp(T100 - T000, T110 - T010, fy), lerp(T101 - T001, T111 - T011, fy), fz)
 *       gy = lerp(lerp(T010 - T000, T110 - T100, fx), lerp(T011 - T001, T111 - T101, fx), fz)
 *       gz = lerp(lerp(T001 - T000, T101 - T100, fx), lerp(T011 - T010, T111 - T110, fx), fy)
 *       g = sqrtf((gx * gx + gy * gy) + gz * gz);  (0, 0, 0) unless g > 0 and finite;  u = (gx / g, gy / g, gz / g)
 *       n_j = (rj0 * ux + rj1 * uy) + rj2 * uz                 (rotated into the camera frame)
 *   A workgroup owns a NRGBD_TSDF_RAYCAST_TILE^2 pixel tile, a wave an 8 x 8 quarter of it.
 *   errors       NRGBD_E_NULL: tsdf, weight, pose, centre or depth NULL;  NRGBD_E_SHAPE: a dimension <= 0, X Y Z > 2^31, H or W >
 *                NRGBD_TSDF_RAYCAST_MAX_SIDE;  NRGBD_E_ARG: voxel_size, step, fx or fy <= 0 or not finite, d_near < d_far not true,
 *                a NaN w_min, a pose or centre entry that is not finite.  Checked in this order, before anything touches the device.
 * nrgbd_tsdf_integrate_color_f32 — no counterpart in the reference: nrgbd_tsdf_integrate_f32 with the frame's colour carried through
 *   the volume.  The colour volume: three planar device arrays color [3][Z][Y][X] (r, g, b; X fastest) beside tsdf and weight, all zeros
 *   when fresh.  Colour SHARES the TSDF's weight: a voxel's colour is averaged over exactly the observations that updated its distance,
 *   with the same w (Open3D's rule); there is no fourth weight plane, so a colour volume is integrated through this entry only.
 *   color        device fp32 [3][Z][Y][X], the volume's three planes
 *   image        device fp32 [3][Hc][Wc], planar, at a size of its own
 *   fxc fyc cxc cyc  the pinhole intrinsics at Hc x Wc
 *   affine       HOST fp32 [6] = a_r a_g a_b b_r b_g b_b, read at the call: the colour of a pixel is image * a + b per channel
 *   per voxel of the box: the chain of nrgbd_tsdf_integrate_f32 unchanged up to t, w — the same skips, the same bits of T' and W' —
 *   and for a voxel that is updated, with xc / zc and yc / zc the quotients the projection formed and C_j its three colour values:
 *     uc = fxc * (xc / zc) + cxc;  vc = fyc * (yc / zc) + cyc
 *     uc = fminf(fmaxf(uc, 0), (float)(Wc - 1));  vc = fminf(fmaxf(vc, 0), (float)(Hc - 1))      (clamped: colour never vetoes a
 *                                                                                                distance update)
 *     icu = (int)floorf(uc);  icv = (int)floorf(vc)
 *     c_j = image[j][icv][icu] * a_j + b_j                                                       (j = r, g, b)
 *     c_r, c_g, c_b all finite:  C_j' = (C_j * Wt + c_j * w) / (Wt + w)      with the OLD Wt: the denominator of T'
 *     else:                      the three colour values keep their bits (T and Wt are updated all the same)
 *   A skipped voxel, a voxel outside the box and a lane group that updates nothing keep their colour bits (the group is neither
 *   loaded nor stored); the image is read only for voxels that passed every test.  Four x-neighbours per lane with 16-byte loads and
 *   stores on all five planes when X % 4 == 0 and tsdf, weight and color are 16-byte aligned, one voxel per lane otherwise: the
 *   same bits.
 *   errors       those of nrgbd_tsdf_integrate_f32 in its order, and with them  NRGBD_E_NULL: color, image or affine NULL;
 *                NRGBD_E_SHAPE: Hc or Wc <= 0 (after H and W, before the box);  NRGBD_E_ARG: a colour intrinsic or an affine entry
 *                that is not finite (after d_near < d_far).  Before anything touches the device.
 * nrgbd_tsdf_extract_points_color, nrgbd_tsdf_extract_mesh_color — no counterpart in the reference: nrgbd_tsdf_extract_points and
 *   nrgbd_tsdf_extract_mesh with the colour of every point / vertex: the same launches, workspaces, counts, order and capacity cut.
 *   color        device fp32 [3][Z][Y][X], the volume's three planes
 *   colors       device fp32 [capacity][3] (the mesh: [vertex_capacity][3]): row p belongs to row p of points / vertices; for the
 *                crossing between a and b = a + e_k at q:   colors[p][j] = C_j(a) + q * (C_j(b) - C_j(a))      (three operations,
 *                the q that places the point); nothing behind the written rows is written.  points / vertices / faces and counts
 *                hold the bits the colourless entries write.
 *   errors       those of the colourless entry in its order;  NRGBD_E_NULL also: color NULL, colors NULL when the (vertex)
 *                capacity is > 0.
 * nrgbd_tsdf_raycast_color_f32 — no counterpart in the reference: nrgbd_tsdf_raycast_f32 with the colour at every hit.
 *   color        device fp32 [3][Z][Y][X], the volume's three planes
 *   rgb          device fp32 [3][H][W], always written: at a hit, with p, i, f as for the normal, (0, 0, 0) unless 0 <= p_a <=
 *                (float)(N_a - 1) on every axis and the eight weights are all >= w_min; then per plane the trilinear interpolant
 *                with T's nesting, lerp(lerp(lerp(C000, C100, fx), lerp(C010, C110, fx), fy), lerp(lerp(C001, C101, fx),
 *                lerp(C011, C111, fx), fy), fz) (the corners are requested only where the test passed).  A miss is (0, 0, 0).  The
 *                colour does not depend on the gradient being non-zero.  depth and normal keep their bits; normal may be NULL.
 *   errors       those of nrgbd_tsdf_raycast_f32 in its order;  NRGBD_E_NULL also: color or rgb NULL.
 * nrgbd_tsdf_reintegrate_f32 — no counterpart in the reference (tsdf_reint.hip): a frame that was integrated is taken out of the volume
 *   again (pose_add NULL), or taken out at pose_remove and put back at pose_add in the same launch — what a pose correction needs
 *   (BundleFusion's re-integration).  One launch, capturable.  Every argument that nrgbd_tsdf_integrate_f32 has means what it means
 *   there; the caller passes the maps the frame was integrated with.
 *   pose_remove  HOST fp32 [12], read at the call: the pose the frame was integrated with
 *   pose_add     HOST fp32 [12], read at the call, or NULL: the removal alone
 *   w_floor      >= 0: a voxel whose weight does not stay above it after the removal is fresh again.  A parameter, not a measurement:
 *                it absorbs the rounding residue of the weight maps' sums (1e-3 is the Python default)
 *   per voxel of the box, removal: the chain of nrgbd_tsdf_integrate_f32 with pose_remove unchanged up to t, w — the same skips, the
 *   same pixel, the same bits —, and for a voxel that passes, with T, Wt its stored values:
 *     Wn = Wt - w
 *     Wn > w_floor not true (a NaN Wn included):   T' = 0;  W' = 0                                  (the voxel is fresh again)
 *     else:   T' = fminf(1, fmaxf(-1, (T * Wt - t * w) / Wn));  W' = Wn
 *   With unit weights the sums are exact integers and removing a voxel's only observation gives exactly (0, 0).  The removal inverts
 *   the integration only while Wt never reached w_max: on a saturated voxel the formula is applied to the clamped weight, and what
 *   comes out is not what the other observations alone would have given (undoing the saturation would take a second weight plane).
 *   pose_add given: then, on the values the removal left (in registers: every plane is loaded once and stored once), the unchanged
 *   update of nrgbd_tsdf_integrate_f32 with pose_add: T' = (T * Wt + t * w) / (Wt + w); W' = fminf(Wt + w, w_max).  Voxels are
 *   independent, so the result is bit for bit that of the removal launch followed by nrgbd_tsdf_integrate_f32.
 *   A voxel that neither pose updates keeps its bits; a lane group without an update is neither loaded nor stored.  Four x-neighbours
 *   per lane with 16-byte accesses when X % 4 == 0 and the planes are 16-byte aligned, one voxel per lane otherwise: the same bits.
 *   errors       those of nrgbd_tsdf_integrate_f32 in its order (NRGBD_E_NULL: tsdf, weight, depth or pose_remove NULL — without a
 *                pose to remove the call is nrgbd_tsdf_integrate_f32), then NRGBD_E_ARG: w_floor negative or not finite.  Before
 *                anything touches the device.
 * nrgbd_tsdf_reintegrate_color_f32 — no counterpart in the reference: the same on a colour volume, with the color, image, colour
 *   intrinsics and affine arguments of nrgbd_tsdf_integrate_color_f32 (the picture the frame was integrated with).  For a voxel the
 *   removal passes, with c_j the colour nrgbd_tsdf_integrate_color_f32 forms for it and C_j, Wt the stored values:
 *     Wn > w_floor not true:        C_j' = 0                                                            (j = r, g, b)
 *     else, c_r c_g c_b all finite: C_j' = (C_j * Wt - c_j * w) / Wn        with the stored Wt, the Wn of T'
 *     else:                         the three colour values keep their bits (the integration left them alone as well)
 *   and the addition is nrgbd_tsdf_integrate_color_f32's.  When X % 4 != 0 or a plane is not 16-byte aligned, remove-and-add runs as
 *   two launches (the removal, then the integration's own kernel): the same bits.
 *   errors       those of nrgbd_tsdf_integrate_color_f32 in its order (pose_remove in pose's place), then NRGBD_E_ARG: w_floor.
 * nrgbd_tsdf_mesh_workspace — no counterpart in the reference: the bytes nrgbd_tsdf_extract_mesh needs for an X Y Z grid (24 per
 *   NRGBD_TSDF_EXTRACT_VOXELS voxels and 4 per voxel; needs no GPU); NRGBD_E_SHAPE: a dimension <= 0, 3 X Y Z > 2^31 - 1.
 * nrgbd_tsdf_extract_mesh — no counterpart in the reference: the volume's surface as an indexed triangle mesh (tsdf_mesh.hip), four
 *   launches (per-workgroup counts of crossings and of triangles; the exclusive scan of both; the vertices and every voxel's first
 *   vertex row; the triangles), no atomics, capturable.
 *   vertices     device fp32 [vertex_capacity][3]: the crossings of nrgbd_tsdf_extract_points — the same predicate, the same q, the
 *                same three operations per coordinate, the same ascending (linear voxel index, axis) order, the same device code: the
 *                first min(found, vertex_capacity) rows, bit for bit what that entry writes; nothing behind them is written
 *   cells        the cell of (ix, iy, iz), ix < X - 1, iy < Y - 1, iz < Z - 1, has the corners c = cx + 2 cy + 4 cz at (ix + cx, iy + cy,
 *                iz + cz) and is VALID iff all eight have W >= w_min && fabsf(T) < 1 (a NaN fails).  Bit c of its case is T_c < 0
 *                (0.0 and -0.0 are both outside, as for the crossings), so every sign-changing edge of a valid cell is a crossing.
 *                A valid cell emits the triangles of its case (csrc/tsdf_mc_table.hpp, generated by tools/gen_mc_table.py from the
 *                rule written there: at most 5, the right-hand normal towards positive T, free space — the side the ray cast's
 *                normals point to; a closed manifold on any sign field; not MC33); an invalid cell emits none.  So a vertex at the
 *                border of the observed region may be referenced by no triangle; and where a corner holds T = 0 exactly, q is 0,
 *                the vertices of its edges coincide and the zero-area triangles between them are kept: the topology is the table's.
 *   faces        device int32 [face_capacity][3]: per triangle the rows its three vertices have in the FULL vertex sequence (whatever
 *                vertex_capacity is): the vertex on edge (voxel v, axis k) has row first(v) + popc(crossings(v) & ((1 << k) - 1)).
 *                Ascending cell order (the linear index of the lowest corner), table order inside a cell; the first min(found,
 *                face_capacity) triangles, nothing behind them.  Either output may be NULL when its capacity is 0.
 *   counts       device int64 [4] = vertices found, vertices written, triangles found, triangles written
 *   workspace    8-byte aligned, at least nrgbd_tsdf_mesh_workspace(X, Y, Z) bytes; rewritten by every call
 *   errors       NRGBD_E_NULL: a NULL pointer (vertices / faces only when their capacity > 0);  NRGBD_E_SHAPE: a dimension <= 0,
 *                3 X Y Z > 2^31 - 1 (a row would not fit an int32), a capacity < 0, a workspace that is too small;  NRGBD_E_ARG:
 *                voxel_size <= 0 or not finite, a NaN w_min;  NRGBD_E_ALIGN: workspace or counts.  Checked in this order, before
 *                anything touches the device.
 */
#define NRGBD_TSDF_EXTRACT_VOXELS 1024
#define NRGBD_TSDF_SCAN_PASS 1024
#define NRGBD_TSDF_RAYCAST_MAX_STEPS 65536
#define NRGBD_TSDF_RAYCAST_TILE 16
#define NRGBD_TSDF_RAYCAST_MAX_SIDE 16384
int nrgbd_tsdf_integrate_f32(float* tsdf, float* weight, int X, int Y, int Z, float ox, float oy, float oz, float voxel_size,
                             const float* depth, const float* gate, float gate_thr, const float* wmap, int H, int W,
                             const float* pose, float fx, float fy, float cx, float cy, float trunc, float d_near, float d_far,
                             float w_max, const int* box, void* stream);
long nrgbd_tsdf_extract_workspace(int X, int Y, int Z);
int nrgbd_tsdf_extract_points(const float* tsdf, const float* weight, int X, int Y, int Z, float ox, float oy, float oz,
                              float voxel_size, float w_min, void* workspace, long workspace_bytes, float* points, long capacity,
                              long long* counts, void* stream);
int nrgbd_tsdf_raycast_f32(const float* tsdf, const float* weight, int X, int Y, int Z, float ox, float oy, float oz,
                           float voxel_size, const float* pose, const float* centre, float fx, float fy, float cx, float cy,
                           int H, int W, float d_near, float d_far, float w_min, float step, float* depth, float* normal,
                           void* stream);
long nrgbd_tsdf_mesh_workspace(int X, int Y, int Z);
int nrgbd_tsdf_extract_mesh(const float* tsdf, const float* weight, int X, int Y, int Z, float ox, float oy, float oz,
                            float voxel_size, float w_min, void* workspace, long workspace_bytes, float* vertices,
                            long vertex_capacity, int* faces, long face_capacity, long long* counts, void* stream);
int nrgbd_tsdf_integrate_color_f32(float* tsdf, float* weight, float* color, int X, int Y, int Z, float ox, float oy, float oz,
                                   float voxel_size, const float* depth, const float* gate, float gate_thr, const float* wmap,
                                   int H, int W, const float* pose, float fx, float fy, float cx, float cy, float trunc,
                                   float d_near, float d_far, float w_max, const int* box, const float* image, int Hc, int Wc,
                                   float fxc, float fyc, float cxc, float cyc, const float* affine, void* stream);
int nrgbd_tsdf_extract_points_color(const float* tsdf, const float* weight, const float* color, int X, int Y, int Z, float ox,
                                    float oy, float oz, float voxel_size, float w_min, void* workspace, long workspace_bytes,
                                    float* points, float* colors, long capacity, long long* counts, void* stream);
int nrgbd_tsdf_extract_mesh_color(const float* tsdf, const float* weight, const float* color, int X, int Y, int Z, float ox,
                                  float oy, float oz, float voxel_size, float w_min, void* workspace, long workspace_bytes,
                                  float* vertices, float* colors, long vertex_capacity, int* faces, long face_capacity,
                                  long long* counts, void* stream);
int nrgbd_tsdf_raycast_color_f32(const float* tsdf, const float* weight, const float* color, int X, int Y, int Z, float ox,
                                 float oy, float oz, float voxel_size, const float* pose, const float* centre, float fx,
                                 float fy, float cx, float cy, int H, int W, float d_near, float d_far, float w_min, float step,
                                 float* depth, float* normal, float* rgb, void* stream);
int nrgbd_tsdf_reintegrate_f32(float* tsdf, float* weight, int X, int Y, int Z, float ox, float oy, float oz, float voxel_size,
                               const float* depth, const float* gate, const float* wmap, const float* pose_remove,
                               const float* pose_add, int H, int W, float fx, float fy, float cx, float cy, float trunc,
                               float d_near, float d_far, float w_max, float w_floor, float gate_thr, const int* box, void* stream);
int nrgbd_tsdf_reintegrate_color_f32(float* tsdf, float* weight, float* color, int X, int Y, int Z, float ox, float oy, float oz,
                                     float voxel_size, const float* depth, const float* gate, const float* wmap,
                                     const float* pose_remove, const float* pose_add, int H, int W, float fx, float fy, float cx,
                                     float cy, float trunc, float d_near, float d_far, float w_max, float w_floor, float gate_thr,
                                     const int* box, const float* image, int Hc, int Wc, float fxc, float fyc, float cxc,
                                     float cyc, const float* affine, void* stream);
/*
 * Frame-to-model tracking (icp.hip; neuralrgbd_amd/tracking.py: FrameTracker; fusion.py: TSDFVolume.track, FusionVideoStream(track=
 * True)): a depth frame registered against the maps nrgbd_tsdf_raycast_f32 writes, by point-to-plane ICP with projective data
 * association (KinectFusion's frame-to-model tracking).  None of the entries has a counterpart in the reference, which takes its poses
 * from an external odometry; the conventions are the ones written here.  Per pixel everything is fp32, from the normal equations on
 * everything is double; every operation below is ONE IEEE operation of its type in the order written (no fused multiply-add, no
 * reciprocal, no library function), there are no atomics, and the same inputs give the same bits in every run.  One Gauss-Newton
 * iteration is two launches on the caller's stream (nrgbd_icp_terms_f32, nrgbd_icp_update); nothing is read back between iterations
 * and the schedule is capturable.
 *
 * state: device memory, NRGBD_ICP_STATE_BYTES, 8-byte aligned:
 *     double T[12]    the motion dT = (R | t), [3][4] row-major, frame camera -> model camera (the camera the model maps were cast from)
 *     float  Tf[12]   the same, each entry rounded once: what nrgbd_icp_terms_f32 reads
 *     int32  flag     0, or the NRGBD_ICP_* reason the iteration stopped for (sticky)
 *     int32  iterations   the steps that updated T since step 0
 * partial: nwg = nrgbd_icp_workgroups(Hs, Ws) records of NRGBD_ICP_RECORD_BYTES (240): double[28] = A_ij for i <= j in row-major
 *   order (A_00, A_01 .. A_05, A_11 ..: 21), g_0 .. g_5, E; then an int64 count; then 8 bytes of padding (written as 0;
 *   nrgbd_icp_terms_photo_f32 writes its int64 count of photometric pairs there).
 *
 * nrgbd_icp_workgroups — no counterpart in the reference: min(ceil(Hs Ws / 256), NRGBD_ICP_MAX_WG); a fixed cap, larger maps are
 *   covered by a grid-stride loop.  NRGBD_E_SHAPE: Hs or Ws <= 0 or > 32768.  Needs no GPU.
 * nrgbd_icp_workspace — no counterpart in the reference: the bytes of `partial` for an Hs x Ws visit (needs no GPU); NRGBD_E_SHAPE alike.
 * nrgbd_icp_terms_f32 — no counterpart in the reference: association, residuals and the partial normal equations, one launch.
 *   depth        device fp32 [H][W]: the frame's z-depth in metres
 *   gate         device fp32 [H][W] or NULL: a pixel counts where gate >= gate_thr (a NaN fails), as nrgbd_tsdf_integrate_f32 takes it
 *   d_near d_far a pixel counts where d is finite, d > d_near and d <= d_far
 *   fx fy cx cy  the frame's pinhole intrinsics at H x W; pixel x covers [x, x + 1)
 *   sub          >= 1: the pixels visited are (y, x) = (sub j + sub / 2, sub i + sub / 2), j < Hs = H / sub, i < Ws = W / sub
 *                (integer divisions)
 *   mdepth       device fp32 [Hm][Wm]: the model's z-depth, 0 = no surface      } what nrgbd_tsdf_raycast_f32 writes
 *   mnormal      device fp32 [3][Hm][Wm]: camera-frame unit normals, (0,0,0) = none }
 *   fxm .. cym   the model maps' intrinsics at Hm x Wm
 *   state        read: Tf = (R | t)
 *   per visited pixel, fp32:
 *     d = depth[y][x];  skip unless d > d_near, d <= d_far and d finite (a NaN fails);  skip unless gate[y][x] >= gate_thr (when given)
 *     xn = (((float)x + 0.5) - cx) / fx;  yn = (((float)y + 0.5) - cy) / fy;  p = (xn * d, yn * d, d)
 *     q_j = ((R_j0 * p_x + R_j1 * p_y) + R_j2 * p_z) + t_j                      (j = x, y, z: the point in the model camera)
 *     skip unless q_z > 0
 *     u = fxm * (q_x / q_z) + cxm;  v = fym * (q_y / q_z) + cym
 *     skip unless u >= 0 && u < (float)Wm && v >= 0 && v < (float)Hm            (a NaN fails)
 *     iu = (int)floorf(u);  iv = (int)floorf(v);  dm = mdepth[iv][iu];  n = mnormal[:][iv][iu]
 *     skip unless dm > 0 (a NaN fails);  skip if n == (0, 0, 0) or a component of n is not finite
 *     m = (((((float)iu + 0.5) - cxm) / fxm) * dm,  ((((float)iv + 0.5) - cym) / fym) * dm,  dm)
 *     e = q - m;  skip unless (e_x * e_x + e_y * e_y) + e_z * e_z <= dist_thr * dist_thr      (a NaN fails)
 *     r = (n_x * e_x + n_y * e_y) + n_z * e_z
 *     c = q x n:  c_x = q_y * n_z - q_z * n_y;  c_y = q_z * n_x - q_x * n_z;  c_z = q_x * n_y - q_y * n_x
 *     J = (n_x, n_y, n_z, c_x, c_y, c_z)          (d r / d(v, omega) of the left perturbation q -> q + v + omega x q)
 *     w = fabsf(r) <= huber ? 1 : huber / fabsf(r)
 *   and for a pixel that was not skipped, in double from the promoted fp32 values (the product of two promoted floats is exact):
 *     A_ij += (double)w * ((double)J_i * (double)J_j)   (i <= j);   g_i += (double)w * ((double)J_i * (double)r);
 *     E += (double)w * ((double)r * (double)r);   count += 1
 *   A lane adds its pixels in visiting order (pixel p = j Ws + i of lane l of workgroup b: p = 256 b + l, + 256 nwg, ...), then the
 *   workgroup folds its lanes in a fixed order (a wave64 shuffle tree, then the 4 waves in wave order) and writes record b.
 *   resid        device fp32 [H][W] or NULL: r at the visited pixels that were not skipped, a quiet NaN at every other pixel of the
 *                map (the pixels that are not visited included): an alignment-error map
 *   errors       NRGBD_E_NULL: depth, mdepth, mnormal, state or partial NULL;  NRGBD_E_SHAPE: H, W, Hm or Wm <= 0 or > 32768,
 *                sub < 1, Hs or Ws 0, partial_bytes < nrgbd_icp_workspace(Hs, Ws);  NRGBD_E_ARG: fx, fy, fxm or fym <= 0 or not
 *                finite, cx, cy, cxm or cym not finite, dist_thr or huber <= 0 or not finite, d_near < d_far not true (a NaN bound
 *                included), a NaN gate_thr beside a gate;  NRGBD_E_ALIGN: state or partial not 8-byte aligned.  Checked in this
 *                order, before anything touches the device.
 * nrgbd_icp_terms_photo_f32 — no counterpart in the reference: nrgbd_icp_terms_f32 with one photometric (intensity) residual more per
 *   pair, added to the same normal equations: a single plane leaves point-to-plane ICP blind to the two in-plane translations and
 *   the rotation about the normal; the surface's texture pins them.  The arguments of nrgbd_icp_terms_f32, and
 *   image        device fp32 [3][H][W]: the frame's picture at the depth map's size
 *   aff_a aff_b  HOST float [3] each: a pixel's colour is image * a + b per channel, as nrgbd_tsdf_integrate_color_f32 takes it
 *   mrgb         device fp32 [3][Hm][Wm]: the model's colour, what nrgbd_tsdf_raycast_color_f32 writes beside mdepth and mnormal
 *   photo_weight the weight of a photometric term beside a geometric one (whose weight is at most 1), > 0 and finite
 *   photo_huber  intensity residuals beyond it are down-weighted, > 0 and finite
 *   per visited pixel, fp32: the sequence of nrgbd_icp_terms_f32 unchanged — resid, the geometric sums and count have that entry's
 *   bits.  Then, for a pixel that was not skipped, with its q, u, v and dm (model pixel n covers [n, n + 1): its centre is at n + 0.5):
 *     c_k = image[k][y][x] * a_k + b_k;  Lf = (0.299f * c_0 + 0.587f * c_1) + 0.114f * c_2         (the visited pixel itself)
 *     ub = u - 0.5f;  vb = v - 0.5f;  x0 = floorf(ub);  y0 = floorf(vb)
 *     skip the photometric term unless x0 >= 0 && x0 + 1 <= (float)(Wm - 1) && y0 >= 0 && y0 + 1 <= (float)(Hm - 1)
 *     the four neighbours (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1), called 00, 10, 01, 11: skip unless each
 *       mdepth_n > 0 and fabsf(mdepth_n - dm) <= dist_thr (a NaN fails: a neighbour on another surface is not interpolated with)
 *     L_n = (0.299f * mrgb[0]_n + 0.587f * mrgb[1]_n) + 0.114f * mrgb[2]_n;  skip unless Lf and the four L_n are finite
 *     fu = ub - x0;  fv = vb - y0;  gu0 = L10 - L00;  gu1 = L11 - L01
 *     Im = (1 - fv) * (L00 + fu * gu0) + fv * (L01 + fu * gu1)                                     (the bilinear interpolant)
 *     gu = (1 - fv) * gu0 + fv * gu1;  gv = (1 - fu) * (L01 - L00) + fu * (L11 - L10)              (its gradient, per model pixel)
 *     ri = Im - Lf
 *     xq = q_x / q_z;  yq = q_y / q_z                                                              (the quotients u and v were formed from)
 *     a_x = (gu * fxm) / q_z;  a_y = (gv * fym) / q_z;  a_z = -(a_x * xq + a_y * yq)                (a = d Im / d q)
 *     ci = q x a:  ci_x = q_y * a_z - q_z * a_y;  ci_y = q_z * a_x - q_x * a_z;  ci_z = q_x * a_y - q_y * a_x
 *     Ji = (a_x, a_y, a_z, ci_x, ci_y, ci_z)       (d ri / d(v, omega) of the same left perturbation as J)
 *     wi = fabsf(ri) <= photo_huber ? photo_weight : photo_weight * (photo_huber / fabsf(ri))
 *   and for a pixel whose photometric term was not skipped, in double from the promoted values, after the pixel's geometric adds and
 *   into the same 28 sums:
 *     A_ij += (double)wi * ((double)Ji_i * (double)Ji_j)   (i <= j);   g_i += (double)wi * ((double)Ji_i * (double)ri);
 *     E += (double)wi * ((double)ri * (double)ri);   photo_count += 1
 *   count stays the geometric pair count; the record's last word (padding, 0, from nrgbd_icp_terms_f32) holds the int64
 *   photo_count, folded like count.  nrgbd_icp_update reads the 28 sums and count alone: it neither reads that word nor changes.
 *   resid        as nrgbd_icp_terms_f32 writes it
 *   resid_photo  device fp32 [H][W] or NULL: ri at the pixels with a photometric term, a quiet NaN at every other pixel of the map
 *                (the pixels that are not visited included)
 *   errors       those of nrgbd_icp_terms_f32 in its order, each class with the new arguments:  NRGBD_E_NULL: also image, mrgb, aff_a
 *                or aff_b NULL;  NRGBD_E_ARG: also (after that entry's own) photo_weight or photo_huber <= 0 or not finite, an entry of
 *                aff_a or aff_b not finite.  Before anything touches the device.
 * nrgbd_icp_update — no counterpart in the reference: the solve and the pose update, one workgroup, one launch.
 *   init         HOST double [12] or NULL (= the identity), read at the call when step == 0
 *   step == 0:   T = init; Tf = (float)T (rounded once); flag = 0; iterations = 0.  partial and log are not touched (may be NULL).
 *   step >= 1:   S = the nwg records added in index order, ((rec_0 + rec_1) + rec_2) + ..., per value, in double / int64;
 *     flag' = flag.  If flag == 0, in this order:
 *       count < min_pairs                          -> flag' = NRGBD_ICP_FEW
 *       a value of S (28 doubles) not finite       -> flag' = NRGBD_ICP_NONFINITE
 *       the factorisation A = L D L^T of the symmetric A (A_ij = A_ji), amax = fmax(.. fmax(A_00, A_11) .., A_55):
 *         for j = 0 .. 5:  D_j = A_jj, then for k = 0 .. j - 1 in turn: D_j = D_j - (L_jk * L_jk) * D_k
 *                          for i = j + 1 .. 5:  s = A_ij, then for k = 0 .. j - 1: s = s - (L_ik * L_jk) * D_k;   L_ij = s / D_j
 *         a pivot with D_j > min_pivot * amax not true (a NaN included) -> flag' = NRGBD_ICP_DEGENERATE
 *       the solve A xi = -g:  for i = 0 .. 5: y_i = -g_i, then for k = 0 .. i - 1: y_i = y_i - L_ik * y_k
 *                             z_i = y_i / D_i
 *                             for i = 5 .. 0: xi_i = z_i, then for k = i + 1 .. 5: xi_i = xi_i - L_ki * xi_k
 *       |xi|^2 = ((((xi_0 xi_0 + xi_1 xi_1) + xi_2 xi_2) + xi_3 xi_3) + xi_4 xi_4) + xi_5 xi_5
 *       xi = (v, omega);  xx = o_x * o_x, yy, zz alike;  theta2 = (xx + yy) + zz
 *       theta2 <= NRGBD_ICP_MAX_THETA2 (0.25: half a radian) not true -> flag' = NRGBD_ICP_LARGE
 *       a = sin(theta) / theta and b = (1 - cos(theta)) / theta^2 as the Taylor polynomials of degree 8 in theta2, Horner form:
 *         a = ca_8, then for k = 7 .. 0: a = a * theta2 + ca_k,  ca_k = (-1)^k / (2k + 1)!   (one division; the factorial is exact)
 *         b = cb_8, then for k = 7 .. 0: b = b * theta2 + cb_k,  cb_k = (-1)^k / (2k + 2)!
 *         (the truncation error is below 1e-22 for theta <= 0.5)
 *       xy = o_x * o_y, xz, yz alike;  Rw = I + a [omega]x + b [omega]x^2 entry by entry:
 *         Rw_00 = 1 - b * (yy + zz)    Rw_01 = b * xy - a * o_z    Rw_02 = b * xz + a * o_y
 *         Rw_10 = b * xy + a * o_z     Rw_11 = 1 - b * (xx + zz)   Rw_12 = b * yz - a * o_x
 *         Rw_20 = b * xz - a * o_y     Rw_21 = b * yz + a * o_x    Rw_22 = 1 - b * (xx + yy)
 *       T'_ij = (Rw_i0 * T_0j + Rw_i1 * T_1j) + Rw_i2 * T_2j  for j = 0 .. 3, then T'_i3 = T'_i3 + v_i    (dR <- Rw dR, dt <- Rw dt + v)
 *       Tf = (float)T' (rounded once);  iterations += 1
 *     A step that sets a flag, or finds one set, leaves T, Tf and iterations alone: their bits stay.
 *     log[4 (step - 1) ..] = ((double)count, E, |xi|^2, (double)flag'), always written; |xi|^2 is 0 where no solve was completed.
 *   errors       NRGBD_E_NULL: state NULL; for step >= 1 partial or log NULL;  NRGBD_E_SHAPE: step < 0; for step >= 1 nwg < 1 or
 *                nwg > NRGBD_ICP_MAX_WG;  NRGBD_E_ARG: step == 0: an init entry that is not finite; step >= 1: min_pivot <= 0 or
 *                not finite, min_pairs < 6;  NRGBD_E_ALIGN: state, and for step >= 1 partial or log, not 8-byte aligned.  Checked in
 *                this order, before anything touches the device.
 */
#define NRGBD_ICP_MAX_WG 256
#define NRGBD_ICP_RECORD_BYTES 240
#define NRGBD_ICP_STATE_BYTES 152
#define NRGBD_ICP_FEW 1
#define NRGBD_ICP_NONFINITE 2
#define NRGBD_ICP_DEGENERATE 3
#define NRGBD_ICP_LARGE 4
#define NRGBD_ICP_MAX_THETA2 0.25
int nrgbd_icp_workgroups(int Hs, int Ws);
long nrgbd_icp_workspace(int Hs, int Ws);
int nrgbd_icp_terms_f32(const float* depth, const float* gate, float gate_thr, int H, int W, float d_near, float d_far,
                        float fx, float fy, float cx, float cy, int sub, const float* mdepth, const float* mnormal, int Hm,
                        int Wm, float fxm, float fym, float cxm, float cym, const void* state, float dist_thr, float huber,
                        void* partial, long partial_bytes, float* resid, void* stream);
int nrgbd_icp_terms_photo_f32(const float* depth, const float* gate, float gate_thr, int H, int W, float d_near, float d_far,
                              float fx, float fy, float cx, float cy, int sub, const float* mdepth, const float* mnormal, int Hm,
                              int Wm, float fxm, float fym, float cxm, float cym, const void* state, float dist_thr, float huber,
                              void* partial, long partial_bytes, float* resid, const float* image, const float* aff_a,
                              const float* aff_b, const float* mrgb, float photo_weight, float photo_huber, float* resid_photo,
                              void* stream);
int nrgbd_icp_update(void* state, const double* init, int step, const void* partial, int nwg, long long min_pairs,
                     double min_pivot, double* log, void* stream);
/*
 * Multi-view depth consistency (consistency.hip; neuralrgbd_amd/fusion.py: filter_depth, FusionVideoStream(consistency=k)): a depth map
 * cross-checked against other views' depth maps before it is fused — the geometric filter of the learned multi-view-stereo pipelines.
 * The network's depth is the expectation of a candidate distribution; at a depth discontinuity it lies between foreground and
 * background, a flying pixel no other view confirms.  No counterpart in the reference, which stops at the maps; the conventions are
 * the ones written here.  Everything is fp32; every operation below is ONE IEEE operation in the order written (no fused
 * multiply-add, no reciprocal, no library function); there are no atomics and no workspace, and the same inputs give the same bits in
 * every run.  One launch on the caller's stream, capturable.
 *
 * nrgbd_depth_consistency_f32 — no counterpart in the reference: per reference pixel the number of source views whose depth map
 *   agrees with it, and the depth map with the pixels too few views confirm set to 0.
 *   depth        device fp32 [H][W]: the reference view's z-depth in metres
 *   gate         device fp32 [H][W] or NULL: a pixel counts where gate >= gate_thr (a NaN fails), as nrgbd_icp_terms_f32 takes it
 *   d_near d_far a pixel (of the reference and of a source) counts where d is finite, d > d_near and d <= d_far
 *   fx fy cx cy  the pinhole intrinsics at H x W, the reference's and every source's; pixel x covers [x, x + 1)
 *   src_depth    device fp32: a stack of [H][W] maps src_stride floats apart (the size and intrinsics of the reference map)
 *   src_gate     the sources' gates in the same layout; NULL exactly when gate is NULL
 *   src_slots    HOST int [n_src]: source s is map src_slots[s] of the stack (repeats allowed)
 *   src_T        HOST fp32 [n_src][12]: (R | t) of source s, [3][4] row-major, reference camera -> source camera s
 *   n_src        0 .. NRGBD_CONSISTENCY_MAX_SRC; with 0 the source pointers may be NULL and the launch folds the pixel's own tests
 *   per reference pixel (y, x), fp32:
 *     d = depth[y][x];  the pixel is valid when d > d_near, d <= d_far and d is finite (a NaN fails each) and, when a gate is given,
 *     gate[y][x] >= gate_thr.  An invalid pixel: votes = -1, depth_out = 0, and no source is read for it.
 *     xn = (((float)x + 0.5) - cx) / fx;  yn = (((float)y + 0.5) - cy) / fy;  p = (xn * d, yn * d, d)
 *     agreeing = 0;  for s = 0 .. n_src - 1 in order:
 *       q_j = ((R_j0 * p_x + R_j1 * p_y) + R_j2 * p_z) + t_j                    (j = x, y, z: the point in source camera s)
 *       skip the source unless q_z > 0
 *       u = fx * (q_x / q_z) + cx;  v = fy * (q_y / q_z) + cy
 *       skip unless u >= 0 && u < (float)W && v >= 0 && v < (float)H            (a NaN fails)
 *       iu = (int)floorf(u);  iv = (int)floorf(v);  ds = src_depth[src_slots[s]][iv][iu]      (nearest: no interpolation across an edge)
 *       skip unless the source pixel is valid: the four tests above on ds and src_gate[src_slots[s]][iv][iu]
 *       agreeing += 1 when fabsf(ds - q_z) <= rel_thr * q_z                     (a NaN fails)
 *   votes        device fp32 [H][W] or NULL: (float)agreeing, -1 at an invalid pixel — a gate for nrgbd_tsdf_integrate_f32 or
 *                nrgbd_icp_terms_f32 (gate_thr = the views asked for)
 *   depth_out    device fp32 [H][W] or NULL: agreeing >= min_views ? d : 0.  May be `depth` itself (a pixel reads its own value only);
 *                must not overlap a source map.
 *   errors       NRGBD_E_NULL: depth NULL; votes and depth_out both NULL; n_src > 0 and src_depth, src_slots or src_T NULL; n_src > 0
 *                and one of gate, src_gate NULL but not the other;  NRGBD_E_SHAPE: H or W <= 0 or > 32768, n_src < 0 or >
 *                NRGBD_CONSISTENCY_MAX_SRC, min_views < 0, n_src > 0 and src_stride < H W, a negative slot;  NRGBD_E_ARG: fx or fy <= 0
 *                or not finite, cx or cy not finite, rel_thr <= 0 or not finite, d_near < d_far not true (a NaN bound included), a
 *                NaN gate_thr beside a gate, an entry of src_T not finite.  Checked in this order, before anything touches the device.
 */
#define NRGBD_CONSISTENCY_MAX_SRC 16
int nrgbd_depth_consistency_f32(const float* depth, const float* gate, float gate_thr, int H, int W, float d_near, float d_far,
                                float fx, float fy, float cx, float cy, const float* src_depth, const float* src_gate,
                                long src_stride, const int* src_slots, const float* src_T, int n_src, float rel_thr,
                                int min_views, float* votes, float* depth_out, void* stream);

/*
 * The moving TSDF volume (tsdf_shift.hip; neuralrgbd_amd/fusion.py: TSDFVolume.shift, follow_shift, FusionVideoStream(follow=...)): the
 * grid moved by whole voxels so that it follows the camera — the scheme of Kintinuous and large-scale KinFu.  Every nrgbd_tsdf_* entry
 * takes the origin per launch, so a moved volume is an ordinary volume at origin + voxel_size s whose contents sit s voxels lower.  No
 * counterpart in the reference.  A pure copy: no arithmetic touches a value, so NaN payloads, signed zeros and denormals come through
 * bit for bit; no atomics, no workspace, the same bits in every run.  One launch on the caller's stream, capturable.
 *
 * nrgbd_tsdf_shift_f32 — no counterpart in the reference: dst = src moved by s = (sx, sy, sz) voxels, the entering region empty, and
 *   (spill) src turned into the spill volume: the part of the model that leaves, in the old frame.
 *   src dst      device fp32 [planes][Z][Y][X], two buffers that do not overlap: planes = 2 (tsdf, weight) or 5 (tsdf, weight, r, g, b)
 *   sx sy sz     the shift in voxels, any int: the new origin is origin + voxel_size s
 *   per dst lattice index i = (ix, iy, iz), in every plane p:
 *     j = i + s;  dst[p][i] = src[p][j] where 0 <= j_k < n_k for k = x, y, z, the bits unchanged; else +0.0f, and nothing is loaded
 *   the old voxels j with j_k < s_k (s_k > 0) or j_k >= n_k + s_k (s_k < 0) for some k LEAVE — no dst voxel holds them —, every other
 *   old voxel is RETAINED: each of its words is read by exactly one lane, the one that owns that plane's dst voxel i = j - s
 *   spill != 0:  the RIM is the set of retained voxels whose new index i_k is 0 (s_k > 0) or n_k - 1 (s_k < 0) for some k: one voxel
 *     thick, on the faces that face the motion only.  Every retained voxel that is not on the rim gets src[0][j] = src[1][j] = +0.0f
 *     (tsdf and weight), each word written by the lane that read it, after its read.  Leaving voxels, rim voxels and planes 2 .. 4 of src keep
 *     their bits.  A mesh cell is emitted only where all eight corners carry weight, so of the old volume's cells exactly those with a
 *     leaving corner survive in src, and exactly those whose corners are all retained are cells of dst: no gap, no duplicate triangle.
 *   spill == 0:  src is only read
 *   |s_k| >= n_k for some k: nothing is retained — dst is all +0.0f and src keeps every bit;  s = 0: a plain copy (every voxel is
 *     retained and none is on the rim: with spill, src's tsdf and weight become 0)
 *   errors       NRGBD_E_NULL: src or dst NULL;  NRGBD_E_SHAPE: planes not 2 or 5, a dimension <= 0 or X Y Z > 2^31;  NRGBD_E_ARG:
 *                the two buffers' byte ranges overlap.  Checked in this order, before anything touches the device.
 *   The vector form (16-byte stores; 16-byte loads when sx % 4 == 0 too) needs X % 4 == 0 and both bases 16-byte aligned; anything
 *   else runs the element form: the same bits.
 */
int nrgbd_tsdf_shift_f32(float* src, float* dst, int planes, int X, int Y, int Z, int sx, int sy, int sz, int spill, void* stream);

/*
 * The moving TSDF volume paged (tsdf_page.hip; neuralrgbd_amd/fusion.py: BlockStore, TSDFVolume.shift(store=...), paged_extract,
 * FusionVideoStream(follow_spill="page")): blocks of NRGBD_TSDF_BLOCK^3 voxels copied between a volume and a dense staging tensor, so
 * that what leaves the window can be kept on the host and put back, bit for bit, when the window covers it again — the re-entry of
 * Kintinuous and the streaming of voxel hashing.  No counterpart in the reference.  Pure copies: no arithmetic touches a value, so NaN
 * payloads, signed zeros and denormals come through bit for bit; no atomics, no workspace, the same bits in every run.  One launch
 * each on the caller's stream, capturable; one workgroup per block, the blocks on the grid's x dimension.
 *
 * nrgbd_tsdf_blocks_gather_f32 — no counterpart in the reference: n blocks read out of a volume, with a flag per block.
 *   vol          device fp32 [planes][Z][Y][X]: planes = 2 (tsdf, weight) or 5 (tsdf, weight, r, g, b), as nrgbd_tsdf_shift_f32 takes it;
 *                only read
 *   origins      device int32 [n][3]: (ox, oy, oz) of block b in grid voxels, any integers with |o| <= 2^30; a block need not be aligned
 *                to anything and may lie partly or wholly outside the grid
 *   n            the number of blocks, 0 <= n <= NRGBD_TSDF_MAX_BLOCKS; n = 0 launches nothing (origins, blocks may then be NULL)
 *   blocks       device fp32 [n][planes][8][8][8], indexed (z, y, x) inside a block, 16-byte aligned; every word is written:
 *     blocks[b][p][k][j][i] = vol[p][oz + k][oy + j][ox + i], the bits unchanged, where 0 <= ox + i < X, 0 <= oy + j < Y and
 *     0 <= oz + k < Z; else +0.0f, and nothing is loaded
 *   nonempty     device int32 [n] or NULL: nonempty[b] = 1 where some in-grid word of some plane of block b has a non-zero bit pattern
 *                (-0.0 and NaN count), else 0.  A block whose flag is 0 holds +0.0f throughout — what a region that enters after a
 *                shift holds —, so it can be dropped without loss
 *   errors       NRGBD_E_NULL: vol NULL, or origins or blocks NULL with n != 0;  NRGBD_E_SHAPE: planes not 2 or 5, a dimension <= 0 or
 *                X Y Z > 2^31, n < 0 or n > NRGBD_TSDF_MAX_BLOCKS;  NRGBD_E_ARG: blocks not 16-byte aligned.  Checked in this order,
 *                before anything touches the device.
 *   The vector form (16-byte accesses of the volume) needs X % 4 == 0, a 16-byte aligned vol and, per block, ox % 4 == 0; anything
 *   else runs the element form: the same bits.
 *
 * nrgbd_tsdf_blocks_scatter_f32 — no counterpart in the reference: the inverse — n blocks written into a volume.
 *   vol          device fp32 [planes][Z][Y][X], as above: vol[p][oz + k][oy + j][ox + i] = blocks[b][p][k][j][i], the bits unchanged,
 *                for every voxel of every block that lies in the grid; the part of a block outside the grid is ignored, and every
 *                voxel outside all the blocks keeps its bits
 *   origins n    as above.  The blocks of one call must not overlap inside the grid (two origins closer than 8 along all three
 *                axes): which block's words such a voxel ends up with is not defined.  The caller's contract; not checked here
 *   blocks       device fp32 [n][planes][8][8][8], 16-byte aligned; only read
 *   errors       as above
 */
#define NRGBD_TSDF_BLOCK        8
#define NRGBD_TSDF_MAX_BLOCKS   (1 << 20)
int nrgbd_tsdf_blocks_gather_f32(const float* vol, int planes, int X, int Y, int Z, const int* origins, int n, float* blocks,
                                 int* nonempty, void* stream);
int nrgbd_tsdf_blocks_scatter_f32(float* vol, int planes, int X, int Y, int Z, const int* origins, int n, const float* blocks,
                                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NRGBD_H */
