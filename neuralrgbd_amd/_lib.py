"""ctypes loader of libnrgbd_hip.so — the C-ABI declared in include/nrgbd.h.

There is deliberately NO fallback: if the HIP library is missing or does not export every
symbol of the header, importing the product path raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libnrgbd_hip.so")

_c = ctypes
_P = _c.c_void_p
_F = _c.c_float
_I = _c.c_int
_L = _c.c_long
_D = _c.c_double
_Z = _c.c_size_t

GATHER_MAX_V = 6        # NRGBD_GATHER_MAX_V
DEPTH_MAX_THRESHOLDS = 512      # NRGBD_DEPTH_MAX_THRESHOLDS
DEPTH_EVAL_MAX_SETS = 8         # NRGBD_DEPTH_EVAL_MAX_SETS
DGF_TILE = (16, 64)             # NRGBD_DGF_TILE_Y, NRGBD_DGF_TILE_X
TSDF_EXTRACT_VOXELS = 1024      # NRGBD_TSDF_EXTRACT_VOXELS
TSDF_SCAN_PASS = 1024           # NRGBD_TSDF_SCAN_PASS
TSDF_RAYCAST_MAX_STEPS = 65536  # NRGBD_TSDF_RAYCAST_MAX_STEPS
TSDF_RAYCAST_TILE = 16          # NRGBD_TSDF_RAYCAST_TILE
TSDF_RAYCAST_MAX_SIDE = 16384   # NRGBD_TSDF_RAYCAST_MAX_SIDE
ICP_MAX_WG = 256                # NRGBD_ICP_MAX_WG
ICP_RECORD_BYTES = 240          # NRGBD_ICP_RECORD_BYTES
ICP_STATE_BYTES = 152           # NRGBD_ICP_STATE_BYTES
ICP_FEW, ICP_NONFINITE, ICP_DEGENERATE, ICP_LARGE = 1, 2, 3, 4     # NRGBD_ICP_*: why an iteration stopped
ICP_MAX_THETA2 = 0.25           # NRGBD_ICP_MAX_THETA2
CONSISTENCY_MAX_SRC = 16        # NRGBD_CONSISTENCY_MAX_SRC


class WindowSlots(ctypes.Structure):
    """nrgbd_window_slots: the ring slots of a window, passed by value (sources in window order, then the reference)."""
    _fields_ = [("idx", _I * (GATHER_MAX_V + 1))]


# name -> (restype, argtypes); one entry per function of include/nrgbd.h
SIGNATURES = {
    "nrgbd_version": (_c.c_char_p, []),
    "nrgbd_strerror": (_c.c_char_p, [_I]),
    "nrgbd_homography_terms": (_I, [_P, _P, _L, _L, _P, _L, _L, _P, _P, _I, _P]),
    "nrgbd_pose_inverse": (_I, [_P, _L, _P, _P, _I, _P]),
    "nrgbd_pack_nhwc": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "nrgbd_costvol_fwd": (_I, [_P, _P, _P, _P, _P, _P, _F, _F, _F, _I, _I, _P, _P,
                               _I, _I, _I, _I, _I, _I, _P]),
    "nrgbd_costvol_fwd_gen": (_I, [_P, _P, _P, _P, _P, _P, _F, _F, _F, _I, _I, _P, _P,
                                   _I, _I, _I, _I, _I, _I, _I, _P]),
    "nrgbd_costvol_bwd_workspace": (_I, [_I, _I, _I, _I, _I, _P]),
    "nrgbd_costvol_bwd": (_I, [_P, _P, _P, _P, _P, _P, _F, _F, _F, _I, _I, _P, _P, _P,
                               _I, _I, _I, _I, _I, _I, _P, _Z, _P]),
    "nrgbd_costvol_bwd_det_workspace": (_I, [_I, _I, _I, _I, _I, _P]),
    "nrgbd_costvol_bwd_det": (_I, [_P, _P, _P, _P, _P, _P, _F, _F, _F, _I, _I, _P, _P, _P,
                                   _I, _I, _I, _I, _I, _I, _P, _Z, _P]),
    "nrgbd_bn_cl_workgroups": (_I, [_L, _I]),
    "nrgbd_bn_cl_fwd": (_I, [_P, _P, _P, _P, _F, _F, _P, _P, _I, _P, _P, _P, _L, _I, _P]),
    "nrgbd_bn_cl_bwd": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _P, _L, _I, _P]),
    "nrgbd_warp_volume": (_I, [_P, _L, _L, _L, _L, _P, _L, _L, _L, _P, _P, _P, _P, _F, _F, _I,
                               _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "nrgbd_warp_volume_cl": (_I, [_P, _L, _L, _L, _L, _P, _L, _L, _L, _P, _P, _P, _P, _F, _F, _I,
                                  _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "nrgbd_dpv_resample": (_I, [_P, _P, _P, _P, _F, _F, _F, _F, _F, _I, _F, _F, _P, _I, _I, _I, _P]),
    "nrgbd_dpv_resample_to": (_I, [_P, _P, _P, _P, _F, _F, _F, _F, _F, _I, _F, _F, _P, _I, _I, _I, _I, _P]),
    "nrgbd_dpv_keyframe_maps": (_I, [_P, _P, _P, _P, _P, _F, _F, _F, _F, _F, _I, _F, _F, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "nrgbd_logsoftmax_d": (_I, [_P, _P, _F, _P, _I, _L, _P]),
    "nrgbd_depth_regress": (_I, [_P, _P, _P, _P, _I, _L, _P]),
    "nrgbd_export_depth_u16": (_I, [_P, _P, _F, _F, _P, _P, _P, _P, _I, _L, _P]),
    "nrgbd_depth_regress_rows": (_I, [_P, _P, _P, _P, _I, _L, _P]),
    "nrgbd_export_depth_u16_rows": (_I, [_P, _P, _F, _F, _P, _P, _P, _P, _I, _L, _P]),
    "nrgbd_warp_depth_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "nrgbd_warp_depth_bwd_workgroups": (_I, [_I, _I]),
    "nrgbd_warp_depth_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "nrgbd_lba_pyramid": (_I, [_P, _I, _I, _I, _P, _I, _P, _P]),
    "nrgbd_lba_workgroups": (_I, [_I, _I]),
    "nrgbd_lba_grad": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "nrgbd_lba_update": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _D, _I, _I, _P]),
    "nrgbd_conv3d_workgroups": (_I, [_I, _I, _I]),
    "nrgbd_conv3d_pack_weights": (_I, [_P, _P, _I, _P]),
    "nrgbd_conv3d_3x3x3_f32": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nrgbd_conv3d_3x3x3_cout1_f32": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _I, _I, _I, _I, _P]),
    "nrgbd_conv3d_cout1_bwd_workgroups": (_I, [_I, _I, _I, _I]),
    "nrgbd_conv3d_cout1_dgrad_f32": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "nrgbd_conv3d_cout1_wgrad_workspace": (_I, [_I, _I, _I, _P]),
    "nrgbd_conv3d_cout1_wgrad_f32": (_I, [_P, _P, _P, _P, _Z, _I, _I, _I, _P]),
    "nrgbd_conv_wino_tiles": (_I, [_I, _I, _I, _I]),
    "nrgbd_conv_wino_rnet_f32": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "nrgbd_conv_wino_rnet_ex_f32": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "nrgbd_conv_wino_rnet_deconv_f32": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "nrgbd_conv_wino_rnet_deconv_pack": (_I, [_P, _P, _I, _P]),
    "nrgbd_conv_wino_pack": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "nrgbd_bn_finalize_cm": (_I, [_P, _I, _I, _L, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P]),
    "nrgbd_conv_wino_f32": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "nrgbd_conv_wino_dw_pack": (_I, [_P, _P, _I, _I, _I, _P]),
    "nrgbd_conv_wino_dw_f32": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nrgbd_conv_wino_dw_workgroups": (_I, [_I, _I, _I, _I]),
    "nrgbd_conv_wino_dw_unit_f32": (_I, [_P, _P, _F, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nrgbd_conv_wino_dw4_pack": (_I, [_P, _P, _I, _I, _I, _P]),
    "nrgbd_conv_wino_dw4_workspace": (_I, [_I, _I, _I, _I, _P]),
    "nrgbd_conv_wino_dw4_f32": (_I, [_P, _P, _I, _F, _P, _P, _P, _P, _c.c_size_t, _I, _I, _I, _I, _I, _P]),
    "nrgbd_conv3d_wgrad_workgroups": (_I, []),
    "nrgbd_conv3d_wgrad_ranges": (_I, []),
    "nrgbd_conv3d_wgrad_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "nrgbd_bn3d_finalize": (_I, [_P, _I, _L, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P]),
    "nrgbd_bn2d_partial_floats": (_I, [_I]),
    "nrgbd_bn2d_train_act": (_I, [_P, _P, _P, _F, _I, _P, _P, _P, _P, _I, _I, _L, _P]),
    "nrgbd_avgpool8": (_I, [_P, _P, _I, _I, _I, _P]),
    "nrgbd_conv2d_few_f32": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "nrgbd_avgpool_cl": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "nrgbd_scatter_channels": (_I, [_P, _L, _L, _L, _I, _I, _I, _P, _I, _I, _I, _L, _P]),
    "nrgbd_bias_act_nchw": (_I, [_P, _P, _F, _I, _I, _L, _P]),
    "nrgbd_conv2d_workgroups": (_I, [_I, _I, _I]),
    "nrgbd_conv2d_wgrad_workgroups": (_I, [_I, _I, _I, _I, _I]),
    "nrgbd_conv2d_wgrad_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "nrgbd_conv2d_taps_f32": (_I, [_P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "nrgbd_space_to_depth2": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "nrgbd_conv_pack_weights": (_I, [_P, _P, _I, _I, _I, _P]),
    "nrgbd_conv2d_3x3_f32": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "nrgbd_conv2d_rnet_f32": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "nrgbd_rnet_pack": (_I, [_P, _P, _I, _P, _I, _I, _L, _P]),
    "nrgbd_bn_finalize": (_I, [_P, _I, _I, _L, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P]),
    "nrgbd_logsoftmax_rows": (_I, [_P, _P, _L, _I, _P]),
    "nrgbd_logsoftmax_d_bwd": (_I, [_P, _P, _F, _P, _I, _L, _P]),
    "nrgbd_logsoftmax_rows_bwd": (_I, [_P, _P, _P, _L, _I, _P]),
    "nrgbd_nll_workgroups": (_I, [_L]),
    "nrgbd_nll_fwd": (_I, [_P, _P, _L, _I, _L, _I, _P, _P, _P]),
    "nrgbd_nll_bwd": (_I, [_P, _L, _P, _P, _P, _I, _L, _I, _P]),
    "nrgbd_adam_step": (_I, [_P, _P, _P, _P, _P, _P, _I, _D, _D, _D, _D, _D, _I, _P]),
    "nrgbd_grad_norm_workspace": (_L, [_P, _I]),
    "nrgbd_grad_norm": (_I, [_P, _P, _I, _D, _P, _Z, _P, _P, _P]),
    "nrgbd_scale_tensors": (_I, [_P, _P, _I, _P, _P]),
    "nrgbd_adam_step_clipped": (_I, [_P, _P, _P, _P, _P, _P, _I, _D, _D, _D, _D, _D, _I, _P, _I, _P]),
    "nrgbd_bias_lrelu_cl_workgroups": (_I, [_L, _I]),
    "nrgbd_bias_lrelu_cl_fwd": (_I, [_P, _P, _F, _P, _L, _I, _P]),
    "nrgbd_bias_lrelu_cl_bwd": (_I, [_P, _P, _F, _P, _P, _P, _L, _I, _P]),
    "nrgbd_upsample_bilinear_ac": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "nrgbd_bn_small_stats": (_I, [_I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "nrgbd_spp_concat": (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _P, _P, _I, _I, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P, _I, _I, _I, _P]),
    "nrgbd_frame_ingest_u8": (_I, [_P, _I, _I, _L, _I, _F, _F, _F, _F, _F, _F, _P, _I, _I, _P]),
    "nrgbd_window_gather": (_I, [_P, _I, _L, WindowSlots, _I, _P, _P, _I, _I, _P]),
    "nrgbd_depth_ingest_u16": (_I, [_P, _I, _I, _L, _P, _P, _P, _P, _P, _P, _F, _P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "nrgbd_depth_eval_workgroups": (_I, [_L]),
    "nrgbd_depth_eval_workspace": (_L, [_L, _I]),
    "nrgbd_depth_eval": (_I, [_P, _P, _P, _L, _F, _F, _P, _I, _P, _L, _P, _P, _P, _P, _P, _P, _P, _P]),
    "nrgbd_dgf_refine_f32": (_I, [_P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _P, _F, _P, _P]),
    "nrgbd_tsdf_integrate_f32": (_I, [_P, _P, _I, _I, _I, _F, _F, _F, _F, _P, _P, _F, _P, _I, _I, _P, _F, _F, _F, _F, _F, _F, _F, _F, _P, _P]),
    "nrgbd_tsdf_extract_workspace": (_L, [_I, _I, _I]),
    "nrgbd_tsdf_extract_points": (_I, [_P, _P, _I, _I, _I, _F, _F, _F, _F, _F, _P, _L, _P, _L, _P, _P]),
    "nrgbd_tsdf_raycast_f32": (_I, [_P, _P, _I, _I, _I, _F, _F, _F, _F, _P, _P, _F, _F, _F, _F, _I, _I, _F, _F, _F, _F, _P, _P, _P]),
    "nrgbd_tsdf_mesh_workspace": (_L, [_I, _I, _I]),
    "nrgbd_tsdf_extract_mesh": (_I, [_P, _P, _I, _I, _I, _F, _F, _F, _F, _F, _P, _L, _P, _L, _P, _L, _P, _P]),
    "nrgbd_tsdf_integrate_color_f32": (_I, [_P, _P, _P, _I, _I, _I, _F, _F, _F, _F, _P, _P, _F, _P, _I, _I, _P, _F, _F, _F, _F, _F, _F, _F, _F,
                                            _P, _P, _I, _I, _F, _F, _F, _F, _P, _P]),
    "nrgbd_tsdf_extract_points_color": (_I, [_P, _P, _P, _I, _I, _I, _F, _F, _F, _F, _F, _P, _L, _P, _P, _L, _P, _P]),
    "nrgbd_tsdf_extract_mesh_color": (_I, [_P, _P, _P, _I, _I, _I, _F, _F, _F, _F, _F, _P, _L, _P, _P, _L, _P, _L, _P, _P]),
    "nrgbd_tsdf_raycast_color_f32": (_I, [_P, _P, _P, _I, _I, _I, _F, _F, _F, _F, _P, _P, _F, _F, _F, _F, _I, _I, _F, _F, _F, _F, _P, _P, _P, _P]),
    "nrgbd_tsdf_reintegrate_f32": (_I, [_P, _P, _I, _I, _I, _F, _F, _F, _F, _P, _P, _P, _P, _P, _I, _I, _F, _F, _F, _F, _F, _F, _F, _F, _F, _F,
                                        _P, _P]),
    "nrgbd_tsdf_reintegrate_color_f32": (_I, [_P, _P, _P, _I, _I, _I, _F, _F, _F, _F, _P, _P, _P, _P, _P, _I, _I, _F, _F, _F, _F, _F, _F, _F, _F,
                                              _F, _F, _P, _P, _I, _I, _F, _F, _F, _F, _P, _P]),
    "nrgbd_icp_workgroups": (_I, [_I, _I]),
    "nrgbd_icp_workspace": (_L, [_I, _I]),
    "nrgbd_icp_terms_f32": (_I, [_P, _P, _F, _I, _I, _F, _F, _F, _F, _F, _F, _I, _P, _P, _I, _I, _F, _F, _F, _F, _P, _F, _F, _P, _L, _P,
                                 _P]),
    "nrgbd_icp_terms_photo_f32": (_I, [_P, _P, _F, _I, _I, _F, _F, _F, _F, _F, _F, _I, _P, _P, _I, _I, _F, _F, _F, _F, _P, _F, _F, _P, _L,
                                       _P, _P, _P, _P, _P, _F, _F, _P, _P]),
    "nrgbd_icp_update": (_I, [_P, _P, _I, _P, _I, _c.c_longlong, _D, _P, _P]),
    "nrgbd_depth_consistency_f32": (_I, [_P, _P, _F, _I, _I, _F, _F, _F, _F, _F, _F, _P, _P, _L, _P, _P, _I, _F, _I, _P, _P, _P]),
    "nrgbd_tsdf_shift_f32": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "nrgbd_tsdf_blocks_gather_f32": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _P, _P]),
    "nrgbd_tsdf_blocks_scatter_f32": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _P]),
    "nrgbd_nhwc_stats_workgroups": (_I, [_L]),
    "nrgbd_nhwc_stats": (_I, [_P, _L, _I, _P, _P]),
    "nrgbd_nhwc_act": (_I, [_P, _P, _I, _P, _P, _I, _P, _L, _I, _I, _P]),
    "nrgbd_nhwc_act_lean": (_I, [_P, _P, _I, _P, _P, _I, _P, _L, _I, _I, _I, _P]),
}

_lib = None


class NrgbdError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise NrgbdError(
            "libnrgbd_hip.so not found at %s — build it with `python -m neuralrgbd_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU / eager fallback for this path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise NrgbdError("libnrgbd_hip.so does not export %s (stale build?)" % name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        msg = load().nrgbd_strerror(int(code)).decode()
        raise NrgbdError("%s failed: %s (code %d)" % (what, msg, code))
