"""neuralrgbd_amd — MI355X-native (gfx950) plane-sweep depth path of NVlabs/neuralrgbd.

Drop-in surface (reference file it replaces):
    neuralrgbd_amd.KVNET            code/models/KVNET.py::KVNET
    neuralrgbd_amd.homography       code/warping/homography.py (the operators on the hot path)
    neuralrgbd_amd.test_step.test   code/test_utils/test_KVNet.py::test
    neuralrgbd_amd.lba_step         code/test_KVNet_LBA.py:306-528 (the LBA step: keyframe maps, pose refinement, stream)
    neuralrgbd_amd.video            code/test_KVNet.py:185-250 (the driver loop: push a frame and its extrinsic, get depth) and the loaders'
                                    image preparation (mdataloader/scanNet.py:368-369,429-430) on the device
    neuralrgbd_amd.train_video      code/train_KVNet.py:283-330 over mdataloader/batch_loader.py (the training driver loop: push a frame, its
                                    depth frame and its extrinsic, get a training step) and the loaders' depth preparation and
                                    digitising (mdataloader/scanNet.py:372-422) on the device
    neuralrgbd_amd.evaluate         code/test_utils/export_res.py:108-116 and the offline scoring behind it: error metrics of the depth maps
                                    against ground truth, per confidence set, as running totals on the device
    neuralrgbd_amd.fusion           (no counterpart) TSDF fusion of the depth stream into a voxel volume on the device, surface points, ray cast
    neuralrgbd_amd.camera           the cam_intrinsics dict of code/mdataloader/scanNet.py:204-272
The compute between the convolutions is hand-written HIP behind the C-ABI of include/nrgbd.h
(libnrgbd_hip.so, built by `python -m neuralrgbd_amd.build`).
"""
import os as _os

# ROCm's hipGraph "packet capture" (pre-recorded AQL packets for kernel nodes, on by default in CLR) is switched off for this process
# unless the caller decided otherwise: with it on, replays of a captured TRAINING iteration came out wrong — deterministically, by
# 0.1-0.3 % of the loss — whenever eager launches of the same kernels had run between the replays (an eager twin in a test, an evaluation
# pass between optimizer steps); serialised launches or this switch remove it, the measured cost is nil (train 29.19 vs 29.24 ms per
# window, config B 30.62 vs 30.64 frames/s, config S 204.4 vs 203.8: DESIGN.md section 7).  The runtime reads the variable when it
# initialises, i.e. at the process's first HIP call: importing this package before touching the GPU is enough.
_os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

from . import camera, synth  # host-only helpers (numpy / torch CPU)


def __getattr__(name):
    # the GPU-facing modules load libnrgbd_hip.so; import them lazily so that host-only tooling
    # (camera, synth, build) works before the library is built
    if name in ("ops", "homography", "kvnet", "nets", "misc", "test_step", "lba_step", "video", "train_video", "evaluate", "fusion", "_lib"):
        import importlib
        return importlib.import_module("." + name, __name__)
    if name == "KVNET":
        from .kvnet import KVNET
        return KVNET
    if name == "VideoDepthStream":
        from .video import VideoDepthStream
        return VideoDepthStream
    if name in ("TrainVideoStream", "DepthLabeler", "run_training_sequence", "pillow_nearest_index", "label_thresholds"):
        from . import train_video
        return getattr(train_video, name)
    if name in ("DepthMetrics", "EvalVideoStream", "evaluate_sequence", "metrics_from_record"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("TSDFVolume", "FusionVideoStream", "fuse_sequence", "frustum_box", "intrinsics_at", "save_ply", "shade", "to_uint8"):
        from . import fusion
        return getattr(fusion, name)
    raise AttributeError(name)
