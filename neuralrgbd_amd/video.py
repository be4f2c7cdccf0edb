"""Frame-at-a-time video depth: push one camera frame and its extrinsic, get depth back.

`DepthStream.step` takes a finished window (normalised fp32 reference / source images and relative poses).  The reference builds
that window in its driver loop (test_KVNet.py:185-250: the last 2r + 1 frames in a list that slides, `split_frame_list`,
`get_rel_extrinsicM` per source, the NaN-pose check of `check_datArray_pose` :23-41 with the state reset of :241-246) from frames its
loaders prepared on the host (mdataloader/scanNet.py:368-369,429-430, utils/preprocess.py:14-35: PIL NEAREST resize to the network
size, ToTensor, Normalize with the ImageNet statistics) — five fp32 images uploaded per depth frame where one uint8 camera frame is
new.  `VideoDepthStream` owns that loop:

  * the last R = 2r + 1 prepared frames live in a ring on the device, frame i in slot i mod R; a pushed uint8 frame is uploaded as it
    is (one pinned staging buffer) and resized / normalised into its slot by one kernel (ops.frame_ingest), bit for bit what the
    loaders compute; an fp32 frame (the reference's dat['img']) is copied into the slot as it is;
  * the window of the centre frame is assembled by one more launch (ops.window_gather);
  * the extrinsics stay on the host as float64 and the relative poses are `homography.get_rel_extrinsicM` in float64 cast to fp32 —
    the reference's own bits — in one [1,V,4,4] upload;
  * the frame itself is `DepthStream.step`, unchanged (hipGraph, pipelining, status probe).
"""
import numpy as np
import torch

from . import _lib, ops
from . import homography as warp_homo
from .streaming import DepthStream

IMAGENET_MEAN = (0.485, 0.456, 0.406)        # utils/preprocess.py:14-15
IMAGENET_STD = (0.229, 0.224, 0.225)


def window_slots(n_pushed, t_win_r):
    """The window that the `n_pushed`-th frame (counted from 1) completes, in a ring of R = 2 t_win_r + 1 slots with frame i (from 0)
    in slot i mod R: (ring slots of the sources in the order of misc.split_frame_list — the t_win_r earlier frames, then the t_win_r
    later ones —, ring slot of the reference, index of the reference frame in push order)."""
    R = 2 * t_win_r + 1
    if t_win_r < 1 or n_pushed < R:
        raise ValueError("window_slots: %d frames pushed, the first window of t_win_r %d needs %d" % (n_pushed, t_win_r, R))
    first = n_pushed - R
    ref = first + t_win_r
    return [i % R for i in range(first, n_pushed) if i != ref], ref % R, ref


def _grid_size(cam_intrinsics):
    return tuple(int(n) for n in cam_intrinsics["unit_ray_array"].shape[:2])


def _layout(shape):
    """'hwc' / 'chw' of a 3-D uint8 frame (interleaved wins where both read: a 3 x W x 3 frame)."""
    if len(shape) == 3 and shape[2] == 3:
        return "hwc"
    if len(shape) == 3 and shape[0] == 3:
        return "chw"
    raise ValueError("a uint8 frame is [H,W,3] or [3,H,W], got %s" % (tuple(shape),))


class VideoDepthStream:
    def __init__(self, model, cam_intrinsics, d_candi, t_win_r=2, mean=IMAGENET_MEAN, std=IMAGENET_STD, net_size=None, device=None,
                 **depth_stream_kwargs):
        """net_size = (H, W) of the network's images, by default 4 x the plane-sweep grid of cam_intrinsics.  The remaining keywords
        (use_graph, pipeline, copy_outputs, allow_eager_fallback) go to the DepthStream this object owns."""
        if t_win_r < 1 or 2 * t_win_r > _lib.GATHER_MAX_V:
            raise ValueError("VideoDepthStream: t_win_r %s, expected 1 .. %d" % (t_win_r, _lib.GATHER_MAX_V // 2))
        if getattr(model, "t_win_r", t_win_r) != t_win_r:
            raise ValueError("VideoDepthStream: the model was built for t_win_r %s, the stream for %s" % (model.t_win_r, t_win_r))
        mean, std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        if len(mean) != 3 or len(std) != 3 or not all(np.isfinite(mean)) or not all(np.isfinite(std)) or 0.0 in std:
            raise ValueError("VideoDepthStream: mean / std take three finite values each, std non-zero")
        if net_size is None:
            h, w = _grid_size(cam_intrinsics)
            net_size = (4 * h, 4 * w)
        self.H, self.W = int(net_size[0]), int(net_size[1])
        if self.H <= 0 or self.W <= 0:
            raise ValueError("VideoDepthStream: net_size %s" % (net_size,))
        self.t_win_r = t_win_r
        self.R = 2 * t_win_r + 1
        self.mean, self.std = mean, std
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        self.stream = DepthStream(model, cam_intrinsics, d_candi, t_win_r=t_win_r, device=self.device, **depth_stream_kwargs)
        self.pipeline = bool(depth_stream_kwargs.get("pipeline", False))
        # the ring: image i at i * stride floats, the stride rounded up to whole 16-byte words so that every slot takes 16-byte stores
        n = 3 * self.H * self.W
        stride = (n + 3) // 4 * 4
        self._ring_buf = torch.empty(self.R * stride, dtype=torch.float32, device=self.device)
        self.ring = self._ring_buf.as_strided((self.R, 3, self.H, self.W), (stride, self.H * self.W, self.W, 1))
        # the window handed to DepthStream.step: written by one launch per push, read by the frame that follows on the same stream
        self._src = torch.empty((1, 2 * t_win_r, 3, self.H, self.W), dtype=torch.float32, device=self.device)
        self._ref = torch.empty((1, 3, self.H, self.W), dtype=torch.float32, device=self.device)
        self._stage = None              # pinned uint8 staging buffer of a host frame, its device twin, the copy's completion
        self._stage_dev = None
        self._stage_event = None
        self.reset()

    # ------------------------------------------------------------------ state
    def reset(self):
        """New trajectory: drops the ring, the extrinsics and the filter state (a pending pipelined frame too)."""
        self.n_pushed = 0
        self._extMs = []                # float64 [4,4] world -> camera of the last R frames, oldest first
        self._owed = None               # pipeline=True: push-order index of the frame whose maps the next step returns
        self.stream.reset()

    def check(self):
        self.stream.check()

    def flush(self):
        """pipeline=True: (ref_index, refined, dpv) of the frame that is still owed, or None."""
        out = self.stream.flush()
        owed, self._owed = self._owed, None
        if out is None:
            return None
        return (owed,) + tuple(out)

    # ------------------------------------------------------------------ one frame into its slot
    def _stage_host(self, arr):
        """A host uint8 frame -> a device uint8 tensor of the same shape, through the pinned buffer (asynchronous)."""
        t = torch.from_numpy(np.ascontiguousarray(arr)) if isinstance(arr, np.ndarray) else arr.contiguous()
        n = t.numel()
        if self._stage is None or self._stage.numel() < n:
            pin = self.device.type == "cuda"
            self._stage = torch.empty(n, dtype=torch.uint8, pin_memory=pin)
            self._stage_dev = torch.empty(n, dtype=torch.uint8, device=self.device)
            self._stage_event = torch.cuda.Event() if pin else None
        elif self._stage_event is not None:
            self._stage_event.synchronize()         # the previous frame's copy has left the buffer (long since, in practice)
        self._stage[:n].copy_(t.reshape(-1))
        self._stage_dev[:n].copy_(self._stage[:n], non_blocking=True)
        if self._stage_event is not None:
            self._stage_event.record(torch.cuda.current_stream(self.device))
        return self._stage_dev[:n].view(t.shape)

    def _ingest(self, frame, slot):
        dst = self.ring[slot]
        if isinstance(frame, np.ndarray):
            if frame.dtype != np.uint8:
                raise ValueError("VideoDepthStream.push: a numpy frame is uint8 (got %s); pass normalised floats as an fp32 tensor"
                                 % frame.dtype)
            layout = _layout(frame.shape)
            ops.frame_ingest(self._stage_host(frame), dst, self.mean, self.std, layout)
        elif isinstance(frame, torch.Tensor) and frame.dtype == torch.uint8:
            layout = _layout(frame.shape)
            if frame.device != self.device:
                frame = self._stage_host(frame) if frame.device.type == "cpu" else frame.to(self.device)
            ops.frame_ingest(frame, dst, self.mean, self.std, layout)
        elif isinstance(frame, torch.Tensor) and frame.dtype == torch.float32:
            # already normalised (the reference's dat['img']): no resize — resizing normalised floats is not the loaders' operation
            if tuple(frame.shape) not in ((3, self.H, self.W), (1, 3, self.H, self.W)):
                raise ValueError("VideoDepthStream.push: an fp32 frame is [3,%d,%d] or [1,3,%d,%d] (the network size), got %s"
                                 % (self.H, self.W, self.H, self.W, tuple(frame.shape)))
            dst.copy_(frame.reshape(3, self.H, self.W), non_blocking=True)
        else:
            raise ValueError("VideoDepthStream.push: a frame is a uint8 array / tensor or an fp32 tensor, got %s"
                             % (getattr(frame, "dtype", type(frame)),))

    @staticmethod
    def _extrinsic(extM):
        """float64 [4,4]; what the loaders hand out for a missing pose (an int, test_KVNet.py:37) becomes NaN."""
        if extM is None or isinstance(extM, int):
            return np.full((4, 4), np.nan)
        if isinstance(extM, torch.Tensor):
            extM = extM.detach().cpu().numpy()
        m = np.asarray(extM, dtype=np.float64)
        if m.shape != (4, 4):
            raise ValueError("VideoDepthStream.push: extM is a 4 x 4 world-to-camera matrix, got %s" % (m.shape,))
        return m

    # ------------------------------------------------------------------ public
    def push(self, frame, extM):
        """frame: uint8 [H,W,3] / [3,H,W] of any size (numpy or tensor, host or device), or an fp32 [3,H,W] / [1,3,H,W] tensor at the
        network size taken as already normalised; extM: its 4 x 4 world-to-camera matrix.
        Returns None until 2 t_win_r + 1 frames are in, and for every window that holds a NaN extrinsic (the filter state is
        dropped: test_KVNet.py:241-246; with pipeline=True the owed frame goes with it, as in DepthStream.reset); else
        (ref_index, refined, dpv) as DepthStream.step returns them, ref_index being the push-order index of the frame the maps
        belong to: the window's centre — t_win_r frames behind the push — or, with pipeline=True, the previous window's centre
        (None while there is none; flush() hands out the last)."""
        ext = self._extrinsic(extM)
        self._ingest(frame, self.n_pushed % self.R)            # raises before anything is counted
        self._extMs.append(ext)
        if len(self._extMs) > self.R:
            self._extMs.pop(0)
        self.n_pushed += 1
        if self.n_pushed < self.R:
            return None
        if any(np.isnan(m.min()) or np.isnan(m.max()) for m in self._extMs):       # check_datArray_pose
            self.stream.reset()
            self._owed = None
            return None
        src_slots, ref_slot, ref_index = window_slots(self.n_pushed, self.t_win_r)
        ext_ref = self._extMs[self.t_win_r]
        ext_src = [m for i, m in enumerate(self._extMs) if i != self.t_win_r]
        poses = np.stack([warp_homo.get_rel_extrinsicM(ext_ref, m).astype(np.float32) for m in ext_src])[None]
        poses = torch.from_numpy(poses).to(self.device)
        ops.window_gather(self.ring, src_slots + [ref_slot], self._src, self._ref)
        first = self.stream.bv_predict is None                  # the first-frame branch answers at once, pipelined or not
        out = self.stream.step(self._ref, self._src, poses)
        if self.pipeline and not first:
            ref_index, self._owed = self._owed, ref_index
        if out is None:
            return None
        return (ref_index,) + tuple(out)


def run_sequence(stream, frames, extMs):
    """The driver loop over a whole sequence: yields what push returns for every window that produced maps, then the flush() result
    (pipeline=True)."""
    for frame, extM in zip(frames, extMs):
        out = stream.push(frame, extM)
        if out is not None:
            yield out
    out = stream.flush()
    if out is not None:
        yield out
