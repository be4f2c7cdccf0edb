"""Frame-at-a-time training: push one camera frame, its ground-truth depth frame and its extrinsic, get a training step.

`train()` and `TrainGraph.step()` take a finished window: normalised fp32 images, relative poses and two int64 label maps on the
device.  The reference builds that window in its training driver (train_KVNet.py:283-330 over mdataloader/batch_loader.py:78-96,239-279:
a list of 2r + 1 loader items that slides, `_check_datArray_pose`, `get_rel_extrinsicM` per source, the `prev_invalid` rule) from items
its loaders prepared on the host (mdataloader/scanNet.py:368-422) — five fp32 images and two int64 maps uploaded per step where one
uint8 frame and one uint16 depth frame are new.  This module owns that loop:

  * `DepthLabeler`: one uint16 depth frame -> `dmap`, `dmap_imgsize_digit` (or `dmap_up4_imgsize_digit`), `dmap_raw`, `dmap_imgsize`
    in one launch (ops.depth_ingest), bit for bit what the loaders compute.  Two things come from the host because only the host can
    state them exactly: the source-index tables of PIL's NEAREST resize (`pillow_nearest_index`: a double accumulated per output
    index, which no integer formula reproduces for every size pair) and the integer thresholds that stand for np.digitize against
    float64 candidates (`label_thresholds`).
  * `TrainVideoStream`: the image ring and window assembly of video.VideoDepthStream, a ring of label slots written at push time (the
    reference frame's labels are read in place r pushes later), the validity rule, float64 relative poses, and one training step per
    valid window with BV_predict kept on the device between pushes.
"""
import numpy as np
import torch

from . import _lib, misc, ops
from . import homography as warp_homo
from .train_step import TrainGraph, _check_clip, _check_dup, train
from .video import IMAGENET_MEAN, IMAGENET_STD, VideoDepthStream, _grid_size, window_slots


def pillow_nearest_index(n_in, n_out):
    """Source index of every output index of PIL.Image.resize(..., NEAREST) along an axis of n_in -> n_out pixels, int64 [n_out].
    Pillow tabulates them by accumulating a double (xo = 0.5 s, then per output index idx = (int) xo, xo += s, with
    s = (double) n_in / n_out), which is NOT ((2 i + 1) n_in) // (2 n_out) wherever the exact position is an integer the accumulated
    sum lands just under (640 -> 96: indices 25, 28, ..., 94 come out one lower)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError("pillow_nearest_index: sizes %d -> %d" % (n_in, n_out))
    s = float(n_in) / float(n_out)
    out = np.empty(n_out, dtype=np.int64)
    xo = 0.5 * s
    for i in range(n_out):
        out[i] = int(xo)
        xo += s
    return np.minimum(out, n_in - 1)


def label_thresholds(d_candi, depth_scale=.001):
    """int32 [n] thresholds T with np.digitize(np.float32(u) * np.float32(depth_scale), d_candi) == #{k : T[k] <= u} for every uint16
    u: T[k] = the smallest u whose fp32 metres, promoted to float64, are >= d_candi[k] (65536: none).  The comparison is numpy's own —
    float64 candidates against the promoted fp32 value — done once over all 65,536 values."""
    d = np.asarray(d_candi, dtype=np.float64).reshape(-1)
    if d.size < 1 or not np.all(np.isfinite(d)) or np.any(np.diff(d) <= 0):
        raise ValueError("label_thresholds: d_candi must be finite and strictly increasing")
    scale = np.float32(depth_scale)
    if not np.isfinite(scale) or scale <= 0:
        raise ValueError("label_thresholds: depth_scale %r" % (depth_scale,))
    metres = np.arange(65536, dtype=np.float32) * scale                 # the loaders' `.float() * .001`
    labels = np.digitize(metres.astype(np.float64), d)                  # non-decreasing in u
    return np.searchsorted(labels, np.arange(1, d.size + 1), side="left").astype(np.int32)


class _PinnedStage:
    """A host array -> a device tensor of the same shape through one pinned buffer (asynchronous), as VideoDepthStream._stage_host."""

    def __init__(self, device, dtype):
        self.device, self.dtype = device, dtype
        self._host = self._dev = self._event = None

    def __call__(self, t):
        t = t.contiguous()
        n = t.numel()
        if self._host is None or self._host.numel() < n:
            pin = self.device.type == "cuda"
            self._host = torch.empty(n, dtype=self.dtype, pin_memory=pin)
            self._dev = torch.empty(n, dtype=self.dtype, device=self.device)
            self._event = torch.cuda.Event() if pin else None
        elif self._event is not None:
            self._event.synchronize()               # the previous frame's copy has left the buffer
        self._host[:n].copy_(t.reshape(-1))
        self._dev[:n].copy_(self._host[:n], non_blocking=True)
        if self._event is not None:
            self._event.record(torch.cuda.current_stream(self.device))
        return self._dev[:n].view(t.shape)


def _depth_bits(depth):
    """A uint16 [Hin,Win] array / tensor -> an int16 tensor of the same bits (host or device, no copy); ValueError otherwise."""
    if isinstance(depth, np.ndarray):
        if depth.dtype != np.uint16:
            raise ValueError("a depth frame is uint16 (got %s)" % depth.dtype)
        depth = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16))
    elif isinstance(depth, torch.Tensor) and depth.dtype == torch.uint16:
        depth = depth.view(torch.int16)
    elif not (isinstance(depth, torch.Tensor) and depth.dtype == torch.int16):
        raise ValueError("a depth frame is a uint16 array / tensor, got %s" % (getattr(depth, "dtype", type(depth)),))
    if depth.dim() == 3 and depth.shape[0] == 1:
        depth = depth[0]
    if depth.dim() != 2 or depth.numel() == 0:
        raise ValueError("a depth frame is [Hin,Win], got %s" % (tuple(depth.shape),))
    return depth


class DepthLabeler:
    """The loaders' depth preparation (mdataloader/scanNet.py:372-422) for one camera on the device."""

    def __init__(self, d_candi, net_size, grid_size, depth_scale=.001, refine_dup=False, device=None):
        """net_size = (H, W) of the images, grid_size = (h, w) of the plane-sweep grid (the loaders' resize_dmap).  refine_dup: the
        image-size label is `dmap_up4_imgsize_digit`, digitised against misc.d_candi_up4(d_candi)."""
        self.H, self.W = int(net_size[0]), int(net_size[1])
        self.h, self.w = int(grid_size[0]), int(grid_size[1])
        if min(self.H, self.W, self.h, self.w) <= 0:
            raise ValueError("DepthLabeler: net_size %s, grid_size %s" % (net_size, grid_size))
        self.depth_scale = float(depth_scale)
        self.refine_dup = bool(refine_dup)
        self.full_key = "dmap_up4_imgsize_digit" if self.refine_dup else "dmap_imgsize_digit"
        self.thr_q = label_thresholds(d_candi, depth_scale)
        self.thr_full = label_thresholds(misc.d_candi_up4(d_candi), depth_scale) if self.refine_dup else self.thr_q
        for t in (self.thr_q, self.thr_full):
            if t.size > _lib.DEPTH_MAX_THRESHOLDS:
                raise ValueError("DepthLabeler: %d candidates, the kernel takes %d" % (t.size, _lib.DEPTH_MAX_THRESHOLDS))
        self.device = torch.device(device if device is not None else "cuda")
        self._tables = {}
        self._stage = _PinnedStage(self.device, torch.int16)

    def host_tables(self, Hin, Win):
        """The six int32 source-index tables of a [Hin,Win] frame: rows / columns of the image-size maps, of the direct resize to
        the grid, and of the grid-size hole mask (the image-size table sampled through the image -> grid table: the reference
        resizes the mask twice, scanNet.py:374-375,389)."""
        rows_full, cols_full = pillow_nearest_index(Hin, self.H), pillow_nearest_index(Win, self.W)
        rows_q, cols_q = pillow_nearest_index(Hin, self.h), pillow_nearest_index(Win, self.w)
        mask_rows = rows_full[pillow_nearest_index(self.H, self.h)]
        mask_cols = cols_full[pillow_nearest_index(self.W, self.w)]
        return tuple(t.astype(np.int32) for t in (rows_full, cols_full, rows_q, cols_q, mask_rows, mask_cols))

    def tables(self, Hin, Win):
        key = (int(Hin), int(Win))
        if key not in self._tables:
            self._tables[key] = tuple(torch.from_numpy(t).to(self.device) for t in self.host_tables(*key))
        return self._tables[key]

    def empty_outputs(self):
        return {"dmap": torch.empty((1, self.h, self.w), dtype=torch.int64, device=self.device),
                self.full_key: torch.empty((1, self.H, self.W), dtype=torch.int64, device=self.device),
                "dmap_raw": torch.empty((1, self.h, self.w), dtype=torch.float32, device=self.device),
                "dmap_imgsize": torch.empty((1, self.H, self.W), dtype=torch.float32, device=self.device)}

    def __call__(self, depth_u16, out=None):
        """depth_u16: uint16 [Hin,Win], numpy or tensor, host (uploaded through a pinned buffer) or device.  out: a dict of output
        tensors under the reference's keys — only the keys it holds are computed; None: all four are allocated.  Returns the dict:
        `dmap` [1,h,w] and `dmap_imgsize_digit` / `dmap_up4_imgsize_digit` [1,H,W] int64, `dmap_raw` [1,h,w] and `dmap_imgsize`
        [1,H,W] fp32 masked metres."""
        depth = _depth_bits(depth_u16)
        if out is None:
            out = self.empty_outputs()
        unknown = set(out) - {"dmap", self.full_key, "dmap_raw", "dmap_imgsize"}
        if unknown or not out:
            raise ValueError("DepthLabeler: outputs %s (this labeler writes dmap, %s, dmap_raw, dmap_imgsize)" % (sorted(out), self.full_key))
        if depth.device != self.device:
            depth = self._stage(depth) if depth.device.type == "cpu" else depth.to(self.device)
        ops.depth_ingest(depth, self.tables(*depth.shape), self.depth_scale, self.thr_q, self.thr_full, labels_q=out.get("dmap"),
                         labels_full=out.get(self.full_key), dmap_raw=out.get("dmap_raw"), dmap_imgsize=out.get("dmap_imgsize"))
        return out


class TrainVideoStream:
    """One trajectory per process (train() asserts N = 1): push(frame, depth, extM) per camera frame, one optimizer step per valid
    window of 2 t_win_r + 1 frames."""

    # the image ring is VideoDepthStream's: its staging and ingest methods work on the attributes this class sets up the same way
    _stage_host = VideoDepthStream._stage_host
    _ingest = VideoDepthStream._ingest
    _extrinsic = staticmethod(VideoDepthStream._extrinsic)

    def __init__(self, model, optimizer, cam_intrinsics, d_candi, t_win_r=2, net_size=None, depth_scale=.001, use_graph=False,
                 refine_dup=False, deterministic=None, grad_clip_max=None, skip_nonfinite=False, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 grad_reducer=None, device=None):
        """net_size = (H, W) of the network's images, by default 4 x the plane-sweep grid of cam_intrinsics.  use_graph: update-branch
        windows run TrainGraph.step (hipGraph replay after its eager warm-up); windows without a BV_predict run eager train().
        deterministic / grad_clip_max / skip_nonfinite / refine_dup: as in train() and TrainGraph."""
        if grad_reducer is not None:
            raise ValueError("TrainVideoStream: multi-rank training and gradient accumulation are not on this path (grad_reducer given)")
        if t_win_r < 1 or 2 * t_win_r > _lib.GATHER_MAX_V:
            raise ValueError("TrainVideoStream: t_win_r %s, expected 1 .. %d" % (t_win_r, _lib.GATHER_MAX_V // 2))
        if getattr(model, "t_win_r", t_win_r) != t_win_r:
            raise ValueError("TrainVideoStream: the model was built for t_win_r %s, the stream for %s" % (model.t_win_r, t_win_r))
        from .nets import require_volume_refiner
        require_volume_refiner(model, "TrainVideoStream")
        _check_dup(model, refine_dup)
        _check_clip(optimizer, grad_clip_max, skip_nonfinite)
        mean, std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        if len(mean) != 3 or len(std) != 3 or not all(np.isfinite(mean)) or not all(np.isfinite(std)) or 0.0 in std:
            raise ValueError("TrainVideoStream: mean / std take three finite values each, std non-zero")
        h, w = _grid_size(cam_intrinsics)
        if net_size is None:
            net_size = (4 * h, 4 * w)
        self.H, self.W = int(net_size[0]), int(net_size[1])
        if self.H <= 0 or self.W <= 0:
            raise ValueError("TrainVideoStream: net_size %s" % (net_size,))
        self.model, self.optimizer, self.cam, self.d_candi = model, optimizer, cam_intrinsics, d_candi
        self.t_win_r, self.R = t_win_r, 2 * t_win_r + 1
        self.mean, self.std = mean, std
        self.refine_dup, self.deterministic = bool(refine_dup), deterministic
        self.grad_clip_max, self.skip_nonfinite = grad_clip_max, bool(skip_nonfinite)
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        self.labeler = DepthLabeler(d_candi, (self.H, self.W), (h, w), depth_scale=depth_scale, refine_dup=refine_dup, device=self.device)
        self.graph = TrainGraph(model, optimizer, t_win_r, d_candi, cam_intrinsics, deterministic=deterministic, refine_dup=refine_dup,
                                grad_clip_max=grad_clip_max, skip_nonfinite=skip_nonfinite) if use_graph else None
        # the image ring and the window buffers, laid out as in VideoDepthStream
        n = 3 * self.H * self.W
        stride = (n + 3) // 4 * 4
        self._ring_buf = torch.empty(self.R * stride, dtype=torch.float32, device=self.device)
        self.ring = self._ring_buf.as_strided((self.R, 3, self.H, self.W), (stride, self.H * self.W, self.W, 1))
        self._src = torch.empty((1, 2 * t_win_r, 3, self.H, self.W), dtype=torch.float32, device=self.device)
        self._ref = torch.empty((1, 3, self.H, self.W), dtype=torch.float32, device=self.device)
        self._stage = self._stage_dev = self._stage_event = None
        # the label ring: frame i's labels in slot i mod R, digitised when the frame is pushed
        self.labels_q = torch.zeros((self.R, 1, h, w), dtype=torch.int64, device=self.device)
        self.labels_full = torch.zeros((self.R, 1, self.H, self.W), dtype=torch.int64, device=self.device)
        self.reset()

    def reset(self):
        """New trajectory: drops the rings' contents, the extrinsics and BV_predict (the weights and the optimizer stay)."""
        self.n_pushed = 0
        self._extMs = []                # float64 [4,4] world -> camera of the last R frames, oldest first
        self._has_depth = []            # whether each of them came with a depth map
        self.bv_predict = None          # None: the next valid window takes the first-frame branch

    def _depth(self, depth):
        """None for a missing depth map (None or the loaders' int, batch_loader.py:88), else the frame's bits; raises on anything else."""
        if depth is None or isinstance(depth, (int, np.integer)):
            return None
        return _depth_bits(depth)

    def push(self, frame, depth, extM):
        """frame: as VideoDepthStream.push takes it (uint8 [H,W,3] / [3,H,W] of any size, or a prepared fp32 image at the network
        size); depth: uint16 [Hin,Win] (numpy or tensor, host or device), or None / an int for a missing map; extM: the 4 x 4
        world-to-camera matrix, or None / an int / NaN for a missing pose.
        Returns None until 2 t_win_r + 1 frames are in and for every window that holds a missing depth map or a NaN pose (no step is
        run; the next valid window starts without a BV_predict: train_KVNet.py:298-303,321-323); else
        (ref_index, loss, r_dpv, dmap_lowres, dmap_highres) of the training step on the window whose centre is frame ref_index —
        device tensors, nothing is read back.  With use_graph=True a replayed step returns None for the three maps (the graph keeps
        the loss and BV_predict only)."""
        ext = self._extrinsic(extM)
        bits = self._depth(depth)                              # both raise before anything is counted
        slot = self.n_pushed % self.R
        self._ingest(frame, slot)
        if bits is not None:
            self.labeler(bits, out={"dmap": self.labels_q[slot], self.labeler.full_key: self.labels_full[slot]})
        self._extMs.append(ext)
        self._has_depth.append(bits is not None)
        if len(self._extMs) > self.R:
            self._extMs.pop(0)
            self._has_depth.pop(0)
        self.n_pushed += 1
        if self.n_pushed < self.R:
            return None
        if not all(self._has_depth) or any(np.isnan(m.min()) or np.isnan(m.max()) for m in self._extMs):    # _check_datArray_pose
            self.bv_predict = None                              # prev_invalid
            return None
        src_slots, ref_slot, ref_index = window_slots(self.n_pushed, self.t_win_r)
        ext_ref = self._extMs[self.t_win_r]
        ext_src = [m for i, m in enumerate(self._extMs) if i != self.t_win_r]
        poses = np.stack([warp_homo.get_rel_extrinsicM(ext_ref, m).astype(np.float32) for m in ext_src])[None]
        poses = torch.from_numpy(poses).to(self.device)
        ops.window_gather(self.ring, src_slots + [ref_slot], self._src, self._ref)
        dmap, dmap_full = self.labels_q[ref_slot], self.labels_full[ref_slot]
        if self.graph is not None and self.bv_predict is not None:
            loss, self.bv_predict = self.graph.step(self._ref, self._src, poses, dmap, dmap_full, self.bv_predict)
            return ref_index, loss.clone(), None, None, None
        ref_dat = {"img": self._ref, "dmap": dmap, self.labeler.full_key: dmap_full}
        src_dats = [{"img": self._src[0, v:v + 1]} for v in range(2 * self.t_win_r)]
        r_dpv, self.bv_predict, loss, lo, hi = train(
            1, self.model, self.optimizer, self.t_win_r, self.d_candi, [ref_dat], [src_dats], poses, self.bv_predict, [self.cam],
            refine_dup=self.refine_dup, deterministic=self.deterministic, grad_clip_max=self.grad_clip_max,
            skip_nonfinite=self.skip_nonfinite)
        return ref_index, loss, r_dpv, lo, hi


def run_training_sequence(stream, frames, depths, extMs):
    """The training driver's loop over one trajectory (train_KVNet.py:284-330): yields what push returns for every valid window."""
    for frame, depth, extM in zip(frames, depths, extMs):
        out = stream.push(frame, depth, extM)
        if out is not None:
            yield out
