"""On-device depth evaluation: error metrics of depth maps against ground truth, per confidence set.

The reference evaluates offline: it writes its maps to files (test_utils/export_res.py:78-159), forms
`np.abs(dmap_ref - dmap) * (dmap_ref > 0)` with numpy on the host (:108-116) and scores the files later.  Here a depth frame costs
two small launches (ops.depth_eval), the sums and counts stay on the device, nothing synchronises — the calls can be captured into a
hipGraph like every other per-frame stage — and the caller pays one device-to-host copy when it asks for the numbers:

  * `DepthMetrics`: the running totals of one (prediction, ground truth) pairing, per confidence set;
  * `metrics_from_record`: sums and counts -> MAE, abs-rel, sq-rel, RMSE, RMSE(log), scale-invariant log error, the three delta
    accuracies, coverage — pure numpy;
  * `EvalVideoStream`: a video.VideoDepthStream, a train_video.DepthLabeler and two DepthMetrics: push a frame, its uint16 depth frame
    and its extrinsic; the refined volume is scored against `dmap_imgsize`, the K-Net DPV against `dmap_raw`, each depth frame against
    the ground truth of the push it belongs to.
"""
import numpy as np
import torch

from . import _lib, misc, ops
from . import homography as warp_homo
from .train_video import DepthLabeler, _depth_bits
from .video import VideoDepthStream, _grid_size

METRICS = ("mae", "abs_rel", "sq_rel", "rmse", "rmse_log", "sc_inv", "delta1", "delta2", "delta3")


def log_thresholds(conf_thresholds):
    """fp32 [J] thresholds on max_k logp for confidences in [0, 1), the first 0: float32(log c_j) with the log taken in float64
    (log 0 = -inf: set 0 holds every pixel)."""
    c = np.asarray(conf_thresholds, dtype=np.float64).reshape(-1)
    if not 1 <= c.size <= _lib.DEPTH_EVAL_MAX_SETS:
        raise ValueError("conf_thresholds: %d values, expected 1 .. %d" % (c.size, _lib.DEPTH_EVAL_MAX_SETS))
    if c[0] != 0 or not np.all((c >= 0) & (c < 1)) or np.any(np.diff(c) <= 0):
        raise ValueError("conf_thresholds: confidences in [0, 1), strictly increasing, the first 0 (got %s)" % (tuple(c),))
    with np.errstate(divide="ignore"):
        thr = np.log(c).astype(np.float32)                      # c is float64: the log in double, rounded once
    if np.any(np.diff(thr) <= 0):
        raise ValueError("conf_thresholds %s are not distinct as fp32 logarithms" % (tuple(c),))
    return thr


def metrics_from_record(sums, counts, header, conf_thresholds=None):
    """sums [J,6] = sums of t0 .. t5, counts [J,4] = n, delta1, delta2, delta3, header [4] = frames, gt-valid pixels, bad pixels, 0
    (the records of nrgbd_depth_eval) -> a list of J dicts, one per confidence set:
        mae = St0 / n, abs_rel = St1 / n, sq_rel = St2 / n, rmse = sqrt(St3 / n), rmse_log = sqrt(St4 / n),
        sc_inv = sqrt(max(St4 / n - (St5 / n)^2, 0)), delta1..3 = deltak / n, coverage = n / gt_valid, bad = bad / gt_valid,
    and n, frames, gt_valid as integers.  An empty set gives NaN metrics and coverage 0 (never raises)."""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 6)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    header = np.asarray(header, dtype=np.int64).reshape(4)
    frames, gt_valid, bad = int(header[0]), int(header[1]), int(header[2])
    out = []
    for j in range(sums.shape[0]):
        n = int(counts[j, 0])
        rec = {"n": n, "frames": frames, "gt_valid": gt_valid}
        if conf_thresholds is not None:
            rec["conf_threshold"] = float(conf_thresholds[j])
        if n > 0:
            nd = np.float64(n)
            s = sums[j] / nd
            rec.update(mae=float(s[0]), abs_rel=float(s[1]), sq_rel=float(s[2]), rmse=float(np.sqrt(s[3])), rmse_log=float(np.sqrt(s[4])),
                       sc_inv=float(np.sqrt(max(s[4] - s[5] * s[5], 0.0))), delta1=float(counts[j, 1] / nd),
                       delta2=float(counts[j, 2] / nd), delta3=float(counts[j, 3] / nd))
        else:
            rec.update({k: float("nan") for k in METRICS})
        rec["coverage"] = float(n / np.float64(gt_valid)) if gt_valid > 0 else 0.0
        rec["bad"] = float(bad / np.float64(gt_valid)) if gt_valid > 0 else float("nan")
        out.append(rec)
    return out


class DepthMetrics:
    """Running error metrics of depth maps against ground truth on the device.  Confidence set j holds the pixels with
    `max_k logp >= float32(log c_j)` for c_j = conf_thresholds[j]; set 0 (c = 0) holds every evaluated pixel.  A pixel is evaluated when
    its ground truth g is > 0 and inside gt_range and its depth is finite and > 0 (else it is counted as bad)."""

    def __init__(self, conf_thresholds=(0.,), gt_range=(1e-3, float("inf")), device=None):
        self.conf_thresholds = tuple(float(c) for c in conf_thresholds)
        self.log_thr = log_thresholds(self.conf_thresholds)
        self.J = int(self.log_thr.size)
        self.gt_range = (float(gt_range[0]), float(gt_range[1]))
        if not self.gt_range[0] <= self.gt_range[1]:
            raise ValueError("DepthMetrics: gt_range %s" % (gt_range,))
        self.device = torch.device(device if device is not None else "cuda")
        J = self.J
        # both records in one buffer of 8-byte words each: sums [J,6] | counts [J,4] | header [4] — result() copies one
        self._words = 10 * J + 4
        self._buf = torch.zeros(2 * self._words, dtype=torch.int64, device=self.device)
        self.frame = self._views(self._buf[:self._words])
        self.total = self._views(self._buf[self._words:])
        self._workspace = None
        self._n = 0

    def _views(self, words):
        J = self.J
        return (words[:6 * J].view(torch.float64).view(J, 6), words[6 * J:10 * J].view(J, 4), words[10 * J:])

    def reset(self):
        """Zeroes the totals (asynchronous)."""
        self._buf[self._words:].zero_()

    def _reserve(self, n):
        if n > self._n:                 # the first call, or a larger map: the only allocation this object makes after __init__
            self._workspace = torch.empty(ops.depth_eval_workspace(n, self.J) // 8, dtype=torch.int64, device=self.device)
            self._n = n

    def update(self, depth, logconf, gt, err_map=None):
        """depth, logconf, gt (and err_map, written: |gt - depth| where gt > 0, else 0): contiguous CUDA fp32 tensors of one shape.
        Adds the frame to the totals and returns `frame` = (sums [J,6], counts [J,4], header [4]), device tensors that hold this
        call's record until the next call.  Allocates nothing once a map of this size has been seen and synchronises nothing."""
        self._reserve(depth.numel())
        ops.depth_eval(depth, logconf, gt, self.log_thr, self.gt_range, self._workspace, self.frame, self.total, err_map)
        return self.frame

    def update_dpv(self, BV_log, d_candi, gt, err_map=None):
        """BV_log [1,D,H,W]: a log-probability volume, planar or the R-Net's channels-last view (read where it lies), over d_candi —
        or over misc.d_candi_up4(d_candi) when it holds 4 len(d_candi) planes; gt [H,W] or [1,H,W]."""
        if BV_log.dim() != 4 or BV_log.shape[0] != 1:
            raise ValueError("update_dpv: BV_log %s is not [1,D,H,W]" % (tuple(BV_log.shape),))
        D = BV_log.shape[1]
        if D == 4 * len(d_candi):
            d_candi = misc.d_candi_up4(d_candi)
        elif D != len(d_candi):
            raise ValueError("update_dpv: a volume of %d planes over %d candidates" % (D, len(d_candi)))
        logp = BV_log[0]
        depth, conf = ops.depth_regress(logp, warp_homo._d_candi_dev(d_candi, BV_log.device), channels_last=ops.is_channels_last_view(logp))
        if gt.numel() != depth.numel():
            raise ValueError("update_dpv: gt %s against maps %s" % (tuple(gt.shape), tuple(depth.shape)))
        if err_map is not None:
            err_map = err_map.view(depth.shape)
        return self.update(depth, conf, gt.view(depth.shape), err_map)

    def result(self):
        """The totals as metrics_from_record gives them: one device-to-host copy (which waits for the launches before it)."""
        host = self._buf[self._words:].cpu().numpy()
        J = self.J
        return metrics_from_record(host[:6 * J].view(np.float64), host[6 * J:10 * J], host[10 * J:], self.conf_thresholds)


def gt_slot(push_index, n_slots):
    """Ring slot of the ground truth of push `push_index` (from 0).  With n_slots = 2 t_win_r + 2 the slot of push i is rewritten by
    push i + 2 t_win_r + 2, and its maps come out at push i + t_win_r (one later when pipelined, or at flush()): never after that."""
    if push_index < 0 or n_slots < 1:
        raise ValueError("gt_slot: push %d, %d slots" % (push_index, n_slots))
    return push_index % n_slots


class GtRing:
    """Which push's ground truth every ring slot holds (host bookkeeping; the maps themselves live in the owner's device tensors)."""

    def __init__(self, n_slots):
        self.n_slots = int(n_slots)
        self.held = [None] * self.n_slots       # push index whose ground truth a slot holds (None: none, or a missing depth frame)

    def clear(self):
        self.held = [None] * self.n_slots

    def store(self, push_index, has_depth):
        """The slot push `push_index` writes its ground truth to (it is the slot's holder from now on, or nobody is)."""
        slot = gt_slot(push_index, self.n_slots)
        self.held[slot] = push_index if has_depth else None
        return slot

    def lookup(self, ref_index):
        """The slot that holds the ground truth of push `ref_index`, or None when that push came without a depth map."""
        slot = gt_slot(ref_index, self.n_slots)
        return slot if self.held[slot] == ref_index else None


class EvalVideoStream:
    """VideoDepthStream + ground truth: push(frame, depth_u16, extM) per camera frame; every depth frame that comes out is scored
    against the ground truth pushed with its reference frame.  `hires`: the refined volume against `dmap_imgsize`; `lowres`: the K-Net
    DPV against `dmap_raw`."""

    def __init__(self, model, cam_intrinsics, d_candi, t_win_r=2, depth_scale=.001, conf_thresholds=(0.,), gt_range=(1e-3, float("inf")),
                 net_size=None, **video_kwargs):
        from .nets import require_volume_refiner
        require_volume_refiner(model, "EvalVideoStream")
        self.video = VideoDepthStream(model, cam_intrinsics, d_candi, t_win_r=t_win_r, net_size=net_size, **video_kwargs)
        self.device, self.t_win_r, self.d_candi = self.video.device, t_win_r, d_candi
        h, w = _grid_size(cam_intrinsics)
        H, W = self.video.H, self.video.W
        self.labeler = DepthLabeler(d_candi, (H, W), (h, w), depth_scale=depth_scale, device=self.device)
        self.hires = DepthMetrics(conf_thresholds, gt_range, device=self.device)
        self.lowres = DepthMetrics(conf_thresholds, gt_range, device=self.device)
        self.n_slots = 2 * t_win_r + 2
        self.gt_ring = GtRing(self.n_slots)
        self.gt_full = torch.zeros((self.n_slots, 1, H, W), dtype=torch.float32, device=self.device)
        self.gt_raw = torch.zeros((self.n_slots, 1, h, w), dtype=torch.float32, device=self.device)

    def reset(self):
        """New trajectory: drops the frames, the filter state and the ground-truth ring; the totals stay (reset them with
        hires.reset() / lowres.reset())."""
        self.video.reset()
        self.gt_ring.clear()

    def check(self):
        self.video.check()

    def _evaluate(self, out):
        if out is None:
            return None
        ref_index, refined, dpv = out
        slot = self.gt_ring.lookup(ref_index)
        if slot is None:                                        # the frame came without a depth map: maps, but no update
            return ref_index, refined, dpv, None, None
        hi = self.hires.update_dpv(refined, self.d_candi, self.gt_full[slot])
        lo = self.lowres.update_dpv(dpv, self.d_candi, self.gt_raw[slot])
        return ref_index, refined, dpv, hi, lo

    def push(self, frame, depth, extM):
        """frame, extM: as VideoDepthStream.push; depth: uint16 [Hin,Win] (numpy or tensor, host or device), or None / an int for a
        missing map.  Returns None where VideoDepthStream.push does (a NaN pose in the window: nothing is evaluated), else
        (ref_index, refined, dpv, hires_frame, lowres_frame): the frame records of the two DepthMetrics, valid until the next
        evaluation, or None twice when frame ref_index was pushed without a depth map."""
        bits = None if depth is None or isinstance(depth, (int, np.integer)) else _depth_bits(depth)       # raises before anything is counted
        index = self.video.n_pushed
        out = self.video.push(frame, extM)
        slot = self.gt_ring.store(index, bits is not None)
        if bits is not None:
            self.labeler(bits, out={"dmap_raw": self.gt_raw[slot], "dmap_imgsize": self.gt_full[slot]})
        return self._evaluate(out)

    def flush(self):
        """pipeline=True: the frame that is still owed, evaluated like any other; None otherwise."""
        return self._evaluate(self.video.flush())

    def result(self):
        return {"hires": self.hires.result(), "lowres": self.lowres.result()}


def evaluate_sequence(stream, frames, depths, extMs):
    """One trajectory through an EvalVideoStream (the loop of test_KVNet.py:185-250 with the scoring the reference does offline):
    resets the stream's trajectory state, pushes every frame, flushes, and returns {'hires': ..., 'lowres': ...} of the totals —
    which keep accumulating over calls: a validation set is many trajectories."""
    stream.reset()
    for frame, depth, extM in zip(frames, depths, extMs):
        stream.push(frame, depth, extM)
    stream.flush()
    stream.check()
    return stream.result()
