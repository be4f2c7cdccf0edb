"""Frame-to-model tracking: a depth frame registered against the fused TSDF volume before it is integrated (KinectFusion's
tracking half; csrc/icp.hip, include/nrgbd.h spells out every operation).

The reference takes its poses from an external odometry, and FusionVideoStream integrates each map at exactly the pose pushed with
it; a drifting pose smears the volume.  `FrameTracker` corrects a pose guess: the volume is ray cast from the guess
(TSDFVolume.raycast: depth and camera-frame normals), the frame's depth map is associated with it projectively, and a few
Gauss-Newton iterations on the point-to-plane residuals — two launches each, ops.icp_terms and ops.icp_update, coarse to fine —
find the motion dT between the frame's camera and the guess.  Nothing is read back between iterations; one device-to-host copy at
the end fetches the state and the iteration log.

The point-to-plane term alone cannot see three motions on a flat surface — the two in-plane translations and the rotation about the
normal — and a wall, a floor or a table top is what an indoor sequence mostly shows.  `FrameTracker(..., photo=True)` on a colour
volume adds a photometric term to the same normal equations (colour ICP): the ray cast also renders the volume's colour, and every
pixel that kept its geometric pair compares its own luminance with the model's, interpolated bilinearly where the point projects
(ops.icp_terms_photo, still two launches per iteration).  Geometry pins the motions it can see, texture the rest.

A pose this tracker (or anything else) corrects later can be applied to a frame that is already fused: TSDFVolume.reintegrate moves
the frame in one launch, FusionVideoStream(history=N).repose / retrack do it for the stream's last N frames (fusion.py).

Deliberately not built: frame normals and a normal-angle gate, relocalisation after a loss, an image pyramid with pre-filtering — the
coarse levels compare the visited pixel's own value with the point-sampled ray cast."""
import math

import numpy as np
import torch

from . import _lib, ops

FLAGS = {0: "ok", _lib.ICP_FEW: "too few pairs", _lib.ICP_NONFINITE: "a sum is not finite", _lib.ICP_DEGENERATE: "degenerate geometry",
         _lib.ICP_LARGE: "a step past half a radian"}
DEFAULT_LEVELS = ((4, 10), (2, 5), (1, 4))


class TrackResult:
    """extM [4,4] float64: the frame's world -> camera pose (the guess when the track was lost); ok: flag == 0; flag: 0 or the
    NRGBD_ICP_* reason (tracking.FLAGS); log [iterations,4] float64 = (pairs, weighted squared error, |xi|^2, flag) per iteration;
    delta [4,4] float64: the motion frame camera -> guess camera that was found."""

    def __init__(self, extM, flag, log, delta):
        self.extM, self.flag, self.log, self.delta = extM, int(flag), log, delta
        self.ok = self.flag == 0

    def __repr__(self):
        return "TrackResult(ok=%s, flag=%d (%s), iterations=%d)" % (self.ok, self.flag, FLAGS.get(self.flag, "?"), len(self.log))


def _levels(levels):
    out = tuple((int(s), int(n)) for s, n in levels)
    if not out or any(s < 1 or n < 1 for s, n in out):
        raise ValueError("FrameTracker: levels = ((sub, iterations), ...), both >= 1; got %s" % (levels,))
    return out


class FrameTracker:
    """Tracks H x W depth frames against `volume`.  size = (H, W); intrinsics: (fx, fy, cx, cy) at that size or a cam_intrinsics
    dict; levels: (sub, iterations) coarse to fine — a level visits every sub-th pixel of the frame and ray casts the model at
    (H // sub, W // sub).  photo=True (a colour volume, else ValueError): the tracker for `track(..., image=...)`, which also owns
    one [3,Hs,Ws] colour map per level and a second residual map.  Owns every buffer (the levels' model maps, the state, the partial
    records, the log, a residual map): after construction `track` allocates nothing on the device."""

    def __init__(self, volume, size, intrinsics, levels=DEFAULT_LEVELS, photo=False):
        from .fusion import intrinsics_at
        self.volume = volume
        self.photo = bool(photo)
        if self.photo and getattr(volume, "color", None) is None:
            raise ValueError("FrameTracker: photo=True needs a colour volume (TSDFVolume(..., color=True))")
        self.H, self.W = (int(n) for n in size)
        self.levels = _levels(levels)
        dev = volume.device
        self._levels = []
        words = 0
        for sub, iters in self.levels:
            Hs, Ws = self.H // sub, self.W // sub
            if Hs < 1 or Ws < 1:
                raise ValueError("FrameTracker: a %d x %d frame has no pixel at sub = %d" % (self.H, self.W, sub))
            if isinstance(intrinsics, dict):
                K = intrinsics_at(intrinsics, Hs, Ws)
            else:
                K = tuple(float(k) / sub for k in intrinsics)
            maps = (torch.empty((Hs, Ws), dtype=torch.float32, device=dev), torch.empty((3, Hs, Ws), dtype=torch.float32, device=dev))
            if self.photo:
                maps += (torch.empty((3, Hs, Ws), dtype=torch.float32, device=dev),)
            self._levels.append((sub, iters, (Hs, Ws), K, maps))
            words = max(words, ops.icp_workspace(Hs, Ws) // 8)
        self.K = intrinsics_at(intrinsics, self.H, self.W) if isinstance(intrinsics, dict) else tuple(float(k) for k in intrinsics)
        if len(self.K) != 4:
            raise ValueError("FrameTracker: intrinsics = (fx, fy, cx, cy)")
        self.iterations = sum(n for _, n in self.levels)
        # the state and the log in one buffer: one copy fetches both
        self._result = torch.zeros(ops.ICP_STATE_WORDS + 4 * self.iterations, dtype=torch.float64, device=dev)
        self._state, self._log = self._result[:ops.ICP_STATE_WORDS], self._result[ops.ICP_STATE_WORDS:]
        self._partial = torch.zeros(words, dtype=torch.float64, device=dev)
        self._resid = torch.empty((self.H, self.W), dtype=torch.float32, device=dev)
        self._resid_photo = torch.empty((self.H, self.W), dtype=torch.float32, device=dev) if self.photo else None

    def _params(self, dist_thr, huber):
        dist_thr = 2.0 * self.volume.trunc if dist_thr is None else float(dist_thr)
        huber = self.volume.voxel_size if huber is None else float(huber)
        return dist_thr, huber

    def _depth(self, depth, gate):
        if depth.dim() == 3 and depth.shape[0] == 1:
            depth = depth[0]
            gate = gate if gate is None else gate.view(depth.shape)
        if tuple(depth.shape) != (self.H, self.W):
            raise ValueError("FrameTracker: depth is [%d,%d], got %s" % (self.H, self.W, tuple(depth.shape)))
        return depth, gate

    def _image(self, image, image_affine, who):
        """An image comes to a photo tracker and to no other; -> the image as [3,H,W]."""
        if (image is not None) != self.photo:
            raise ValueError("FrameTracker.%s: %s" % (who, "a tracker built with photo=True takes an image" if self.photo else
                                                      "an image takes a tracker built with photo=True"))
        if image is None and image_affine is not None:
            raise ValueError("FrameTracker.%s: image_affine comes with image" % who)
        if image is not None and tuple(image.shape) != (3, self.H, self.W):
            raise ValueError("FrameTracker.%s: image is [3,%d,%d], got %s" % (who, self.H, self.W, tuple(image.shape)))
        return image

    def _terms(self, depth, sub, maps, K, dist_thr, huber, depth_range, gate, gate_thr, image, image_affine, photo_weight, photo_huber,
               resid=None, resid_photo=None):
        gate_thr = 0.0 if gate_thr is None else gate_thr
        if image is None:
            return ops.icp_terms(depth, self.K, sub, maps[0], maps[1], K, self._state, self._partial, dist_thr, huber,
                                 depth_range=depth_range, gate=gate, gate_thr=gate_thr, resid=resid)
        return ops.icp_terms_photo(depth, self.K, sub, maps[0], maps[1], K, self._state, self._partial, dist_thr, huber, image, maps[2],
                                   photo_weight, photo_huber, image_affine=image_affine, depth_range=depth_range, gate=gate,
                                   gate_thr=gate_thr, resid=resid, resid_photo=resid_photo)

    def track(self, depth, extM_guess, gate=None, gate_thr=None, depth_range=(0., float("inf")), w_min=1., dist_thr=None, huber=None,
              min_frac=0.1, min_pivot=1e-6, image=None, image_affine=None, photo_weight=0.1, photo_huber=0.1):
        """depth [H,W] (or [1,H,W]) CUDA fp32 against the volume seen from extM_guess (host [3,4] or [4,4] world -> camera; the ray
        casts use float32(extM_guess[:3,:4])).  gate / gate_thr and depth_range = (d_near, d_far] as TSDFVolume.integrate takes them;
        w_min: the ray cast's weight threshold; dist_thr: a pair is dropped beyond this distance (default 2 trunc); huber: residuals
        beyond it are down-weighted (default voxel_size) — parameters, not measurements; min_frac: a level needs
        max(6, ceil(min_frac Hs Ws)) pairs; min_pivot: the relative pivot below which the geometry counts as degenerate.
        image (a tracker built with photo=True takes one, another refuses one): the frame's picture, CUDA fp32 [3,H,W] at the depth
        map's size; image_affine = (a [3], b [3]): a pixel's colour is image * a + b per channel, as TSDFVolume.integrate's
        color_affine; photo_weight: the weight of a photometric term beside a geometric one (intensities in [0, 1] against metres);
        photo_huber: intensity residuals beyond it are down-weighted — like dist_thr and huber parameters, not measurements.  With
        an image every level's ray cast also renders the colour and the iterations run ops.icp_terms_photo; without one the
        launches are exactly those of a tracker without photo.  pairs in the log stay the geometric pairs.
        Per level one ray cast and its iterations of two launches each; dT carries over between the levels.  Returns a TrackResult:
        extM = dT^-1 T_g in float64 on the host, T_g the float32-rounded guess promoted — the guess itself when the track was lost.
        Reads the state and the log back at the end: the one place this object synchronises (as TSDFVolume.points does)."""
        from .fusion import _host_matrix
        if (gate is None) != (gate_thr is None):
            raise ValueError("FrameTracker.track: gate and gate_thr come together")
        depth, gate = self._depth(depth, gate)
        image = self._image(image, image_affine, "track")
        g = _host_matrix(extM_guess, "FrameTracker.track")
        Tg = np.eye(4)
        Tg[:3, :4] = g[:3, :4].astype(np.float32).astype(np.float64)
        dist_thr, huber = self._params(dist_thr, huber)
        ops.icp_update(self._state, 0)
        step = 0
        for sub, iters, (Hs, Ws), K, maps in self._levels:
            self.volume.raycast(Tg, K, (Hs, Ws), depth_range=depth_range, w_min=w_min, normals=True, out=maps, color=self.photo)
            min_pairs = max(6, int(math.ceil(min_frac * Hs * Ws)))
            for _ in range(iters):
                step += 1
                nwg = self._terms(depth, sub, maps, K, dist_thr, huber, depth_range, gate, gate_thr, image, image_affine, photo_weight,
                                  photo_huber)
                ops.icp_update(self._state, step, self._partial, nwg, min_pairs=min_pairs, min_pivot=min_pivot, log=self._log)
        host = self._result.cpu().numpy()                           # the single synchronisation
        delta = np.eye(4)
        delta[:3, :4] = host[:12].reshape(3, 4)
        flag = int(host[ops.ICP_STATE_WORDS - 1:ops.ICP_STATE_WORDS].view(np.int32)[0])
        log = host[ops.ICP_STATE_WORDS:].reshape(-1, 4).copy()
        extM = np.linalg.solve(delta, Tg) if flag == 0 else Tg
        return TrackResult(extM, flag, log, delta)

    def residual_map(self, depth, extM, extM_model=None, gate=None, gate_thr=None, depth_range=(0., float("inf")), w_min=1.,
                     dist_thr=None, huber=None, image=None, image_affine=None, photo_weight=0.1, photo_huber=0.1):
        """The point-to-plane residual of every pixel of `depth` seen from extM against the volume ray cast at full size from
        extM_model (default: extM itself, the final pose of a track): [H,W] CUDA fp32, NaN where a pixel has no pair — one more
        icp_terms call (owned buffer: overwritten by the next call).  With image (a photo tracker): the pair (geometric,
        photometric), the second the intensity residual of every pixel with a photometric pair, NaN elsewhere.  Synchronises
        nothing."""
        from .fusion import _host_matrix
        if (gate is None) != (gate_thr is None):
            raise ValueError("FrameTracker.residual_map: gate and gate_thr come together")
        depth, gate = self._depth(depth, gate)
        image = self._image(image, image_affine, "residual_map")
        Tf = np.eye(4)
        Tf[:3, :4] = _host_matrix(extM, "FrameTracker.residual_map")[:3, :4]
        Tm = Tf
        if extM_model is not None:
            Tm = np.eye(4)
            Tm[:3, :4] = _host_matrix(extM_model, "FrameTracker.residual_map")[:3, :4].astype(np.float32).astype(np.float64)
        sub, _, size, K, maps = min(self._levels, key=lambda l: l[0])
        dist_thr, huber = self._params(dist_thr, huber)
        self.volume.raycast(Tm, K, size, depth_range=depth_range, w_min=w_min, normals=True, out=maps, color=self.photo)
        ops.icp_update(self._state, 0, init=Tm @ np.linalg.inv(Tf))
        self._terms(depth, sub, maps, K, dist_thr, huber, depth_range, gate, gate_thr, image, image_affine, photo_weight, photo_huber,
                    resid=self._resid, resid_photo=self._resid_photo)
        return self._resid if image is None else (self._resid, self._resid_photo)
