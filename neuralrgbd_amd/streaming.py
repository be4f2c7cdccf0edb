"""Streaming depth filter: one object per video stream, DPV state resident on the GPU.

The reference's driver loop (test_KVNet.py:190-250) calls `test()` once per frame: ~600 kernel launches from
Python, one device->host probe (`valid_dpv`), a host-built point grid and its H2D copy.  `DepthStream` keeps the
same per-frame semantics (KVNET.forward + PREDICT, i.e. exactly `neuralrgbd_amd.test_step.test`) but

  * keeps BV_predict and the validity flag on its own side (no device->host read in the steady state),
  * captures the whole update-branch frame into ONE hipGraph (torch.cuda.CUDAGraph) after a warm-up frame, and
    replays it per frame: every kernel of libnrgbd_hip.so is capture-safe (no allocation, no host sync, no
    algorithm search — there is no vendor convolution on the path).  A capture that fails RAISES unless the stream
    was built with allow_eager_fallback=True (then it stays eager, on every slot, and `graph_error` says why).
  * reads the path's status word (BatchNorm variance collapse, nets.check_status) without stalling: every step
    queues a 4-byte copy to pinned host memory behind the frame and inspects the PREVIOUS step's copy.

  * optionally PIPELINES the two halves of consecutive frames of the one video (pipeline=True): the D-Net of frame t + 1
    (feature CNN, texel pack, fused warp + cost volume: KVNET.measure — nothing in it depends on the filter state) runs on
    a second HIP stream while the K-Net / DPV update / R-Net / PREDICT of frame t run on the first.
    Every frame is computed in full by the same kernels on the same inputs, so the outputs are the sequential ones bit for
    bit (tests/test_gpu_fullsize.py); step() then returns the result of the PREVIOUS call's frame (one frame of latency)
    and flush() the last one.  What it buys is the idle tail of every launch: +5 % frames/s at config B.

One frame body (`_frame`), one kind of static memory (`_Slot`: one for the sequential graph, two for the pipelined halves) and
one capture (`_capture`, all graphs or none) serve both forms.  The co-resident form of the K-Net's residual passes is an
argument of the captured back half (`KVNET.forward(knet_lean_passes=)`), nothing is set on the model.

Config 5 of BASELINE.json (a 300-frame high-resolution stream) is this object in a loop.
"""
import math
import weakref

import torch

from . import homography as warp_homo
from . import nets
from . import ops
from .distributed import graph_capture_mode


_PIPELINED = weakref.WeakSet()      # the live DepthStream(pipeline=True) objects: a stream counts its neighbours when it captures


def _gpu_index(device):
    d = torch.device(device)
    return d.index if d.index is not None else torch.cuda.current_device()


class _Slot:
    """The static memory of one frame in flight: its inputs, its D-Net record (pipeline=True), its outputs and the hipGraphs that
    read and write them.  Sequential stream: one slot, `gb` is the whole frame.  Pipelined: two slots, front `gf` and back `gb`."""

    def __init__(self, *inputs):
        self.ref, self.src, self.poses, self.pose_next = (torch.empty_like(t) for t in inputs)
        self.rec = self.out = self.gf = self.gb = None
        self.consts = None                      # K / rays / d_candi the graphs read: kept alive with them
        self.ev_front = torch.cuda.Event()      # the record is complete

    def load(self, *inputs):
        for dst, t in zip((self.ref, self.src, self.poses, self.pose_next), inputs):
            dst.copy_(t)


class DepthStream:
    # pipeline=True: workgroups per CU of the K-Net residual passes in the captured back half (ops.nhwc_act_lean; 0 = the plain pass).
    # Used only by a stream that is the one pipelined stream of its device when it captures: beside further videos a pass can land next
    # to another video's K-Net convolution or run alone, where the plain pass is the faster one
    lean_passes = 1

    def __init__(self, model, cam_intrinsics, d_candi, t_win_r=2, use_graph=True, device=None, copy_outputs=False,
                 allow_eager_fallback=False, pipeline=False):
        self.model = model
        self.cam = cam_intrinsics
        self.d_candi = d_candi
        self.t_win_r = t_win_r
        self.use_graph = use_graph
        # Once the hipGraph is active, step() hands out the graph's STATIC output buffers: the next step() overwrites them
        # in place, so a caller that keeps per-frame results (a list for export / evaluation) must either pass
        # copy_outputs=True (clones: +0.2 GB/s of HBM traffic at config B) or clone what it keeps.  The eager path
        # returns fresh tensors either way.
        self.copy_outputs = copy_outputs
        self.device = device if device is not None else next(model.parameters()).device
        self.bv_predict = None          # [1,D,h,w] log-DPV predicted for the next frame, or None (fresh stream)
        self._eager_updates = 0
        self.graph_error = None
        self.allow_eager_fallback = allow_eager_fallback
        self._status_host = None        # pinned int32: the status word as of the previous step
        self._status_event = None
        # pipeline=True: two slots, the one whose frame has been measured but not filtered yet, the second HIP stream
        self.pipeline = bool(pipeline)
        if self.pipeline:
            _PIPELINED.add(self)
        self._slots = None
        self._pending = None
        self._side = None

    @property
    def _graph(self):
        """Not None: the graphs are active.  _capture leaves a graph on every slot or on none, so the first one answers."""
        return self._slots[0].gb if self._slots else None

    def reset(self):
        """Invalid pose / new trajectory: drop the filter state (test_KVNet.py:241-246); a pending pipelined frame is dropped too.
        Its front half may still run on the side stream: the caller's stream waits for it (an event, no host sync), so that the next
        first window's D-Net and the next copies into the slot come after it."""
        if self._pending is not None:
            torch.cuda.current_stream(self.device).wait_event(self._pending.ev_front)
        self.bv_predict = None
        self._pending = None

    # ------------------------------------------------------------------ one frame, in one piece or in two halves
    def _frame(self, ref, src, poses, pose_next, bv, measured=None, lean=None):
        """KVNET.forward + PREDICT -> (refined, DPV, the state predicted for the next frame).  bv None: the first window of a stream
        (D-Net only).  measured: the window's D-Net record (_front), None = measure here.  lean: KVNET.forward(knet_lean_passes=)."""
        with torch.no_grad():
            # test_KVNet.py:50 `.inverse()` as a path kernel (fixed operation order, capture-safe): inside the hipGraph
            pose_next_inv = ops.pose_inverse(pose_next)
            r_cur, r_kv, bv_cur, dpv = self.model(ref, src, poses, torch.zeros(1), cam_intrinsics=[self.cam], BV_predict=bv,
                                                  dpv_valid=bv is not None, measured=measured, knet_lean_passes=lean)
            pad = math.log(1. / float(len(self.d_candi)))
            nxt = warp_homo.resample_vol_cuda(src_vol=dpv, rel_extM=pose_next_inv, cam_intrinsic=self.cam,
                                              d_candi=self.d_candi, padding_value=pad, clamp=(-1000., 0.)).unsqueeze(0)
        return r_kv, dpv, nxt

    def _front(self, sl):
        with torch.no_grad():
            sl.rec = self.model.measure(sl.ref, sl.src, sl.poses)

    def _back(self, sl, lean=None):
        sl.out = self._frame(sl.ref, sl.src, sl.poses, sl.pose_next, self._bv, sl.rec, lean)

    def _finish(self, sl, copy):
        """The slot's frame from its record (or, sequential slot, from its inputs) to the outputs on the caller's stream: replayed
        or, on the pipelined stream's warm-up frames, eager — counted in _eager_updates from step() and from flush() alike."""
        main = torch.cuda.current_stream(self.device)
        if self.pipeline:                       # the record comes from the side stream
            main.wait_event(sl.ev_front)
        self._bv.copy_(self.bv_predict)
        if sl.gb is not None:
            sl.gb.replay()
        else:
            self._back(sl)
            self._eager_updates += 1
        r, dpv, self.bv_predict = sl.out        # static with a graph: copied into _bv by the next call
        if self.pipeline:
            self._ev_back.record(main)
        return (r.clone(), dpv.clone()) if copy else (r, dpv)

    # ------------------------------------------------------------------ static memory and its graphs
    def _setup(self, *inputs):
        self._slots = [_Slot(*inputs) for _ in range(2 if self.pipeline else 1)]
        self._bv = torch.empty_like(self.bv_predict)            # the filter state every graph of the stream reads
        if self.pipeline:
            self._side = torch.cuda.Stream(self.device)
            self._ev_back = torch.cuda.Event()                  # the last back half is on the caller's stream

    def _record(self, fn):
        """One hipGraph of fn().  capture_error_mode: see distributed.graph_capture_mode."""
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode=graph_capture_mode()):
            fn()
        return g

    def _capture(self, *inputs):
        """Every hipGraph of the stream, or none.  Sequential: the whole frame of the one slot.  Pipelined: both halves of both slots
        (a slot's record lives in its front graph's pool and is read by its back graph: static buffers on both sides); the back half
        is replayed beside the next frame's front half, so its K-Net residual passes are captured in their co-resident form
        (lean_passes), only without further pipelined videos on the device.  Needs every cache warm: called after eager frames.
        A failure clears every slot's graphs and sets graph_error; it is re-raised unless allow_eager_fallback."""
        pend, rec = self._pending, self._pending and self._pending.rec
        try:
            lean = None
            if self.pipeline:
                if not isinstance(getattr(self.model, "kv_net", None), nets.KalmanGainNet):
                    raise RuntimeError("DepthStream(pipeline=True): the model has no nets.KalmanGainNet to capture a back half of")
                alone = not any(s is not self and _gpu_index(s.device) == _gpu_index(self.device) for s in _PIPELINED)
                lean = self.lean_passes if alone else 0
            if self._slots is None:
                self._setup(*inputs)
            torch.cuda.synchronize(self.device)
            for sl in self._slots:
                if self.pipeline:
                    sl.gf = self._record(lambda: self._front(sl))
                sl.gb = self._record(lambda: self._back(sl, lean))
                sl.consts = warp_homo.cache_snapshot()
            if pend is not None:
                # capture does not execute: the pending frame's record, produced eagerly, is rebuilt in its slot's static buffers
                main = torch.cuda.current_stream(self.device)
                main.wait_event(self._ev_back)
                pend.gf.replay()
                pend.ev_front.record(main)
        except Exception as e:
            for sl in self._slots or ():
                sl.gf = sl.gb = None
            if pend is not None:
                pend.rec = rec              # the eager record again, not static memory that no kernel has written
            self.graph_error = repr(e)
            if not self.allow_eager_fallback:      # a library user must not silently run at eager speed
                raise
            print("[DepthStream] hipGraph capture failed, staying eager: %s" % self.graph_error)

    def _step_pipelined(self, *inputs):
        """front(t) on the side stream, back(t - 1) on the caller's stream; returns the outputs of frame t - 1 (None on the first
        pipelined call, whose predecessor was handled by the sequential path)."""
        main = torch.cuda.current_stream(self.device)
        if self._slots is None:
            self._setup(*inputs)
        sl = self._slots[1 if self._pending is self._slots[0] else 0]       # the free slot
        # frame t's inputs -> its slot (on the caller's stream, after the back half that last read this slot: same stream), then the
        # front half on the side stream
        sl.load(*inputs)
        if sl.gf is not None:
            ev_in = torch.cuda.Event()
            ev_in.record(main)
            with torch.cuda.stream(self._side):
                self._side.wait_event(ev_in)
                sl.gf.replay()
                sl.ev_front.record(self._side)
        else:
            # eager warm-up frames: both halves on the caller's stream, in order (tensors allocated under one stream and read under
            # another would need record_stream bookkeeping; only the graphs — static buffers — overlap)
            self._front(sl)
            sl.ev_front.record(main)
        out = self._finish(self._pending, self.copy_outputs) if self._pending is not None else None
        self._pending = sl
        return out

    def flush(self):
        """pipeline=True: run the back half of the frame that is still owed and return its outputs (None if nothing is pending).
        The outputs and the state left in bv_predict are clones."""
        if self._pending is None:
            return None
        out = self._finish(self._pending, True)
        self.bv_predict = self.bv_predict.clone()
        self._pending = None
        return out

    def _probe_status(self):
        """Deferred, stall-free read of the status word: raise on what the PREVIOUS step's copy shows, queue this step's copy."""
        if self._status_event is not None and self._status_event.query() and int(self._status_host[0]) != 0:
            nets.check_status(self.device)          # reads, clears and raises
        word = nets.status_word(self.device)
        if self._status_host is None:
            self._status_host = torch.zeros(1, dtype=torch.int32).pin_memory()
            self._status_event = torch.cuda.Event()
        self._status_stage = word.clone()           # a device-side copy first (see nets.check_status: no memcpy from the word itself)
        self._status_host.copy_(self._status_stage, non_blocking=True)
        self._status_event.record(torch.cuda.current_stream(self.device))

    def check(self):
        """Synchronous form of the status probe (end of a sequence): raises NrgbdError on a reported variance collapse."""
        nets.check_status(self.device)

    # ------------------------------------------------------------------ public step
    def step(self, ref_frame, src_frames, src_cam_poses, cam_pose_next=None):
        """ref_frame [1,3,H,W], src_frames [1,V,3,H,W], src_cam_poses [1,V,4,4] (device tensors).
        Returns (refined DPV [1,D,H,W] — [1,4D,H,W] from a model with if_upsample_d —, DPV [1,D,h,w]); the predicted state for the next frame is kept inside.
        pipeline=True: the pair belongs to the PREVIOUS call's frame (None when there is none yet); flush() returns the last one.
        With the hipGraph active and copy_outputs=False the returned tensors are only valid until the next step()."""
        pose = src_cam_poses[0, self.t_win_r] if cam_pose_next is None else cam_pose_next
        # the pose of the next reference frame, NOT inverted: the inversion happens inside the frame (nrgbd_pose_inverse); a host
        # tensor is accepted as before
        inputs = (ref_frame, src_frames, src_cam_poses, pose.to(device=self.device, dtype=torch.float32).contiguous())
        if self.bv_predict is None:                      # first window of the stream: D-Net only
            r, dpv, self.bv_predict = self._frame(*inputs, None)
            out = r, dpv
        else:
            # warm-up: one eager update before the sequential capture; two, and a frame pending, before the pipelined one
            if (self.use_graph and self._graph is None and self.graph_error is None
                    and (self._eager_updates >= 2 and self._pending is not None if self.pipeline else self._eager_updates >= 1)):
                self._capture(*inputs)
            if self.pipeline:
                out = self._step_pipelined(*inputs)
            elif self._graph is not None:
                self._slots[0].load(*inputs)
                out = self._finish(self._slots[0], self.copy_outputs)       # valid until the next step() (see copy_outputs)
            else:
                r, dpv, self.bv_predict = self._frame(*inputs, self.bv_predict)
                self._eager_updates += 1
                out = r, dpv
        self._probe_status()
        return out
