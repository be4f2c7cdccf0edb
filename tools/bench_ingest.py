"""Frame-ingest benchmark: what VideoDepthStream.push does in front of the frame — upload of one uint8 camera frame, nrgbd_frame_ingest_u8
into the ring, nrgbd_window_gather of the 5-frame window — beside the same work as torch operations on the device (nearest index,
permute, float().div(255).sub(mean).div(std), torch.stack of the window), at config B's image size: 1024 x 768 from a 1296 x 968 frame.

    python tools/bench_ingest.py [--reps 200] [--warmup 20] [--repeats 3] [--json out.json]
    python tools/bench_ingest.py --trace-only         # a few calls of each form for `rocprofv3 --kernel-trace --stats -- python ...`

Timing: HIP events around `reps` back-to-back calls after `warmup` untimed ones, per call; `repeats` such measurements give the
run-to-run spread.  These kernels take microseconds: the per-call figure is bounded below by the rate at which the host issues the
calls, so the kernels' own durations come from the kernel trace (--trace-only), and the window's 94 MB stay in the 256 MB last-level
cache between back-to-back calls: the gather's rate is a cache figure, not an HBM one.  `push` is VideoDepthStream.push with DepthStream.step stubbed out (the frame itself is bench.py's business), from
a host frame (pinned staging + upload) and from a frame already on the device.  Bytes: the ingest must read the camera frame once
(3 Hin Win) and write 12 Hout Wout; the gather reads and writes 5 x 12 Hout Wout each."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralrgbd_amd import ops, video  # noqa: E402

DEV = "cuda:0"
HBM_TBS = 8.0
HIN, WIN, HOUT, WOUT, R_WIN = 968, 1296, 768, 1024, 2


class _NoFrame:
    """DepthStream without the frame: push() is timed up to the call of step()."""
    def __init__(self, *a, **k):
        self.bv_predict = None

    def reset(self):
        pass

    def step(self, ref, src, poses):
        return ref, src

    def flush(self):
        return None


def time_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    host = rng.randint(0, 256, (HIN, WIN, 3)).astype(np.uint8)
    dev = torch.from_numpy(host).to(DEV)
    R = 2 * R_WIN + 1
    ring = torch.randn(R, 3, HOUT, WOUT, device=DEV)
    src, ref = torch.empty(1, R - 1, 3, HOUT, WOUT, device=DEV), torch.empty(1, 3, HOUT, WOUT, device=DEV)
    slots = video.window_slots(R + 2, R_WIN)
    slots = slots[0] + [slots[1]]
    mean, std = video.IMAGENET_MEAN, video.IMAGENET_STD
    sy = torch.from_numpy(((2 * np.arange(HOUT) + 1) * HIN) // (2 * HOUT)).to(DEV)
    sx = torch.from_numpy(((2 * np.arange(WOUT) + 1) * WIN) // (2 * WOUT)).to(DEV)
    m, s = torch.tensor(mean, device=DEV)[:, None, None], torch.tensor(std, device=DEV)[:, None, None]

    def torch_ingest():
        ring[1].copy_(dev[sy][:, sx].permute(2, 0, 1).float().div(255).sub(m).div(s))

    def torch_gather():
        src[0].copy_(torch.stack([ring[i] for i in slots[:-1]]))
        ref[0].copy_(ring[slots[-1]])

    real = video.DepthStream
    video.DepthStream = _NoFrame
    try:
        vs = video.VideoDepthStream(None, None, None, t_win_r=R_WIN, net_size=(HOUT, WOUT), device=DEV)
    finally:
        video.DepthStream = real
    E = np.eye(4)
    forms = {
        "hip_ingest": lambda: ops.frame_ingest(dev, ring[1], mean, std),
        "torch_ingest": torch_ingest,
        "hip_gather": lambda: ops.window_gather(ring, slots, src, ref),
        "torch_gather": torch_gather,
        "push_device_frame": lambda: vs.push(dev, E),
        "push_host_frame": lambda: vs.push(host, E),
    }
    ingest_bytes = 3 * HIN * WIN + 12 * HOUT * WOUT
    gather_bytes = 2 * R * 12 * HOUT * WOUT
    bytes_of = {"hip_ingest": ingest_bytes, "torch_ingest": ingest_bytes, "hip_gather": gather_bytes, "torch_gather": gather_bytes,
                "push_device_frame": ingest_bytes + gather_bytes, "push_host_frame": ingest_bytes + gather_bytes + 2 * 3 * HIN * WIN}
    want = ((torch.from_numpy(host)[sy.cpu()][:, sx.cpu()].permute(2, 0, 1).float().div(255)
             - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None])
    if a.trace_only:
        for _ in range(20):
            for fn in forms.values():
                fn()
        torch.cuda.synchronize()
        return 0
    forms["hip_ingest"]()
    same = torch.equal(ring[1].cpu(), want)
    out = {"version": ops.version(), "frame": [HIN, WIN], "net": [HOUT, WOUT], "t_win_r": R_WIN, "hip_ingest_equals_torch_cpu": same}
    for name, fn in forms.items():
        t = [time_ms(fn, a.reps, a.warmup) for _ in range(a.repeats)]
        med = float(np.median(t))
        out[name] = {"ms": t, "median_ms": med, "spread_ms": max(t) - min(t), "bytes": bytes_of[name],
                     "hbm_fraction": bytes_of[name] / (med * 1e-3) / (HBM_TBS * 1e12)}
        print("%-18s %.4f ms (spread %.4f)  %6.1f MB  = %.3f of %g TB/s" % (name, med, max(t) - min(t), bytes_of[name] / 1e6,
                                                                            out[name]["hbm_fraction"], HBM_TBS))
    print("hip ingest equals the torch-CPU formula bit for bit: %s" % same)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
