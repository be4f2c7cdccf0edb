"""Benchmark of the guided-filter refinement net: nrgbd_dgf_refine_f32 (one launch, csrc/dgf.hip) beside the same map made with
torch device operations that follow the reference formula (F.interpolate, two 1 x 1 convolutions, cumsum box filters), at
256 x 384 and 768 x 1024 for n = 1 and 2 targets; and DepthStream frames/s of a DGF model and of the DPV model at config B.

    python tools/bench_dgf.py [--reps 200] [--warmup 20] [--repeats 3] [--json out.json] [--no-trace] [--no-stream]
    python tools/bench_dgf.py --trace-only --size 768x1024 --n 2 --form hip      # 50 calls of one form (what the traces run)

Timing is recorded twice.  HIP events around `reps` back-to-back calls after `warmup` untimed ones: for the one-launch form that
figure is bounded below by the rate at which the host issues the calls, and between back-to-back calls every byte stays in the
last-level cache.  And a kernel trace: unless --no-trace, the tool starts `rocprofv3 --kernel-trace --stats` over a child run of
--trace-only for every (size, n, form) — a process and a run of their own each, under a time limit — and reads the kernels' own
durations and the launch count per call from the trace.  For the hip form only the rows of dgf_refine_kernel are counted: the kernel's
own figures.  For the torch form every kernel of the child process is counted and divided by its 51 calls, so the few setup kernels of
forms() (a fill of H x W, small copies) add about 0.1 launch and a fraction of a microsecond per call to its figures.
A trace child runs in a session of its own; when one exits non-zero or exceeds its time limit, its whole process group is killed and the
tool stops there with a non-zero exit status: nothing further is started on the GPU.  Only a missing rocprofv3 degrades to a note.
Bytes: 12 read and 4 n written per pixel.  No number here is a gate."""
import argparse
import csv
import glob
import json
import os
import shutil
import signal
import subprocess
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
TRACE_CALLS = 50
SIZES = {"256x384": (64, 96, 4), "768x1024": (192, 256, 4)}
FLOPS_PER_X = 64 * 5 * 2 - 64                # 3 fma + max + fma per hidden unit


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


def _box(x):
    """GF/box_filter.py with r = 1: differences of cumsums."""
    c = x.cumsum(dim=2)
    c = torch.cat([c[:, :, 1:3], c[:, :, 3:] - c[:, :, :-3], c[:, :, -1:] - c[:, :, -3:-2]], dim=2).cumsum(dim=3)
    return torch.cat([c[:, :, :, 1:3], c[:, :, :, 3:] - c[:, :, :, :-3], c[:, :, :, -1:] - c[:, :, :, -3:-2]], dim=3)


def make_inputs(h, w, s, seed):
    """(depth [2,h,w] in [0.1, 5] m, noise image [3,sh,sw], w1, b1, w2, b2 at RefineNet_DGF's initialiser), fp32 numpy."""
    rng = np.random.RandomState(seed)
    depth = (0.1 + 4.9 * rng.rand(2, h, w)).astype(np.float32)
    img = rng.randn(3, s * h, s * w).astype(np.float32)
    w1, w2 = (rng.randn(64, 3) * np.sqrt(2.0 / 64)).astype(np.float32), (rng.randn(64) * np.sqrt(2.0)).astype(np.float32)
    b1, b2 = (rng.uniform(-1, 1, 64) / np.sqrt(3.0)).astype(np.float32), (rng.uniform(-1, 1, 1) / 8.0).astype(np.float32)
    return depth, img, w1, b1, w2, b2


def forms(size, n):
    from neuralrgbd_amd import ops
    h, w, s = SIZES[size]
    depth, img, w1, b1, w2, b2 = (torch.from_numpy(a).to(DEV) for a in make_inputs(h, w, s, 7))
    depth = depth[:n].contiguous()
    out = torch.empty((n, 1, s * h, s * w), device=DEV)
    cw1, cw2 = w1.reshape(64, 3, 1, 1), w2.reshape(1, 64, 1, 1)
    ones = torch.ones((1, 1, s * h, s * w), device=DEV)

    def torch_form():
        """Refine.py:637-639 and guided_filter.py:76-97 with library operations on the device."""
        y = F.interpolate(depth[:, None], scale_factor=s, mode="bilinear", align_corners=True)
        x = F.conv2d(torch.relu(F.conv2d(img[None], cw1, b1)), cw2, b2)
        N = _box(ones)
        mx, my = _box(x) / N, _box(y) / N
        cov = _box(x * y) / N - mx * my
        var = _box(x * x) / N - mx * mx
        A = cov / (var + 1e-8)
        b = my - A * mx
        return _box(A) / N * x + _box(b) / N

    return {"hip": lambda: ops.dgf_refine(depth, img, w1, b1, w2, b2, 1e-8, out=out), "torch": torch_form}


class TraceFailed(RuntimeError):
    """A GPU child run exited non-zero or exceeded its time limit: the tool starts nothing further."""


def trace(size, n, form, timeout_s=240):
    """{kernel microseconds, launches} per call from a rocprofv3 kernel trace of a child run of --trace-only (the hip form: the rows of
    dgf_refine_kernel alone; the torch form: every kernel of the child), or a string when rocprofv3 is not installed.  The child runs
    in a session of its own; a non-zero exit or the time limit kills its process group and raises TraceFailed."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return "rocprofv3 not found"
    what = "trace of %s n=%d %s" % (size, n, form)
    tmp = tempfile.mkdtemp(prefix="bench_dgf_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--trace-only", "--size", size, "--n", str(n), "--form", form]
        child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
        try:
            _, err = child.communicate(timeout=timeout_s)
        except subprocess.TimeoutExpired:
            try:
                os.killpg(child.pid, signal.SIGKILL)             # rocprofv3 AND the traced python: nothing keeps the GPU open
            except ProcessLookupError:
                pass
            child.communicate()
            raise TraceFailed("%s exceeded %d s: its process group was killed" % (what, timeout_s))
        if child.returncode != 0:
            raise TraceFailed("%s exited with status %d: %s" % (what, child.returncode, err[-300:]))
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise TraceFailed("%s: no kernel_stats.csv in the trace output" % what)
        us = calls = 0.0
        top = []
        with open(found[0]) as fh:
            for row in csv.DictReader(fh):
                if form == "hip" and "dgf_refine_kernel" not in row["Name"]:
                    continue
                us += float(row["TotalDurationNs"]) / 1e3
                calls += float(row["Calls"])
                top.append((float(row["TotalDurationNs"]) / 1e3 / (TRACE_CALLS + 1), row["Name"][:80]))
        return {"kernel_us_per_call": us / (TRACE_CALLS + 1), "launches_per_call": calls / (TRACE_CALLS + 1),
                "top": sorted(top, reverse=True)[:3]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def stream_fps(refine, frames=20, warm=5):
    """DepthStream (hipGraph, sequential) frames/s at config B (image 768 x 1024, D = 64, 5-frame window) of a DGF or DPV model."""
    import neuralrgbd_amd
    from neuralrgbd_amd import camera, synth
    from neuralrgbd_amd.streaming import DepthStream
    H, W, D = 768, 1024, 64
    cam = camera.scannet_intrinsics(W // 4, H // 4)
    d_candi = np.linspace(0.1, 5.0, D)
    model = neuralrgbd_amd.KVNET(64, cam, d_candi, 10.0, 64, None, if_refined=True, refineNet_name=refine, t_win_r=2)
    model.load_state_dict(synth.seeded_state_dict(model, 0))
    model = model.to(DEV)
    wins = [tuple(t.to(DEV) for t in synth.noise_window(40 + i, H, W)) for i in range(3)]
    ds = DepthStream(model, cam, d_candi, t_win_r=2, use_graph=True)
    for i in range(warm):
        ds.step(*wins[i % 3])
    assert ds._graph is not None, ds.graph_error
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(frames):
        ds.step(*wins[i % 3])
    e1.record()
    torch.cuda.synchronize()
    ds.check()
    return frames / (e0.elapsed_time(e1) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-stream", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--size", choices=sorted(SIZES), default="768x1024")
    ap.add_argument("--n", type=int, choices=(1, 2), default=2)
    ap.add_argument("--form", choices=("hip", "torch"), default="hip")
    a = ap.parse_args()
    if a.trace_only:
        fn = forms(a.size, a.n)[a.form]
        for _ in range(TRACE_CALLS + 1):
            fn()
        torch.cuda.synchronize()
        return 0
    from neuralrgbd_amd import ops
    out = {"version": ops.version(), "tile": list(ops.DGF_TILE)}
    for size in sorted(SIZES):
        h, w, s = SIZES[size]
        pixels = s * h * s * w
        for n in (1, 2):
            fs = forms(size, n)
            diff = float((fs["hip"]().double() - fs["torch"]().double()).abs().max())
            res = {"pixels": pixels, "n": n, "bytes": (12 + 4 * n) * pixels, "max_abs_hip_minus_torch_form": diff}
            for form, fn in fs.items():
                t = [time_ms(fn, a.reps if form == "hip" else max(a.reps // 10, 5), a.warmup if form == "hip" else 3) for _ in range(a.repeats)]
                res[form] = {"events_ms_per_call": t, "median_ms": float(np.median(t)), "spread_ms": max(t) - min(t)}
                if not a.no_trace:
                    res[form]["trace"] = trace(size, n, form)
                tr = res[form].get("trace")
                print("%-9s n=%d %-6s HIP events %.4f ms per call (spread %.4f)%s" % (
                    size, n, form, res[form]["median_ms"], res[form]["spread_ms"],
                    "" if tr is None else ("; trace: %s" % tr if isinstance(tr, str) else
                                           "; trace: %.2f us of kernels in %.1f launches per call" % (tr["kernel_us_per_call"], tr["launches_per_call"]))))
            tr = res["hip"].get("trace")
            if isinstance(tr, dict):
                sec = tr["kernel_us_per_call"] * 1e-6
                halo = (ops.DGF_TILE[0] + 4) * (ops.DGF_TILE[1] + 4) / float(ops.DGF_TILE[0] * ops.DGF_TILE[1])
                res["hip"]["gb_per_s"] = res["bytes"] / sec / 1e9
                res["hip"]["network_tflops"] = FLOPS_PER_X * halo * pixels / sec / 1e12
                print("          kernel: %.1f GB/s of compulsory traffic, %.2f Tflop/s in the guide network alone" % (
                    res["hip"]["gb_per_s"], res["hip"]["network_tflops"]))
            print("          max |hip - torch form| %.3e m (the torch form is the reference's cancelling fp32 arithmetic)" % diff)
            out["%s_n%d" % (size, n)] = res
    if not a.no_stream:
        out["stream_config_B_frames_per_s"] = {name: stream_fps(name) for name in ("DGF", "DPV")}
        print("DepthStream at config B: DGF model %.2f frames/s, DPV model %.2f frames/s" % (
            out["stream_config_B_frames_per_s"]["DGF"], out["stream_config_B_frames_per_s"]["DPV"]))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    try:
        sys.exit(main())
    except TraceFailed as e:
        print("bench_dgf: %s; stopping, nothing further is started on the GPU" % e, file=sys.stderr)
        sys.exit(1)
