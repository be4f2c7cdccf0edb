#!/usr/bin/env python
"""bench.py — depth frames/s of the plane-sweep path on MI355X + roofline of the fused warp kernel.

    python bench.py --gpus N --steps K --warmup W            (N=1)
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One *step* = one depth frame of one video stream = one call of the reference's
test_utils/test_KVNet.py::test in the update branch: KVNET.forward with a valid BV_predict (D-Net,
K-Net, DPV update, both R-Net calls) + the PREDICT resample.  Inputs are synthetic windows that are
resident in HBM before the timed region; weights are seeded random (no checkpoints offline).
Each rank streams its own independent video (replicas, no data-path collective) => weak scaling,
value = all ranks' frames / max-over-ranks time.

Workload (BASELINE.json configs[1]): plane-sweep grid 256x192 (image
1024x768), 64 depth candidates, 5-frame window (1 reference + 4 sources), fp32.

A plain run sets up, warms up, times exactly --steps steps and prints the headline line (metric, value in frames/s,
ms_per_step, ...).  `--dump-outputs DIR` then also writes what the last timed step returned to its caller (refined DPV and
DPV of every stream of rank 0; float32 .npy, at most 64 MB: see dump_outputs) — inputs and weights are seeded, so two builds can be
compared output for output.  `--full` adds everything else below, each taking runs of its own after the timed steps.

With --full the JSON line also carries
  roofline      HBM roofline of the dominant sampling kernel (fused warp + cost volume + log-softmax):
                algorithmic bytes 4[(V+1)*67*hw + D*hw] per launch / its mean launch duration, measured
                with HIP events on the launch stream inside the timed steps (peak 8.0 TB/s);
                `traffic` = HBM-side bytes per launch from a committed rocprofv3 --pmc measurement of this bench's
                own windows (tools/pmc_traffic.sh -> profiles/r6_costvol_traffic.json), reported only while the kernel's
                sources still hash to what the measurement recorded;
  cpu_baseline  the CPU oracle (oracle/kvnet_oracle.py: the reference algorithm restated on torch-CPU
                + the C sampling oracle) timed on this node's host cores on update frames of the same
                workload: 1 warm-up + median of 2 (rank 0, N=1 only);
  parity        the GPU frame vs that oracle frame on the same window and filter state: max / mean |d| and
                arg-max depth-index mismatches of BV_cur, DPV, BV_predict and the refined DPV;
  config.sequential_frames_per_s  the same stream without the pipelining of consecutive frames;
  other_configs short child runs of configs S / K / H and of the training step (config B, N = 1).
`--mode train` prints a separate, labelled line for the training iteration at BASELINE config 4's shape (with --full: the
K-Net layer's roofline, the all-reduce alone at N > 1 and the CPU baseline).
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # before the first HIP call: see neuralrgbd_amd/__init__.py (hipGraph replay hazard)

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CONFIGS = {
    "S": dict(H=256, W=384, D=64, d_min=0.1, d_max=5.0, name="ScanNet demo 384x256 image, grid 96x64x64"),
    "B": dict(H=768, W=1024, D=64, d_min=0.1, d_max=5.0, name="plane-sweep grid 256x192x64cand (image 1024x768)"),
    "K": dict(H=256, W=768, D=64, d_min=1.0, d_max=60.0, name="KITTI 768x256 image, grid 192x64x64"),
    "H": dict(H=480, W=640, D=128, d_min=0.1, d_max=5.0, name="480x640 image, grid 160x120x128"),
}
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: dense fp32 matrix peak (256 CUs x 256 FLOP/clk x 2.4 GHz)
# HBM-side bytes per launch of the fused sampling kernel from the L2's fabric counters.  Counters cannot be read from inside
# this process, so they come from a committed measurement of THIS bench's own windows: tools/pmc_traffic.sh runs
# `bench.py --no-graph` under rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes) and writes the per-launch mean of
# the costvol kernel's dispatches to profiles/r2_costvol_traffic.json (FETCH_SIZE doubled as MI355X_MICROARCH.md §HBM
# prescribes for gfx950).  Configs without an entry report null.
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "r6_costvol_traffic.json")
COSTVOL_SOURCES = ("costvol_quad.hip", "costvol.hip", "costvol.hpp", "common.hpp")   # what the measured kernel is built from


def costvol_source_hash():
    """sha256 over the sources of the fused sampling kernel: the committed PMC measurement records it (tools/
    pmc_traffic_json.py) and is only valid for the kernel it was taken on."""
    import hashlib
    h = hashlib.sha256()
    for name in COSTVOL_SOURCES:
        with open(os.path.join(ROOT, "neuralrgbd_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def pmc_traffic(cfg):
    """(bytes per launch | None, note).  A measurement taken on other kernel sources is REFUSED (None), not reported."""
    try:
        with open(TRAFFIC_FILE) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        return None, "no committed measurement"
    rec = doc.get(cfg)
    if not rec:
        return None, "no committed measurement for this config"
    if doc.get("kernel_source_sha16") != costvol_source_hash():
        return None, "refused: %s was measured on kernel sources %s, the tree has %s — re-run tools/pmc_traffic.sh" % (
            os.path.basename(TRAFFIC_FILE), doc.get("kernel_source_sha16"), costvol_source_hash())
    return rec.get("traffic_bytes"), "rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE per launch on this bench's windows (tools/pmc_traffic.sh -> profiles/%s, kernel sources %s)" % (os.path.basename(TRAFFIC_FILE), doc.get("kernel_source_sha16"))


SQ_PASS = ("SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_LDS_IDX_ACTIVE", "SQ_LDS_BANK_CONFLICT", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY",
           "SQ_BUSY_CYCLES", "GRBM_GUI_ACTIVE")      # 7 SQ slots (of 8) + 1 GRBM slot: one pass


def live_pmc_traffic(cfg, timeout_s=240):
    """Counters of the fused sampling kernel MEASURED IN THIS RUN: this script is re-run as a child under rocprofv3 --pmc —
    FETCH_SIZE, WRITE_SIZE and the SQ set above in three separate passes, no trace domain beside them (MI355X_MICROARCH.md,
    HBM / PMC sections) — with eager launches on the same windows (3 frames); the per-dispatch counters of the sampling kernel
    are averaged, FETCH_SIZE is doubled as the guide prescribes for gfx950.
    Returns (HBM-side bytes per launch | None, note, sq | None): sq = per-launch means of SQ_PASS.  None when rocprofv3 is not
    there / fails / times out — the caller then falls back to the committed measurement (pmc_traffic)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found", None
    if "HSA_TOOLS_LIB" in os.environ or any(k.startswith(("ROCP_", "ROCPROFILER_")) for k in os.environ):
        return None, "this process is itself running under a profiler", None     # no nested rocprofv3
    vals = {}
    root = tempfile.mkdtemp(prefix="nrgbd_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    try:
        for tag, counters in (("FETCH_SIZE", ("FETCH_SIZE",)), ("WRITE_SIZE", ("WRITE_SIZE",)), ("SQ", SQ_PASS)):
            out = os.path.join(root, tag)
            cmd = [exe, "--pmc"] + list(counters) + ["--output-format", "csv", "-d", out, "-o", "p", "--", sys.executable,
                   os.path.abspath(__file__), "--config", cfg, "--steps", "2", "--warmup", "1", "--no-graph", "--full", "--no-cpu-baseline",
                   "--no-live-traffic"]
            try:
                subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s, check=True)
            except (OSError, subprocess.SubprocessError) as e:
                if tag == "SQ":
                    break                       # the traffic stands without the SQ pass
                return None, "rocprofv3 --pmc %s failed (%s)" % (tag, type(e).__name__), None
            got = {c: [] for c in counters}
            for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
                with open(f) as fh:
                    for row in csv.DictReader(fh):
                        if "costvol_quad" in row["Kernel_Name"] and row["Counter_Name"] in got:
                            got[row["Counter_Name"]].append(float(row["Counter_Value"]))
            if tag != "SQ" and not got[tag]:
                return None, "no %s rows for the sampling kernel in the rocprofv3 output" % tag, None
            for c in counters:
                if got[c]:
                    vals[c] = (sum(got[c]) / len(got[c]), len(got[c]))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    f, w = vals["FETCH_SIZE"], vals["WRITE_SIZE"]
    sq = {c: vals[c][0] for c in SQ_PASS if c in vals} or None
    return int(2 * f[0] * 1024 + w[0] * 1024), ("measured in this run: rocprofv3 --pmc FETCH_SIZE (x2, gfx950) + WRITE_SIZE in two child passes of this "
                                                "script (eager launches, same windows), mean over %d / %d dispatches of the sampling kernel; "
                                                "FETCH_SIZE %.0f KB, WRITE_SIZE %.0f KB" % (f[1], w[1], f[0], w[0])), sq


def sq_fractions(sq, n_cu=256):
    """VALU / LDS utilisation of a kernel from its SQ counters (MI355X_MICROARCH.md, PMC and cycle-constant sections):
    GRBM_GUI_ACTIVE sums the 8 XCDs' busy cycles -> kernel cycles = / 8; SQ_ACTIVE_INST_VALU counts quad-cycles (x4) of VALU
    issue summed over all SIMDs (4 per CU); SQ_LDS_IDX_ACTIVE counts LDS-array cycles summed over the CUs."""
    if not sq or not sq.get("GRBM_GUI_ACTIVE"):
        return {}
    cyc = sq["GRBM_GUI_ACTIVE"] / 8.0
    out = {"kernel_cycles": cyc}
    if "SQ_ACTIVE_INST_VALU" in sq:
        out["valu_frac"] = 4.0 * sq["SQ_ACTIVE_INST_VALU"] / (cyc * 4 * n_cu)
    if "SQ_LDS_IDX_ACTIVE" in sq:
        out["lds_frac"] = sq["SQ_LDS_IDX_ACTIVE"] / (cyc * n_cu)
        if "SQ_LDS_BANK_CONFLICT" in sq:
            out["lds_bank_conflict_frac"] = sq["SQ_LDS_BANK_CONFLICT"] / max(sq["SQ_LDS_IDX_ACTIVE"], 1.0)
    if "SQ_WAVE_CYCLES" in sq and "SQ_WAIT_ANY" in sq:
        out["waves_waiting_frac"] = sq["SQ_WAIT_ANY"] / max(sq["SQ_WAVE_CYCLES"], 1.0)
        out["mean_waves_per_simd"] = 4.0 * sq["SQ_WAVE_CYCLES"] / (cyc * 4 * n_cu)
    return out


def costvol_bytes(V, C, D, h, w):
    """Algorithmic bytes of the fused warp + cost-volume kernel."""
    return 4 * ((V + 1) * C * h * w + D * h * w)


class KernelTimer:
    """Duration of one kernel of the frame (ops.costvol: the sampling kernel the metric names; ops.conv3d: the K-Net
    layer that dominates the frame time) from HIP events on torch's current stream (= the
    stream the kernel is launched on).  Frames are replayed as one hipGraph, inside which single kernels cannot be
    bracketed, so the wrapper remembers the arguments of the last in-model launch (same tensors, same shapes) and
    `measure()` re-launches exactly that K times back to back between two events right after the timed region."""

    def __init__(self, keep=lambda a, k: True):
        self.last = None
        self.fn = None
        self.keep = keep
        self.in_frame = None       # a list while an EAGER frame is being timed: (event before, event after) of every matching call

    def wrap(self, fn):
        self.fn = fn

        def remembering(*a, **k):
            hit = self.keep(a, k)
            if hit:
                self.last = (a, k)
            if hit and self.in_frame is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(*a, **k)
                e1.record()
                self.in_frame.append((e0, e1))
                return out
            return fn(*a, **k)
        return remembering

    def in_frame_ms(self):
        """Mean duration of the matching calls of the eager frame bracketed by `in_frame = []` ... synchronize: the kernel where it
        sits in the frame (cold operands, the neighbours' tails), beside measure()'s steady-state figure."""
        if not self.in_frame:
            return None
        v = [e0.elapsed_time(e1) for e0, e1 in self.in_frame]
        self.in_frame = None
        return sum(v) / len(v), len(v)

    def measure(self, launches, warm=1):
        """`warm` untimed launches first: after any idle gap (a host sync, the CPU baseline, a profiler child process) the part
        takes 5-20 launches to come back to its steady state — the first ones run 15-30 % slow (profiles/r4_inframe_gap.txt:
        2.6-2.8 ms against 2.18 ms sustained for the K-Net layer; round 3's "in-frame 2.50 ms" was this ramp, measured behind
        the PMC child passes) — and the frame itself runs in the steady state."""
        a, k = self.last
        for _ in range(max(1, warm)):
            self.fn(*a, **k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            self.fn(*a, **k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches


def cpu_baseline(cfg, cam, d_candi, sd, window, bv_pred, sigma):
    """Update-branch frames of the SAME workload through the CPU oracle on the host cores: one warm-up frame, then the
    median (= mean) of two timed frames.  Returns (json dict, the oracle's outputs of the frame) — the
    outputs are what the `parity` block of the JSON line is computed against."""
    from oracle import cpu_oracle, kvnet_oracle
    # torch-CPU convolutions stop scaling long before this host's 256 hardware threads: measured on the
    # MI355X node (2 x EPYC 9575F) with tools/cpu_threads_probe.py, one config-S frame takes 1.49 / 1.47 /
    # 2.33 / 4.6 s at 16 / 32 / 64 / 128 threads and 8x longer at 256 — so the baseline uses its best: 32.
    # "port": the oracle is a restatement (C sampling + the ATen CPU ops the reference itself calls); the unmodified
    # reference cannot travel to the GPU box (/root/reference does not exist there).
    cores = min(32, os.cpu_count() or 1)
    torch.set_num_threads(cores)
    cpu_oracle.set_threads(cores)
    sd_cpu = {k: v.cpu() for k, v in sd.items()}
    r, s, p = (t.cpu() for t in window)
    bv = bv_pred.cpu()
    times, out = [], None
    for _ in range(3):
        t0 = time.time()
        out = kvnet_oracle.step(sd_cpu, r, s, p, cam, d_candi, sigma, bv)
        times.append(time.time() - t0)
    dt = 0.5 * (times[1] + times[2])
    return {"value": 1.0 / dt, "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": "update-branch frames (KVNET.forward + PREDICT) of config %s through oracle/kvnet_oracle.py: 1 warm-up "
                      "(%.1f s) + 2 timed (%.1f, %.1f s), median reported" % (cfg, times[0], times[1], times[2])}, out


def cpu_baseline_train(model, cam, d_candi, wins, sigma):
    """--mode train: the same training window through oracle/train_oracle.py (the CPU restatement of the reference's train()
    under torch autograd, pinned to tests/golden/train_small.npz) on the host cores: one first-frame iteration to create the
    filter state and the Adam moments, then one timed update-branch iteration (4 NLL terms, backward, Adam, PREDICT)."""
    from oracle import cpu_oracle, train_oracle
    cores = min(32, os.cpu_count() or 1)
    torch.set_num_threads(cores)
    cpu_oracle.set_threads(cores)
    leaves = train_oracle.leaf_state({k: v.detach().cpu() for k, v in model.state_dict().items()})
    opt = torch.optim.Adam(train_oracle.parameters(leaves), lr=1e-5, betas=(.9, .999))
    pred, times, loss = None, [], None
    for ref, src, p in wins[:2]:
        srcs = torch.cat([s_["img"] for s_ in src[0]], dim=0).unsqueeze(0).cpu()
        t0 = time.time()
        loss, pred = train_oracle.train_iteration(leaves, opt, ref[0]["img"].cpu(), srcs, p.cpu(), ref[0]["dmap"].cpu(),
                                                  ref[0]["dmap_imgsize_digit"].cpu(), cam, d_candi, sigma, pred)
        times.append(time.time() - t0)
    return {"value": 1.0 / times[1], "unit": "windows/s", "cores": cores, "kind": "port", "loss": float(loss),
            "sample": "one update-branch training iteration of the same window shape through oracle/train_oracle.py (%.1f s), after "
                      "one first-frame iteration (%.1f s, untimed)" % (times[1], times[0])}


def max_tie_flips(ties, mean_abs, tie_tol=1e-3):
    """= tests/conftest.py::max_tie_flips: twice the expected number of arg-max flips among `ties` near-tie pixels at the measured
    L1 (a flip needs the two candidates' error difference, <= 2 mean|d| in expectation, to exceed a gap spread over [0, tie_tol])."""
    return max(2, int(np.ceil(ties * min(1.0, 4.0 * float(mean_abs) / tie_tol))))


def parity_block(cfg, gpu, oracle_out):
    """GPU frame vs the oracle's frame on the same window and the same filter state: max / mean |d| and arg-max
    depth-index mismatches of BV_cur, DPV, BV_predict and the refined DPV (BASELINE.json gates: L1 < 1e-4, arg-max exact)."""
    names = ("refined", "dpv", "bv_cur", "bv_predict")
    blk = {"config": cfg, "against": "oracle/kvnet_oracle.py (CPU), same window, same BV_predict"}
    for name, g, o in zip(names, gpu, oracle_out):
        g, o = g[0].float().cpu(), o[0].float()
        d = (g - o).abs()
        ig, io = g.argmax(0), o.argmax(0)
        bad = ig != io
        # a flipped pixel is a TIE when the oracle's own values at the two indices are within 1e-3 of each other
        gap = (o.gather(0, io[None]) - o.gather(0, ig[None]))[0]
        top2 = o.topk(2, dim=0).values
        ties = int(((top2[0] - top2[1]) < 1e-3).sum())            # the oracle-side tie population: where two fp32 evaluations may flip
        blk[name] = {"max": float(d.max()), "mean": float(d.mean()), "argmax_mismatch": int(bad.sum()),
                     "argmax_mismatch_beyond_tie_1e-3": int((bad & (gap > 1e-3)).sum()), "pixels": int(g[0].numel()),
                     "oracle_ties_within_1e-3": ties, "argmax_mismatch_bound": max_tie_flips(ties, float(d.mean()))}
    # gates: L1 < 1e-4 on every volume; arg-max identical on the depth volumes (BV_predict's faces are overwritten with a
    # constant, so its arg-max is a tie by construction: reported only).  "pass_strict" = bit-exact arg-max; "pass" also
    # accepts flips at pixels whose two best candidates are within 1e-3 in the oracle itself, at most max_tie_flips(tie population
    # of the oracle's volume, measured L1) of them — the policy of the parity tests (tests/conftest.py), a bound the
    # unmodified reference obeys against itself on every fixture (ref_self below)
    depth_vols = ("refined", "dpv", "bv_cur")
    l1 = all(blk[n]["mean"] < 1e-4 for n in names)
    blk["max_abs_gate"] = MAX_ABS_GATE
    mx = all(blk[n]["max"] <= MAX_ABS_GATE for n in names)
    blk["pass_strict"] = l1 and all(blk[n]["max"] <= 1e-4 for n in names) and all(blk[n]["argmax_mismatch"] == 0 for n in depth_vols)
    blk["pass"] = l1 and mx and all(blk[n]["argmax_mismatch_beyond_tie_1e-3"] == 0 and blk[n]["argmax_mismatch"] <= blk[n]["argmax_mismatch_bound"]
                                    for n in depth_vols)
    # a trilinear resample is a convex combination: with the pose inverse owned by the path (same matrix on both sides)
    # BV_predict cannot differ by more than the DPV it resamples does
    blk["pass"] = blk["pass"] and blk["bv_predict"]["max"] <= blk["dpv"]["max"] + 2e-4
    return blk


def other_configs(skip, timeout_s=240):
    """BASELINE.json's other configurations on the same lease, each as a short child run of this script (5 steps after 3 warm-up
    frames — config H: its 300-frame stream —, no CPU baseline, no counter passes): {frames/s, ms per frame, the sampling kernel's time and fraction of the HBM roofline};
    plus one `--mode train` step pair at config 4's shape.  Driver-visible companions of the headline number, not part of it."""
    import subprocess
    out = {}
    base = [sys.executable, os.path.abspath(__file__), "--full", "--no-cpu-baseline", "--no-live-traffic", "--no-other-configs"]
    for cfg in [c for c in ("S", "K", "H") if c != skip]:
        steps = 300 if cfg == "H" else 5        # BASELINE config 5 IS a 300-frame sequence of one stream (state resident): sustained rate
        try:
            r = subprocess.run(base + ["--config", cfg, "--steps", str(steps), "--warmup", "3"], capture_output=True, text=True, timeout=timeout_s)
            doc = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            out[cfg] = {"workload": doc["config"]["workload"], "frames_per_s": doc["value"], "ms_per_frame": doc["ms_per_step"],
                        "costvol_kernel_ms": doc["roofline"]["kernel_ms"], "costvol_hbm_frac": doc["roofline"]["frac"],
                        "knet_layer_mfma_frac": doc.get("roofline_mfma", {}).get("frac"), "steps": steps, "warmup": 3,
                        "sequential_frames_per_s": doc["config"].get("sequential_frames_per_s"),
                        "peak_hbm_gb": doc["config"].get("peak_hbm_gb")}
        except Exception as e:      # a companion must never cost the headline line
            out[cfg] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    # the small grids with several independent videos per GPU (each its own model replica, filter state, hipGraphs and HIP stream):
    # config S / K launches fill a fraction of the chip, so concurrent streams recover the idle CUs
    for cfg, ns in (("S", 4), ("K", 3)):
        if cfg == skip:
            continue
        try:
            r = subprocess.run(base + ["--config", cfg, "--streams", str(ns), "--steps", "20", "--warmup", "6"], capture_output=True, text=True, timeout=timeout_s)
            doc = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            out["%s_x%d_streams" % (cfg, ns)] = {"workload": doc["config"]["workload"], "streams_per_gpu": ns, "frames_per_s": doc["value"],
                                                 "ms_per_step_all_streams": doc["ms_per_step"], "steps": 20, "warmup": 6,
                                                 "note": "whole-GPU throughput over %d concurrent videos; the per-video rate is this / %d" % (ns, ns)}
        except Exception as e:
            out["%s_x%d_streams" % (cfg, ns)] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    try:
        r = subprocess.run(base + ["--mode", "train", "--steps", "2", "--warmup", "1"], capture_output=True, text=True, timeout=timeout_s)
        doc = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        out["train"] = {"workload": doc["config"]["workload"], "windows_per_s": doc["value"], "ms_per_window": doc["ms_per_window"],
                        "ms_per_step": doc["ms_per_step"], "accum_steps": doc["config"]["accum_steps"], "launch": doc["config"]["launch"], "steps": 2, "warmup": 1}
    except Exception as e:
        out["train"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    return out


def respawn_under_torchrun(gpus):
    """`python bench.py --gpus N` (N > 1) started WITHOUT a torchrun environment: re-exec this command line as
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free> bench.py ...`,
    one rank per GPU.  Never returns.  (With RANK / WORLD_SIZE already set — the driver's own torchrun — nothing happens here.)"""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush(); sys.stderr.flush()
    os.execv(sys.executable, cmd)


FP64_FIXTURES = {   # config -> (file under tests/golden, window seeds, pixel stride of the stored float64 volumes)
    "S": ("net_fp64_S.npz", (101, 102), 4),     # oracle/gen_golden.py::gen_fp64_S
    "B": ("net_fp64_B.npz", (131, 132), 8),     # oracle/gen_golden.py::gen_fp64_B
}
MAX_ABS_GATE = 1e-3      # = tests/conftest.py::MAX_ABS_TOL
TOLERANCE_POLICY = (
    "north_star: arg-max depth index bit-exact, DPV floats within 1e-4.  Asserted here (pass): mean |d| (L1) < 1e-4 on every volume; "
    "max |d| <= 1e-3 on every volume (HARD); arg-max identical except at pixels whose two best candidates are within 1e-3 in the ORACLE's "
    "own volume (ties: at most max_tie_flips(oracle-side tie population, measured L1) per frame and volume — `argmax_mismatch_bound` —, none beyond a tie).  Why "
    "not 1e-4 max: the `ref_self` sub-block — the UNMODIFIED reference against ITSELF on the config-S windows when only its execution "
    "changes (oneDNN convolutions on / off, 8 threads / 1; tests/golden/ref_selfnoise_{S,K,ST}.npz, oracle/gen_golden.py selfnoise*: config S, config K "
    "and config S with trained-like weights) — differs by up to 6.2e-4 (max) in DPV and flips 1-2 arg-max indices among K's ~500 near-tie pixels; the `fp64` sub-block shows both fp32 evaluations 1e-3-class (max) away from the same graph in float64.  "
    "pass_strict = the gates as north_star words them (max <= 1e-4, no arg-max flip at all).")


def ref_self_block():
    """What two executions of the unmodified reference agree to (tests/golden/ref_selfnoise_<tag>.npz: config S, config K, config S
    with the trained-like weight family): per volume of the update frame [max |d|, mean |d|, arg-max flips, flips beyond a 1e-3
    tie, pixels] + the reference-side tie population the flip bound is taken from."""
    out = {"layout": "[max |d|, mean |d|, arg-max flips, flips beyond a 1e-3 tie, pixels]"}
    desc = {"S": "config S (two frames, noise windows, seeds 101 / 102)", "K": "config K: KITTI grid 64x192, candidates 1-60 m (seeds 111 / 112)",
            "ST": "config S with the trained-like weight family (synth.trained_like_state_dict; seeds 151 / 152)"}
    for tag in ("S", "K", "ST"):
        path = os.path.join(ROOT, "tests", "golden", "ref_selfnoise_%s.npz" % tag)
        if not os.path.isfile(path):
            continue
        g = np.load(path)
        blk = {"fixture": "tests/golden/ref_selfnoise_%s.npz" % tag, "config": desc[tag]}
        for var in ("onednn_off", "threads_1"):
            blk[var] = {k: [float(x) for x in g["%s_%s_f2" % (var, k)]] for k in ("refined", "dpv", "bv_cur", "pred")}
        blk["ties_within_1e-3"] = {k: int(g["base_%s_f2_ties" % k]) for k in ("refined", "dpv", "bv_cur")}
        out[tag] = blk
    return out if len(out) > 1 else None


def fp64_block(cfg, model, cam, d_candi, H, W, dev):
    """|GPU - float64| beside |fp32 CPU oracle - float64| for a FIXED first-frame + update-frame sequence (the windows of the
    config's parity test): the float64 evaluation of the same graph was generated once (oracle/fp64_ref.py via gen_golden.py) and
    is stored sub-sampled under tests/golden/ together with the oracle's measured distance from it."""
    import math
    from neuralrgbd_amd import homography as warp_homo, ops, synth
    if cfg not in FP64_FIXTURES:
        return None
    name, seeds, sub = FP64_FIXTURES[cfg]
    path = os.path.join(ROOT, "tests", "golden", name)
    if not os.path.isfile(path):
        return None
    g = dict(np.load(path))
    pred, outs = None, {}
    pad = math.log(1. / float(len(d_candi)))
    for fi, seed in enumerate(seeds):
        r, s_, p = (t.to(dev) for t in synth.noise_window(seed, H, W))
        with torch.no_grad():
            _, _, bv_cur, dpv = model(r, s_, p, torch.zeros(1), cam_intrinsics=[cam], BV_predict=pred)
            pred = warp_homo.resample_vol_cuda(dpv, ops.pose_inverse(p[0, 2].contiguous()), cam_intrinsic=cam, d_candi=d_candi,
                                               padding_value=pad, clamp=(-1000., 0.)).unsqueeze(0)
        outs["bv_cur_f%d" % (fi + 1)] = bv_cur
        if fi == 1:
            outs["dpv_f2"], outs["pred_f2"] = dpv, pred
    blk = {"fixture": "tests/golden/" + name, "windows": "noise windows, seeds %s: first frame + update frame" % (seeds,),
           "pixels": "every %dth grid pixel in both directions" % sub}
    for key in ("bv_cur_f1", "bv_cur_f2", "dpv_f2", "pred_f2"):
        if key not in g:
            continue
        a = outs[key][0, :, ::sub, ::sub].double().cpu().numpy()
        e = np.abs(a - g[key])
        rec = {"gpu_minus_fp64_mean": float(e.mean()), "gpu_minus_fp64_max": float(e.max()),
               "gpu_argmax_flips_vs_fp64": int((a.argmax(0) != g[key].argmax(0)).sum()), "pixels": int(a[0].size)}
        for src_k, dst_k in (("oracle_err_mean_sub_" + key, "oracle_minus_fp64_mean"), ("oracle_err_max_sub_" + key, "oracle_minus_fp64_max"),
                             ("oracle_err_max_" + key, "oracle_minus_fp64_max_all_pixels"), ("oracle_argmax_flips_" + key, "oracle_argmax_flips_vs_fp64_all_pixels")):
            if src_k in g:
                rec[dst_k] = float(g[src_k])
        blk[key] = rec
    return blk


def init_world(gpus, backend):
    """(world, rank, local) from the torchrun environment; the process group is created for world > 1.  The world size must
    equal --gpus: a mismatch is an error, never a silent single-GPU run."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != gpus:
        raise SystemExit("--gpus %d does not match WORLD_SIZE %d" % (gpus, world))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    return world, rank, local


def verified_ranks(world, device):
    """Ranks that actually took part in a collective: an all-reduce (sum) of ones on `device` (RCCL for cuda tensors)."""
    if world == 1:
        return 1
    t = torch.ones(1, dtype=torch.float32, device=device)
    torch.distributed.all_reduce(t)
    n = int(round(float(t.item())))
    if n != world:
        raise SystemExit("the collective saw %d ranks, the launch has %d" % (n, world))
    return n


def rank_times(world, steps, device):
    """ms per step of every rank: its own work (before the closing barrier) gathered from all ranks — stragglers show here."""
    own = getattr(timed_steps, "own", None)
    if own is None:
        return None
    if world == 1:
        return {"own_ms_per_step": [1e3 * own / steps]}
    t = torch.tensor([own], dtype=torch.float64, device=device)
    allt = [torch.zeros_like(t) for _ in range(world)]
    torch.distributed.all_gather(allt, t)
    v = [1e3 * float(x.item()) / steps for x in allt]
    return {"own_ms_per_step": v, "min": min(v), "max": max(v), "timed_region_ms_per_step": [1e3 * x / steps for x in timed_steps.per_rank]}


def allreduce_probe(reducer, world, device, reps=10):
    """The bucketed gradient all-reduce ALONE (the same buckets, the same index order, no backward around it): ms per call and
    the bus bandwidth a ring all-reduce of that size implies, 2 (N - 1) / N x bytes / time, beside one xGMI link's 153 GB/s."""
    if reducer is None or world == 1:
        return None
    nbytes = 4 * reducer.numel
    for _ in range(2):
        reducer.prepare()
        reducer()
    torch.cuda.synchronize()
    torch.distributed.barrier()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        reducer.prepare()
        reducer()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    t = torch.tensor([ms], dtype=torch.float64, device=device)
    torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
    ms = float(t.item())
    return {"allreduce_ms": ms, "bytes": nbytes, "buckets": len(reducer.buckets),
            "bus_gb_s": 2.0 * (world - 1) / world * nbytes / (ms * 1e-3) / 1e9, "xgmi_link_gb_s": 153.0,
            "note": "prepare (zero the buckets) + %d all-reduces + division, max over ranks" % len(reducer.buckets)}


def timed_steps(frame, steps, world, device):
    """The bench contract: barrier + synchronize, EXACTLY `steps` steps, barrier + synchronize, MAX over ranks."""
    def barrier():
        if world > 1:
            torch.distributed.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize()

    barrier()
    t0 = time.perf_counter()
    for i in range(steps):
        frame(i)
    if device.type == "cuda":
        torch.cuda.synchronize()
    timed_steps.own = time.perf_counter() - t0          # this rank's own work, before it waits for the others
    barrier()
    dt = time.perf_counter() - t0
    timed_steps.per_rank = [dt]
    if world > 1:
        # every rank's own clock around the same barrier-bracketed region (MAX = the contract's number; MIN beside it shows a
        # straggler: with the closing barrier inside the region the two differ only by the barrier's own skew)
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        allt = [torch.zeros_like(t) for _ in range(world)]
        torch.distributed.all_gather(allt, t)
        timed_steps.per_rank = [float(x.item()) for x in allt]
        dt = max(timed_steps.per_rank)
    return dt


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES):
    """{name: tensor} -> out_dir/<name>.npy in float32, at most `limit` bytes in all.  An array larger than its equal share of
    the limit is written as <name>_sampled.npy instead: every leading entry (the depth candidates) at a fixed, seeded
    sample of its pixel positions (the last two dimensions), sorted, [numel / pixels, P] — the same positions for the same
    shape in every run, and arg-max over depth stays comparable."""
    os.makedirs(out_dir, exist_ok=True)
    share = limit // max(1, len(arrays)) - 1024        # room for the .npy header
    for name, t in arrays.items():
        a = t.detach().float()
        if a.numel() * 4 <= share:
            np.save(os.path.join(out_dir, name + ".npy"), a.cpu().numpy())
            continue
        pix = a.shape[-1] * a.shape[-2]
        rows = a.numel() // pix
        keep = min(pix, share // (4 * rows))
        idx = np.sort(np.random.RandomState(0).choice(pix, keep, replace=False))
        sample = a.reshape(rows, pix).index_select(1, torch.from_numpy(idx).to(a.device))
        np.save(os.path.join(out_dir, name + "_sampled.npy"), sample.cpu().numpy())


def stub_main(args):
    """Harness self-test without a GPU (tests/test_dist_cpu.py): the same init / barrier / MAX-over-ranks / rank-0 JSON
    path as the real run on a gloo group, with a frame function that only sleeps (rank r sleeps (r+1) x 5 ms, so the MAX
    is visible).  The line is marked "stub": true and carries no metric."""
    world, rank, _ = init_world(args.gpus, "gloo")
    ranks = verified_ranks(world, torch.device("cpu"))
    frame = lambda i: time.sleep(0.005 * (rank + 1))
    for i in range(args.warmup):
        frame(i)
    dt = timed_steps(frame, args.steps, world, torch.device("cpu"))
    per_rank = rank_times(world, args.steps, torch.device("cpu"))
    if rank == 0:
        print(json.dumps({"stub": True, "n_gpus": world, "collective_ranks": ranks, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": 1e3 * dt / args.steps, "value": args.steps * world / dt, "scaling": "weak", "per_rank": per_rank}))
    if world > 1:
        torch.distributed.barrier()      # rank 0 is still measuring kernels / printing: nobody tears its communicator down before that
        torch.distributed.destroy_process_group()


def train_main(args):
    """--mode train: BASELINE config 4 shape (ScanNet 384x256 image, grid 96x64, 64 candidates; the reference's global batch 32
    = 8 GPUs x 4 sequential N = 1 windows).  One step = ONE optimizer step = `--accum` (default 4) windows per GPU through
    neuralrgbd_amd.train_step (forward under autograd, 4 NLL terms, backward — accumulated over the windows —, ONE bucketed
    RCCL all-reduce of the 21 MB gradient when N > 1, division by accum x N, Adam, PREDICT per window); hipGraph replay at
    every N (train_step.TrainGraph: the split form for N > 1 or accum > 1).  Not the headline metric: a separate, labelled line."""
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    world, rank, local = init_world(args.gpus, "nccl")
    ranks = verified_ranks(world, dev)
    import neuralrgbd_amd
    from neuralrgbd_amd import camera, distributed as nd, ops, synth
    from neuralrgbd_amd.optim import FusedAdam
    from neuralrgbd_amd.train_step import TrainGraph, train
    H, W, D, A = 256, 384, 64, max(1, args.accum)
    cam = camera.scannet_intrinsics(W // 4, H // 4)
    d_candi = np.linspace(0.1, 5, D)
    model = neuralrgbd_amd.KVNET(64, cam, d_candi, 10.0, 64, None, if_refined=True, refineNet_name="DPV", t_win_r=2)
    model.load_state_dict(synth.seeded_state_dict(model, 0))
    model = model.to(dev)
    use_graph = not args.no_graph
    opt = FusedAdam(model.parameters(), lr=1e-5, betas=(.9, .999))      # local_train_scanNet.sh's optim.Adam on csrc/optim.hip
    reducer = nd.GradAllReduce(model) if world > 1 else None
    tg = TrainGraph(model, opt, 2, d_candi, cam, warmup=0, grad_reducer=reducer, accum_steps=A) if use_graph else None
    rng = np.random.RandomState(rank)
    n_ring = 3
    wins = []                 # wins[slot][k]: the k-th window of accumulation slot `slot` (every slot is its own trajectory)
    for slot in range(A):
        ring = []
        for it in range(n_ring):
            r, s_, p = synth.noise_window(1000 * rank + 10 * slot + it, H, W)
            ring.append(({"img": r.to(dev), "dmap": torch.from_numpy(rng.randint(0, D, (1, H // 4, W // 4))).to(dev),
                          "dmap_imgsize_digit": torch.from_numpy(rng.randint(0, D, (1, H, W))).to(dev)},
                         [{"img": s_[0, v:v + 1].to(dev)} for v in range(4)], p.to(dev)))
        wins.append(ring)
    # the K-Net's 64 -> 64 layers run through ops.conv_wino_dw (forward and data gradient: autograd.Conv3dCL)
    knet_timer = KernelTimer(keep=lambda a, k: a[0].shape[-1] == 64)
    if args.full:
        ops.conv_wino_dw = knet_timer.wrap(ops.conv_wino_dw)
    state = {"pred": [None] * A, "loss": None}

    def step(i, eager=False):
        batch = [wins[slot][i % n_ring] for slot in range(A)]
        if tg is not None and not eager:
            windows = [(ref["img"], torch.cat([s_["img"] for s_ in src], dim=0).unsqueeze(0), p, ref["dmap"],
                        ref["dmap_imgsize_digit"], state["pred"][slot]) for slot, (ref, src, p) in enumerate(batch)]
            if tg.split:
                state["loss"], state["pred"] = tg.step_windows(windows)
            else:
                loss, pred = tg.step(*windows[0])
                state["pred"], state["loss"] = [pred.clone()], loss      # the graph's outputs are static buffers
            return
        _, pred, state["loss"], _, _ = train(world, model, opt, 2, d_candi, [b_[0] for b_ in batch], [b_[1] for b_ in batch],
                                             torch.cat([b_[2] for b_ in batch], dim=0), state["pred"], [cam],
                                             grad_reducer=reducer, accum_steps=A)
        state["pred"] = list(pred.split(1, dim=0))
    for i in range(2):      # first frame + one update frame launched from Python: filter state, optimizer state, caches
        step(i, eager=True)
    for i in range(max(args.warmup, 2)):
        step(i + 2)
    dt = timed_steps(step, args.steps, world, dev)
    if args.dump_outputs and rank == 0:
        # what train() hands its caller: the loss of the last window and the predicted filter state of every accumulation slot
        dump_outputs(args.dump_outputs, dict([("loss", state["loss"].reshape(1))] +
                                             [("bv_predict_slot%d" % k, p_) for k, p_ in enumerate(state["pred"])]))
    assert bool(torch.isfinite(state["loss"])), "training loss went non-finite"
    per_rank = rank_times(world, args.steps, dev)
    ar = allreduce_probe(reducer, world, dev) if args.full else None
    if rank == 0:
        line = {"metric": "training windows/sec @grid 96x64x64cand, 5-view window, N=1 per forward (BASELINE config 4 shape)",
                "value": args.steps * A * world / dt, "unit": "windows/s", "n_gpus": world, "rccl_ranks": ranks, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "ms_per_window": 1e3 * dt / (args.steps * A),
                "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                "config": {"workload": "ScanNet training window 384x256 image, grid 96x64x64cand, Adam lr 1e-5", "mode": "train",
                           "accum_steps": A, "global_batch": A * world,
                           "launch": ("hipGraph replay (%s)" % ("forward+backward graph x%d, all-reduce, optimizer graph" % A
                                                                if tg.split else "one graph")) if tg is not None else "eager",
                           "parallelism": "data-parallel x%d, %d windows per rank and step, one bucketed gradient all-reduce per step (%.2f MB fp32)" %
                                          (world, A, 4e-6 * sum(p.numel() for p in set(model.parameters()))),
                           "loss": float(state["loss"])}}
        if per_rank is not None:
            line["per_rank"] = per_rank
        if ar is not None:
            line["allreduce"] = ar
        if knet_timer.last is not None:
            c_ms = knet_timer.measure(20, warm=30)
            a0 = knet_timer.last[0][0]
            blocks = (-(-a0.shape[0] // 2)) * (-(-a0.shape[1] // 2)) * (-(-a0.shape[2] // 2))
            flops = 2.0 * blocks * 64 * 64 * 64               # issued in the Winograd domain: 64 multiplies per 2x2x2 outputs and (ci, co)
            tf = flops / (c_ms * 1e-3) / 1e12
            line["roofline"] = {"bound": "mfma", "kernel": "conv_wino_dw_kernel<false,false,false> (K-Net 3x3x3 64->64, Winograd in all three "
                                "dimensions: forward and data gradient of the 10 such layers dominate the iteration)", "achieved": tf,
                                "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf / MFMA_F32_PEAK_TFLOPS,
                                "flops": flops, "direct_conv_flops": 2.0 * a0.shape[0] * a0.shape[1] * a0.shape[2] * 64 * 64 * 27,
                                "traffic": None, "kernel_ms": c_ms}
        if world == 1 and args.full and not args.no_cpu_baseline:
            flat = [([ref], [src], p) for ring in wins for (ref, src, p) in ring]
            line["cpu_baseline"] = cpu_baseline_train(model, cam, d_candi, flat, 10.0)
        print(json.dumps(line))
    if world > 1:
        torch.distributed.barrier()      # rank 0 is still measuring kernels / printing: nobody tears its communicator down before that
        torch.distributed.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="B", choices=sorted(CONFIGS))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel from Python instead of replaying the captured hipGraph")
    ap.add_argument("--no-live-traffic", action="store_true", help="roofline.traffic from the committed PMC file instead of two rocprofv3 "
                    "--pmc child passes of this script (about a minute; N = 1 only)")
    ap.add_argument("--streams", type=int, default=1, help="independent video streams per GPU, each on its own HIP stream "
                    "(a step is then one frame of EVERY stream; the extra streams fill the tails of each other's kernels)")
    ap.add_argument("--back-to-back", action="store_true", help="(kept for old command lines: roofline.back_to_back_ms — the sampling kernel re-launched "
                    "20x back to back between one pair of events, the figure of rounds 1-4 — is always reported with --full now)")
    ap.add_argument("--no-pipeline", action="store_true", help="strictly sequential frames (one hipGraph per frame) instead of the default: the D-Net "
                    "of frame t + 1 on a second HIP stream under the K-Net / R-Net / PREDICT of frame t (same video, same kernels, same bits)")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the short companion runs of configs S / K / H and of one "
                    "training step (N = 1, headline config only; about a minute)")
    ap.add_argument("--full", action="store_true", help="also measure what the headline figure does not need, each in runs of its own "
                    "after the timed steps: the kernel rooflines, the strictly sequential rate, the CPU baseline and parity, the other "
                    "configurations (the --no-* options above switch single parts off)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last one returned to its caller as "
                    "DIR/<name>.npy (float32, at most 64 MB: larger outputs as a fixed, seeded sample of their pixels)")
    ap.add_argument("--stub", action="store_true", help=argparse.SUPPRESS)   # CPU self-test of the N>1 harness
    ap.add_argument("--accum", type=int, default=4, help="--mode train: windows per GPU and optimizer step (gradient accumulation; "
                    "BASELINE config 4 = global batch 32 = 8 GPUs x 4)")
    ap.add_argument("--mode", default="infer", choices=["infer", "train"], help="train: a separate, labelled line for the "
                    "training iteration at BASELINE config 4's shape (not the headline metric)")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        respawn_under_torchrun(args.gpus)          # never print n_gpus: 1 for --gpus N
    if args.stub:
        if args.dump_outputs:
            ap.error("--dump-outputs: the --stub self-test computes nothing")
        return stub_main(args)
    if args.mode == "train":
        return train_main(args)

    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    world, rank, local = init_world(args.gpus, "nccl")
    ranks = verified_ranks(world, dev)     # an actual RCCL all-reduce at N > 1: the line's "rccl_ranks"

    import neuralrgbd_amd
    from neuralrgbd_amd import camera, ops, synth
    from neuralrgbd_amd.streaming import DepthStream

    cfg = CONFIGS[args.config]
    H, W, D, V = cfg["H"], cfg["W"], cfg["D"], 4
    h, w = H // 4, W // 4
    sigma = 10.0
    cam = camera.scannet_intrinsics(w, h) if args.config != "K" else camera.kitti_intrinsics(w, h)
    d_candi = np.linspace(cfg["d_min"], cfg["d_max"], D)
    model = neuralrgbd_amd.KVNET(64, cam, d_candi, sigma, 64, None, if_refined=True, refineNet_name="DPV", t_win_r=2)
    sd = synth.seeded_state_dict(model, 0)
    model.load_state_dict(sd)
    model = model.to(dev)  # stays in train() mode like the reference

    # a short ring of synthetic windows per rank, resident in HBM (different video per rank)
    ring = [tuple(t.to(dev) for t in synth.noise_window(1000 * rank + i, H, W, V)) for i in range(2)]

    # --full: the kernels of the two rooflines, timed where they sit in eager frames after the timed region
    timer = KernelTimer()
    # the K-Net's plain 64->64 layer (BatchNorm+ReLU prologue, no residual operand, nothing materialised): 5 of its 12 layers
    knet_timer = KernelTimer(keep=lambda a, k: a[0].shape[-1] == 64 and k.get("res") is None and k.get("x_ss") is not None
                             and not k.get("materialize"))
    # ... which runs on csrc/wino_dw4.hip (F(4,3) along depth) where D % 4 == 0: the same filter picks its clamped-FMA-ReLU launches
    knet_timer4 = KernelTimer(keep=lambda a, k: a[0].shape[-1] == 64 and k.get("x_ss") is not None and bool(k.get("x_unit")))
    if args.full:
        ops.costvol = timer.wrap(ops.costvol)
        ops.conv_wino_dw = knet_timer.wrap(ops.conv_wino_dw)
        ops.conv_wino_dw4 = knet_timer4.wrap(ops.conv_wino_dw4)

    # the streaming driver: same per-frame work as test_utils/test_KVNet.py::test (R_net=True), state resident,
    # the update-branch frame captured into one hipGraph after an eager warm-up frame.  Extra streams per GPU are
    # further independent videos with their own model replica, filter state, graph and HIP stream.
    import copy
    S = max(1, args.streams)
    models = [model] + [copy.deepcopy(model) for _ in range(S - 1)]
    hip_streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(dev) for _ in range(S - 1)]
    pipe = (not args.no_pipeline) and (not args.no_graph)
    streams = [DepthStream(m, cam, d_candi, t_win_r=2, use_graph=not args.no_graph, device=dev, pipeline=pipe) for m in models]
    stream = streams[0]

    def frame(i):
        out = []
        for k in range(S):
            r, s_, p = ring[(i + k) % len(ring)]
            with torch.cuda.stream(hip_streams[k]):
                out.append(streams[k].step(r, s_, p))
        frame.last = out                 # what every stream's step() returned: --dump-outputs
        return out[-1]

    frame(0)                       # first window of the stream: D-Net only, creates the filter state
    # >= 2: one eager update frame, then the capture frame; pipelined: two eager frames, the capture, one replay of either slot
    for i in range(max(args.warmup, 6 if pipe else 2)):
        frame(i + 1)

    dt = timed_steps(frame, args.steps, world, dev)
    if args.dump_outputs and rank == 0:
        # the (refined DPV, DPV) pair step() returned in the last timed step (pipelined: the frame before it), every stream;
        # graph outputs are static buffers, so they are read before anything else runs on the streams
        outs = {}
        for k, o in enumerate(frame.last):
            if o is not None:
                sfx = "" if S == 1 else "_stream%d" % k
                outs["refined_dpv" + sfx], outs["dpv" + sfx] = o
        dump_outputs(args.dump_outputs, outs)
    seq_fps = None
    if pipe and args.full:
        # the same stream once more WITHOUT the overlap (one hipGraph per frame, strictly sequential): reported beside the headline
        for st_ in streams:
            st_.flush()
        seq = [DepthStream(m, cam, d_candi, t_win_r=2, use_graph=True, device=dev, pipeline=False) for m in models]

        def seq_frame(i):
            for k in range(S):
                r, s_, p = ring[(i + k) % len(ring)]
                with torch.cuda.stream(hip_streams[k]):
                    seq[k].step(r, s_, p)
        for i in range(4):
            seq_frame(i)
        dt_seq = timed_steps(seq_frame, args.steps, world, dev)
        seq_fps = args.steps * S * world / dt_seq
    pred = stream.bv_predict
    assert bool(torch.isfinite(pred).all()), "filter state went non-finite"
    per_rank = rank_times(world, args.steps, dev)

    if rank == 0:
        line = {
            "metric": "depth frames/sec @256x192x64cand, 5-view window; warp-kernel HBM GB/s vs peak",
            "value": args.steps * S * world / dt, "unit": "frames/s", "n_gpus": world, "rccl_ranks": ranks, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": cfg["name"], "config_id": args.config, "grid_hw": [h, w], "depth_candidates": D,
                       "views": V + 1, "streams_per_gpu": S, "streams_total": S * world,
                       "launch": ("hipGraph replay, the two halves of consecutive frames of the video pipelined: D-Net (feature CNN + fused warp / cost volume) of "
                                  "frame t+1 on a second HIP stream under K-Net + DPV update + R-Net + PREDICT of frame t; every frame computed in full, "
                                  "outputs bit-identical to the sequential order (tests/test_gpu_fullsize.py), one frame of latency"
                                  if pipe and stream._graph is not None else "hipGraph replay" if stream._graph is not None else "eager"),
                       "parallelism": "replicas x%d (independent video streams)" % world,
                       "peak_hbm_gb": torch.cuda.max_memory_allocated(dev) / 1e9},
        }
        if per_rank is not None:
            line["per_rank"] = per_rank
        if args.full:
            # ---- the two roofline kernels WHERE THEY SIT: consecutive EAGER frames of one window and filter state right behind the timed
            # region (the timed frames are hipGraph replays, inside which a single kernel cannot be bracketed), every matching launch
            # between its own pair of HIP events on the launch stream.  Until round 5 the sampling kernel was re-launched 20x back to back
            # between ONE pair of events instead: that loop measures 0.235 ms where the kernel takes 0.20 ms in the frame and 0.193 ms per
            # launch once events separate the launches (tools/r5_cv_gap.py) — without anything between them a launch runs into the previous
            # one's end-of-kernel write-back of 25 MB of dirty cost / log-probability lines.  `--back-to-back` still reports that figure.
            from neuralrgbd_amd import homography as warp_homo
            pred = pred.clone()
            r_, s_, p_ = ring[0]

            def eager_frame():
                with torch.no_grad():
                    _, r_kv_, bv_cur_, dpv_ = model(r_, s_, p_, torch.zeros(1), cam_intrinsics=[cam], BV_predict=pred, dpv_valid=True)
                    nxt_ = warp_homo.resample_vol_cuda(dpv_, ops.pose_inverse(p_[0, 2].contiguous()), cam_intrinsic=cam, d_candi=d_candi,
                                                       padding_value=float(np.log(1.0 / D)), clamp=(-1000., 0.)).unsqueeze(0)
                return r_kv_, dpv_, bv_cur_, nxt_
            for _ in range(2):       # untimed: the allocator's blocks outside the graph's pool are created here (a hipMalloc drains the GPU)
                eager_frame()
            torch.cuda.synchronize()
            timer.in_frame, knet_timer.in_frame, knet_timer4.in_frame = [], [], []
            n_eager = max(8, min(args.steps, 20))
            for _ in range(n_eager):
                gpu_out = eager_frame()
            torch.cuda.synchronize()
            k_ms, n_k = timer.in_frame_ms()
            got4 = knet_timer4.in_frame_ms()
            got = got4 if got4 is not None else knet_timer.in_frame_ms()
            depth_f43 = got4 is not None
            c_ms, n_c = got if got is not None else (None, 0)
            b2b_ms = timer.measure(20, warm=20)      # rounds 1-4's figure, always beside the in-frame one (rounds stay comparable)
            algo = costvol_bytes(V, 67, D, h, w)
            achieved = algo / (k_ms * 1e-3) / 1e9
            traffic, traffic_note, sq = (None, "", None)
            if world == 1 and not args.no_live_traffic and not args.no_graph and S == 1:
                traffic, traffic_note, sq = live_pmc_traffic(args.config)      # measured now, by three rocprofv3 --pmc child passes
            if traffic is None:
                t2, n2 = pmc_traffic(args.config)                          # the committed measurement (refused if the kernel changed)
                traffic, traffic_note = t2, (n2 if not traffic_note else "%s; live measurement unavailable: %s" % (n2, traffic_note))
            line["config"]["sequential_frames_per_s"] = seq_fps
            line["config"]["peak_hbm_gb"] = torch.cuda.max_memory_allocated(dev) / 1e9      # with the eager frames' blocks
            line["roofline"] = {"bound": "hbm", "kernel": "costvol_quad<L2,3> (fused warp + cost volume + log-softmax over depth, one launch)",
                                "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                                "algorithmic_bytes": algo, "kernel_ms": k_ms, "launches_timed": n_k,
                                "timing": "mean over the kernel's launches in %d consecutive eager frames right behind the timed region (2 untimed ones first), each "
                                          "launch between its own pair of HIP events on the launch stream; the log-softmax is part of the launch" % n_eager,
                                "traffic": traffic, "traffic_source": traffic_note}
            if b2b_ms is not None:
                line["roofline"]["back_to_back_ms"] = b2b_ms
            if sq:
                # the HBM target is structurally out of reach for this kernel (118 flop/B against a machine balance of 20, SURVEY.md
                # 8d): what binds it is VALU issue and the LDS gather — their utilisation from the kernel's own SQ counters
                line["roofline"].update(sq_fractions(sq))
                line["roofline"]["sq_counters_per_launch"] = sq
            if c_ms is not None:   # secondary roofline: the matrix-core kernel that takes most of the frame
                # F(2x2,3x3) in the plane and F(2,3) along depth: 64 multiplies per 2x2x2 outputs and (ci, co) instead of 216 -> the
                # MFMAs the kernel actually issues; the 27-tap figure is what a direct convolution would need for the same layer
                nominal = 2.0 * D * h * w * 64 * 64 * 27
                if depth_f43:   # F(4,3) along depth: 6 x 16 transform points per 4 x 2 x 2 outputs and (ci, co)
                    blocks = (-(-D // 4)) * (-(-h // 2)) * (-(-w // 2))
                    flops = 2.0 * blocks * 64 * 64 * 96
                else:
                    blocks = (-(-D // 2)) * (-(-h // 2)) * (-(-w // 2))
                    flops = 2.0 * blocks * 64 * 64 * 64
                tf = flops / (c_ms * 1e-3) / 1e12
                line["roofline_mfma"] = {"bound": "mfma", "kernel": ("conv_wino_dw4_kernel<CLAMP> (F(2x2,3x3) in the plane x F(4,3) along depth: 6 multiplies per "
                                         "output voxel)" if depth_f43 else "conv_wino_dw_kernel<CLAMP> (F(2x2,3x3) x F(2,3): 8 multiplies per output voxel)") +
                                         ", the frame's own calls: one K-Net 3x3x3 64->64 layer with a BatchNorm + ReLU input (the 10 64->64 layers are ~50 % of the "
                                         "frame); `achieved` counts the MFMA flops the kernel ISSUES", "achieved": tf,
                                         "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf / MFMA_F32_PEAK_TFLOPS,
                                         "flops": flops, "direct_conv_flops": nominal,
                                         "direct_conv_equivalent_tflops": nominal / (c_ms * 1e-3) / 1e12, "kernel_ms": c_ms,
                                         "launches_timed": n_c, "timing": "mean over the 5 matching layer launches of each of the same eager frames, every launch "
                                         "between its own pair of HIP events (no idle gap in front of them: steady state, profiles/r4_inframe_gap.txt)"}
            if world == 1 and not args.no_cpu_baseline:
                # the same frame on both sides: window ring[0] filtered with the stream's state — the last of the eager frames above
                r_kv, dpv, bv_cur, nxt = gpu_out
                line["cpu_baseline"], o = cpu_baseline(args.config, cam, d_candi, sd, ring[0], pred, sigma)
                line["parity"] = parity_block(args.config, (r_kv, dpv, bv_cur, nxt), o)
                line["parity"]["tolerance_policy"] = TOLERANCE_POLICY
                f64 = fp64_block(args.config, model, cam, d_candi, H, W, dev)
                if f64 is not None:
                    line["parity"]["fp64"] = f64
                rs = ref_self_block()
                if rs is not None:
                    line["parity"]["ref_self"] = rs
            if world == 1 and args.config == "B" and not args.no_other_configs and not args.no_graph and S == 1:
                line["other_configs"] = other_configs(args.config)
        print(json.dumps(line))
    if world > 1:
        torch.distributed.barrier()      # rank 0 is still measuring kernels / printing: nobody tears its communicator down before that
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
