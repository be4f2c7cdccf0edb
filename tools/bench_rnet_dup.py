"""Frames per second of the streaming driver with and without candidate up-sampling in the R-Net (KVNET(if_upsample_d=True)).

    python tools/bench_rnet_dup.py [--config S|B] [--steps 200] [--upsample 0|1|both] [--once]

bench.py's timing loop (its windows, its warm-up, `timed_steps`) around DepthStream(pipeline=True) at the configuration's 64 candidates;
bench.py itself is untouched and measures the path without up-sampling.  Prints one JSON line per variant.  `--once`: a few eager
frames (no hipGraph) — the run to put under `rocprofv3 --kernel-trace --stats` for the per-kernel times of the three full-resolution
layers (conv2, conv2_1, conv2_2: the launches at the image's resolution with 272 / 272 / 256 input channels).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import neuralrgbd_amd  # noqa: E402
from neuralrgbd_amd import camera, synth  # noqa: E402
from neuralrgbd_amd.streaming import DepthStream  # noqa: E402


def run(config, steps, warmup, upsample, graph=True):
    cfg = bench.CONFIGS[config]
    H, W, D = cfg["H"], cfg["W"], cfg["D"]
    dev = torch.device("cuda:0")
    cam = camera.scannet_intrinsics(W // 4, H // 4)
    d_candi = np.linspace(cfg["d_min"], cfg["d_max"], D)
    model = neuralrgbd_amd.KVNET(64, cam, d_candi, 10.0, 64, None, if_refined=True, refineNet_name="DPV", t_win_r=2,
                                 if_upsample_d=bool(upsample))
    model.load_state_dict(synth.seeded_state_dict(model, 0))
    model = model.to(dev)
    ring = [tuple(t.to(dev) for t in synth.noise_window(i, H, W, 4)) for i in range(2)]
    stream = DepthStream(model, cam, d_candi, t_win_r=2, use_graph=graph, device=dev, pipeline=graph)

    def frame(i):
        return stream.step(*ring[i % len(ring)])
    frame(0)
    for i in range(max(warmup, 6)):
        frame(i + 1)
    dt = bench.timed_steps(frame, steps, 1, dev)
    out = stream.flush() if graph else frame(0)
    torch.cuda.synchronize()
    stream.check()
    return {"config": config, "if_upsample_d": bool(upsample), "candidates": D, "refined_shape": list(out[0].shape), "steps": steps,
            "graph": stream._graph is not None, "frames_per_s": steps / dt, "ms_per_frame": 1e3 * dt / steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B", choices=["S", "B"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--upsample", default="both", choices=["0", "1", "both"])
    ap.add_argument("--once", action="store_true", help="eager frames only, two timed steps: the run for a kernel trace")
    a = ap.parse_args()
    for up in ((0, 1) if a.upsample == "both" else (int(a.upsample),)):
        print(json.dumps(run(a.config, 2 if a.once else a.steps, a.warmup, up, graph=not a.once)), flush=True)


if __name__ == "__main__":
    main()
