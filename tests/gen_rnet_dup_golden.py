"""Fixture for the R-Net with candidate up-sampling (KVNET(if_upsample_d=True), train(refine_dup=True)): tests/golden/rnet_dup_d32.npz.

    python tests/gen_rnet_dup_golden.py

runs the UNMODIFIED reference (through oracle/ref_shim.py, on the CPU) with `if_upsample_d=True` at image 256 x 256 (the SPP window
of 64 forbids less), grid 64 x 64, D = 32 (the refined volumes have 128 candidates), t_win_r = 2, and records
  * two inference frames, the body of test_utils/test_KVNet.py::test: first frame, PREDICT, update frame (low-resolution volumes at
    pixel stride SUB_Q, the refined [128, ., .] volumes at SUB_R);
  * one UPDATE-branch iteration of train_utils/train_KVNet.py::train(refine_dup=True) (plain SGD, so a weight change is lr x gradient)
    from the seeded weights, the seeded volume `train_bv_predict()` and the seeded labels `labels()` (image size: bins in [0, 4 D),
    0 = ignore): loss, BV_predict (stride SUB_T), and of each tensor of PROBES the weight change at PROBE_SAMPLES evenly spread
    elements with the largest change of the whole tensor, and its sums over all but the first axis, which every element enters (a
    refined layer of this net has up to 200,000 weights: the file stays below 1 MB);
  * the reference model's state-dict keys and shapes;
  * a condition the reference meets on its own: its R-Net evaluated in float64 on the inputs its fp32 R-Net saw, and the fp32
    volumes held against that under the gates of tests/test_gpu_parity_configs.py::_check on the stored pixels (asserted here, on the
    host; a seed that fails is changed, never the gate).  Stored: the float64 volumes' tie counts and the fp32 errors.
The file holds data only.  The tests (test_rnet_dup_host.py, test_gpu_rnet_dup.py) read it, the inputs below and nothing of the reference.
"""
import copy
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

from neuralrgbd_amd import camera, synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
PATH = os.path.join(OUT, "rnet_dup_d32.npz")
DUP = dict(H=256, W=256, D=32, r=2, sigma=10.0, d_min=0.1, d_max=5.0, weight_seed=0, lr=1e-3, label_seed=23, bv_seed=29,
           seeds=(271, 272))
SUB_Q, SUB_R, SUB_T = 2, 16, 4
VOLUMES = (("bv_cur_f1", SUB_Q), ("pred_f1", SUB_Q), ("refined_cur_f1", SUB_R), ("bv_cur_f2", SUB_Q), ("dpv_f2", SUB_Q),
           ("refined_cur_f2", SUB_R), ("refined_f2", SUB_R))
REFINED = ("refined_cur_f1", "refined_cur_f2", "refined_f2")
PROBE_SAMPLES = 1024


def probes():
    from oracle import gen_golden
    return tuple(gen_golden.TRAIN["probes"]) + ("r_net.trans_conv1.0.weight",)       # TRAIN's already hold r_net.conv2_2.weight


def setup():
    """(cam, d_candi) of the fixture."""
    t = DUP
    return camera.scannet_intrinsics(t["W"] // 4, t["H"] // 4), np.linspace(t["d_min"], t["d_max"], t["D"])


def windows():
    """The two seeded noise windows (ref [1,3,H,W], src [1,4,3,H,W], poses [1,4,4,4])."""
    return [synth.noise_window(s, DUP["H"], DUP["W"], V=2 * DUP["r"]) for s in DUP["seeds"]]


def labels():
    """Integer depth-bin labels (0 = ignore) of the training iteration: quarter resolution in [0, D), image resolution in [0, 4 D)."""
    t = DUP
    rng = np.random.RandomState(t["label_seed"])
    return (torch.from_numpy(rng.randint(0, t["D"], (1, t["H"] // 4, t["W"] // 4))),
            torch.from_numpy(rng.randint(0, 4 * t["D"], (1, t["H"], t["W"]))))


def train_bv_predict():
    """The predicted volume the training iteration starts from, [1, D, h, w]: a seeded log-softmax, computed in float64."""
    t = DUP
    z = np.random.RandomState(t["bv_seed"]).standard_normal((t["D"], t["H"] // 4, t["W"] // 4)) * 2.0
    z = z - z.max(axis=0, keepdims=True)
    return torch.from_numpy((z - np.log(np.exp(z).sum(axis=0, keepdims=True))).astype(np.float32))[None]


def state_dict_lines(g):
    """[(key, shape tuple)] of the reference model, from the loaded fixture."""
    rows = [ln.rsplit(" ", 1) for ln in bytes(g["state_dict"]).decode().split("\n")]
    return [(k, tuple(int(n) for n in sh.split(",")) if sh else ()) for k, sh in rows]


def sample(delta):
    """The stored elements of a weight change: PROBE_SAMPLES evenly spread ones (all of a smaller tensor)."""
    flat = np.asarray(delta).reshape(-1)
    return flat[np.linspace(0, flat.size - 1, min(PROBE_SAMPLES, flat.size)).astype(np.int64)]


def row_sums(delta):
    """Sum of a weight change over everything but its first axis, in float64: every element enters one of them."""
    d = np.asarray(delta, dtype=np.float64)
    return d.reshape(d.shape[0], -1).sum(axis=1)


def generate():
    from oracle import gen_golden, ref_shim
    from test_gpu_parity_configs import _check
    from conftest import tie_count
    ref = ref_shim.load()
    import train_utils.train_KVNet as tk
    t = DUP
    r = t["r"]
    cam, d_candi = setup()
    with ref_shim.quiet():
        model = ref.KVNET.KVNET(64, cam, d_candi, t["sigma"], 64, None, if_refined=True, refineNet_name="DPV", t_win_r=r,
                                if_upsample_d=True)
    model.load_state_dict(synth.seeded_state_dict(model, t["weight_seed"]))
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    out = {"state_dict": np.frombuffer("\n".join("%s %s" % (k, ",".join(str(n) for n in v.shape)) for k, v in sd0.items()).encode(),
                                       dtype=np.uint8),      # "key shape" lines as bytes (a unicode array of them is 4 bytes a character)
           "weights_checksum": gen_golden.checksum(sd0.values())}
    # ---- two inference frames; the R-Net's inputs are kept for the float64 evaluation
    seen = []
    hook = model.r_net.register_forward_hook(lambda m, args, kwargs, res: seen.append((args, kwargs, res)), with_kwargs=True)
    wins = windows()
    pad = math.log(1. / float(len(d_candi)))
    pred, frames = None, []
    for (rf, s, p) in wins:
        with torch.no_grad():
            R_cur, R_kv, bv_cur, dpv = model(ref_frame=rf, src_frames=s, src_cam_poses=p, BatchIdx=torch.FloatTensor(np.arange(1)),
                                             cam_intrinsics=[cam], BV_predict=pred)
        if pred is None:
            dpv, R_kv = bv_cur, R_cur
        pred = ref.homography.resample_vol_cuda(src_vol=dpv[0].unsqueeze(0), rel_extM=p[0, r].inverse(), cam_intrinsic=cam,
                                                d_candi=d_candi, padding_value=pad).clamp(max=0, min=-1000.).unsqueeze(0)
        frames.append(dict(refined_cur=R_cur[0].numpy(), refined=R_kv[0].numpy(), bv_cur=bv_cur[0].numpy(), dpv=dpv[0].numpy(),
                           pred=pred[0].numpy()))
    hook.remove()
    assert frames[0]["refined_cur"].shape == (4 * t["D"], t["H"], t["W"])
    for key, sub in VOLUMES:
        name, f = key.rsplit("_f", 1)
        out[key] = np.ascontiguousarray(frames[int(f) - 1][name][:, ::sub, ::sub])
    # ---- the reference's own fp32 R-Net against its float64 evaluation, under the gates the project is held to
    assert len(seen) == 3, len(seen)                     # R(BV_cur) of frame 1; R(BV_cur), R(DPV) of frame 2
    r64 = copy.deepcopy(model.r_net).double()
    to64 = lambda x: [to64(y) for y in x] if isinstance(x, (list, tuple)) else x.double()
    for key, (args, kwargs, res) in zip(REFINED, seen):
        with torch.no_grad():
            want = r64(*[to64(a) for a in args], **{k: to64(v) for k, v in kwargs.items()})
        want = want[:, :, ::SUB_R, ::SUB_R].float()
        got = res.detach()[:, :, ::SUB_R, ::SUB_R]
        assert np.array_equal(got[0].numpy(), out[key])
        mx = _check("reference fp32 vs its float64 R-Net: %s" % key, got, want)
        out["f64_ties_" + key] = tie_count(want[0].numpy())
        out["f64_max_" + key] = mx
        out["f64_l1_" + key] = float((got - want).abs().mean())
    # ---- one update-branch training iteration with the up-sampled label
    rf, s, p = wins[1]
    dm, dmf = labels()
    opt = torch.optim.SGD(model.parameters(), lr=t["lr"])
    Rd = [{"img": rf, "dmap": dm, "dmap_up4_imgsize_digit": dmf, "dmap_raw": torch.zeros(1, t["H"] // 4, t["W"] // 4),
           "dmap_imgsize": torch.zeros(1, t["H"], t["W"])}]
    Sd = [[{"img": s[0, v:v + 1]} for v in range(2 * r)]]
    with ref_shim.quiet():
        _, tpred, loss, _, _ = tk.train(1, model, opt, r, d_candi, Rd, Sd, p, train_bv_predict(), [cam], refine_dup=True)
    out["train_loss"] = float(loss)
    out["train_pred"] = np.ascontiguousarray(tpred[0].detach().numpy()[:, ::SUB_T, ::SUB_T])
    for k in probes():
        delta = (model.state_dict()[k].detach() - sd0[k]).numpy()
        out["train_delta_" + k] = sample(delta)
        out["train_delta_max_" + k] = np.abs(delta).max()
        out["train_delta_rows_" + k] = row_sums(delta)
    np.savez_compressed(PATH, **out)
    size = os.path.getsize(PATH)
    print("rnet_dup_d32: %d state-dict keys, train loss %.6f, %.0f KB" % (len(sd0), float(loss), size / 1024.))
    assert size < 1000 * 1024


if __name__ == "__main__":
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    generate()
