"""Fixtures of the guided-filter refinement net (refineNet_name='DGF'): tests/golden/dgf_<case>.npz and dgf_model.npz.

    python tests/gen_dgf_golden.py

runs the UNMODIFIED reference (through oracle/ref_shim.py, on the CPU) and records, per case of CASES (low-resolution grid -> image,
noise guide):
  * the weights of a seeded models/Refine.py::RefineNet_DGF (its own initialiser under torch.manual_seed),
  * the inputs: a depth map in [0.1, 5] m on the low-resolution grid and a noise image,
  * the reference's output in fp32 (`ref32`) and with the module and the inputs cast to float64 (`ref64`), and the max / mean of
    |ref32 - ref64| (`ref32_err`): the reference's own fp32 error, the yardstick of tests/test_gpu_dgf.py.
Noise guides on purpose: only there is the reference's fp32 output meaningful (on smooth images its cumsum box filter and its
E[x^2] - E[x]^2 variance cancel, and the output is metres off: README, "DGF").
dgf_model.npz: the state-dict keys and shapes of models/KVNET.py::KVNET(..., refineNet_name='DGF') and the shapes a first and an
update frame return at the shape of the twin fixtures (256 x 256, D = 8).
The files hold data only.  The tests (test_dgf_host.py, test_gpu_dgf.py, test_gpu_dgf_net.py) read them and nothing of the reference.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from neuralrgbd_amd import camera, synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
# name: (h, w, H, W, seed)
CASES = {"8x12": (8, 12, 32, 48, 301), "9x17": (9, 17, 18, 34, 302), "24x40": (24, 40, 96, 160, 303)}
MODEL = dict(H=256, W=256, D=8, sigma=10.0, d_min=0.1, d_max=5.0, weight_seed=0, r=2, seeds=(181, 182))


def path(case):
    return os.path.join(OUT, "dgf_%s.npz" % case)


def model_path():
    return os.path.join(OUT, "dgf_model.npz")


def inputs(h, w, H, W, seed):
    """(depth [1,1,h,w] in [0.1, 5], image [1,3,H,W] noise) of a case, fp32."""
    rng = np.random.RandomState(seed)
    depth = (0.1 + 4.9 * rng.rand(1, 1, h, w)).astype(np.float32)
    img = rng.randn(1, 3, H, W).astype(np.float32)
    return torch.from_numpy(depth), torch.from_numpy(img)


def model_setup():
    m = MODEL
    return camera.scannet_intrinsics(m["W"] // 4, m["H"] // 4), np.linspace(m["d_min"], m["d_max"], m["D"])


def model_windows():
    return [synth.noise_window(s, MODEL["H"], MODEL["W"], V=2 * MODEL["r"]) for s in MODEL["seeds"]]


def generate_case(ref_refine, case):
    h, w, H, W, seed = CASES[case]
    torch.manual_seed(seed)
    net = ref_refine.RefineNet_DGF(3)
    depth, img = inputs(h, w, H, W, seed)
    with torch.no_grad():
        ref32 = net(depth, img)[0, 0].numpy().copy()
        w1, b1 = net.feature_ext[0].weight.detach().numpy().reshape(64, 3).copy(), net.feature_ext[0].bias.detach().numpy().copy()
        w2, b2 = net.feature_ext[2].weight.detach().numpy().reshape(64).copy(), net.feature_ext[2].bias.detach().numpy().copy()
        ref64 = net.double()(depth.double(), img.double())[0, 0].numpy().copy()
    err = np.abs(ref32.astype(np.float64) - ref64)
    np.savez(path(case), w1=w1, b1=b1, w2=w2, b2=b2, depth=depth[0, 0].numpy(), img=img[0].numpy(), ref32=ref32, ref64=ref64,
             ref32_err=np.array([err.max(), err.mean()]))
    print("dgf_%s: reference fp32 - float64 max %.3e mean %.3e, %.0f KB" % (case, err.max(), err.mean(), os.path.getsize(path(case)) / 1024.))


def generate_model(ref, ref_shim):
    m = MODEL
    cam, d_candi = model_setup()
    with ref_shim.quiet():
        model = ref.KVNET.KVNET(64, cam, d_candi, m["sigma"], 64, None, if_refined=True, refineNet_name="DGF", t_win_r=m["r"])
    sd = model.state_dict()
    model.load_state_dict(synth.seeded_state_dict(model, m["weight_seed"]))
    out = {"state_dict_keys": np.array(list(sd.keys())),
           "state_dict_shapes": np.array([",".join(str(n) for n in v.shape) for v in sd.values()])}
    pred = None
    for f, (rf, s, p) in enumerate(model_windows(), 1):
        with torch.no_grad():
            res = model(ref_frame=rf, src_frames=s, src_cam_poses=p, BatchIdx=torch.FloatTensor(np.arange(1)), cam_intrinsics=[cam],
                        BV_predict=pred)
        out["shapes_f%d" % f] = np.array([",".join(str(n) for n in t.shape) for t in res])
        if pred is None:
            out["first_frame_pairs"] = np.array([res[0] is res[1], res[2] is res[3]])
        pred = res[3]           # any valid volume selects the update branch: only the shapes are recorded
    np.savez(model_path(), **out)
    print("dgf_model: %d state-dict keys, frame shapes %s / %s" % (len(sd), list(out["shapes_f1"]), list(out["shapes_f2"])))


if __name__ == "__main__":
    from oracle import ref_shim
    ref_ = ref_shim.load()
    import models.Refine as ref_refine_
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    for case_ in CASES:
        generate_case(ref_refine_, case_)
    generate_model(ref_, ref_shim)
