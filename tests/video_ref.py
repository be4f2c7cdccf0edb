"""What the video stream (neuralrgbd_amd/video.py) is held against, on the CPU: the loaders' image preparation as torch-CPU
operations, the integer nearest-resize rule, seeded frames and a smooth seeded trajectory, and the reference's driver loop
(test_KVNet.py:185-250) written out with a list that slides.  Shared by tests/test_video_host.py and tests/test_gpu_video.py."""
import numpy as np
import torch

from neuralrgbd_amd import homography, misc

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def nearest_index(n_in, n_out):
    """Source index of every output index: nearest at pixel centres in integers, ((2 i + 1) n_in) // (2 n_out)."""
    i = np.arange(n_out, dtype=np.int64)
    return ((2 * i + 1) * n_in) // (2 * n_out)


def resize_nearest(hwc, Hout, Wout):
    """[Hin,Win,3] -> [Hout,Wout,3] by numpy indexing with the integer rule."""
    return hwc[nearest_index(hwc.shape[0], Hout)][:, nearest_index(hwc.shape[1], Wout)]


def normalise(hwc, mean=MEAN, std=STD):
    """ToTensor then Normalize of a uint8 [H,W,3] array as torchvision computes them on the CPU: fp32 [3,H,W]."""
    t = torch.from_numpy(np.ascontiguousarray(hwc)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.as_tensor(std, dtype=torch.float32)[:, None, None]
    return t.sub_(m).div_(s)


def noise_frames(seed, n, H, W):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(n)]


def trajectory(seed, n):
    """n world-to-camera matrices (float64) of a camera that drifts and turns a little per frame."""
    rng = np.random.RandomState(seed)
    w, v = rng.uniform(-0.01, 0.01, 3), rng.uniform(-0.02, 0.02, 3)
    out = []
    for i in range(n):
        a = w * i + 0.002 * np.sin(0.7 * i + np.arange(3))
        Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
        M = np.eye(4)
        M[:3, :3] = Rz @ Ry @ Rx
        M[:3, 3] = v * i + 0.005 * np.cos(0.5 * i + np.arange(3))
        out.append(M)
    return out


def driver_loop(images, extMs, r):
    """test_KVNet.py:185-250 over prepared frames: per iteration (index of the reference frame, valid, reference image, list of
    source images, relative poses fp32 [2r,4,4] or None when the window holds a NaN pose)."""
    dat_array = [{"img": images[i], "extM": extMs[i], "idx": i} for i in range(2 * r + 1)]
    out = []
    nxt = 2 * r + 1
    while True:
        valid = not any(np.isnan(d["extM"].min()) or np.isnan(d["extM"].max()) for d in dat_array)
        ref_dat, src_dats = misc.split_frame_list(dat_array, r)
        poses = None
        if valid:
            poses = np.stack([homography.get_rel_extrinsicM(ref_dat["extM"], d["extM"]).astype(np.float32) for d in src_dats])
        out.append((ref_dat["idx"], valid, ref_dat["img"], [d["img"] for d in src_dats], poses, [d["idx"] for d in src_dats]))
        if nxt == len(images):
            return out
        dat_array.pop(0)
        dat_array.append({"img": images[nxt], "extM": extMs[nxt], "idx": nxt})
        nxt += 1
