"""What the training video stream (neuralrgbd_amd/train_video.py) is held against, on the CPU: the loaders' depth preparation
(mdataloader/scanNet.py:372-422) restated with the reference's own tools — real PIL.Image.resize(..., NEAREST) on a mode-I frame and on
its mode-L hole mask, torch's `.float() * .001`, np.digitize against float64 candidates, the clamp to [0, n - 1] —, seeded depth frames,
and the training driver's loop (train_KVNet.py:283-330 over mdataloader/batch_loader.py:78-96,239-279) written out with a list that
slides.  Nothing here calls the helpers of the module under test.  Shared by tests/test_train_video_host.py,
tests/test_gpu_depth_ingest.py and tests/test_gpu_train_video.py."""
import numpy as np
import torch
from PIL import Image

from neuralrgbd_amd import homography, misc


def integer_nearest_index(n_in, n_out):
    """The integer nearest rule of the uint8 frame ingest, ((2 i + 1) n_in) // (2 n_out): NOT Pillow's for every size pair."""
    i = np.arange(n_out, dtype=np.int64)
    return ((2 * i + 1) * n_in) // (2 * n_out)


def pil_nearest_index(n_in, n_out, mode="I"):
    """Source index of every output index, read off a real Pillow resize of an image whose pixels name their own position (mode 'I':
    int32; 'L' / 'F' for n_in <= 256 / any)."""
    ramp = np.arange(n_in)
    arr = {"I": ramp.astype(np.int32), "L": ramp.astype(np.uint8), "F": ramp.astype(np.float32)}[mode]
    assert mode != "L" or n_in <= 256
    row = np.asarray(Image.fromarray(np.stack([arr, arr]), mode=None).resize((n_out, 2), Image.NEAREST))[0]
    col = np.asarray(Image.fromarray(np.stack([arr, arr], axis=1)).resize((2, n_out), Image.NEAREST))[:, 0]
    assert np.array_equal(row, col)                              # the two axes follow the same rule
    return row.astype(np.int64)


def up4(d_candi):
    """The loaders' dup4_candi (scanNet.py:327)."""
    d_candi = np.asarray(d_candi)
    return np.linspace(d_candi.min(), d_candi.max(), 4 * len(d_candi))


def _digit(dmap, d_candi):
    """mloader_misc.dMap_to_indxMap + the two clamps of scanNet.py:409-411 -> int64 tensor."""
    idx = np.digitize(dmap.cpu().numpy(), np.asarray(d_candi, dtype=np.float64))
    label_max, label_min = len(d_candi) - 1, 0
    idx[idx >= label_max] = label_max
    idx[idx <= label_min] = label_min
    return torch.from_numpy(idx.astype(np.int64))


def prepare_depth(depth_u16, net_size, grid_size, d_candi, depth_scale=.001):
    """scanNet.py:372-422 for a uint16 [Hin,Win] frame, img_size = net_size (H, W), the resized map at grid_size (h, w):
    {dmap, dmap_imgsize_digit, dmap_up4_imgsize_digit: int64 [1,.,.]; dmap_raw, dmap_imgsize: fp32 [1,.,.]}."""
    (H, W), (h, w) = net_size, grid_size
    dmap_raw = Image.fromarray(np.ascontiguousarray(depth_u16).astype(np.int32))                 # what PIL opens a 16-bit PGM as
    assert dmap_raw.mode == "I"
    mask_imgsize = Image.fromarray((np.asarray(dmap_raw) < 0.01).astype(np.uint8) * 255).resize([W, H], Image.NEAREST)
    assert mask_imgsize.mode == "L"
    dmap_imgsize = torch.from_numpy(np.asarray(dmap_raw.resize([W, H], Image.NEAREST)).copy()).float() * depth_scale
    mask = mask_imgsize.resize([w, h], Image.NEAREST)                                            # the mask goes through two resizes
    dmap_small = torch.from_numpy(np.asarray(dmap_raw.resize([w, h], Image.NEAREST)).copy()).float() * depth_scale
    keep = 1 - (torch.from_numpy(np.asarray(mask).copy()) > 0).to(torch.uint8)
    keep_imgsize = 1 - (torch.from_numpy(np.asarray(mask_imgsize).copy()) > 0).to(torch.uint8)
    dmap_small = dmap_small * keep.type_as(dmap_small)
    dmap_imgsize = dmap_imgsize * keep_imgsize.type_as(dmap_imgsize)
    return {"dmap": _digit(dmap_small, d_candi)[None],
            "dmap_imgsize_digit": _digit(dmap_imgsize, d_candi)[None],
            "dmap_up4_imgsize_digit": _digit(dmap_imgsize, up4(d_candi))[None],
            "dmap_raw": dmap_small[None], "dmap_imgsize": dmap_imgsize[None]}


def depth_frames(seed, n, Hin, Win):
    """n seeded uint16 [Hin,Win] frames: a smooth surface in 0 .. 6000 with noise, a sprinkle of far values up to 65,535, and about
    30 % holes (zeros) — rectangular blobs plus isolated pixels."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:Hin, 0:Win].astype(np.float64)
    out = []
    for _ in range(n):
        a, b, c = rng.uniform(0.5, 3.0, 3)
        d = 3000 + 2400 * np.sin(a * y / Hin * 3 + c) * np.cos(b * x / Win * 3) + rng.uniform(-600, 600, (Hin, Win))
        d = np.clip(d, 1, 6000)
        far = rng.rand(Hin, Win) < 0.01
        d[far] = rng.randint(6000, 65536, int(far.sum()))
        hole = rng.rand(Hin, Win) < 0.08                                # isolated pixels
        for _ in range(6):                                              # blobs: about a quarter of the frame
            bh, bw = rng.randint(max(2, Hin // 8), max(3, Hin // 3)), rng.randint(max(2, Win // 8), max(3, Win // 3))
            y0, x0 = rng.randint(0, Hin), rng.randint(0, Win)
            hole[y0:y0 + bh, x0:x0 + bw] = True
        d[hole] = 0
        out.append(d.astype(np.uint16))
    return out


def all_values_frame(seed=0):
    """256 x 256 holding every uint16 value exactly once, shuffled."""
    return np.random.RandomState(seed).permutation(65536).astype(np.uint16).reshape(256, 256)


def driver_loop(items, r):
    """train_KVNet.py:283-330 for one trajectory over loader items {'dmap': a map or an int for a missing one, 'extM': float64 [4,4],
    'idx': i}: per frame_count (index of the reference frame, valid, whether the step runs WITHOUT a BV_predict, relative poses fp32
    [2r,4,4] or None, indices of the sources)."""
    dat_array = [items[i] for i in range(2 * r + 1)]
    out, nxt, frame_count, prev_invalid = [], 2 * r + 1, 0, False
    while True:
        valid = True                                                     # batch_loader._check_datArray_pose
        for dat in dat_array:
            if isinstance(dat["dmap"], int):
                valid = False
                break
            elif np.isnan(dat["extM"].min()) or np.isnan(dat["extM"].max()):
                valid = False
                break
        ref_dat, src_dats = misc.split_frame_list(dat_array, r)
        poses, first = None, None
        if valid:
            poses = np.stack([homography.get_rel_extrinsicM(ref_dat["extM"], d["extM"]).astype(np.float32) for d in src_dats])
            first = frame_count == 0 or prev_invalid
            prev_invalid = False
        else:
            prev_invalid = True
        out.append((ref_dat["idx"], valid, first, poses, [d["idx"] for d in src_dats]))
        if nxt == len(items):
            return out
        dat_array.pop(0)
        dat_array.append(items[nxt])
        nxt += 1
        frame_count += 1
