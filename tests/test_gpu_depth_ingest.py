"""nrgbd_depth_ingest_u16 (neuralrgbd_amd/csrc/depth_ingest.hip) through train_video.DepthLabeler: every output equal, bit for bit,
to the loaders' depth preparation restated with real Pillow and np.digitize (tests/train_video_ref.py).  Labels are integers; the
fp32 metres are compared with torch.equal."""
import numpy as np
import pytest
import torch

import train_video_ref as tr
from neuralrgbd_amd import train_video
from neuralrgbd_amd.train_step import _capture_mode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                     # elements in front of and behind every output (a multiple of 4: keeps 16-byte alignment)

CANDI = {"s8": np.linspace(.1, 5, 8), "s32": np.linspace(.1, 5, 32), "s64": np.linspace(.1, 5, 64), "s128": np.linspace(.1, 5, 128),
         "k64": np.linspace(1, 60, 64)}


def _guarded(shape, dtype):
    """An output tensor [1,*shape] in the middle of a buffer whose guard words a test can check afterwards."""
    n = int(np.prod(shape))
    fill = -7 if dtype == torch.int64 else -7.5
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(1, *shape)


def _run(lab, frame, skip=None):
    """The labeler's outputs written into guarded buffers; `skip`: the key left out (that output pointer is NULL)."""
    bufs, out = {}, {}
    for key, shape, dtype in (("dmap", (lab.h, lab.w), torch.int64), (lab.full_key, (lab.H, lab.W), torch.int64),
                              ("dmap_raw", (lab.h, lab.w), torch.float32), ("dmap_imgsize", (lab.H, lab.W), torch.float32)):
        if key != skip:
            bufs[key], out[key] = _guarded(shape, dtype)
    got = lab(frame, out=out)
    torch.cuda.synchronize()
    assert got is out
    for key, buf in bufs.items():
        fill = -7 if buf.dtype == torch.int64 else -7.5
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all()), "guard words of %s" % key
    return {k: v.cpu() for k, v in out.items()}


def _assert_equal(got, want, lab):
    for key, v in got.items():
        assert v.dtype == want[key].dtype and tuple(v.shape) == tuple(want[key].shape), key
        bad = int((v != want[key]).sum())
        assert torch.equal(v, want[key]), "%s: %d of %d elements differ" % (key, bad, v.numel())


@pytest.fixture(scope="module")
def all_values():
    return tr.all_values_frame(5)


@pytest.mark.parametrize("name,dup", [(n, d) for n in sorted(CANDI) for d in (False, True)])
def test_every_uint16_value_gets_the_loaders_label(all_values, name, dup):
    """256 x 256 holding every value once, no resize at the image size, grid 64 x 64: every threshold of every candidate set, the
    up-sampled sets included (4 x 128 = 512 candidates fills the kernel's threshold table)."""
    d = CANDI[name]
    want = tr.prepare_depth(all_values, (256, 256), (64, 64), d)
    lab = train_video.DepthLabeler(d, (256, 256), (64, 64), refine_dup=dup, device=DEV)
    got = _run(lab, all_values)
    assert len(got) == 4 and len(torch.unique(got[lab.full_key])) == len(lab.thr_full)           # every label occurs
    _assert_equal(got, want, lab)


SIZES = {"scannet": ((480, 640), (256, 384), (64, 96), None),         # Pillow leaves the integer rule (640 -> 96); the mask composes
         "upsample_pitch": ((37, 53), (64, 96), (16, 24), 64),        # up-sampling, odd source sizes, padded rows
         "tail": ((30, 41), (18, 27), (9, 13), None)}                 # widths that are no multiple of 4: element stores


@pytest.fixture(scope="module")
def cases():
    """(frame as pushed, labeler, comparator's maps) per size — computed once, read by the tests below."""
    out = {}
    d = CANDI["s64"]
    for i, (name, ((Hin, Win), net, grid, pitch)) in enumerate(sorted(SIZES.items())):
        frame = tr.depth_frames(20 + i, 1, Hin, Win)[0]
        want = tr.prepare_depth(frame, net, grid, d)
        pushed = frame
        if pitch is not None:                                         # a device frame whose rows are `pitch` elements apart
            buf = np.full((Hin, pitch), 12345, dtype=np.uint16)
            buf[:, :Win] = frame
            pushed = torch.from_numpy(buf).to(DEV)[:, :Win]
            assert pushed.stride() == (pitch, 1)
        out[name] = (pushed, train_video.DepthLabeler(d, net, grid, device=DEV), want, frame)
    return out


@pytest.mark.parametrize("name", sorted(SIZES))
def test_resized_masked_maps_equal_the_loaders(cases, name):
    pushed, lab, want, frame = cases[name]
    assert 0.2 < float((frame == 0).mean()) < 0.5 and int(frame.max()) > 6000
    got = _run(lab, pushed)
    _assert_equal(got, want, lab)
    assert int((got["dmap"] == 0).sum()) > 0 and int(got["dmap"].max()) == 63
    # a second call returns the same bits
    again = _run(lab, pushed)
    assert all(torch.equal(again[k], got[k]) for k in got)
    # the up-sampled label of the same frame
    lab4 = train_video.DepthLabeler(CANDI["s64"], (lab.H, lab.W), (lab.h, lab.w), refine_dup=True, device=DEV)
    got4 = _run(lab4, pushed)
    _assert_equal(got4, want, lab4)
    assert "dmap_up4_imgsize_digit" in got4 and int(got4["dmap_up4_imgsize_digit"].max()) == 255


def test_scannet_case_keeps_its_teeth(cases):
    """What the 480 x 640 case is there to catch does occur in it: the integer resize rule and a directly resized mask both give
    other maps than the loaders'."""
    _, lab, want, frame = cases["scannet"]
    rq, cq = tr.pil_nearest_index(480, 64), tr.pil_nearest_index(640, 96)
    direct = frame[rq][:, cq]
    assert int(((direct == 0) != (want["dmap_raw"][0].numpy() == 0)).sum()) > 0                   # direct mask != composed mask
    integer = frame[tr.integer_nearest_index(480, 64)][:, tr.integer_nearest_index(640, 96)]
    assert int((integer != direct).sum()) > 0


@pytest.mark.parametrize("name", sorted(SIZES))
@pytest.mark.parametrize("skip", ["dmap", "dmap_imgsize_digit", "dmap_raw", "dmap_imgsize"])
def test_each_output_may_be_left_out(cases, name, skip):
    pushed, lab, want, _ = cases[name]
    got = _run(lab, pushed, skip=skip)
    assert sorted(got) == sorted(set(["dmap", "dmap_imgsize_digit", "dmap_raw", "dmap_imgsize"]) - {skip})
    _assert_equal(got, want, lab)


def test_one_part_alone(cases):
    pushed, lab, want, _ = cases["scannet"]
    for keys in (("dmap",), ("dmap_imgsize",), ("dmap_raw", "dmap")):
        out = {k: torch.full_like(want[k], -3).to(DEV) for k in keys}
        lab(pushed, out=out)
        assert all(torch.equal(out[k].cpu(), want[k]) for k in keys)
    with pytest.raises(ValueError):
        lab(pushed, out={})


def test_host_frames_and_tensor_forms(cases):
    _, lab, want, frame = cases["scannet"]
    for form in (frame, torch.from_numpy(frame), torch.from_numpy(frame).to(DEV), torch.from_numpy(frame.view(np.int16)).to(DEV)[None]):
        got = {k: v.cpu() for k, v in lab(form).items()}
        _assert_equal(got, want, lab)
    # the pinned buffer is re-used by a smaller frame that follows at once
    small = frame[:100, :200].copy()
    got = {k: v.cpu() for k, v in lab(small).items()}
    _assert_equal(got, tr.prepare_depth(small, (256, 384), (64, 96), CANDI["s64"]), lab)


@pytest.mark.parametrize("name", ["scannet", "tail"])
def test_launch_is_capturable_and_replays_the_same_bits(cases, name):
    pushed, lab, want, frame = cases[name]
    static = torch.from_numpy(pushed.view(np.int16)).to(DEV)             # the frame's bits; refilled below
    out = lab.empty_outputs()
    lab(static, out=out)                                               # the tables are uploaded before the capture
    for v in out.values():
        v.fill_(-1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=_capture_mode()):
        lab(static, out=out)
    g.replay()
    torch.cuda.synchronize()
    _assert_equal({k: v.cpu() for k, v in out.items()}, want, lab)
    # a replay on another frame in the same buffer
    other = tr.depth_frames(77, 1, *frame.shape)[0]
    static.copy_(torch.from_numpy(other.view(np.int16)).to(DEV))
    g.replay()
    torch.cuda.synchronize()
    _assert_equal({k: v.cpu() for k, v in out.items()}, tr.prepare_depth(other, (lab.H, lab.W), (lab.h, lab.w), CANDI["s64"]), lab)
