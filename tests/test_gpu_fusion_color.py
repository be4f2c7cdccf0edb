"""GPU: fusion.FusionVideoStream(color=True) against the loop written out — VideoDepthStream.push -> ops.depth_regress ->
TSDFVolume.integrate with the picture in the reference frame's ring slot, the stream's intrinsics at the network size and (std, mean)
as the affine — on the model, sizes and sequence of tests/test_gpu_fusion_stream.py.  The five planes are compared bit for bit: eager,
hipGraph, pipelined through flush(), r = 1 and 2, both sources; tsdf and weight also against the colourless stream; constant-colour
uint8 frames come back as exactly that colour on every vertex; render(color=True) against the restatement."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_fusion_stream as fsr
import test_gpu_video as tv
from neuralrgbd_amd import fusion, video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _volume(color=True):
    return fusion.TSDFVolume(fsr.DIMS, fsr.VOXEL, fsr.ORIGIN, device=DEV, color=color)


@functools.lru_cache(maxsize=None)
def _hand(r):
    """The sequence of radius r, and per reference frame the maps of a bare eager VideoDepthStream and the picture its ring slot held
    when the maps came out (eager, not pipelined: the frame is r pushes old and its slot has not been reused)."""
    frames, _, extMs = tv._sequence(r)
    model, cam, d_candi = tv._model(r)
    vs = video.VideoDepthStream(model, cam, d_candi, t_win_r=r, copy_outputs=True, use_graph=False)
    maps, pictures = {}, {}
    for f, e in zip(frames, extMs):
        out = vs.push(f, e)
        if out is not None:
            maps[out[0]] = (out[1].clone(), out[2].clone())
            pictures[out[0]] = vs.ring[out[0] % vs.R].clone()
    torch.cuda.synchronize()
    vs.check()
    return frames, extMs, maps, pictures, (vs.mean, vs.std, vs.H, vs.W)


def _hand_integrate(vol, r, source):
    frames, extMs, maps, pictures, (mean, std, H, W) = _hand(r)
    cam, d_candi = tv.gt.setup()
    for ci in sorted(maps):
        v = maps[ci][0 if source == "refined" else 1][0]
        depth = fsr._regress(v, d_candi)[0]
        kw = {}
        if vol.color is not None:
            kw = dict(color=pictures[ci], color_intrinsics=fusion.intrinsics_at(cam, H, W), color_affine=(std, mean))
        assert vol.integrate(depth, extMs[ci], cam, depth_range=fsr.DEPTH_RANGE, **kw)


@functools.lru_cache(maxsize=None)
def _colourless_stream(r, source):
    frames, extMs = _hand(r)[:2]
    vol = _volume(False)
    fsr._stream(r, frames, extMs, vol, source=source, use_graph=False)
    return vol


MODES = {"eager": dict(use_graph=False), "graph": dict(use_graph=True), "pipeline": dict(use_graph=True, pipeline=True)}


@pytest.mark.parametrize("r,mode,source", [(2, "eager", "refined"), (2, "graph", "dpv"), (2, "pipeline", "refined"), (1, "eager", "dpv"),
                                           (1, "graph", "refined"), (1, "pipeline", "dpv")])
def test_colour_stream_equals_the_hand_built_loop(r, mode, source):
    frames, extMs, maps, pictures, _ = _hand(r)
    want = _volume()
    _hand_integrate(want, r, source)
    vol = _volume()
    fs, outs = fsr._stream(r, frames, extMs, vol, source=source, color=True, **MODES[mode])
    if MODES[mode]["use_graph"]:
        assert fs.stream._graph is not None, fs.stream.graph_error
    assert sorted(outs) == list(range(r, len(frames) - r)) and fs.n_integrated == len(outs)      # the last through flush() when pipelined
    fsr._same_maps(outs, maps)
    assert torch.equal(vol.color.view(torch.int32), want.color.view(torch.int32)), "colour differs"
    fsr._same_volume(vol, want)
    plain = _colourless_stream(r, source)
    fsr._same_volume(vol, plain)
    assert int((want.weight > 0).sum()) > 1000 and bool(want.color.any())
    seen = want.color[:, want.weight > 0]
    assert float(seen.min()) >= -1e-6 and float(seen.max()) <= 1 + 1e-6      # (std, mean) undo the normalisation: colours in [0, 1]


def test_constant_colour_frames_come_back_exactly_and_render_colour():
    r = 1
    frames, extMs = _hand(r)[:2]
    rgb = (200, 31, 117)
    flat = [np.broadcast_to(np.array(rgb, np.uint8), f.shape).copy() for f in frames]
    plain_vol = _volume(False)
    model, cam, d_candi = tv._model(r)
    vol = _volume()
    fs = fusion.FusionVideoStream(model, cam, d_candi, vol, t_win_r=r, depth_range=fsr.DEPTH_RANGE, color=True, use_graph=False)
    for f, e in zip(flat, extMs):
        fs.push(f, e)
    torch.cuda.synchronize()
    v, f, c, (nv, nf) = fs.mesh(colors=True)
    assert fs.n_integrated > 0 and nv == len(v) == len(c)
    assert nv > 1000 and nf > 1000
    assert torch.equal(fusion.to_uint8(c).cpu(), torch.tensor(rgb, dtype=torch.uint8).expand(nv, 3))
    pts, pc, found = vol.points(colors=True)
    assert found == nv and torch.equal(pc.view(torch.int32), c.view(torch.int32))
    seen = vol.color[:, vol.weight > 0]
    assert bool((vol.weight > 0).any()) and torch.equal(fusion.to_uint8(seen).cpu(), torch.tensor(rgb, dtype=torch.uint8)[:, None].expand_as(seen))
    # render: three maps, zero at the same pixels and zero wherever depth is zero.  A hit is black as well where one of the eight
    # weights around the HIT point is below w_min (include/nrgbd.h: the rule that also leaves such a hit without a normal); the march
    # only tested the cells of its two samples.  Measured on this sequence: 154 of 61272 hits (r = 1, w_min = 1).  So the maps are
    # compared with the restatement bit for bit, and "zero exactly where depth is zero" is asserted on every pixel that rule colours.
    import tsdf_color_ref as cref
    depth, col = fs.render(color=True)
    d2, n2, col2 = fs.render(normals=True, color=True)
    assert torch.equal(depth, fs.render()) and torch.equal(d2, depth) and torch.equal(col2, col) and tuple(col.shape) == (3, fs.H, fs.W)
    lit, hit = (col != 0).cpu().numpy(), (depth != 0).cpu().numpy()
    cast = {"depth": depth.cpu().numpy(), "hit": hit}
    want, _, ok, rows = cref.raycast(np.float32, cast, vol.weight.cpu().numpy(), vol.color.cpu().numpy(), vol.origin, vol.voxel_size, fs.last_ext,
                                     fusion.intrinsics_at(cam, fs.H, fs.W), (fs.H, fs.W), 1.0)
    assert np.array_equal(col.cpu().numpy().view(np.int32), want.view(np.int32))
    coloured = np.zeros(hit.size, bool)
    coloured[rows] = ok
    coloured = coloured.reshape(hit.shape)
    print("[fusion colour] render: %d hits, %d of them beside an under-weight corner (black)" % (hit.sum(), (hit & ~coloured).sum()))
    assert np.array_equal(lit[0], lit[1]) and np.array_equal(lit[0], lit[2]) and not (lit[0] & ~hit).any()
    assert np.array_equal(lit[0], coloured) and hit.sum() > 1000 and (hit & ~coloured).sum() < hit.sum() // 50
    assert not bool((n2[:, torch.from_numpy(hit & ~coloured).to(DEV)] != 0).any())       # the same hits have no normal either
    with pytest.raises(ValueError):
        fusion.FusionVideoStream(model, cam, d_candi, plain_vol, t_win_r=r, color=True)
    with pytest.raises(ValueError):
        fusion.FusionVideoStream(model, cam, d_candi, vol, t_win_r=r)
