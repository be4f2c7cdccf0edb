"""GPU: FusionVideoStream.render — the fused model ray-cast from the stream — on the tiny model, windows and synthetic sequence of
tests/test_gpu_fusion_stream.py: render() after every push equals ops.tsdf_raycast on the stream's volume at the extrinsic pushed with
the last integrated frame, bit for bit (eager, hipGraph, pipelined with flush()); the stream's maps and volume are the same bits with
and without render calls in between; a render launches one kernel, the library's; evaluate.DepthMetrics scores a rendered map."""
import numpy as np
import pytest
import torch

import test_gpu_fusion_stream as fsm
import test_gpu_video as tv
import tsdf_raycast_ref as rc
import tsdf_ref as ref
from neuralrgbd_amd import evaluate, fusion, ops
from test_gpu_tsdf import _run_plane

pytestmark = pytest.mark.gpu
DEV = fsm.DEV


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("mode", ["eager", "graph", "pipeline"])
def test_render_equals_raycast_at_the_last_integrated_extrinsic(mode):
    r, frames, extMs, maps = fsm._hand(1)
    kw = fsm.SETTINGS[mode][0]
    model, cam, d_candi = tv._model(r)
    vol = fsm._volume()
    fs = fusion.FusionVideoStream(model, cam, d_candi, vol, t_win_r=r, depth_range=fsm.DEPTH_RANGE, copy_outputs=True, **kw)
    with pytest.raises(ValueError, match="no frame has been integrated"):
        fs.render()
    K = fusion.intrinsics_at(cam, fs.H, fs.W)
    outs, rendered, hits = {}, 0, 0

    def note(o):
        nonlocal rendered, hits
        if o is None:
            return
        outs[o[0]] = (o[1].clone(), o[2].clone())
        depth, normal = fs.render(normals=True)
        want = ops.tsdf_raycast(vol.tsdf, vol.weight, vol.origin, vol.voxel_size, extMs[o[0]], K, (fs.H, fs.W), fsm.DEPTH_RANGE, normals=True)
        assert _same(depth, want[0]) and _same(normal, want[1]), "render after frame %d" % o[0]
        assert tuple(depth.shape) == (fs.H, fs.W) and _same(fs.render(), want[0])
        rendered += 1
        hits += int((depth > 0).sum())
    for f, e in zip(frames, extMs):
        note(fs.push(f, e))
    note(fs.flush())
    torch.cuda.synchronize()
    fs.check()
    if kw["use_graph"]:
        assert fs.stream._graph is not None, fs.stream.graph_error
    assert rendered == len(maps) == fs.n_integrated and hits > 0
    # another pose, size and parameters go through to the ray cast
    small = fs.render(extM=extMs[0], size=(17, 15), w_min=2.0, step=vol.voxel_size / 2)
    want = ops.tsdf_raycast(vol.tsdf, vol.weight, vol.origin, vol.voxel_size, extMs[0], fusion.intrinsics_at(cam, 17, 15), (17, 15),
                            fsm.DEPTH_RANGE, w_min=2.0, step=vol.voxel_size / 2)
    assert _same(small, want)
    # the same maps and the same volume as a stream that never rendered
    bare_vol = fsm._volume()
    _, bare = fsm._stream(r, frames, extMs, bare_vol, **kw)
    fsm._same_maps(outs, maps)
    fsm._same_maps(bare, maps)
    fsm._same_volume(vol, bare_vol)


def test_a_render_launches_one_kernel_of_the_library():
    from torch.profiler import ProfilerActivity, profile
    r, frames, extMs, _ = fsm._hand(1)
    model, cam, d_candi = tv._model(r)
    fs = fusion.FusionVideoStream(model, cam, d_candi, fsm._volume(), t_win_r=r, depth_range=fsm.DEPTH_RANGE, use_graph=False)
    for f, e in zip(frames, extMs):
        fs.push(f, e)
    fs.render(normals=True)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fs.render(normals=True)
        fs.render()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
             and "memset" not in e.name.lower()]
    assert len(names) == 2 and all("nrgbd::" in n and "tsdf_raycast_kernel" in n for n in names), names


def test_depth_metrics_score_a_rendered_map():
    """Misses (depth 0) count as bad, coverage = hits / gt-valid pixels."""
    case, vol = _run_plane(True)
    size = ref.PLANE_SIZE
    m, K = rc.held_out(case["views"][0]["extM"]), rc.render_K(*size)
    depth = vol.raycast(m, K, size, depth_range=(0.3, 3.0))
    gt = torch.from_numpy(ref.plane_depth(m, K, *size)).to(DEV)
    metrics = evaluate.DepthMetrics(device=DEV)
    metrics.update(depth, torch.zeros_like(depth), gt)
    res = metrics.result()[0]
    hits = int((depth > 0).sum())
    assert res["gt_valid"] == depth.numel() and res["n"] == hits and 0 < hits < depth.numel()
    assert res["coverage"] == hits / depth.numel() and res["bad"] == (depth.numel() - hits) / depth.numel()
    assert res["mae"] <= 0.25 * case["vs"]                          # every hit lies within the gate of the plane
