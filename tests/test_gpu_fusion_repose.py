"""GPU: fusion.FusionVideoStream(history=N) — the maps of the last N integrated frames kept on the device, `repose` and `retrack` — on the
smallest configuration of tests/test_gpu_fusion_stream.py (r = 1, its model, sizes and synthetic sequence).  The history perturbs
neither the maps nor the volume; `repose` is the hand-written TSDFVolume.reintegrate and `retrack` the hand-written deintegrate /
track / integrate, bit for bit on every plane, eager and pipelined, with colour; a trajectory pushed with perturbed poses and reposed
to the true ones gives the volume of the true poses inside a bound derived below; eviction, reset; no kernel of another library."""
import numpy as np
import pytest
import torch

import test_gpu_fusion_color as fcol
import test_gpu_fusion_stream as fsn
import test_gpu_video as tv
import tsdf_ref as ref
from neuralrgbd_amd import fusion, synth, video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 1
U = ref.U


def _copy(vol):
    out = fusion.TSDFVolume(vol.dims, vol.voxel_size, vol.origin, trunc=vol.trunc, w_max=vol.w_max, device=DEV, color=vol.color is not None)
    out._buf.copy_(vol._buf)
    return out


def _same_buf(a, b, what=""):
    assert torch.equal(a._buf.view(torch.int32), b._buf.view(torch.int32)), "the volumes differ " + what


def _moved(extM, k):
    return synth.random_pose(np.random.RandomState(70 + k), 0.02, 0.03) @ np.asarray(extM, np.float64)


def _frame_maps(maps, ci, weight, c):
    """What the stream integrates frame ci with, from the bare stream's maps: (depth, keywords of integrate / reintegrate)."""
    d_candi = tv.gt.setup()[1]
    v = maps[ci][0][0]
    depth, logconf, d_dev, cl = fsn._regress(v, d_candi)
    thr = None if c == 0 else float(np.log(np.float64(c)).astype(np.float32))
    wmap = fsn.ops.export_depth_u16(v, d_dev, channels_last=cl)[1] if weight == "conf" else None
    return depth, dict(gate=None if thr is None else logconf, gate_thr=thr, weight=wmap, depth_range=fsn.DEPTH_RANGE)


def _colour_kw(ci):
    pictures, (mean, std, H, W) = fcol._hand(R)[3:]
    return dict(color=pictures[ci], color_intrinsics=fusion.intrinsics_at(tv.gt.setup()[0], H, W), color_affine=(std, mean))


MODES = {"eager": (dict(use_graph=False), "uniform", False, False), "pipeline": (dict(use_graph=True, pipeline=True), "conf", True, True)}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_history_leaves_maps_and_volume_alone_and_holds_the_last_frames(mode):
    r, frames, extMs, maps = fsn._hand(R)
    kw, weight, gated, color = MODES[mode]
    c = fsn._median_confidence(maps, "refined", tv.gt.setup()[1]) if gated else 0.0
    kw = dict(kw, weight=weight, conf_threshold=c, color=color)
    bare, held = fcol._volume(color), fcol._volume(color)
    fs0, outs0 = fsn._stream(r, frames, extMs, bare, **kw)
    fs, outs = fsn._stream(r, frames, extMs, held, history=2, **kw)
    fsn._same_maps(outs, maps)
    fsn._same_maps(outs0, maps)
    _same_buf(held, bare)
    assert fs0.history == 0 and fs0._slots is None and fs0.history_poses() == []       # nothing constructed
    got = fs.history_poses()
    last = sorted(maps)[-2:]
    assert [i for i, _ in got] == last and all(np.array_equal(m, np.asarray(extMs[i], np.float64)) for i, m in got)
    for ci in last:                                                 # the slots hold what the frame was integrated with
        h, depth, hkw = fs._held_frame(ci, "test")
        want_depth, want = _frame_maps(maps, ci, weight, c)
        assert torch.equal(depth.view(torch.int32), want_depth.view(torch.int32))
        for key in ("gate", "weight"):
            assert (hkw[key] is None) == (want[key] is None)
            assert want[key] is None or torch.equal(hkw[key].view(torch.int32), want[key].view(torch.int32))
        assert hkw["gate_thr"] == want["gate_thr"]
        if color:
            assert torch.equal(hkw["color"], _colour_kw(ci)["color"])
    assert {k for k, v in fs._slots.items() if v is not None} == {"depth"} | ({"gate", "wmap", "image"} if gated else set())
    with pytest.raises(ValueError):
        fusion.FusionVideoStream(tv._model(r)[0], *tv.gt.setup(), fsn._volume(), t_win_r=r, history=-1)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_repose_equals_the_hand_written_reintegrate(mode):
    r, frames, extMs, maps = fsn._hand(R)
    kw, weight, gated, color = MODES[mode]
    c = fsn._median_confidence(maps, "refined", tv.gt.setup()[1]) if gated else 0.0
    vol = fcol._volume(color)
    fs, _ = fsn._stream(r, frames, extMs, vol, history=len(maps), weight=weight, conf_threshold=c, color=color, **kw)
    cam = tv.gt.setup()[0]
    order = sorted(maps)
    poses = {ci: np.asarray(extMs[ci], np.float64) for ci in order}
    for n, ci in enumerate((order[1], order[-1], order[1], order[0])):      # a frame in the middle (twice: from its new pose on), the last
        new = _moved(extMs[ci], n)
        want = _copy(vol)
        depth, hkw = _frame_maps(maps, ci, weight, c)
        if color:
            hkw.update(_colour_kw(ci))
        assert want.reintegrate(depth, poses[ci], new, cam, **hkw)
        before = fs.last_ext.copy()
        assert fs.repose(ci, new) is True
        _same_buf(vol, want, "after repose(%d)" % ci)
        poses[ci] = new
        assert [i for i, _ in fs.history_poses()] == order
        assert all(np.array_equal(m, poses[i]) for i, m in fs.history_poses())
        assert np.array_equal(fs.last_ext, new if ci == order[-1] else before)
    assert int((vol.weight > 0).sum()) > 1000                       # the sequence lies inside the volume
    with pytest.raises(KeyError):
        fs.repose(99, extMs[0])
    with pytest.raises(ValueError):
        fs.repose(order[0], np.full((4, 4), np.nan))


def test_eviction_and_reset():
    r, frames, extMs, maps = fsn._hand(R)
    vol = fsn._volume()
    fs, _ = fsn._stream(r, frames, extMs, vol, history=2, use_graph=False)
    order = sorted(maps)
    before = vol._buf.clone()
    for ci in order[:-2]:
        with pytest.raises(KeyError):                               # fell out of the history: fused for good
            fs.repose(ci, extMs[ci])
    with pytest.raises(ValueError):
        fs.retrack(order[-1])                                       # track=False
    assert torch.equal(before.view(torch.int32), vol._buf.view(torch.int32))
    assert fs.repose(order[-1], _moved(extMs[order[-1]], 0)) and not torch.equal(before.view(torch.int32), vol._buf.view(torch.int32))
    slots = fs._slots["depth"].data_ptr()
    fs.reset()
    assert fs.history_poses() == []
    with pytest.raises(KeyError):
        fs.repose(order[-1], extMs[order[-1]])
    assert fusion.fuse_sequence(fs, frames, extMs) == len(maps)     # the next trajectory fills the same slots
    assert [i for i, _ in fs.history_poses()] == order[-2:] and fs._slots["depth"].data_ptr() == slots


def test_reposing_every_frame_to_its_true_pose_gives_the_volume_of_the_true_poses():
    """The trajectory pushed with perturbed poses, every held frame reposed to the pose it should have had: against the volume that
    integrates the SAME maps (the network saw the perturbed poses) at the true ones.  Uniform weights: every weight is an exact
    integer, so the weights are equal bit for bit (their summation bound is 0) and no voxel saturates (5 frames, w_max = 64).  T: per
    voxel, with e the distance of the stored value to the exact weighted mean of its current observations (tsdf_deint_ref's header;
    d = 0 here), the initial fusion gives e = 8 u W; a removal at weight W gives e <- amp (e + 2 u) + 3 u with amp = (W + 1) / (W - 1)
    — or exactly 0 when W = 1: the voxel is emptied —, an addition e <- e + 8 u; the volume of the true poses is within 8 u W of the
    same mean.  The masks are tsdf_ref.chain's on the downloaded maps."""
    r, frames, extMs, _ = fsn._hand(R)
    cam = tv.gt.setup()[0]
    off = [_moved(m, 10 + i) for i, m in enumerate(extMs)]
    vol = fsn._volume()
    fs, outs = fsn._stream(r, frames, off, vol, history=len(frames), use_graph=False)
    want = fsn._volume()
    fsn._hand_integrate(want, outs, extMs, "refined", "uniform", 0.0)
    order = sorted(outs)
    assert [i for i, _ in fs.history_poses()] == order
    d_candi = tv.gt.setup()[1]
    X, Y, Z = fsn.DIMS
    W = vol.weight.cpu().numpy().astype(np.float64)
    e = 8 * U * W
    for ci in order:
        depth = fsn._regress(outs[ci][0][0], d_candi)[0]
        K = fusion.intrinsics_at(cam, *depth.shape)
        obs = [ref.chain(np.float32, fsn.DIMS, fsn.ORIGIN, fsn.VOXEL, np.float32(np.asarray(m, np.float64)[:3, :4]), K, depth.cpu().numpy(),
                         vol.trunc, fsn.DEPTH_RANGE[0], fsn.DEPTH_RANGE[1])["ok"] for m in (off[ci], extMs[ci])]
        assert fs.repose(ci, extMs[ci])
        with np.errstate(all="ignore"):
            amp = np.where(W > 1, (W + 1) / (W - 1), 0.0)
        e = np.where(obs[0], np.where(W > 1, amp * (e + 2 * U) + 3 * U, 0.0), e)
        W = W - obs[0]
        e = np.where(obs[1], e + 8 * U, e)
        W = W + obs[1]
    assert torch.equal(vol.weight.view(torch.int32), want.weight.view(torch.int32))
    assert np.array_equal(W, want.weight.cpu().numpy()) and W.max() < 64
    diff = np.abs(vol.tsdf.cpu().numpy().astype(np.float64) - want.tsdf.cpu().numpy())
    bound = 1.01 * (e + 8 * U * W)
    print("[fusion-repose] %d voxels, worst |dT| %.1f u, worst share of the bound %.3f"
          % (int((W > 0).sum()), diff.max() / U, (diff / np.maximum(bound, 1e-30))[W > 0].max()))
    assert (W > 0).sum() > 1000 and (diff <= bound).all()
    assert not vol.tsdf[vol.weight == 0].any()
    assert all(np.array_equal(m, np.asarray(extMs[i], np.float64)) for i, m in fs.history_poses())


def test_retrack_equals_the_three_hand_written_calls():
    """De-integrate, track against what remains, integrate at the tracked pose — or, lost, back at the stored one: bit for bit, both
    branches (min_frac = 2 cannot be met: that call is lost whatever the maps are), and after a lost retrack the volume differs
    from before by rounding only: the removal's own roundings scaled by amp, 2 u amp + 3 u, and the addition's 8 u; the weights
    (uniform) exactly."""
    r, frames, extMs, maps = fsn._hand(R)
    cam = tv.gt.setup()[0]
    vol = fsn._volume()
    fs, _ = fsn._stream(r, frames, extMs, vol, history=len(maps), track=True, use_graph=False)
    order = sorted(maps)
    flags = []
    for ci, tkw in ((order[2], {}), (order[-1], {}), (order[1], dict(min_frac=2.0)), (order[-1], dict(min_frac=2.0))):
        old = dict(fs.history_poses())[ci]
        depth, hkw = _frame_maps(maps, ci, "uniform", 0.0)
        before = _copy(vol)
        want = _copy(vol)
        assert want.deintegrate(depth, old, cam, **hkw)
        res = want.track(depth, old, cam, depth_range=fsn.DEPTH_RANGE, **tkw)
        pose = res.extM if res.ok else old
        assert want.integrate(depth, pose, cam, **hkw)
        prev = None if fs._prev is None else (fs._prev[0].copy(), fs._prev[1].copy())
        got = fs.retrack(ci, **tkw)
        assert got.ok == res.ok and got.flag == res.flag and np.array_equal(got.extM, res.extM)
        _same_buf(vol, want, "after retrack(%d)" % ci)
        assert np.array_equal(dict(fs.history_poses())[ci], pose)
        if ci == order[-1]:
            assert np.array_equal(fs.last_ext, pose) and np.array_equal(fs._prev[1], pose) and np.array_equal(fs._prev[0], prev[0])
        else:
            assert np.array_equal(fs._prev[1], prev[1])
        flags.append(bool(res.ok))
        if not res.ok:
            assert torch.equal(vol.weight.view(torch.int32), before.weight.view(torch.int32))
            W = before.weight.cpu().numpy().astype(np.float64)
            with np.errstate(all="ignore"):
                amp = np.where(W > 1, (W + 1) / (W - 1), 0.0)
            diff = np.abs(vol.tsdf.cpu().numpy().astype(np.float64) - before.tsdf.cpu().numpy())
            assert (diff <= 1.01 * U * (2 * amp + 11)).all()
    print("[fusion-repose] retrack flags %s" % flags)
    assert True in flags and False in flags


def test_a_history_push_and_a_repose_launch_no_kernel_of_another_library():
    """The check of tests/test_gpu_fusion_stream.py: every kernel of a steady-state push with a history (gate, weight map and
    picture held: filling the slots is memory copies) and of a repose is a kernel of the library (nrgbd::) or one the bare
    VideoDepthStream launches as well."""
    from torch.profiler import ProfilerActivity, profile
    import neuralrgbd_amd
    r, frames, extMs, _ = fsn._hand(R)
    cam = tv.gt.setup()[0]
    d_candi = np.linspace(tv.gt.TWIN["d_min"], tv.gt.TWIN["d_max"], 64)
    model = neuralrgbd_amd.KVNET(64, cam, d_candi, tv.gt.TWIN["sigma"], 64, None, if_refined=True, refineNet_name="DPV", t_win_r=r)
    model.load_state_dict(synth.seeded_state_dict(model, tv.gt.TWIN["weight_seed"]))
    model = model.to(DEV)
    streams = {"plain": video.VideoDepthStream(model, cam, d_candi, t_win_r=r, use_graph=False),
               "history": fusion.FusionVideoStream(model, cam, d_candi, fcol._volume(True), t_win_r=r, weight="conf", conf_threshold=0.05,
                                                   depth_range=fsn.DEPTH_RANGE, use_graph=False, color=True, history=2)}
    kernels = lambda prof: {e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                            and "memset" not in e.name.lower()}
    names = {}
    for key, s in streams.items():
        for f, e in zip(frames[:-1], extMs[:-1]):                   # caches warm, the slots allocated and all in use
            s.push(f, e)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            out = s.push(frames[-1], extMs[-1])
            torch.cuda.synchronize()
        assert out is not None
        names[key] = kernels(prof)
    fs = streams["history"]
    held = [i for i, _ in fs.history_poses()]
    assert fs.n_integrated == len(frames) - 2 * r and len(held) == 2
    new = names["history"] - names["plain"]
    assert any("tsdf_integrate_kernel" in n for n in new) and len(names["plain"]) > 5
    assert not sorted(n for n in new if "nrgbd::" not in n), sorted(new)
    fs.repose(held[0], _moved(extMs[held[0]], 3))                   # once outside the trace: nothing left to load
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fs.repose(held[1], _moved(extMs[held[1]], 4))
        torch.cuda.synchronize()
    moved = kernels(prof)
    assert any("tsdf_reintegrate_kernel" in n for n in moved) and all("nrgbd::" in n for n in moved), sorted(moved)
