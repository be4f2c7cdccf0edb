"""GPU: the moving volume through the public interface — fusion.TSDFVolume.shift and fusion.FusionVideoStream(follow=distance).
TSDFVolume.shift: offset, origin, the re-pointed attributes, the spill volume's mesh() and points(colors=True) against the restatement
(tests/tsdf_shift_ref.py with the extraction restatements), the triangle partition on the device, a stale spill, and integrate /
raycast / track on a shifted dyadic volume against a freshly built volume at the shifted origin with the same contents.  The window
scenario of tests/test_tsdf_shift_host.py through ops.tsdf_integrate and TSDFVolume.shift against the static volume.  The stream, on the
smallest configuration of tests/test_gpu_fusion_stream.py (r = 1) with its camera translating so that the volume moves twice, against
the loop written out by hand — eager, pipelined, with colour, with tracking; the history across a shift; follow=None."""
import functools

import numpy as np
import pytest
import torch

import icp_ref as ir
import test_gpu_fusion_consistency as fcons
import test_gpu_fusion_repose as frp
import test_gpu_fusion_stream as fsn
import test_gpu_video as tv
import tsdf_color_ref as cref
import tsdf_mesh_ref as mref
import tsdf_ref as ref
import tsdf_shift_ref as sr
from neuralrgbd_amd import fusion, ops, video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 1
FOLLOW = dict(follow=2.0, follow_margin=0.25, follow_step=8)


def _fill(vol, planes):
    vol._buf.copy_(torch.from_numpy(np.ascontiguousarray(planes).view(np.int32)).to(DEV).view(torch.float32))


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32) if t.dtype == torch.float32 else t.detach().cpu().numpy()


# ---- TSDFVolume.shift ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _colour_fixture():
    T, Wt, C = cref.fused("front", ref.PLANE_GRID, ref.PLANE_SIZE, "x4")[-1]
    case = ref.make_case("front", ref.PLANE_GRID, ref.PLANE_SIZE)
    return np.concatenate([np.stack([T, Wt]), C]).astype(np.float32), case["origin"], case["vs"]


@pytest.mark.parametrize("s", [(8, 0, 0), (-4, 5, 0), (3, -6, 7)], ids=str)
def test_shift_moves_the_volume_and_hands_out_the_spill(s):
    planes, origin, vs = _colour_fixture()
    vol = fusion.TSDFVolume(ref.PLANE_GRID, vs, origin, device=DEV, color=True)
    _fill(vol, planes)
    assert vol._spare is None and vol.offset == (0, 0, 0) and vol.shift((0, 0, 0), spill=True) is None and vol._spare is None
    old_mesh = vol.mesh(w_min=1.0)
    first, tsdf_before = vol._buf, vol.tsdf
    spill = vol.shift(s, spill=True)
    want_dst, want_src = sr.shift(planes, s, spill=True)
    assert vol.offset == s and vol.origin == tuple(o + vs * k for o, k in zip(origin, s)) and spill.origin == tuple(origin)
    assert vol._spare is first and spill._buf is first and tsdf_before.data_ptr() == spill.tsdf.data_ptr()
    assert vol.tsdf.data_ptr() == vol._buf[0].data_ptr() and vol.weight.data_ptr() == vol._buf[1].data_ptr()
    assert vol.color.data_ptr() == vol._buf[2].data_ptr() and spill.color.data_ptr() == first[2].data_ptr()
    assert np.array_equal(_bits(vol._buf), sr.bits(want_dst)) and np.array_equal(_bits(spill._buf), sr.bits(want_src))
    # the spill is an ordinary volume to the extractions
    v, f, c, (nv, nf) = spill.mesh(w_min=1.0, colors=True)
    wv, wf = mref.mesh(want_src[0], want_src[1], origin, vs, 1.0)
    wc = cref.extract(np.float32, want_src[0], want_src[1], want_src[2:], 1.0)
    assert (nv, nf) == (len(wv), len(wf)) and np.array_equal(_bits(v), sr.bits(wv)) and np.array_equal(_bits(f), wf)
    assert np.array_equal(_bits(c), sr.bits(wc))
    p, pc, found = spill.points(w_min=1.0, colors=True)
    assert found == len(wv) and np.array_equal(_bits(p), sr.bits(wv)) and np.array_equal(_bits(pc), sr.bits(wc))
    # the partition, on the device
    live = vol.mesh(w_min=1.0)
    print("[follow] shift %s: triangles old %d = spill %d + live %d" % (s, len(old_mesh[1]), nf, len(live[1])))
    assert len(old_mesh[1]) == nf + len(live[1]) and nf > 0 and len(live[1]) > 0
    tri = lambda m: sr.triangles(m[0].cpu().numpy(), m[1].cpu().numpy())
    assert np.isin(tri((v, f)), tri(old_mesh)).all()
    depth = spill.raycast(np.eye(4), ir.CORNER["K"], (48, 64))
    assert tuple(depth.shape) == (48, 64)
    # the next shift reuses the buffer: the spill is stale
    assert vol.shift((-1, 0, 0)) is None and vol._buf is first and vol.offset == (s[0] - 1, s[1], s[2])
    for call in (lambda: spill.mesh(), lambda: spill.points(), lambda: spill.raycast(np.eye(4), ir.CORNER["K"], (48, 64))):
        with pytest.raises(ValueError, match="stale"):
            call()


def test_a_shifted_volume_is_an_ordinary_volume_at_the_shifted_origin():
    """integrate, raycast and track, bit for bit, on a dyadic lattice (origin0 + vs * offset is then exact in fp32 too)."""
    C = ir.CORNER
    vs, origin, s = 2.0 ** -4, (-1.5, -1.5, 0.0), (8, -4, 4)
    T, Wt = ir.corner_field(C["dims"], origin, vs, 3 * vs, C["planes"])
    rng = np.random.RandomState(3)
    planes = np.concatenate([np.stack([T, Wt]), rng.rand(3, *T.shape).astype(np.float32)])
    moved = fusion.TSDFVolume(C["dims"], vs, origin, trunc=3 * vs, device=DEV, color=True)
    _fill(moved, planes)
    moved.shift(s)
    fresh = fusion.TSDFVolume(C["dims"], vs, tuple(o + vs * k for o, k in zip(origin, s)), trunc=3 * vs, device=DEV, color=True)
    assert fresh.origin == moved.origin
    fresh._buf.copy_(moved._buf)
    truth, guess = ir.corner_poses()
    outs = [v.raycast(truth, C["K"], C["size"], normals=True, color=True) for v in (moved, fresh)]
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    depth = outs[0][0].clone()
    assert int((depth > 0).sum()) > 1000
    res = [v.track(depth, guess, C["K"]) for v in (moved, fresh)]
    assert res[0].ok == res[1].ok and np.array_equal(res[0].extM, res[1].extM) and res[0].flag == res[1].flag
    image = torch.rand(3, *C["size"], device=DEV)
    for v in (moved, fresh):
        assert v.integrate(depth, truth, C["K"], color=image)
    frp._same_buf(moved, fresh)


def test_a_window_that_follows_the_camera_equals_the_static_volume():
    sc = sr.window_scenario()
    static = fusion.TSDFVolume(sr.STATIC_DIMS, sr.VS, sr.WINDOW_ORIGIN, trunc=sr.WINDOW_TRUNC, device=DEV)
    live = fusion.TSDFVolume(sr.WINDOW_DIMS, sr.VS, sr.WINDOW_ORIGIN, trunc=sr.WINDOW_TRUNC, device=DEV)
    spills = []
    for extM, depth, at in sc["views"]:
        if at != live.offset[0]:
            old = live.offset[0]
            spill = live.shift((at - old, 0, 0), spill=True)
            spills.append((old, spill._buf.clone()))
        d = torch.from_numpy(depth).to(DEV)
        for vol in (live, static):
            ops.tsdf_integrate(vol.tsdf, vol.weight, vol.origin, vol.voxel_size, d, extM, sr.WINDOW_K, vol.trunc, sr.WINDOW_RANGE)
    assert len(spills) == 8 and live.offset == (sr.STATIC_DIMS[0] - sr.WINDOW_DIMS[0], 0, 0)
    want = static._buf.view(torch.int32)
    for at, spill in spills:
        assert torch.equal(spill.view(torch.int32)[:, :, :, :sr.WINDOW_STEP], want[:, :, :, at:at + sr.WINDOW_STEP])
        assert (spill[1, :, :, :sr.WINDOW_STEP] > 0).any()
    off = live.offset[0]
    assert torch.equal(live._buf.view(torch.int32), want[:, :, :, off:off + sr.WINDOW_DIMS[0]]) and int((live.weight > 0).sum()) > 100


# ---- FusionVideoStream(follow=...) --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _hand():
    """The sequence of tests/test_gpu_video.py at r = 1 with the camera carried 0.9 m further along world x at every frame, and per
    reference frame the maps of a bare eager VideoDepthStream and the picture its ring slot held."""
    frames, _, extMs = tv._sequence(R)
    moved = []
    for i, m in enumerate(extMs):
        t = np.eye(4)
        t[0, 3] = -0.9 * i                                          # world -> the frame the original pose was given in
        moved.append(np.asarray(m, np.float64) @ t)
    model, cam, d_candi = tv._model(R)
    vs = video.VideoDepthStream(model, cam, d_candi, t_win_r=R, copy_outputs=True, use_graph=False)
    maps, pictures = {}, {}
    for f, e in zip(frames, moved):
        out = vs.push(f, e)
        if out is not None:
            maps[out[0]] = (out[1].clone(), out[2].clone())
            pictures[out[0]] = vs.ring[out[0] % vs.R].clone()
    torch.cuda.synchronize()
    vs.check()
    return frames, moved, maps, pictures, (vs.mean, vs.std, vs.H, vs.W)


def _volume(color=False):
    return fusion.TSDFVolume(fsn.DIMS, fsn.VOXEL, fsn.ORIGIN, device=DEV, color=color)


def _host(t):
    return tuple(a.cpu().numpy() for a in t)


def _hand_follow(vol, color, track, spill="mesh"):
    """The loop written out: VideoDepthStream's maps, then follow_shift, shift, the extraction and integrate -> (chunks, shifts)."""
    frames, extMs, maps, pictures, (mean, std, H, W) = _hand()
    cam, d_candi = tv.gt.setup()
    chunks, shifts, prev = [], [], None
    for ci in sorted(maps):
        depth = fsn._regress(maps[ci][0][0], d_candi)[0]
        pushed = np.asarray(extMs[ci], np.float64)
        pose = pushed
        if track and prev is not None:
            pose = pushed @ np.linalg.solve(prev[0], prev[1])
        s = fusion.follow_shift(pose, vol, FOLLOW["follow"], FOLLOW["follow_margin"], FOLLOW["follow_step"])
        if s != (0, 0, 0):
            out = vol.shift(s, spill=True)
            shifts.append((ci, s))
            chunks.append(_host(out.mesh(w_min=1.0, colors=color)[:-1] if spill == "mesh" else out.points(w_min=1.0, colors=color)[:-1]))
        if track and prev is not None:
            pose = vol.track(depth, pose, cam, depth_range=fsn.DEPTH_RANGE).extM
        kw = dict(color=pictures[ci], color_intrinsics=fusion.intrinsics_at(cam, H, W), color_affine=(std, mean)) if color else {}
        assert vol.integrate(depth, pose, cam, depth_range=fsn.DEPTH_RANGE, **kw)
        prev = (pushed, np.asarray(pose, np.float64))
    return chunks, shifts


def _same_chunks(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert isinstance(x, np.ndarray) and x.dtype == y.dtype and np.array_equal(x.view(np.int32), y.view(np.int32))


MODES = {"eager": dict(use_graph=False), "pipeline": dict(use_graph=True, pipeline=True)}


@pytest.mark.parametrize("mode,color,track", [("eager", False, False), ("pipeline", False, False), ("eager", True, False),
                                              ("pipeline", True, False), ("eager", False, True), ("pipeline", True, True)])
def test_following_stream_equals_the_hand_written_loop(mode, color, track):
    frames, extMs, maps, _, _ = _hand()
    want = _volume(color)
    chunks, shifts = _hand_follow(want, color, track)
    print("[follow] %s colour %d track %d: shifts %s, chunk triangles %s" % (mode, color, track, shifts, [len(c[1]) for c in chunks]))
    assert len(shifts) >= 2 and sum(len(c[1]) for c in chunks) > 0
    vol = _volume(color)
    fs, outs = fsn._stream(R, frames, extMs, vol, color=color, track=track, **FOLLOW, **MODES[mode])
    if MODES[mode]["use_graph"]:
        assert fs.stream._graph is not None, fs.stream.graph_error
    fsn._same_maps(outs, maps)                                      # following perturbs nothing of the network's
    assert fs.n_shifts == len(shifts) and vol.offset == want.offset == tuple(sum(s[k] for _, s in shifts) for k in range(3))
    assert vol.origin == want.origin and fs.n_integrated == len(maps)
    frp._same_buf(vol, want)
    _same_chunks(fs.chunks, chunks)
    got = fs.world_mesh()
    live = _host(want.mesh(w_min=1.0, colors=color)[:-1])
    parts = chunks + [live]
    base = np.cumsum([0] + [len(p[0]) for p in parts[:-1]])
    assert len(got) == (3 if color else 2) and got[1].dtype == np.int32
    assert np.array_equal(got[0].view(np.int32), np.concatenate([p[0] for p in parts]).view(np.int32))
    assert np.array_equal(got[1], np.concatenate([p[1] + b for p, b in zip(parts, base)]))
    if color:
        assert np.array_equal(got[2].view(np.int32), np.concatenate([p[2] for p in parts]).view(np.int32))
    assert len(live[1]) > 0 and got[1].max() < len(got[0])
    pts = fs.world_points()
    assert len(pts) == (2 if color else 1) and np.array_equal(pts[0].view(np.int32), got[0].view(np.int32))
    fs.reset()
    assert len(fs.chunks) == len(chunks) and fs.n_shifts == len(shifts)      # the chunks stay, like the volume


def test_points_chunks_and_a_callable():
    frames, extMs, maps, _, _ = _hand()
    want = _volume()
    chunks, shifts = _hand_follow(want, False, False, spill="points")
    vol = _volume()
    fs, _ = fsn._stream(R, frames, extMs, vol, follow_spill="points", use_graph=False, **FOLLOW)
    _same_chunks(fs.chunks, chunks)
    frp._same_buf(vol, want)
    with pytest.raises(ValueError):
        fs.world_mesh()
    live = want.points(w_min=1.0)[0].cpu().numpy()
    assert np.array_equal(fs.world_points()[0].view(np.int32), np.concatenate([c[0] for c in chunks] + [live]).view(np.int32))
    seen = []
    for spill in (lambda v: seen.append((v.origin, int(v.points()[1]))), None):
        vol = _volume()
        fs, _ = fsn._stream(R, frames, extMs, vol, follow_spill=spill, use_graph=False, **FOLLOW)
        frp._same_buf(vol, want)
        assert fs.chunks == [] and fs.n_shifts == len(shifts)
    assert len(seen) == len(shifts) and seen[0][0] == tuple(fsn.ORIGIN)


def test_the_history_across_a_shift():
    """A frame integrated before a shift cannot be reposed any more; it still votes in the consistency filter."""
    frames, extMs, maps, _, _ = _hand()
    vol = _volume()
    fs, _ = fsn._stream(R, frames, extMs, vol, history=fcons.HISTORY, consistency=fcons.VIEWS, consistency_rel=fcons.REL, track=True,
                        use_graph=False, **FOLLOW)
    assert fs.n_shifts >= 2
    held = [i for i, _ in fs.history_poses()]
    before = [i for i in held if [h.shifts for h in fs._held if h.ref_index == i][0] != fs.n_shifts]
    after = [i for i in held if i not in before]
    print("[follow] history: held %s, integrated before the last shift %s" % (held, before))
    assert before and after == held[len(before):]
    keep = frp._copy(vol)
    for i in before:
        with pytest.raises(ValueError, match="before the volume shifted"):
            fs.repose(i, frp._moved(extMs[i], 1))
        with pytest.raises(ValueError, match="before the volume shifted"):
            fs.retrack(i)
    assert torch.equal(vol._buf.view(torch.int32), keep._buf.view(torch.int32))
    assert fs.repose(after[-1], frp._moved(fs.history_poses()[-1][1], 2))
    assert not torch.equal(vol._buf.view(torch.int32), keep._buf.view(torch.int32))


def test_a_pre_shift_frame_is_still_a_consistency_source():
    frames, extMs, maps, _, _ = _hand()
    vol = _volume()
    fs, _ = fsn._stream(R, frames, extMs, vol, history=fcons.HISTORY, consistency=fcons.VIEWS, consistency_rel=fcons.REL, use_graph=False,
                        **FOLLOW)
    order = sorted(maps)
    last = order[-1]
    sources = order[max(0, len(order) - 1 - fcons.HISTORY):-1]       # the frames held when the last one came out
    assert fs.n_shifts >= 2 and [h.shifts for h in fs._held if h.ref_index == sources[1]][0] < fs.n_shifts
    want = fcons._hand_filter(maps, last, sources, {i: extMs[i] for i in order}, 0.0)[0]
    assert torch.equal(fs.last_votes.view(torch.int32), want.view(torch.int32)) and float(want.max()) >= 1


def test_follow_none_is_the_stream_without_the_argument():
    frames, extMs, maps, _, _ = _hand()
    runs = []
    for extra in ({}, dict(follow=None), dict(follow=None, follow_margin=0.4, follow_step=4, follow_spill=None, follow_w_min=3.0)):
        vol = _volume()
        fs, outs = fsn._stream(R, frames, extMs, vol, use_graph=False, **extra)
        fsn._same_maps(outs, maps)
        assert fs.follow is None and fs.n_shifts == 0 and fs.chunks == [] and vol._spare is None and vol.offset == (0, 0, 0)
        assert vol.origin == tuple(fsn.ORIGIN) and [h.shifts for h in fs._held if h.shifts] == []
        runs.append(vol)
    for vol in runs[1:]:
        frp._same_buf(vol, runs[0])
    assert int((runs[0].weight > 0).sum()) > 1000
    model, cam, d_candi = tv._model(R)
    for kw in (dict(follow=2.0, follow_step=6), dict(follow=2.0, follow_margin=0.5), dict(follow=float("nan")), dict(follow=2.0, follow_spill="ply")):
        with pytest.raises(ValueError):
            fusion.FusionVideoStream(model, cam, d_candi, _volume(), t_win_r=R, **kw)
