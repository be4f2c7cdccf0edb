"""GPU: the paged moving volume through the public interface — fusion.TSDFVolume.shift(store=...), fusion.paged_extract and
fusion.FusionVideoStream(follow_spill="page").  The out-and-back window scenario of tests/tsdf_page_ref.py through ops.tsdf_integrate
and TSDFVolume.shift(store=...) against the static volume, with the host test's counts.  The tracking corner: a wall that leaves the
window and comes back is there again, bit for bit, and the tracker finds what it found before; without a store it is gone.  The
stream, on the smallest configuration of tests/test_gpu_fusion_follow.py (r = 1) with the camera carried out along world x and back
so that the volume moves twice each way, against the loop written out by hand — eager, pipelined, with colour, with tracking —, its
world mesh against paged_extract of the hand loop and against one large static volume fused from the same maps at the same poses; a
store loaded from a file; the construction refusals; follow_spill='mesh' unchanged on the same sequence."""
import functools
import types

import numpy as np
import pytest
import torch

import icp_ref as ir
import test_gpu_fusion_follow as ff
import test_gpu_fusion_repose as frp
import test_gpu_fusion_stream as fsn
import test_gpu_video as tv
import tsdf_page_ref as pr
import tsdf_shift_ref as sr
from neuralrgbd_amd import fusion, ops, video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 1


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _store_dict(st):
    return {k: st.get([k])[1][0] for k in st.keys()}


# ---- 1. the out-and-back window scenario -------------------------------------------------------------------------------------------

def test_out_and_back_window_with_a_store_equals_the_static_volume():
    static = fusion.TSDFVolume(sr.STATIC_DIMS, sr.VS, sr.WINDOW_ORIGIN, trunc=sr.WINDOW_TRUNC, device=DEV)
    live = fusion.TSDFVolume(sr.WINDOW_DIMS, sr.VS, sr.WINDOW_ORIGIN, trunc=sr.WINDOW_TRUNC, device=DEV)
    st = fusion.BlockStore(2)
    shifts, staging = 0, None
    views = pr.out_and_back()
    for extM, depth, at in views:
        while at != live.offset[0]:
            step = sr.WINDOW_STEP if at > live.offset[0] else -sr.WINDOW_STEP
            assert live.shift((step, 0, 0), store=st) is None
            shifts += 1
            staging = staging or live._page_out
            assert live._page_out is staging
        box = sr.unclipped_box(extM, live.origin, sr.WINDOW_DIMS)   # the condition: the view touches nothing outside the window
        assert min(box[:3]) >= 0 and all(b <= n for b, n in zip(box[3:], sr.WINDOW_DIMS)), (box, live.offset)
        d = torch.from_numpy(depth).to(DEV)
        for vol in (live, static):
            ops.tsdf_integrate(vol.tsdf, vol.weight, vol.origin, vol.voxel_size, d, extM, sr.WINDOW_K, vol.trunc, sr.WINDOW_RANGE)
    counts = dict(shifts=shifts, out=st.n_put, dropped=st.n_dropped, left=len(st), **{"in": st.n_taken})
    print("[page] out and back on the device: %s, %d voxels of the last window with weight >= 2" % (counts, int((live.weight >= 2).sum())))
    assert len(views) == 84 and counts == pr.SCENARIO_COUNTS
    want = _bits(static._buf)
    off = live.offset[0]
    assert live.offset == (0, 0, 0) and live.origin == tuple(sr.WINDOW_ORIGIN)
    assert np.array_equal(_bits(live._buf), want[:, :, :, off:off + sr.WINDOW_DIMS[0]])
    whole, lo = pr.world(live._buf.cpu().numpy(), live.offset, _store_dict(st), bounds=((0, 0, 0), sr.STATIC_DIMS))
    assert lo == (0, 0, 0) and np.array_equal(sr.bits(whole), want)
    assert int((live.weight >= 2).sum()) >= 100
    # the whole world as a mesh: as many triangles as the static volume's, each within 4 ulp of the largest coordinate
    v, f = fusion.paged_extract(live, st, "mesh", w_min=1.0)
    sv, sf, _ = static.mesh(w_min=1.0)
    assert len(f) == len(sf) > 500 and f.dtype == np.int32 and f.max() < len(v)
    a, b = pr.sorted_triangles(v, f), pr.sorted_triangles(sv.cpu().numpy(), sf.cpu().numpy())
    ulp = np.spacing(np.float32(np.abs(b).max()))
    assert np.abs(a.astype(np.float64) - b.astype(np.float64)).max() <= 4 * ulp
    wv, wf, _ = pr.tiled_mesh(pr.tiles(live._buf.cpu().numpy(), live.offset, _store_dict(st), sr.WINDOW_DIMS), sr.WINDOW_ORIGIN, sr.VS, 1.0)
    assert np.array_equal(sr.bits(v), sr.bits(wv)) and np.array_equal(f, wf)
    pts = fusion.paged_extract(live, st, "points", w_min=1.0)
    assert len(pts) == 1 and np.array_equal(sr.bits(pts[0]), sr.bits(v))
    assert len(st) == 13 and np.array_equal(_bits(live._buf), want[:, :, :, off:off + sr.WINDOW_DIMS[0]])     # nothing was modified


# ---- 2. the tracking corner --------------------------------------------------------------------------------------------------------

def test_a_wall_that_left_and_came_back_is_tracked_as_before():
    C = ir.CORNER
    vs, origin = 2.0 ** -4, (-1.5, -1.5, 0.0)
    T, Wt = ir.corner_field(C["dims"], origin, vs, 3 * vs, C["planes"])
    rng = np.random.RandomState(3)
    planes = np.concatenate([np.stack([T, Wt]), rng.rand(3, *T.shape).astype(np.float32)])
    make = lambda: fusion.TSDFVolume(C["dims"], vs, origin, trunc=3 * vs, device=DEV, color=True)
    never, paged, plain = make(), make(), make()
    for v in (never, paged, plain):
        ff._fill(v, planes)
    st = fusion.BlockStore(5)
    paged.shift((-16, 0, 0), store=st)
    assert len(st) == 2 * 6 * 6 and st.n_dropped == 0               # the two block layers beyond x = 0.5, the wall x = 0.9 among them
    assert not torch.equal(paged._buf.view(torch.int32), never._buf.view(torch.int32))
    paged.shift((16, 0, 0), store=st)
    assert len(st) == 0 and st.n_taken == st.n_put == 72 and paged.offset == (0, 0, 0) and paged.origin == never.origin
    frp._same_buf(paged, never, "after out and back with a store")
    plain.shift((-16, 0, 0))
    plain.shift((16, 0, 0))
    assert int((plain.weight > 0).sum()) < int((never.weight > 0).sum())
    assert not torch.equal(plain._buf.view(torch.int32), never._buf.view(torch.int32))
    truth, guess = ir.corner_poses()
    depth = never.raycast(truth, C["K"], C["size"])
    assert int((depth > 0).sum()) > 1000
    want, got = never.track(depth, guess, C["K"]), paged.track(depth, guess, C["K"])
    assert want.ok and got.ok == want.ok and got.flag == want.flag and np.array_equal(got.extM, want.extM)


# ---- 3. FusionVideoStream(follow_spill="page") -------------------------------------------------------------------------------------
# A dyadic lattice (origin0 + voxel offset is then exact in fp32 too), so that the window's voxels are the static volume's bit for bit.
DIMS, VOXEL, ORIGIN = (64, 64, 48), 0.125, (-4.0, -4.0, 0.5)
DEPTH_RANGE = fsn.DEPTH_RANGE                                       # the frustum out to 4.9 m + trunc is 50 voxels wide: inside the window
FOLLOW = dict(follow=3.0, follow_margin=0.125, follow_step=8)
PATH = (0, 15, 31, 15, -1, -1, 0)                                   # the camera's x in voxels, per frame: out and back
W_MIN = 1.0


@functools.lru_cache(maxsize=None)
def _hand():
    """The sequence of tests/test_gpu_video.py at r = 1 with the camera carried along world x by PATH, and per reference frame the
    maps of a bare eager VideoDepthStream and the picture its ring slot held."""
    frames, _, extMs = tv._sequence(R)
    assert len(extMs) == len(PATH)
    moved = []
    for x, m in zip(PATH, extMs):
        t = np.eye(4)
        t[0, 3] = -VOXEL * x
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


def _volume(color=False, dims=DIMS, origin=ORIGIN):
    return fusion.TSDFVolume(dims, VOXEL, origin, device=DEV, color=color)


def _hand_page(vol, st, color, track):
    """The loop written out: VideoDepthStream's maps, then follow_shift, shift(store=...) and integrate -> (shifts, [(ci, depth,
    integrated pose, integrate's keywords)])."""
    frames, extMs, maps, pictures, (mean, std, H, W) = _hand()
    cam, d_candi = tv.gt.setup()
    shifts, fused, prev = [], [], None
    for ci in sorted(maps):
        depth = fsn._regress(maps[ci][0][0], d_candi)[0]
        pushed = np.asarray(extMs[ci], np.float64)
        pose = pushed
        if track and prev is not None:
            pose = pushed @ np.linalg.solve(prev[0], prev[1])
        s = fusion.follow_shift(pose, vol, FOLLOW["follow"], FOLLOW["follow_margin"], FOLLOW["follow_step"])
        if s != (0, 0, 0):
            vol.shift(s, store=st)
            shifts.append((ci, s))
        if track and prev is not None:
            pose = vol.track(depth, pose, cam, depth_range=DEPTH_RANGE).extM
        box = _unclipped_box(vol, pose, cam, H, W)
        assert 0 <= box[0] and box[3] <= DIMS[0], (ci, box)         # along x the frame touches nothing outside the window
        kw = dict(color=pictures[ci], color_intrinsics=fusion.intrinsics_at(cam, H, W), color_affine=(std, mean)) if color else {}
        assert vol.integrate(depth, pose, cam, depth_range=DEPTH_RANGE, **kw)
        fused.append((ci, depth, np.asarray(pose, np.float64), kw))
        prev = (pushed, np.asarray(pose, np.float64))
    return shifts, fused


def _unclipped_box(vol, pose, cam, H, W):
    """fusion.frustum_box without the clip to the grid (a grid grown by 2^12 voxels on every side, moved back)."""
    big = 1 << 12
    grown = types.SimpleNamespace(dims=tuple(n + 2 * big for n in vol.dims), origin=tuple(o - VOXEL * big for o in vol.origin), voxel_size=VOXEL)
    box = fusion.frustum_box(pose, fusion.intrinsics_at(cam, H, W), (H, W), DEPTH_RANGE[1] + vol.trunc, grown)
    return tuple(b - big for b in box)


def _stream(vol, **kw):
    frames, extMs, _, _, _ = _hand()
    model, cam, d_candi = tv._model(R)
    fs = fusion.FusionVideoStream(model, cam, d_candi, vol, t_win_r=R, depth_range=DEPTH_RANGE, copy_outputs=True, **kw)
    outs = {}
    for f, e in zip(frames, extMs):
        o = fs.push(f, e)
        if o is not None:
            outs[o[0]] = (o[1].clone(), o[2].clone())
    o = fs.flush()
    if o is not None:
        outs[o[0]] = (o[1].clone(), o[2].clone())
    torch.cuda.synchronize()
    fs.check()
    return fs, outs


def _same_store(got, want):
    assert got.keys() == want.keys()
    for k in want.keys():
        assert np.array_equal(sr.bits(got.get([k])[1]), sr.bits(want.get([k])[1])), k


def _same_arrays(got, want):
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert isinstance(x, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32))


@pytest.mark.parametrize("mode,color,track", [("eager", False, False), ("pipeline", False, False), ("eager", True, False),
                                              ("pipeline", False, True)])
def test_paging_stream_equals_the_hand_written_loop(mode, color, track):
    frames, extMs, maps, _, _ = _hand()
    want, want_store = _volume(color), fusion.BlockStore(5 if color else 2)
    shifts, fused = _hand_page(want, want_store, color, track)
    out, back = [s for _, s in shifts if s[0] > 0], [s for _, s in shifts if s[0] < 0]
    print("[page] %s colour %d track %d: shifts %s, paged out %d, in %d, dropped %d, %d blocks left"
          % (mode, color, track, shifts, want_store.n_put, want_store.n_taken, want_store.n_dropped, len(want_store)))
    assert len(out) >= 2 and len(back) >= 2 and all(s[1] == s[2] == 0 for _, s in shifts)
    assert want_store.n_put > 0 and want_store.n_taken > 0          # something left, and something came back
    vol = _volume(color)
    fs, outs = _stream(vol, color=color, track=track, follow_spill="page", **FOLLOW, **ff.MODES[mode])
    if ff.MODES[mode]["use_graph"]:
        assert fs.stream._graph is not None, fs.stream.graph_error
    fsn._same_maps(outs, maps)                                      # paging perturbs nothing of the network's
    assert fs.n_shifts == len(shifts) and vol.offset == want.offset and vol.origin == want.origin and fs.n_integrated == len(maps)
    assert fs.chunks == [] and (fs.n_paged_out, fs.n_paged_in) == (want_store.n_put, want_store.n_taken)
    frp._same_buf(vol, want)
    _same_store(fs.store, want_store)
    # the world: the stream's against paged_extract of the hand loop, and against one large static volume
    got = fs.world_mesh()
    _same_arrays(got, fusion.paged_extract(want, want_store, "mesh", w_min=W_MIN, colors=color))
    assert len(got) == (3 if color else 2) and got[1].dtype == np.int32 and len(got[1]) > 0 and got[1].max() < len(got[0])
    pts = fs.world_points()
    assert len(pts) == (2 if color else 1)
    _same_arrays(pts, fusion.paged_extract(want, want_store, "points", w_min=W_MIN, colors=color))
    offs = np.cumsum([s for _, s in [(0, (0, 0, 0))] + shifts], axis=0)[:, 0]
    lo, hi = int(offs.min()), int(offs.max())
    static = _volume(color, dims=(DIMS[0] + hi - lo,) + DIMS[1:], origin=(ORIGIN[0] + VOXEL * lo,) + ORIGIN[1:])
    cam = tv.gt.setup()[0]
    for ci, depth, pose, kw in fused:
        assert static.integrate(depth, pose, cam, depth_range=DEPTH_RANGE, **kw)
    n_static = static.mesh(w_min=W_MIN)[-1][1]
    print("[page] world mesh: %d triangles, the static %s volume's %d" % (len(got[1]), static.dims, n_static))
    assert len(got[1]) == n_static > 100                            # a surface, not a few stray cells
    fs.reset()
    assert len(fs.store) == len(want_store) and fs.n_shifts == len(shifts)      # the store stays, like the volume


def test_a_saved_store_continues_and_the_refusals(tmp_path):
    frames, extMs, maps, _, _ = _hand()
    model, cam, d_candi = tv._model(R)
    # two first passes, bit-identical; the second pass runs on one with the store it built, on the other with that store saved and loaded
    first = []
    for _ in range(2):
        vol = _volume()
        fs, _ = _stream(vol, follow_spill="page", use_graph=False, **FOLLOW)
        first.append((vol, fs.store))
    frp._same_buf(first[0][0], first[1][0])
    _same_store(first[0][1], first[1][1])
    assert len(first[0][1]) > 0
    path = str(tmp_path / "map.npz")
    first[1][1].save(path)
    loaded = fusion.BlockStore.load(path)
    _same_store(loaded, first[0][1])
    second = []
    for (vol, _), store in zip(first, (first[0][1], loaded)):
        fs, _ = _stream(vol, follow_spill="page", follow_store=store, use_graph=False, **FOLLOW)
        assert fs.store is store and fs.n_paged_in > 0 and fs.n_paged_out > 0       # what the first pass left came back
        second.append(fs)
    assert (second[0].n_paged_in, second[0].n_paged_out) == (second[1].n_paged_in, second[1].n_paged_out)
    frp._same_buf(first[0][0], first[1][0], "after the second pass")
    _same_store(second[1].store, second[0].store)
    # the construction refusals
    for kw, v in ((dict(follow_step=4), _volume()), (dict(follow_step=12), _volume()), (dict(), _volume(dims=(60, 64, 48))),
                  (dict(follow_store=fusion.BlockStore(5)), _volume()), (dict(follow_store={}), _volume())):
        with pytest.raises(ValueError):
            fusion.FusionVideoStream(model, cam, d_candi, v, t_win_r=R, **dict(dict(FOLLOW, follow_spill="page"), **kw))
    for kw in (dict(follow_spill="mesh", follow_store=fusion.BlockStore(2), **FOLLOW), dict(follow_spill="page", follow_store=fusion.BlockStore(2))):
        with pytest.raises(ValueError):
            fusion.FusionVideoStream(model, cam, d_candi, _volume(), t_win_r=R, **kw)
    off = _volume()
    off.shift((4, 0, 0))
    with pytest.raises(ValueError):
        fusion.FusionVideoStream(model, cam, d_candi, off, t_win_r=R, follow_spill="page", **FOLLOW)
    # a frame integrated before a paged shift can still not be reposed
    vol = _volume()
    fs, _ = _stream(vol, follow_spill="page", history=4, use_graph=False, **FOLLOW)
    before = [h.ref_index for h in fs._held if h.shifts != fs.n_shifts]
    assert before
    with pytest.raises(ValueError, match="before the volume shifted"):
        fs.repose(before[0], frp._moved(extMs[before[0]], 1))


def test_follow_spill_mesh_is_what_it_was_on_the_same_sequence():
    """follow_spill='mesh' on the out-and-back sequence: the loop of tests/test_gpu_fusion_follow.py written out, bit for bit — the
    returning camera finds the region empty and the world mesh holds both passes' surfaces."""
    frames, extMs, maps, _, _ = _hand()
    cam, d_candi = tv.gt.setup()
    want, chunks, shifts = _volume(), [], []
    for ci in sorted(maps):
        depth = fsn._regress(maps[ci][0][0], d_candi)[0]
        pose = np.asarray(extMs[ci], np.float64)
        s = fusion.follow_shift(pose, want, FOLLOW["follow"], FOLLOW["follow_margin"], FOLLOW["follow_step"])
        if s != (0, 0, 0):
            shifts.append(s)
            chunks.append(ff._host(want.shift(s, spill=True).mesh(w_min=W_MIN)[:-1]))
        assert want.integrate(depth, pose, cam, depth_range=DEPTH_RANGE)
    vol = _volume()
    fs, outs = _stream(vol, follow_spill="mesh", use_graph=False, **FOLLOW)
    fsn._same_maps(outs, maps)
    assert fs.store is None and (fs.n_paged_out, fs.n_paged_in) == (0, 0) and fs.n_shifts == len(shifts) >= 4
    frp._same_buf(vol, want)
    ff._same_chunks(fs.chunks, chunks)
    paged = _volume()
    ps, _ = _stream(paged, follow_spill="page", use_graph=False, **FOLLOW)
    assert paged.offset == vol.offset and int((paged.weight > 0).sum()) >= int((vol.weight > 0).sum())     # the first pass is still there
    assert not torch.equal(paged._buf.view(torch.int32), vol._buf.view(torch.int32)) and ps.n_paged_in > 0
