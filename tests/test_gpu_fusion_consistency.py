"""GPU: fusion.FusionVideoStream(history=N, consistency=k) and fusion.filter_depth — every depth map cross-checked against the held
frames' raw maps before it is tracked and fused — on the smallest configuration of tests/test_gpu_fusion_repose.py (r = 1, its model,
sizes and synthetic sequence).  The stream equals the loop written out by hand (VideoDepthStream's maps, ops.depth_regress,
ops.depth_consistency, TSDFVolume.integrate) bit for bit, eager, captured and pipelined; consistency=0 is the stream without the
argument; the first frame is fused as before; on the corner fixture of tests/consistency_ref.py the seeded flying pixels never enter
the volume; a repose counts for the next frame's votes, and a repose followed by its inverse restores the volume inside the bound
derived below."""
import numpy as np
import pytest
import torch

import consistency_ref as cr
import icp_ref as ir
import test_gpu_fusion_repose as frp
import test_gpu_fusion_stream as fsn
import test_gpu_video as tv
import tsdf_ref as ref
from neuralrgbd_amd import fusion, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 1
U = ref.U
HISTORY, VIEWS = 3, 2
REL = 0.05                      # the sequence is noise through seeded weights: a threshold at which some pixels stay and some go


def _raw(maps, ci):
    d_candi = tv.gt.setup()[1]
    depth, logconf, d_dev, cl = fsn._regress(maps[ci][0][0], d_candi)
    return depth, logconf, d_dev, cl


def _hand_filter(maps, ci, held, poses, c, pose=None):
    """The filter launch of frame ci written out: the held frames `held` (oldest first) at `poses` are the sources -> (votes,
    filtered map, raw depth, raw gate)."""
    cam = tv.gt.setup()[0]
    thr = None if c == 0 else float(np.log(np.float64(c)).astype(np.float32))
    depth, logconf = _raw(maps, ci)[:2]
    K = fusion.intrinsics_at(cam, *depth.shape)
    T_ref = np.asarray(poses[ci] if pose is None else pose, np.float64)
    kw = dict(src_depth=None, src_T=None)
    if held:
        src = [_raw(maps, h)[:2] for h in held]
        kw = dict(src_depth=torch.stack([s[0] for s in src]), src_gate=None if thr is None else torch.stack([s[1] for s in src]),
                  src_T=np.stack([(np.asarray(poses[h], np.float64) @ np.linalg.inv(T_ref))[:3] for h in held]).astype(np.float32))
    votes, out = ops.depth_consistency(depth, K, rel_thr=REL, min_views=min(VIEWS, len(held)), depth_range=fsn.DEPTH_RANGE,
                                       gate=None if thr is None else logconf, gate_thr=0.0 if thr is None else thr, **kw)
    return votes, out, depth, logconf


def _hand_loop(vol, maps, extMs, weight, c):
    """VideoDepthStream's maps, regressed, filtered against the last HISTORY frames' raw maps, integrated without a gate."""
    cam = tv.gt.setup()[0]
    held, votes = [], {}
    for ci in sorted(maps):
        votes[ci], out, _, _ = _hand_filter(maps, ci, held[-HISTORY:], extMs, c)
        d_dev, cl = _raw(maps, ci)[2:]
        wmap = ops.export_depth_u16(maps[ci][0][0], d_dev, channels_last=cl)[1] if weight == "conf" else None
        assert vol.integrate(out, extMs[ci], cam, weight=wmap, depth_range=fsn.DEPTH_RANGE)
        held.append(ci)
    return votes


MODES = {"eager": (dict(use_graph=False), "uniform", False), "graph": (dict(use_graph=True), "conf", True),
         "pipeline": (dict(use_graph=True, pipeline=True), "conf", True)}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_stream_equals_the_hand_written_loop(mode):
    r, frames, extMs, maps = fsn._hand(R)
    kw, weight, gated = MODES[mode]
    c = fsn._median_confidence(maps, "refined", tv.gt.setup()[1]) if gated else 0.0
    want = fsn._volume()
    votes = _hand_loop(want, maps, extMs, weight, c)
    order = sorted(maps)
    kept = [int((votes[ci] >= min(VIEWS, n)).sum()) for n, ci in enumerate(order)]
    valid = [int((votes[ci] >= 0).sum()) for ci in order]
    print("[fusion-consistency] %s: pixels kept %s of valid %s" % (mode, kept, valid))
    assert kept[0] == valid[0] and 0 < sum(kept[2:]) < sum(valid[2:])       # the filter drops some but not all pixels
    vol = fsn._volume()
    fs, outs = fsn._stream(r, frames, extMs, vol, weight=weight, conf_threshold=c, history=HISTORY, consistency=VIEWS,
                           consistency_rel=REL, **kw)
    if kw["use_graph"]:
        assert fs.stream._graph is not None, fs.stream.graph_error
    fsn._same_maps(outs, maps)                                      # the filter perturbs nothing of the network's
    frp._same_buf(vol, want)
    assert fs.n_integrated == len(maps) and int((want.weight > 0).sum()) > 1000
    assert torch.equal(fs.last_votes.view(torch.int32), votes[order[-1]].view(torch.int32))
    # the history: the filtered map that was integrated, and the raw map and gate later frames are checked against
    assert {k for k, v in fs._slots.items() if v is not None} == {"depth", "raw"} | ({"gate", "wmap"} if gated else set())
    for ci in order[-HISTORY:]:
        h, depth, hkw = fs._held_frame(ci, "test")
        n = order.index(ci)
        _, out, raw, logconf = _hand_filter(maps, ci, order[max(0, n - HISTORY):n], extMs, c)
        assert torch.equal(depth.view(torch.int32), out.view(torch.int32)) and hkw["gate"] is None and hkw["gate_thr"] is None
        assert torch.equal(fs._slots["raw"][h[2]].view(torch.int32), raw.view(torch.int32))
        assert not gated or torch.equal(fs._slots["gate"][h[2]].view(torch.int32), logconf.view(torch.int32))


def test_consistency_0_is_the_stream_without_the_argument():
    r, frames, extMs, maps = fsn._hand(R)
    c = fsn._median_confidence(maps, "refined", tv.gt.setup()[1])
    kw = dict(weight="conf", conf_threshold=c, history=HISTORY, use_graph=False)
    runs = []
    for extra in ({}, dict(consistency=0), {}, dict(consistency=0, consistency_rel=0.5)):
        vol = fsn._volume()
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
        fs, outs = fsn._stream(r, frames, extMs, vol, **kw, **extra)
        runs.append((vol, torch.cuda.memory_stats(DEV)["allocation.all.allocated"] - before))
        fsn._same_maps(outs, maps)
        assert fs.consistency == 0 and fs.last_votes is None and fs._votes is None and fs._slots["raw"] is None
    print("[fusion-consistency] allocations per run: %s" % [n for _, n in runs])
    for vol, n in runs[1:]:
        frp._same_buf(vol, runs[0][0])
    assert runs[2][1] == runs[3][1] == runs[1][1]                   # (the first run also warms the caches)


def test_the_first_frame_is_fused_unfiltered():
    r, frames, extMs, maps = fsn._hand(R)
    c = fsn._median_confidence(maps, "refined", tv.gt.setup()[1])
    first = sorted(maps)[0]
    n = first + r + 1                                               # the pushes after which frame `first` has come out
    vol, want = fsn._volume(), fsn._volume()
    fs, outs = fsn._stream(r, frames[:n], extMs[:n], vol, conf_threshold=c, history=HISTORY, consistency=VIEWS, consistency_rel=REL,
                           use_graph=False)
    assert sorted(outs) == [first] and fs.n_integrated == 1
    passing, total = fsn._hand_integrate(want, outs, extMs, "refined", "uniform", c)        # as before: the gate, no filter
    frp._same_buf(vol, want)
    votes = fs.last_votes.cpu().numpy()
    assert 0 < passing < total and int((votes == 0).sum()) >= 1 and set(np.unique(votes)) <= {-1.0, 0.0}
    assert int((want.weight > 0).sum()) > 100


def _corner_volume():
    C = ir.CORNER
    return fusion.TSDFVolume(C["dims"], C["vs"], C["origin"], trunc=C["trunc"], device=DEV)


def _off_plane(vol):
    """points() farther than one voxel from all three walls."""
    C = ir.CORNER
    p = vol.points(w_min=1.0)[0].cpu().numpy().astype(np.float64)
    dist = np.abs(np.asarray(C["planes"])[None] - p).min(1)
    return int((dist > C["vs"]).sum()), len(p)


def test_corner_fixture_fliers_never_enter_the_volume():
    """filter_depth on the corner fixture, one view confirming (min_views = 1, at which the host test finds every seeded outlier
    dropped): the volume fused from the filtered frame is the volume fused from the frame with the outlier pixels zeroed by hand."""
    fx = cr.corner_fixture()
    depth, sources = torch.from_numpy(np.array(fx["depth"])).to(DEV), torch.from_numpy(np.array(fx["sources"])).to(DEV)
    out, votes = fusion.filter_depth(depth, fx["pose"], sources, fx["poses"], fx["K"], rel=cr.CORNER_REL, min_views=1)
    v = cr.corner_votes(np.float32)["votes"]
    assert np.array_equal(votes.cpu().numpy().view(np.int32), v.view(np.int32))
    assert np.array_equal(out.cpu().numpy().view(np.int32), cr.filtered(fx["depth"], v, 1).view(np.int32))
    by_hand = torch.from_numpy(np.where(fx["outlier"], np.float32(0), fx["depth"])).to(DEV)
    vols = {}
    for name, d in (("filtered", out), ("by hand", by_hand), ("unfiltered", depth)):
        vols[name] = _corner_volume()
        assert vols[name].integrate(d, fx["pose"], fx["K"])
    frp._same_buf(vols["filtered"], vols["by hand"], "(filtered against zeroed by hand)")
    counts = {k: _off_plane(v) for k, v in vols.items()}
    print("[fusion-consistency] corner: points off the walls (of all points): unfiltered %s, filtered %s; %d seeded outliers"
          % (counts["unfiltered"], counts["filtered"], int(fx["outlier"].sum())))
    fliers = counts["unfiltered"][0] - counts["filtered"][0]
    assert counts["filtered"] == counts["by hand"] and fliers > 0
    assert counts["filtered"][0] == counts["unfiltered"][0] - fliers and counts["filtered"][1] > 1000
    # a list of maps and a cam_intrinsics-free tuple, votes and the map written in place
    again, v2 = fusion.filter_depth(depth, fx["pose"], list(sources), fx["poses"], fx["K"], rel=cr.CORNER_REL, min_views=1,
                                    votes=torch.empty_like(depth), out=depth)
    assert again is depth and torch.equal(depth.view(torch.int32), out.view(torch.int32)) and torch.equal(v2, votes)


def test_a_repose_counts_for_the_next_frames_votes():
    r, frames, extMs, maps = fsn._hand(R)
    order = sorted(maps)
    vol = fsn._volume()
    model, cam, d_candi = tv._model(r)
    fs = fusion.FusionVideoStream(model, cam, d_candi, vol, t_win_r=r, depth_range=fsn.DEPTH_RANGE, use_graph=False, history=HISTORY,
                                  consistency=VIEWS, consistency_rel=REL)
    for f, e in zip(frames[:-1], extMs[:-1]):
        fs.push(f, e)
    held = [i for i, _ in fs.history_poses()]
    assert held == order[-1 - HISTORY:-1]
    moved = frp._moved(extMs[held[-1]], 5)
    assert fs.repose(held[-1], moved)
    out = fs.push(frames[-1], extMs[-1])
    assert out is not None and out[0] == order[-1]
    poses = {i: extMs[i] for i in order}
    stale = _hand_filter(maps, order[-1], held, poses, 0.0)[0]
    poses[held[-1]] = moved
    want = _hand_filter(maps, order[-1], held, poses, 0.0)[0]
    assert torch.equal(fs.last_votes.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(want, stale)
    print("[fusion-consistency] repose: %d of %d votes changed" % (int((want != stale).sum()), want.numel()))


def test_a_repose_and_its_inverse_restore_the_volume():
    """A held (filtered) frame moved away and back: the weights (uniform: integers) return bit for bit; the distances inside the
    bound of tests/test_gpu_fusion_repose.py's retrack test applied twice — with e the distance to what the voxel held before, a
    removal at weight W gives e <- amp (e + 2 u) + 3 u, amp = (W + 1) / (W - 1) (W = 1: the voxel is emptied and what is added
    next is stored exactly), an addition e <- e + 8 u; whatever the two poses see of it, every voxel is charged a removal and an
    addition per move — the first at the weight it had before, the second at the weight in between, with a factor of at least 1 so
    that a voxel the second move only adds to keeps the first move's error."""
    r, frames, extMs, maps = fsn._hand(R)
    vol = fsn._volume()
    fs, _ = fsn._stream(r, frames, extMs, vol, history=HISTORY, consistency=VIEWS, consistency_rel=REL, use_graph=False)
    ci = fs.history_poses()[1][0]
    before = frp._copy(vol)
    assert fs.repose(ci, frp._moved(extMs[ci], 6))
    mid = vol.weight.cpu().numpy().astype(np.float64)
    assert not torch.equal(vol._buf.view(torch.int32), before._buf.view(torch.int32))
    assert fs.repose(ci, extMs[ci])
    assert torch.equal(vol.weight.view(torch.int32), before.weight.view(torch.int32))
    W = before.weight.cpu().numpy().astype(np.float64)
    with np.errstate(all="ignore"):
        amp = [np.where(w > 1, (w + 1) / (w - 1), 0.0) for w in (W, mid)]
    e1 = U * (2 * amp[0] + 11)
    e2 = np.maximum(amp[1], 1.0) * (e1 + 2 * U) + 11 * U
    diff = np.abs(vol.tsdf.cpu().numpy().astype(np.float64) - before.tsdf.cpu().numpy())
    print("[fusion-consistency] repose and back: worst |dT| %.1f u, worst share of the bound %.3f" % (diff.max() / U, (diff / (1.01 * e2)).max()))
    assert (diff <= 1.01 * e2).all() and np.array_equal(dict(fs.history_poses())[ci], np.asarray(extMs[ci], np.float64))


def test_argument_errors():
    r = R
    model, cam, d_candi = tv._model(r)
    new = lambda **kw: fusion.FusionVideoStream(model, cam, d_candi, fsn._volume(), t_win_r=r, depth_range=fsn.DEPTH_RANGE, **kw)
    for kw in (dict(consistency=1), dict(history=1, consistency=2), dict(history=2, consistency=-1), dict(history=2, consistency=1.5),
               dict(history=2, consistency=1, consistency_rel=0.0), dict(history=2, consistency=1, consistency_rel=-0.01),
               dict(history=2, consistency=1, consistency_rel=float("nan")), dict(history=2, consistency=1, consistency_rel=float("inf"))):
        with pytest.raises(ValueError):
            new(**kw)
    fs = new(history=2, consistency=2)
    assert fs.consistency == 2 and fs.consistency_rel == 0.01 and fs.last_votes is None
    depth = torch.ones(4, 6, device=DEV)
    with pytest.raises(ValueError):
        fusion.filter_depth(depth, np.eye(4), [depth], [np.eye(4), np.eye(4)], (5., 5., 3., 2.))
    with pytest.raises(ValueError):
        fusion.filter_depth(depth, np.eye(4), [depth], [np.eye(4)], (5., 5., 3., 2.), gate=depth, gate_thr=0.5)
