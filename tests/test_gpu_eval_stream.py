"""GPU: evaluate.EvalVideoStream against a hand-built loop — VideoDepthStream.push -> DepthLabeler -> ops.depth_regress ->
DepthMetrics.update on the ground truth of the reference frame's push — on the model, sizes and synthetic sequence of
tests/test_gpu_video.py with the depth frames of tests/train_video_ref.py.  Per-frame records, totals and the returned maps are compared
bit for bit; the totals also against the float64 comparator on the downloaded maps, within the gates of tests/test_gpu_eval_depth.py."""
import numpy as np
import pytest
import torch

import depth_eval_ref as ref
import test_gpu_video as tv
import train_video_ref as tr
from test_gpu_eval_depth import _check_record
from neuralrgbd_amd import evaluate, ops, video
from neuralrgbd_amd import homography as warp_homo
from neuralrgbd_amd.train_video import DepthLabeler

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONF = (0., .13, .2)                 # D = 8 candidates: a flat volume has confidence 1 / 8
DEPTH_SIZE = (120, 160)


def _depths(r, n):
    return tr.depth_frames(930 + r, n, *DEPTH_SIZE)


def _add(total, frame):
    """total = total + frame as the finaliser does it: IEEE double / int64 adds in sequence."""
    return [t + f for t, f in zip(total, frame)]


def _hand_loop(r, frames, depths, extMs):
    """-> ({ref_index: (refined, dpv)}, {ref_index: (hires frame record, lowres frame record)} as numpy, {ref_index: downloaded
    (depth, conf, gt) per resolution}, the two DepthMetrics)."""
    model, cam, d_candi = tv._model(r)
    vs = video.VideoDepthStream(model, cam, d_candi, t_win_r=r, copy_outputs=True, use_graph=False)
    h, w = cam["unit_ray_array"].shape[:2]
    lab = DepthLabeler(d_candi, (tv.H, tv.W), (h, w), device=DEV)
    gts = [None if d is None else lab(d) for d in depths]
    hi, lo = (evaluate.DepthMetrics(CONF, device=DEV) for _ in range(2))
    d_dev = warp_homo._d_candi_dev(d_candi, torch.device(DEV))
    maps, records, host = {}, {}, {}
    for f, e in zip(frames, extMs):
        out = vs.push(f, e)
        if out is None:
            continue
        c, refined, dpv = out
        maps[c] = (refined.clone(), dpv.clone())
        if gts[c] is None:
            continue
        rec, dl = [], []
        for ev, vol, gt in ((hi, refined, gts[c]["dmap_imgsize"][0]), (lo, dpv, gts[c]["dmap_raw"][0])):
            depth, conf = ops.depth_regress(vol[0], d_dev, channels_last=ops.is_channels_last_view(vol[0]))
            rec.append([t.cpu().numpy().copy() for t in ev.update(depth, conf, gt)])
            dl.append((depth.cpu().numpy(), conf.cpu().numpy(), gt.cpu().numpy()))
        records[c], host[c] = rec, dl
    assert vs.flush() is None
    torch.cuda.synchronize()
    vs.check()
    return maps, records, host, (hi, lo)


@pytest.fixture(scope="module", params=[2, 1])
def hand(request):
    r = request.param
    frames, _, extMs = tv._sequence(r)
    depths = _depths(r, len(frames))
    return (r, frames, depths, extMs) + _hand_loop(r, frames, depths, extMs)


def _stream(r, frames, depths, extMs, **kw):
    model, cam, d_candi = tv._model(r)
    es = evaluate.EvalVideoStream(model, cam, d_candi, t_win_r=r, conf_thresholds=CONF, copy_outputs=True, **kw)
    assert es.n_slots == 2 * r + 2
    outs = {}
    for i, (f, d, e) in enumerate(zip(frames, depths, extMs)):
        d = d if d is None or i % 2 else torch.from_numpy(d.view(np.int16)).to(DEV)        # host numpy and device tensors in turn
        o = es.push(f, d, e)
        if o is not None:
            assert o[0] not in outs
            outs[o[0]] = (o[1].clone(), o[2].clone(), None if o[3] is None else [[t.cpu().numpy().copy() for t in rec] for rec in o[3:]])
    o = es.flush()
    if o is not None:
        outs[o[0]] = (o[1].clone(), o[2].clone(), None if o[3] is None else [[t.cpu().numpy().copy() for t in rec] for rec in o[3:]])
    torch.cuda.synchronize()
    es.check()
    return es, outs


def _same_stream(es, outs, maps, records, metrics):
    assert sorted(outs) == sorted(maps)
    for c, (refined, dpv, rec) in outs.items():
        assert torch.equal(refined, maps[c][0]) and torch.equal(dpv, maps[c][1]), "maps of frame %d differ" % c      # evaluation perturbs nothing
        assert (rec is None) == (c not in records)
        if rec is not None:
            for got, want in zip(rec, records[c]):
                for a, b in zip(got, want):
                    assert np.array_equal(a.view(np.int64), b.view(np.int64)), "frame record of frame %d differs" % c
    for ev, want in zip((es.hires, es.lowres), metrics):
        for a, b in zip(ev.total, want.total):
            assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["eager", "graph", "pipeline"])
def test_stream_equals_the_hand_built_loop(hand, mode):
    r, frames, depths, extMs, maps, records, _, metrics = hand
    kw = {"eager": dict(use_graph=False), "graph": dict(use_graph=True), "pipeline": dict(use_graph=True, pipeline=True)}[mode]
    es, outs = _stream(r, frames, depths, extMs, **kw)
    if mode != "eager":
        assert es.video.stream._graph is not None, es.video.stream.graph_error
    assert sorted(outs) == list(range(r, len(frames) - r)) and sorted(records) == sorted(outs)
    _same_stream(es, outs, maps, records, metrics)
    assert int(es.hires.total[2][0]) == len(frames) - 2 * r == int(es.lowres.total[2][0])
    res = es.result()
    assert sorted(res) == ["hires", "lowres"] and len(res["hires"]) == len(CONF) and res["hires"][0]["frames"] == len(frames) - 2 * r
    assert res["hires"][0]["n"] > 1000 and res["lowres"][0]["n"] > 100 and np.isfinite(res["hires"][0]["rmse_log"])


def test_totals_against_the_comparator(hand):
    r, _, _, _, _, records, host, metrics = hand
    thr = ref.log_thresholds(CONF)
    for k, ev in enumerate(metrics):
        frames = [ref.evaluate(*host[c][k], thr, (1e-3, np.inf)) for c in sorted(host)]
        for c, w in zip(sorted(host), frames):
            assert np.array_equal(records[c][k][1], w["counts"]) and np.array_equal(records[c][k][2], w["header"])
        _check_record(ev.total, ref.add_records(frames), what="r=%d %s totals" % (r, ("hires", "lowres")[k]))


def test_a_missing_depth_frame_yields_maps_but_no_update(hand):
    r, frames, depths, extMs, maps, records, _, metrics = hand
    missing = r + 1
    es, outs = _stream(r, frames, [None if i == missing else d for i, d in enumerate(depths)], extMs, use_graph=False)
    assert sorted(outs) == sorted(maps) and outs[missing][2] is None
    assert all(torch.equal(outs[c][0], maps[c][0]) and torch.equal(outs[c][1], maps[c][1]) for c in maps)
    for k, (ev, full) in enumerate(zip((es.hires, es.lowres), metrics)):
        want = None
        for c in sorted(records):
            if c != missing:
                want = records[c][k] if want is None else _add(want, records[c][k])
        for a, b in zip(ev.total, want):
            assert np.array_equal(a.cpu().numpy().view(np.int64), np.asarray(b).view(np.int64))
        assert int(ev.total[2][0]) == int(full.total[2][0]) - 1


def test_a_nan_pose_evaluates_no_frame_of_its_windows():
    r = 1
    frames, _, extMs = tv._sequence(r)
    depths = _depths(r, len(frames))
    extMs[3] = np.full((4, 4), np.nan)
    maps, records, _, metrics = _hand_loop(r, frames, depths, extMs)
    es, outs = _stream(r, frames, depths, extMs, use_graph=False)
    assert sorted(outs) == [1, 5] == sorted(records)
    _same_stream(es, outs, maps, records, metrics)
    assert int(es.hires.total[2][0]) == 2
    # reset() starts a new trajectory and keeps the totals
    es.reset()
    assert es.video.n_pushed == 0 and int(es.hires.total[2][0]) == 2 and es.gt_ring.held == [None] * es.n_slots
