"""Static and near-static windows: a camera that stands still (tripod shot, paused robot, the first frames of a sequence).

The feature CNN's BatchNorms use batch statistics over the V + 1 = 5 frames of the window (the reference never leaves train
mode).  The SPP 64-window branch pools each frame to ONE cell, so its BatchNorm sees five values per channel,
and when the frames agree they agree to a few ulps: a variance taken as E[y^2] - mean^2 has no digit left there.  The
reference (ATen: two-pass / Welford) still normalises such a channel to about beta; so must this path.

  * the SPP branches' statistics (ops.bn_small_stats) against float64 F.batch_norm at counts 2 .. 480 and on exactly constant,
    near-constant, all-zero and healthy channels — values as spp_concat consumes them, and the running statistics;
  * the feature CNN (inference kernels and module composition) on static windows against the checker;
  * KVNET.forward and DepthStream (eager, hipGraph, pipelined) on consecutive static frames against the CPU oracle.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import report
from neuralrgbd_amd import camera, synth
from oracle import kvnet_oracle as ko

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24                       # unit roundoff of fp32


# ------------------------------------------------------------------ windows
def static_window(kind, H, W, seed=0, V=4):
    """(ref [1,3,H,W], src [1,V,3,H,W], poses [1,V,4,4]) of a camera that (nearly) stands still.
    identical:   V + 1 copies of one image, identity poses (every depth candidate ties: values only, no arg-max)
    posed:       V + 1 copies of one image under ordinary non-identity poses (the images alone reach the feature CNN)
    noisy:       copies + independent N(0, (1/255)^2) noise per frame, identity poses
    near_static: renderings of one textured scene from cameras a millimetre apart"""
    rng = np.random.RandomState(seed)
    tex = synth.smooth_texture(rng, 3, H, W)
    eye = np.broadcast_to(np.eye(4, dtype=np.float32), (1, V, 4, 4)).copy()
    if kind == "near_static":
        z = synth.smooth_texture(rng, 1, H, W, octaves=2)[0]
        z = (z - z.min()) / (z.max() - z.min() + 1e-12)
        depth = (0.6 + 3.4 * z).astype(np.float32)
        K = camera.scannet_intrinsics(W, H)["intrinsic_M"][:3, :3]
        poses = synth.random_poses(rng, V, rot_sigma=2e-4, trans_sigma=1e-3)
        tex_t, depth_t = torch.from_numpy(tex)[None], torch.from_numpy(depth)[None, None]
        views = [synth._render_view(tex_t, depth_t, K, np.linalg.inv(K), poses[v].astype(np.float64), H, W, 0.6, 4.0)
                 for v in range(V)]
        return tex_t.float(), torch.stack(views)[None], torch.from_numpy(poses[None])
    frames = np.broadcast_to(tex, (V + 1, 3, H, W)).copy()
    if kind == "noisy":
        frames = (frames + rng.normal(0, 1.0 / 255, frames.shape)).astype(np.float32)
    poses = synth.random_poses(rng, V)[None] if kind == "posed" else eye
    return torch.from_numpy(frames[V:]), torch.from_numpy(frames[:V])[None], torch.from_numpy(poses)


# ------------------------------------------------------------------ (a) small-count statistics against float64
SHAPES = {2: (2, 1, 1), 5: (5, 1, 1), 10: (5, 1, 2), 30: (5, 2, 3), 60: (5, 3, 4), 120: (5, 4, 6), 480: (5, 8, 12)}


def _channels(rng, n):
    """[n, 32]: 0-3 exactly constant (mean 1e-3, 1, 50, -300), 4-8 near-constant (std/|mean| 1e-7 .. 1e-2), 9 all zero,
    10-31 healthy."""
    x = np.empty((n, 32), np.float64)
    for j, m in enumerate((1e-3, 1.0, 50.0, -300.0)):
        x[:, j] = m
    for j, (m, r) in enumerate(zip((1.0, -40.0, 7.0, 300.0, -0.5), (1e-7, 1e-5, 1e-3, 3e-3, 1e-2))):
        x[:, 4 + j] = m * (1.0 + r * rng.standard_normal(n))
    x[:, 9] = 0.0
    x[:, 10:] = rng.normal(rng.normal(0, 3, 22), rng.uniform(0.1, 5, 22), (n, 22))
    return x.astype(np.float32)


@pytest.mark.parametrize("counts", [(2, 5, 10, 30), (60, 120, 5, 2), (5, 30, 120, 480), (5,)])
def test_small_count_batch_statistics_vs_float64(counts):
    """ops.bn_small_stats (the SPP branches' BatchNorm statistics) against two-pass float64 F.batch_norm(training=True).
    Bounds from the arithmetic: the statistics are exact to ~1e-15 in float64; what is left is the rounding of invstd, of
    scale = gamma * invstd and of shift = beta - mean * scale to fp32 and the fma that applies them — a few ulps of
    |z * scale|, |mean * scale|, |beta| and |y|.  Running statistics: a few ulps of their terms (unbiased variance)."""
    from neuralrgbd_amd import nets, ops
    rng = np.random.RandomState(sum(counts) * 7 + len(counts))
    status = nets.status_word(DEV)
    status.zero_()
    xs, gammas, betas, rms, rvs, nbts, momenta = [], [], [], [], [], [], []
    for n in counts:
        xs.append(torch.from_numpy(_channels(rng, n).reshape(SHAPES[n] + (32,))).to(DEV))
        g = rng.uniform(0.2, 2.5, 32) * np.where(rng.rand(32) < 0.2, -1.0, 1.0)
        gammas.append(torch.tensor(g, dtype=torch.float32, device=DEV))
        betas.append(torch.tensor(rng.normal(0, 0.5, 32), dtype=torch.float32, device=DEV))
        rms.append(torch.tensor(rng.normal(0, 2, 32), dtype=torch.float32, device=DEV))
        rvs.append(torch.tensor(rng.uniform(0.5, 2, 32), dtype=torch.float32, device=DEV))
        nbts.append(torch.zeros((), dtype=torch.int64, device=DEV))
        momenta.append(0.1 if n != 5 else 0.3)
    rm0 = [t.double().cpu() for t in rms]
    rv0 = [t.double().cpu() for t in rvs]
    sss = ops.bn_small_stats(xs, gammas, betas, 1e-5, momenta, rms, rvs, nbts)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    for i, n in enumerate(counts):
        z = xs[i].reshape(n, 32).double().cpu()
        g, b = gammas[i].double().cpu(), betas[i].double().cpu()
        rm, rv = rm0[i].clone(), rv0[i].clone()
        want = F.batch_norm(z, rm, rv, g, b, training=True, momentum=momenta[i], eps=1e-5)   # updates rm, rv (unbiased)
        mean = z.mean(0)
        var = ((z - mean) ** 2).mean(0)
        sc64 = g / torch.sqrt(var + 1e-5)
        ss = sss[i].double().cpu()
        assert torch.isfinite(ss).all()
        got = torch.relu(z * ss[:, 0] + ss[:, 1])                    # what spp_concat's taps compute (one fma per value)
        want = torch.relu(want)
        tol = 6 * U * ((z * sc64).abs() + (mean * sc64).abs() + b.abs() + want.abs()) + 1e-30
        bad = (got - want).abs() > tol
        assert not bad.any(), "count %d: channels %s exceed the rounding bound (max |d| %.3e)" % (
            n, sorted(set(bad.nonzero()[:, 1].tolist())), (got - want).abs().max().item())
        m = momenta[i]
        tol_m = 4 * U * ((1 - m) * rm0[i].abs() + m * mean.abs()) + 1e-30
        tol_v = 4 * U * ((1 - m) * rv0[i].abs() + m * var * n / max(n - 1, 1)) + 1e-30
        assert ((rms[i].double().cpu() - rm).abs() <= tol_m).all(), "count %d: running_mean" % n
        assert ((rvs[i].double().cpu() - rv).abs() <= tol_v).all(), "count %d: running_var (unbiased)" % n
        assert int(nbts[i].item()) == 1
        # the exactly constant and all-zero channels normalise to beta, as the reference's do
        for j in (0, 1, 2, 3, 9):
            assert (got[:, j] - want[:, j]).abs().max().item() <= tol[:, j].max().item()


def test_small_stats_rejects_bad_arguments():
    from neuralrgbd_amd import ops
    x = torch.zeros(5, 1, 1, 32, device=DEV)
    g, b = torch.ones(32, device=DEV), torch.zeros(32, device=DEV)
    with pytest.raises(ValueError):
        ops.bn_small_stats([x] * 5, [g] * 5, [b] * 5, 1e-5, 0.1)                 # at most four segments
    with pytest.raises(ValueError):
        ops.bn_small_stats([x, torch.zeros(5, 1, 1, 16, device=DEV)], [g] * 2, [b] * 2, 1e-5, 0.1)   # one channel count


# ------------------------------------------------------------------ (b) the feature CNN on static windows
@pytest.mark.parametrize("H,W", [(256, 256), (256, 384), (480, 640)])
@pytest.mark.parametrize("weights", ["seeded", "trained"])
@pytest.mark.parametrize("kind", ["identical", "noisy", "near_static"])
def test_feature_cnn_on_static_window(H, W, weights, kind):
    """forward_channels_last (inference kernels) and fe(x) (the autograd-capable module composition) on the five frames of a
    static window against oracle/kvnet_oracle.feature_cnn, with the gates of test_gpu_cnn.py::test_trunk_matrix_core_vs_vendor_
    forward.  No variance collapse may be reported: the SPP branch statistics are exact (pivot-shifted, float64).
    Where the SPP-64 channels' spread across the frames is far below sqrt(eps) (1/255 noise or millimetre baselines at 256 x 256
    and 256 x 384), that BatchNorm multiplies every fp32 rounding of its input by up to |gamma| / sqrt(1e-5) ~ 800 (trained-like
    gammas), and the checker's OWN fp32 execution lands up to ~1e-1 away from the float64 graph (measured on one MI355X: 5e-3 to
    9e-2, while this path stays within 4e-4).  Where the checker itself misses the gate, the same gate applies against float64."""
    from neuralrgbd_amd import nets
    fe = nets.FeatureExtractor(feature_dim=64, multi_scale=True)
    sd = (synth.seeded_state_dict if weights == "seeded" else synth.trained_like_state_dict)(fe, 5)
    fe.load_state_dict(sd)
    fe = fe.to(DEV)
    ref, src, _ = static_window(kind, H, W, seed=H + W)
    x = torch.cat((src[0], ref), 0).to(DEV)
    nets.status_word(DEV).zero_()
    with torch.no_grad():
        half_ref, feat_ref = ko.feature_cnn({k: v.to(DEV) for k, v in sd.items()}, "feature_extraction", x)
        half_mod, feat_mod = fe(x)
        half, feat = fe.forward_channels_last(x)
        nets.check_status(DEV)                                           # raises NrgbdError on a reported collapse
        sd64 = {k: (v.double() if v.is_floating_point() else v).to(DEV) for k, v in sd.items()}
        _, feat64 = ko.feature_cnn(sd64, "feature_extraction", x.double())
    e_ref64 = (feat_ref.double() - feat64).abs().max().item()          # the checker's own fp32 execution vs exact arithmetic
    for tag, hh, ff in (("inference kernels", half.permute(0, 3, 1, 2), feat.permute(0, 3, 1, 2)), ("module composition", half_mod, feat_mod)):
        assert torch.isfinite(hh).all() and torch.isfinite(ff).all(), tag
        e1 = (hh - half_ref).abs().max().item()
        e2 = (ff - feat_ref).abs().max().item()
        e64 = (ff.double() - feat64).abs().max().item()
        print("[parity] static CNN %s %dx%d %s, %s: layer1 max|d|=%.3e (|.|max %.2f)  feat max|d|=%.3e (|.|max %.2f)  "
              "|feat - fp64| %.3e (checker %.3e)" % (kind, H, W, weights, tag, e1, half_ref.abs().max().item(), e2,
                                                       feat_ref.abs().max().item(), e64, e_ref64))
        assert e1 < 1e-4 * max(1.0, half_ref.abs().max().item())
        gate = 2e-4 * max(1.0, feat_ref.abs().max().item())
        assert e2 < gate or (e64 < gate and e_ref64 >= gate)


# ------------------------------------------------------------------ (c) the whole path on consecutive static frames
def _model(cam, d_candi):
    import neuralrgbd_amd
    m = neuralrgbd_amd.KVNET(64, cam, d_candi, 10.0, 64, None, if_refined=True, refineNet_name="DPV", t_win_r=2)
    sd = synth.seeded_state_dict(m, 0)
    m.load_state_dict(sd)
    return m.to(DEV), sd


def _stream_outputs(cam, d_candi, wins, **kw):
    from neuralrgbd_amd.streaming import DepthStream
    model, _ = _model(cam, d_candi)
    stream = DepthStream(model, cam, d_candi, copy_outputs=True, **kw)
    outs = []
    for r, s, p in wins:
        o = stream.step(r.to(DEV), s.to(DEV), p.to(DEV))
        if o is not None:
            outs.append((o[0].clone(), o[1].clone()))
    if kw.get("pipeline"):
        outs.append(stream.flush())
    torch.cuda.synchronize()
    stream.check()                                                       # a reported collapse raises here
    return stream, outs


@pytest.mark.parametrize("kind", ["identical", "posed", "near_static"])
def test_static_frames_through_kvnet_and_depth_stream(kind):
    """Three consecutive frames of a camera standing still (config S grid): KVNET.forward + PREDICT against ko.step_full frame by
    frame with the gates of test_gpu_parity_configs._check (arg-max only where the depth is defined: not for identical images
    under identity poses, where every candidate ties), then DepthStream eager, with hipGraph capture and pipelined — no
    NrgbdError, finite volumes, and the three streams equal bit for bit."""
    from test_gpu_parity_configs import _check, _gpu_two_frames
    H, W, D = 256, 384, 64
    cam = camera.scannet_intrinsics(W // 4, H // 4)
    d_candi = np.linspace(0.1, 5.0, D)
    win = static_window(kind, H, W, seed=11)
    wins = [win] * 3      # each static frame sharpens the same belief, and the fp32 differences grow with it (DPV max|d| ~1.7x per frame)
    argmax = kind != "identical"
    model, sd = _model(cam, d_candi)
    outs = _gpu_two_frames(model, cam, d_candi, wins, refined=True)
    pred = None
    torch.set_num_threads(16)
    for f, (bv, dpv, nxt, r_cur, r_kv) in enumerate(outs):
        for name, t in (("BV_cur", bv), ("DPV", dpv), ("BV_predict", nxt), ("R(BV_cur)", r_cur), ("R(DPV)", r_kv)):
            assert torch.isfinite(t).all(), "%s frame %d: %s not finite" % (kind, f, name)
        o = ko.step_full(sd, *win, cam, d_candi, 10.0, pred)              # (R_cur, R_kv, DPV, BV_cur, BV_predict_next)
        tag = "static %s f%d" % (kind, f + 1)
        m_bv = _check(tag + " BV_cur", bv, o[3], argmax=argmax)
        m_dpv = _check(tag + " DPV", dpv, o[2], argmax=argmax)
        _check(tag + " BV_predict", nxt, o[4], argmax=False, max_abs=max(m_bv, m_dpv) + 2e-4)
        _check(tag + " R(BV_cur)", r_cur, o[0], argmax=argmax)
        _check(tag + " R(DPV)", r_kv, o[1], argmax=argmax)
        pred = o[4]
    got = {}
    for label, kw in (("eager", dict(use_graph=False)), ("graph", dict(use_graph=True)), ("pipelined", dict(use_graph=True, pipeline=True))):
        stream, got[label] = _stream_outputs(cam, d_candi, wins, **kw)
        if label != "eager":
            assert stream._graph is not None or stream.pipeline, stream.graph_error
        assert len(got[label]) == len(wins)
    for f, (a, b, c) in enumerate(zip(got["eager"], got["graph"], got["pipelined"])):
        assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
        assert torch.equal(a[1], outs[f][1]), "frame %d: stream DPV != KVNET.forward DPV" % f
        for x, y in ((a, b), (a, c)):
            assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]), "frame %d" % f
