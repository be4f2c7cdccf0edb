"""Temporal windows of 3 and 7 frames (t_win_r = 1 and 3) on the GPU, at the smallest shape that reaches every kernel of the path
(image 256 x 256: the SPP window forbids less; grid 64 x 64: whole 8 x 16 tiles; D = 8: two F(4,3) depth tiles; D = 6 where the
choice falls to wino_dw.hip): the K-Net input volume of nrgbd_warp_volume_cl bit for bit against the planar kernel, the first layer
on zero-padded 16-channel blocks against float64, whole frames and one training iteration against the UNMODIFIED reference
(tests/golden/twin_r<r>.npz, tests/gen_twin_golden.py), the stream forms against each other, and the 5-frame window's dispatch."""
import contextlib
import copy
import ctypes
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_twin_golden as gt
import warp_exact as wx
import neuralrgbd_amd
from neuralrgbd_amd import _lib, camera, nets, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, D = gt.TWIN["H"], gt.TWIN["W"], gt.TWIN["D"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the volume kernel ----------------------------------------------------------------------------------------------------

def _texels(case, V, offset):
    """[V + 1, h, w, 68] texels (sources, then the reference), the RGB word at channels offset .. offset + 2, noise elsewhere."""
    _, Cs, h, w = case["src"].shape
    tex = np.random.RandomState(5).standard_normal((V + 1, h, w, 68)).astype(np.float32) * 100
    tex[:V, :, :, offset:offset + Cs] = case["src"][:V].transpose(0, 2, 3, 1)
    tex[V, :, :, offset:offset + Cs] = case["ref"].transpose(1, 2, 0)
    return _dev(tex)


def _geometry(case, V):
    return (_dev(case["KR"][:V]), _dev(case["Kt"][:V]), _dev(case["rays"]), _dev(case["d_candi"]), case["cx"], case["cy"])


def _volume_cl(case, V, align, Cp, offset=64, entry=False):
    """The padded channels-last volume from the texel layout the model uses: through ops.warp_volume(pad_channels=), or (entry) from
    nrgbd_warp_volume_cl itself — the only way to hand it V = 4, which ops keeps on nrgbd_warp_volume's own fast form."""
    _, Cs, h, w = case["src"].shape
    tex = _texels(case, V, offset)
    src, ref = tex[:V, :, :, offset:], tex[V, :, :, offset:]
    ss, rs = (h * w * 68, 1, w * 68, 68), (1, w * 68, 68)
    KR, Kt, rays, d, cx, cy = _geometry(case, V)
    bv, bp = _dev(case["bv_cur"]), _dev(case["bv_pred"])
    if not entry:
        out = ops.warp_volume(src, ss, ref, rs, KR, Kt, rays, d, cx, cy, V, Cs, h, w, bv_cur=bv, bv_pred=bp, align_corners=align,
                              channels_last=True, pad_channels=Cp)
    else:
        out = torch.full((len(case["d_candi"]), h, w, Cp), float("nan"), device=DEV)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = _lib.load().nrgbd_warp_volume_cl(p(src), *ss, p(ref), *rs, p(KR), p(Kt), p(rays), p(d), float(cx), float(cy), int(align),
                                              p(bv), p(bp), p(out), V, Cs, Cp, out.shape[0], h, w, None)
        assert rc == 0
    torch.cuda.synchronize()
    return out


def _volume_planar(case, V, align):
    """The existing planar kernel's warped sources + reference [3V + 3, D, h, w], then BV_cur - BV_predict (KVNET.py:163-166)."""
    _, Cs, h, w = case["src"].shape
    KR, Kt, rays, d, cx, cy = _geometry(case, V)
    warped = ops.warp_volume(_dev(case["src"][:V]), (Cs * h * w, h * w, w, 1), _dev(case["ref"]), (h * w, w, 1), KR, Kt, rays, d, cx, cy,
                             V, Cs, h, w, align_corners=align)
    return torch.cat((warped, (_dev(case["bv_cur"]) - _dev(case["bv_pred"]))[None]), dim=0)


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("family", ["large", "border", "behind"])        # footprints that leave the source image, either side of it
@pytest.mark.parametrize("h,w,Dv", [(33, 65, 8), (20, 36, 6), wx.BORDER_POW2 + (5,)])
@pytest.mark.parametrize("V", [2, 6])
def test_volume_kernel_is_the_planar_volume_then_zeros(V, h, w, Dv, family, align):
    case = wx.make_case(h, w, Dv, 6, 3, family)
    C, Cp = 3 * V + 4, nets.padded_channels(3 * V + 4)
    want = _volume_planar(case, V, align).permute(1, 2, 3, 0)
    for offset in (64, 65):      # 65: the RGB word 4 bytes off a 16-byte boundary -> the general kernel writes the same padded voxel
        got = _volume_cl(case, V, align, Cp, offset)
        assert tuple(got.shape) == (Dv, h, w, Cp)
        assert torch.equal(_bits(got[..., :C]), _bits(want)), "V %d offset %d: real channels differ from the planar kernel" % (V, offset)
        assert not got[..., C:].any() and not torch.signbit(got[..., C:]).any(), "V %d offset %d: padding is not +0" % (V, offset)


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("family", ["large", "on_plane"])
def test_new_entry_at_V4_has_the_bits_of_cl16(family, align):
    h, w, Dv = 33, 65, 8
    case = wx.make_case(h, w, Dv, 4, 3, family)
    cl16 = _volume_cl(case, 4, align, 16)                 # pad_channels == 16 == the assembly: nrgbd_warp_volume, warp_volume_cl16_kernel
    new = _volume_cl(case, 4, align, 16, entry=True)
    assert torch.equal(_bits(cl16), _bits(new))


def test_volume_entry_argument_checks():
    lib = _lib.load()
    x = torch.zeros(4096, device=DEV)
    p = ctypes.c_void_p(x.data_ptr())

    def call(V=2, Cp=16, ref=p, bv=p, D_=1):
        return lib.nrgbd_warp_volume_cl(p, 16, 1, 8, 4, ref, 1, 8, 4, p, p, p, p, 1.0, 1.0, 0, bv, p, p, V, 3, Cp, D_, 2, 2, None)
    assert call(Cp=8) == -2 and call(Cp=18) == -2 and call(V=17, Cp=64) == -2 and call(D_=65536) == -2
    assert call(ref=None) == -1 and call(bv=None) == -1
    with pytest.raises(ValueError):
        ops.warp_volume(x, (16, 1, 8, 4), x, (1, 8, 4), x[:18], x[:6].view(2, 3), x[:12].view(3, 4), x[:1], 1.0, 1.0, 2, 3, 2, 2,
                        pad_channels=16)       # no bv_cur / bv_pred, not channels-last
    torch.cuda.synchronize()


# ---- 2. the first layer on zero-padded 16-channel blocks ----------------------------------------------------------------------

# acceptance of tests/test_gpu_knet.py for the same layer at 16 -> 64, per kernel: max |y - float64| < factor * max(1, max |y|)
# (test_conv_wino_dw4_plain_vs_torch, test_conv_wino_dw_plain_vs_torch, test_conv_wino_pc_3d_first_layer_16_channels,
# test_conv3d_plain_vs_torch)
KNET_ACCEPT = {"dw4": 4e-5, "dw": 2e-5, "pc": 2e-5, "direct": 2e-5}
FIRST_LAYER = [(22, "dw4", 8), (22, "dw", 6), (22, "pc", 8), (22, "pc", 5),
               (10, "dw4", 8), (10, "dw", 6), (10, "pc", 8), (10, "pc", 5), (10, "direct", 8)]


def _run_kind(kind, x, wp):
    if kind == "dw4":
        return ops.conv_wino_dw4(x, wp, 64, want_stats=False)[0]
    if kind == "dw":
        return ops.conv_wino_dw(x, wp, 64, want_stats=False)[0]
    if kind == "pc":
        return ops.conv_wino(x, wp, 64, 3, want_stats=False)[0]
    return ops.conv3d(x, wp, want_stats=False)[0]


@pytest.mark.parametrize("C,kind,Dv", FIRST_LAYER)
def test_first_layer_on_the_padded_volume_vs_fp64(C, kind, Dv):
    """dres0.0 with its [64, C, 3, 3, 3] parameter on a volume of Cp = 16 ceil(C / 16) channels, the stream packed where the net packs
    it (nets._packed): against float64 F.conv3d on the C real channels; and garbage in the padding of the INPUT changes no bit, because
    the packed weights are zero there."""
    Cp = nets.padded_channels(C)
    assert kind in (nets.KalmanGainNet.kernels32 if Cp == 32 else nets.KalmanGainNet.kernels[Cp])
    torch.manual_seed(C + Dv)
    net = nets.KalmanGainNet(C, feature_dim=64).to(DEV)
    conv = net.dres0[0][0]
    with torch.no_grad():
        conv.weight.copy_(torch.randn(64, C, 3, 3, 3) * 0.1)
    assert tuple(conv.weight.shape) == (64, C, 3, 3, 3)
    x = torch.randn(Dv, 64, 64, C, device=DEV)
    want = F.conv3d(x.permute(3, 0, 1, 2)[None].double().cpu(), conv.weight.detach().double().cpu(), padding=1)[0].permute(1, 2, 3, 0)
    xp = torch.cat((x, torch.zeros(Dv, 64, 64, Cp - C, device=DEV)), dim=-1)
    wp = nets._packed(net, conv, kind, 1.0, Cp)
    y = _run_kind(kind, xp, wp)
    err, scale = (y.double().cpu() - want).abs().max().item(), want.abs().max().item()
    print("[parity] first layer %d (-> %d) -> 64 on %s, D = %d: max|d vs fp64| %.3e (|y|max %.2f)" % (C, Cp, kind, Dv, err, scale))
    assert err < KNET_ACCEPT[kind] * max(1.0, scale)
    if Cp != C:
        xg = xp.clone()
        xg[..., C:] = torch.randn(Dv, 64, 64, Cp - C, device=DEV) * 1e3
        assert torch.equal(_run_kind(kind, xg, wp), y), "the packed stream of %s carries non-zero weights in the padding" % kind
    assert net.__dict__["_wp_cache"][(kind, id(conv))][0][-1] == Cp      # the cache key carries the padded width


# ---- 3. whole frames against the unmodified reference -------------------------------------------------------------------------

def _model(r):
    cam, d_candi = gt.setup()
    m = neuralrgbd_amd.KVNET(64, cam, d_candi, gt.TWIN["sigma"], 64, None, if_refined=True, refineNet_name="DPV", t_win_r=r)
    sd = synth.seeded_state_dict(m, gt.TWIN["weight_seed"])
    m.load_state_dict(sd)
    return m.to(DEV), sd, cam, d_candi


@pytest.fixture(scope="module", params=[1, 3])
def twin(request):
    r = request.param
    g = dict(np.load(gt.path(r)))
    from oracle import gen_golden
    model, sd, cam, d_candi = _model(r)
    assert abs(gen_golden.checksum(sd.values()) - float(g["weights_checksum"])) < 1e-6 * float(g["weights_checksum"])
    return r, g, model, cam, d_candi


def _two_frames(model, cam, d_candi, wins, r):
    """KVNET.forward + PREDICT into source view r per frame (test_utils/test_KVNet.py::test), every output kept."""
    import math
    from neuralrgbd_amd import homography as Hm
    outs, pred = [], None
    pad = math.log(1. / float(len(d_candi)))
    for (rf, s, p) in wins:
        with torch.no_grad():
            r_cur, r_kv, bv_cur, dpv = model(rf.cuda(), s.cuda(), p.cuda(), torch.zeros(1), cam_intrinsics=[cam], BV_predict=pred)
            nxt = Hm.resample_vol_cuda(dpv, ops.pose_inverse(p[0, r].cuda().contiguous()), cam_intrinsic=cam, d_candi=d_candi,
                                       padding_value=pad, clamp=(-1000., 0.)).unsqueeze(0)
        outs.append(dict(bv_cur=bv_cur.clone(), dpv=dpv.clone(), pred=nxt.clone(), refined_cur=r_cur.clone(), refined=r_kv.clone()))
        pred = nxt
    return outs


def test_two_frames_vs_the_reference(twin):
    """First frame, PREDICT, update frame (the K-Net on the padded volume), PREDICT: BV_cur, DPV, both refined volumes and BV_predict
    under the gates of tests/test_gpu_parity_configs.py (_check: L1 contract, hard max gate, the arg-max rule of tests/conftest.py) on
    the pixels the fixture stores."""
    from test_gpu_parity_configs import _check
    r, g, model, cam, d_candi = twin
    outs = _two_frames(model, cam, d_candi, gt.windows(r), r)
    worst = {}
    for key, sub in gt.VOLUMES:
        name, f = key.rsplit("_f", 1)
        got = outs[int(f) - 1][name][:, :, ::sub, ::sub]
        assert torch.isfinite(got).all(), key
        kw = {}
        if name == "pred":       # a resampled volume: no depth estimate, and no further from the reference than what it resamples
            kw = dict(argmax=False, max_abs=worst["bv_cur_f1" if f == "1" else "dpv_f2"] + 2e-4)
        worst[key] = _check("t_win_r %d %s vs REFERENCE" % (r, key), got, torch.from_numpy(g[key])[None], **kw)


# ---- 4. the stream ------------------------------------------------------------------------------------------------------------

def _stream_outputs(r, wins, **kw):
    from neuralrgbd_amd.streaming import DepthStream
    model, _, cam, d_candi = _model(r)
    stream = DepthStream(model, cam, d_candi, t_win_r=r, copy_outputs=True, **kw)
    outs = []
    for rf, s, p in wins:
        o = stream.step(rf.to(DEV), s.to(DEV), p.to(DEV))
        if o is not None:
            outs.append((o[0].clone(), o[1].clone()))
    if kw.get("pipeline"):
        outs.append(stream.flush())
    torch.cuda.synchronize()
    stream.check()
    return stream, outs


@pytest.mark.parametrize("r", [1, 3])
def test_depth_stream_graph_and_pipeline_equal_eager(r):
    """DepthStream over four frames: the hipGraph replay (captured at the third frame) and the pipelined form equal the eager stream
    bit for bit; two more frames for the pipelined form, whose four graphs are captured at its sixth call."""
    wins = [synth.noise_window(180 + 10 * r + i, H, W, V=2 * r) for i in range(6)]
    _, eager = _stream_outputs(r, wins, use_graph=False)
    st_g, graph = _stream_outputs(r, wins[:4], use_graph=True)
    st_p, piped = _stream_outputs(r, wins, use_graph=True, pipeline=True)
    assert st_g._graph is not None, st_g.graph_error
    assert st_p._graph is not None, st_p.graph_error
    assert len(eager) == 6 and len(graph) == 4 and len(piped) == 6
    for f, (a, b) in enumerate(zip(eager, graph)):
        assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "graph replay differs from eager at frame %d" % f
    for f, (a, c) in enumerate(zip(eager, piped)):
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]), "pipelined differs from sequential at frame %d" % f
    assert not torch.equal(eager[1][1], eager[2][1])


@pytest.mark.parametrize("r", [1, 3])
def test_lba_depth_stream_runs_the_window(r):
    """LBADepthStream (misc.get_twin_rel_pose picks the 2 r sources) for two keyframes: finite volumes, the window's indices."""
    import lba_step_inputs as li
    from neuralrgbd_amd import lba_step
    n = 2 * r + 6
    cams = [camera.scannet_intrinsics(W // k, H // k) for k in (4, 2, 1)]
    d_candi = np.linspace(0.5, 5.0, D)
    model = neuralrgbd_amd.KVNET(64, cams[0], d_candi, 10.0, 64, None, if_refined=True, refineNet_name="DPV", t_win_r=r)
    model.load_state_dict(synth.seeded_state_dict(model, 0))
    model = model.to(DEV)
    gen = torch.Generator().manual_seed(78)
    frames = [{"img": torch.randn(1, 3, H, W, generator=gen)} for _ in range(n)]
    traj, _, _ = li.index_traj(n, seed=9)
    s = lba_step.LBADepthStream(model, cams, d_candi, r, 1, traj, LBA_max_iter=2, LBA_step=0.005, opt_vars=[1, 1])
    for ref in (r + 1, r + 2):
        with contextlib.redirect_stdout(io.StringIO()):
            BV, P, idx = s.step(ref, frames)
        assert BV.shape == (1, D, H, W) and torch.isfinite(BV).all() and len(P) == 2 * r
        assert list(idx) == lba_step.window_indices(ref + 1, r, 1)
    assert s.bv_predict is not None and torch.isfinite(s.bv_predict).all()


# ---- 5. training --------------------------------------------------------------------------------------------------------------

def _train_args(r, wins, cam, d_candi, which=1):
    rf, s, p = wins[which]
    dm, dmf = gt.labels(r)
    return (r, d_candi, [{"img": rf, "dmap": dm, "dmap_imgsize_digit": dmf}], [[{"img": s[0, v:v + 1]} for v in range(2 * r)]], p)


def test_update_iteration_vs_the_reference(twin):
    """One UPDATE-branch iteration of train() (4 NLL terms; the K-Net forward, data gradient and weight gradient on the padded
    volume) from the fixture's weights and predicted volume, plain SGD: loss, BV_predict and the weight change of the six probe tensors
    at the tolerances tests/test_gpu_train.py::test_training_iterations_vs_reference_golden applies to its update iteration."""
    from neuralrgbd_amd.train_step import train
    from oracle import gen_golden
    r, g, _, _, _ = twin
    model, sd, cam, d_candi = _model(r)
    opt = torch.optim.SGD(model.parameters(), lr=gt.TWIN["lr"])
    before = {k: model.state_dict()[k].detach().clone() for k in gen_golden.TRAIN["probes"]}
    a = _train_args(r, gt.windows(r), cam, d_candi)
    pred0 = torch.from_numpy(g["pred_f1"])[None].to(DEV)
    _, pred, loss, _, _ = train(1, model, opt, *a, pred0, [cam])
    w0 = model.kv_net.dres0[0][0].weight
    assert tuple(w0.shape) == tuple(w0.grad.shape) == (64, 6 * r + 4, 3, 3, 3)
    want = float(g["train_loss"])
    e_pred = np.abs(pred[0].cpu().numpy() - g["train_pred"])
    print("[parity] t_win_r %d train update iteration: loss %.6f vs reference %.6f; BV_predict mean|d| %.2e max %.2e" %
          (r, float(loss), want, e_pred.mean(), e_pred.max()))
    assert abs(float(loss) - want) < 2e-5 * want
    assert e_pred.mean() < 2e-3
    for k in gen_golden.TRAIN["probes"]:
        delta = (model.state_dict()[k].detach() - before[k]).cpu().numpy()
        ref_d = g["train_delta_" + k]
        assert delta.shape == ref_d.shape and np.abs(ref_d).max() > 0
        rel = np.abs(delta - ref_d).max() / np.abs(ref_d).max()
        print("[parity]   d %-62s rel err %.2e (|lr grad| max %.2e)" % (k, rel, np.abs(ref_d).max()))
        assert rel < 5e-2, (k, rel)


@pytest.mark.parametrize("r", [1, 3])
def test_train_graph_equals_eager_train(r):
    """TrainGraph.step against train() on an identical twin, the comparison of
    tests/test_gpu_train.py::test_graph_captured_iteration_equals_eager_iteration."""
    from neuralrgbd_amd.train_step import TrainGraph, train
    model, _, cam, d_candi = _model(r)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, betas=(.9, .999), capturable=True)
    rng = np.random.RandomState(r)

    def window(i):
        rf, s, p = synth.noise_window(270 + 10 * r + i, H, W, V=2 * r)
        return (rf, s, p, torch.from_numpy(rng.randint(0, D, (1, H // 4, W // 4))), torch.from_numpy(rng.randint(0, D, (1, H, W))))

    def call(m, o, w_, pred):
        rf, s, p, dm, dmf = w_
        return train(1, m, o, r, d_candi, [{"img": rf, "dmap": dm, "dmap_imgsize_digit": dmf}],
                     [[{"img": s[0, v:v + 1]} for v in range(2 * r)]], p, pred, [cam])
    pred = None
    for i in range(2):
        _, pred, _, _, _ = call(model, opt, window(i), pred)
    twin_m = copy.deepcopy(model)
    opt2 = torch.optim.Adam(twin_m.parameters(), lr=1e-4, betas=(.9, .999), capturable=True)
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    w2 = window(2)
    _, pred_e, loss_e, _, _ = call(model, opt, w2, pred)
    tg = TrainGraph(twin_m, opt2, r, d_candi, cam, warmup=0)
    loss_g, pred_g = tg.step(*[t.to(DEV) for t in w2], pred)
    torch.cuda.synchronize()
    assert tg._graph is not None
    print("[parity] t_win_r %d train graph vs eager: loss %.6f vs %.6f, max|d BV_predict|=%.2e" %
          (r, float(loss_g), float(loss_e), (pred_g - pred_e).abs().max().item()))
    assert abs(float(loss_g) - float(loss_e)) < 1e-3 * abs(float(loss_e))
    assert (pred_g - pred_e).abs().mean().item() < 1e-3
    for a, b in ((model.kv_net.dres1[0][0].weight, twin_m.kv_net.dres1[0][0].weight),
                 (model.kv_net.dres0[0][0].weight, twin_m.kv_net.dres0[0][0].weight)):
        assert (a - b).abs().max().item() < 5e-4


@pytest.mark.parametrize("form", ["train", "graph", "graph_split"])
@pytest.mark.parametrize("r", [1, 3])
def test_deterministic_training_is_bit_reproducible(r, form):
    """deterministic=True: two runs (first frame, then update iterations) give bit-identical weights — eager train(), TrainGraph in
    its one-graph form and in its split (accumulating) form."""
    from neuralrgbd_amd.optim import FusedAdam
    from neuralrgbd_amd.test_step import test as infer
    from neuralrgbd_amd.train_step import TrainGraph, train
    accum = 2 if form == "graph_split" else 1
    rng = np.random.RandomState(30 + r)
    wins = []
    for i in range(4 * accum):
        rf, s, p = synth.noise_window(4300 + 10 * r + i, H, W, V=2 * r)
        wins.append((rf.to(DEV), s.to(DEV), p.to(DEV), torch.from_numpy(rng.randint(0, D, (1, H // 4, W // 4))).to(DEV),
                     torch.from_numpy(rng.randint(0, D, (1, H, W))).to(DEV)))

    def run():
        model, _, cam, d_candi = _model(r)
        opt = FusedAdam(model.parameters(), lr=1e-4)
        if form == "train":
            pred = None
            for rf, s, p, dm, dmf in wins[:3]:
                _, pred, loss, _, _ = train(1, model, opt, r, d_candi, [{"img": rf, "dmap": dm, "dmap_imgsize_digit": dmf}],
                                            [[{"img": s[0, v:v + 1]} for v in range(2 * r)]], p, pred, [cam], deterministic=True)
        else:
            tg = TrainGraph(model, opt, r, d_candi, cam, warmup=1, accum_steps=accum, deterministic=True)
            with torch.no_grad():
                preds = [infer(model, d_candi, [cam], r, [{"img": w_[0]}], [[{"img": w_[1][0, v:v + 1]} for v in range(2 * r)]], w_[2],
                               None)[1].clone() for w_ in wins[:accum]]
            for it in range(3):                       # eager warm-up, capture + first replay, one more replay
                ws = wins[accum * (it + 1):accum * (it + 2)]
                if accum == 1:
                    loss, nxt = tg.step(*ws[0], preds[0])
                    preds = [nxt.clone()]
                else:
                    loss, preds = tg.step_windows([w_ + (preds[k],) for k, w_ in enumerate(ws)])
                assert (tg._graph is None) == (it == 0)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss))
        return {k: v.detach().clone() for k, v in model.state_dict().items()}
    s1, s2 = run(), run()
    bad = [k for k in s1 if not torch.equal(s1[k], s2[k])]
    assert not bad, "t_win_r %d %s: %d tensors differ between two deterministic runs, first %s" % (r, form, len(bad), bad[0])
    fresh = _model(r)[0].state_dict()
    assert not torch.equal(fresh["kv_net.dres0.0.0.weight"], s1["kv_net.dres0.0.0.weight"])      # the padded layer's weights moved


# ---- 6. the 5-frame window is untouched ----------------------------------------------------------------------------------------

def test_five_frame_window_still_takes_cl16_and_16_inputs(monkeypatch):
    """One update frame at t_win_r = 2: the volume comes from nrgbd_warp_volume (V = 4, channels-last: warp_volume_cl16_kernel), never
    from the new entry, is 16 channels wide, and the first layer is chosen at Cin = 16 from the 16-input tuple."""
    cam, d_candi = gt.setup()
    model = neuralrgbd_amd.KVNET(64, cam, d_candi, 10.0, 64, None, if_refined=True, refineNet_name="DPV", t_win_r=2)
    model.load_state_dict(synth.seeded_state_dict(model, 0))
    model = model.to(DEV)
    seen = {"entries": [], "first": [], "vol": []}
    lib = _lib.load()

    class Spy(object):
        def __getattr__(self, name):
            if name.startswith("nrgbd_warp_volume"):
                seen["entries"].append(name)
            return getattr(lib, name)
    monkeypatch.setattr(_lib, "load", lambda: Spy())
    choose = ops.conv3d_kernel

    def spy_choose(D_, H_, W_, Cin, Cout, cands):
        kind = choose(D_, H_, W_, Cin, Cout, cands)
        seen["first"].append((Cin, tuple(cands), kind))
        return kind
    monkeypatch.setattr(ops, "conv3d_kernel", spy_choose)
    fcl = model.kv_net.forward_channels_last
    monkeypatch.setattr(model.kv_net, "forward_channels_last", lambda vol, *a, **k: (seen["vol"].append(tuple(vol.shape)), fcl(vol, *a, **k))[1])
    outs = _two_frames(model, cam, d_candi, [synth.noise_window(s, H, W) for s in (191, 192)], 2)
    assert torch.isfinite(outs[1]["dpv"]).all()
    assert seen["entries"] == ["nrgbd_warp_volume"], seen["entries"]
    assert seen["vol"] == [(D, H // 4, W // 4, 16)]
    assert seen["first"][0] == (16, ("dw4", "dw", "pc", "direct"), "dw4"), seen["first"][0]
    assert all(c[0] == 64 for c in seen["first"][1:])
