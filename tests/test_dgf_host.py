"""Host-side checks of the guided-filter refinement net (refineNet_name='DGF'): the float64 comparator against the unmodified
reference, DGFRefineNet on host tensors, the error bound of tests/dgf_ref.py (not vacuous: a cap and six mutants), the model surface
and the refusals of the C entry and of the drivers that are out of scope.  No GPU."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import dgf_ref
import gen_dgf_golden as gg
from conftest import ROOT
from neuralrgbd_amd import _lib, nets

TILE = _lib.DGF_TILE
SHAPES = dgf_ref.gpu_shapes(TILE)
GUIDES = (False, True)          # noise; noise with a constant patch
MUTANTS = ("align_corners_false", "n9", "shift", "no_eps", "cov_xx", "no_clamp")


@functools.lru_cache(maxsize=None)
def _reference(h, w, s, patch):
    inp = dgf_ref.shape_inputs(h, w, s, patch)
    return inp, dgf_ref.dgf(*inp, bound=True)


def _golden(case):
    g = np.load(gg.path(case))
    return {k: g[k] for k in g.files}


def _net(w1, b1, w2, b2, dtype):
    net = nets.DGFRefineNet(3)
    net.load_state_dict({"feature_ext.0.weight": torch.from_numpy(w1).reshape(64, 3, 1, 1), "feature_ext.0.bias": torch.from_numpy(b1),
                         "feature_ext.2.weight": torch.from_numpy(w2).reshape(1, 64, 1, 1), "feature_ext.2.bias": torch.from_numpy(b2)})
    return net.to(dtype)


# ---- 1. the comparator is the unmodified algorithm
@pytest.mark.parametrize("case", sorted(gg.CASES))
def test_comparator_equals_the_reference_in_float64(case):
    g = _golden(case)
    out = dgf_ref.dgf(g["depth"][None], g["img"], g["w1"], g["b1"], g["w2"], g["b2"])
    err = np.abs(out[0] - g["ref64"]).max()
    print("[dgf] %s comparator - reference float64: max %.3e" % (case, err))
    assert err <= 1e-10
    # the fixture's own record of the reference's fp32 error is what the arrays say
    e = np.abs(g["ref32"].astype(np.float64) - g["ref64"])
    assert np.array_equal(g["ref32_err"], np.array([e.max(), e.mean()]))


# ---- 2. DGFRefineNet on host tensors
def _host_cases():
    for case in sorted(gg.CASES):
        yield case
    for h, w, s in SHAPES:
        for patch in GUIDES:
            yield (h, w, s, patch)


@pytest.mark.parametrize("case", list(_host_cases()), ids=str)
def test_host_net_equals_the_comparator(case):
    if isinstance(case, str):
        g = _golden(case)
        inp = (g["depth"][None], g["img"], g["w1"], g["b1"], g["w2"], g["b2"])
        want, bound = dgf_ref.dgf(*inp, bound=True)
    else:
        inp, (want, bound) = _reference(*case)
    depth, img = torch.from_numpy(inp[0])[:, None], torch.from_numpy(inp[1])[None]
    with torch.no_grad():
        got64 = _net(*inp[2:], torch.float64)(depth.double(), img.double())[:, 0].numpy()
        got32 = _net(*inp[2:], torch.float32)(depth, img)[:, 0].numpy().astype(np.float64)
    e64, e32 = np.abs(got64 - want), np.abs(got32 - want)
    print("[dgf] %s host float64 - comparator max %.3e; host fp32 max %.3e, worst |d| / bound %.3f"
          % (case, e64.max(), e32.max(), (e32 / bound).max()))
    assert e64.max() <= 1e-12
    assert (e32 <= bound).all()


def test_net_surface():
    net = nets.DGFRefineNet(3)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {
        "feature_ext.0.weight": (64, 3, 1, 1), "feature_ext.0.bias": (64,), "feature_ext.2.weight": (1, 64, 1, 1), "feature_ext.2.bias": (1,)}
    with pytest.raises(ValueError, match="in_channels"):
        nets.DGFRefineNet(4)
    d, img = torch.rand(1, 1, 2, 3), torch.rand(1, 3, 4, 6)
    for bad_d, bad_img in ((d[0], img), (d.repeat(1, 2, 1, 1), img), (d, img[:, :2]), (d, torch.rand(1, 3, 4, 9)), (d, torch.rand(1, 3, 2, 3)),
                           (torch.rand(1, 1, 1, 1), torch.rand(1, 3, 3, 3))):
        with pytest.raises(AssertionError):
            net(bad_d, bad_img)
    assert tuple(net(d, img).shape) == (1, 1, 4, 6)


# ---- 3. the bound is not vacuous
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bound_is_capped_on_every_gpu_input(shape):
    for patch in GUIDES:
        _, (_, bound) = _reference(*shape, patch)
        print("[dgf] %s patch %s: bound max %.3e mean %.3e" % (shape, patch, bound.max(), bound.mean()))
        assert np.isfinite(bound).all() and bound.max() <= 1e-3


@pytest.mark.parametrize("case", sorted(gg.CASES))
def test_bound_is_capped_on_the_golden_inputs(case):
    g = _golden(case)
    _, bound = dgf_ref.dgf(g["depth"][None], g["img"], g["w1"], g["b1"], g["w2"], g["b2"], bound=True)
    assert np.isfinite(bound).all() and bound.max() <= 1e-3


# shapes with at least one window inside the constant patch and more than one low-resolution row (the first two GPU shapes have
# neither: 4 x 4 from one value, and a 2 x 2 patch)
@pytest.mark.parametrize("shape", SHAPES[2:], ids=str)
@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_leave_the_bound(mutant, shape):
    inp, (want, bound) = _reference(*shape, mutant == "no_eps")            # eps matters where var = 0: the constant patch
    got = dgf_ref.dgf(*inp, mutant=mutant)
    frac = float((~(np.abs(got - want) <= bound)).mean())                   # a NaN is outside the bound
    print("[dgf] mutant %s at %s: %.1f %% of the pixels outside the bound" % (mutant, shape, 100 * frac))
    assert frac >= 0.01


def test_constant_guide_gives_the_double_box_mean():
    """Where the guide is constant var = 0 and A = 0: the comparator's output there is the double box mean of y."""
    for shape in (SHAPES[-2], SHAPES[-1]):              # two tiles plus s per axis, and 256 x 384: the patch has an interior
        inp, (want, bound) = _reference(*shape, True)
        H, W = inp[1].shape[1:]
        y, _ = dgf_ref.upsample(inp[0].astype(np.float64), H, W)
        inner = np.zeros((H, W), bool)
        inner[H // 3 + 2:H - H // 3 - 2, W // 3 + 2:W - W // 3 - 2] = True      # every window of every contributing A inside the patch
        assert inner.any()
        assert (np.abs(want - dgf_ref.box_mean_twice(y))[:, inner] <= bound[:, inner]).all()


# ---- 4. the model surface
def _model(**kw):
    import neuralrgbd_amd
    cam, d_candi = gg.model_setup()
    m = gg.MODEL
    return neuralrgbd_amd.KVNET(64, cam, d_candi, m["sigma"], 64, None, if_refined=True, refineNet_name="DGF", t_win_r=m["r"], **kw), cam, d_candi


def test_state_dict_keys_and_shapes_equal_the_reference():
    g = np.load(gg.model_path())
    for kw in ({}, {"if_upsample_d": True}):            # if_upsample_d has no effect on a DGF model, as in the reference
        model, _, _ = _model(**kw)
        sd = model.state_dict()
        assert list(sd.keys()) == [str(k) for k in g["state_dict_keys"]]
        assert [",".join(str(n) for n in v.shape) for v in sd.values()] == [str(s) for s in g["state_dict_shapes"]]
    assert isinstance(model.r_net, nets.DGFRefineNet) and not model.feature_extractor.multi_scale and not model.d_net.output_features


def test_host_forward_returns_the_reference_shapes_and_first_frame_tuple():
    """The D-Net has no host path (its kernels refuse host tensors), so the frame starts from a measure() record of host tensors:
    everything behind the D-Net — regression, the DGF net, the return tuple — runs in torch."""
    g = np.load(gg.model_path())
    model, cam, d_candi = _model()
    m = gg.MODEL
    torch.manual_seed(5)
    ref = torch.randn(1, 3, m["H"], m["W"])
    bv = torch.log_softmax(torch.randn(1, m["D"], m["H"] // 4, m["W"] // 4), dim=1)
    rec = {"BV_cur": bv, "features": [ref], "texels": None, "rgb4": None}
    with torch.no_grad():
        out = model(ref, None, None, torch.zeros(1), cam_intrinsics=[cam], BV_predict=None, measured=rec)
        nan = model(ref, None, None, torch.zeros(1), cam_intrinsics=[cam], BV_predict=torch.full_like(bv, float("nan")), measured=rec)
    for res in (out, nan):                              # first frame, and an invalid BV_predict
        assert [",".join(str(n) for n in t.shape) for t in res] == [str(s) for s in g["shapes_f1"]]
        assert [res[0] is res[1], res[2] is res[3]] == list(g["first_frame_pairs"]) == [True, True]
        assert res[2] is bv
    # the refined map is the DGF net on the regressed depth under the reference frame
    low = (torch.exp(bv) * torch.as_tensor(d_candi, dtype=torch.float32).view(1, -1, 1, 1)).sum(1, keepdim=True)
    with torch.no_grad():
        assert torch.equal(out[0], model.r_net(low, ref))
    assert list(g["shapes_f2"]) == list(g["shapes_f1"])           # the update frame's shapes: checked on the GPU (test_gpu_dgf_net.py)


def test_unknown_refinement_net_is_refused_by_name():
    import neuralrgbd_amd
    cam, d_candi = gg.model_setup()
    with pytest.raises(NotImplementedError, match="XYZ"):
        neuralrgbd_amd.KVNET(64, cam, d_candi, 10.0, 64, None, if_refined=True, refineNet_name="XYZ")
    with pytest.raises(ValueError, match="in_channels"):
        neuralrgbd_amd.KVNET(64, cam, d_candi, 10.0, 64, None, if_refined=True, refineNet_name="DGF", refine_channel=1)


# ---- 5. the C entry and the drivers that are out of scope
def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nrgbd.h")).read()
    assert "nrgbd_dgf_refine_f32(" in header and "Refine.py:620-641" in header and "guided_filter.py:54-97" in header
    decl = re.search(r"int nrgbd_dgf_refine_f32\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
    assert decl.count(",") + 1 == len(_lib.SIGNATURES["nrgbd_dgf_refine_f32"][1]) == 14
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "nrgbd_dgf_refine_f32")
    assert header.count('#define NRGBD_INTERFACE_VERSION "0.10"') == 1
    from neuralrgbd_amd import ops
    assert ops.DGF_TILE == TILE == (int(re.search(r"#define NRGBD_DGF_TILE_Y (\d+)", header).group(1)),
                                    int(re.search(r"#define NRGBD_DGF_TILE_X (\d+)", header).group(1)))


def test_entry_refuses_bad_arguments_without_a_gpu():
    fn = _lib.load().nrgbd_dgf_refine_f32
    P = ctypes.c_void_p(64)                            # never dereferenced: every call below is refused before anything touches the device
    E_NULL, E_SHAPE, E_ARG = -1, -2, -4

    def call(n=1, h=8, w=12, H=32, W=48, eps=1e-8, null=None):
        ptr = [None if i == null else P for i in range(7)]          # depth_lr, img, w1, b1, w2, b2, out
        return fn(ptr[0], n, h, w, ptr[1], H, W, ptr[2], ptr[3], ptr[4], ptr[5], eps, ptr[6], None)
    for i in range(7):
        assert call(null=i) == E_NULL
    for kw in (dict(h=0), dict(w=-1), dict(H=0), dict(W=0), dict(H=33), dict(W=50), dict(H=16, W=48), dict(H=32, W=24),
               dict(h=32, w=48), dict(h=1, w=1, H=3, W=3), dict(h=1, w=2, H=2, W=4), dict(h=2, w=1, H=4, W=2), dict(h=1, w=8, H=3, W=24),
               dict(h=8192, w=4, H=32768, W=16)):
        assert call(**kw) == E_SHAPE, kw
    for kw in (dict(n=0), dict(n=3), dict(n=-1), dict(eps=-1e-8), dict(eps=float("nan"))):
        assert call(**kw) == E_ARG, kw
    assert call(null=0, h=0, n=3) == E_NULL and call(h=0, n=3) == E_SHAPE          # the order of the checks


def test_ops_refuses_host_tensors():
    from neuralrgbd_amd import ops
    with pytest.raises(_lib.NrgbdError):
        ops.dgf_refine(torch.zeros(1, 8, 12), torch.zeros(3, 32, 48), torch.zeros(64, 3), torch.zeros(64), torch.zeros(64), torch.zeros(1))


def test_out_of_scope_drivers_refuse_a_dgf_model_by_name():
    from neuralrgbd_amd import evaluate, export_res, lba_step, train_step, train_video
    model, cam, d_candi = _model()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    match = "refineNet_name='DGF'"
    with pytest.raises(_lib.NrgbdError, match=match):
        train_step.train(1, model, opt, 2, d_candi, [{}], [[{}]], torch.zeros(1, 4, 4, 4), None, [cam])
    with pytest.raises(NotImplementedError, match="DGF"):
        train_step.train(1, model, opt, 2, d_candi, [{}], [[{}]], torch.zeros(1, 4, 4, 4), None, [cam], loss_type="L1")
    with pytest.raises(_lib.NrgbdError, match=match):
        train_step.TrainGraph(model, opt, 2, d_candi, cam)
    with pytest.raises(_lib.NrgbdError, match=match):
        train_video.TrainVideoStream(model, opt, cam, d_candi, t_win_r=2)
    with pytest.raises(_lib.NrgbdError, match=match):
        evaluate.EvalVideoStream(model, cam, d_candi, t_win_r=2)
    with pytest.raises(_lib.NrgbdError, match=match):
        lba_step.LBADepthStream(model, [cam, cam, cam], d_candi, 2, 5, [np.eye(4)] * 11)
    dmap = torch.zeros(1, 1, 16, 16)
    with pytest.raises(_lib.NrgbdError, match=match):
        export_res.depth_conf_u16(dmap, d_candi)
    with pytest.raises(_lib.NrgbdError, match=match):
        export_res.export_res_img({"img": torch.zeros(1, 3, 16, 16)}, dmap, d_candi, "/nonexistent", 0)
