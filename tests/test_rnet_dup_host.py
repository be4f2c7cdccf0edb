"""The R-Net with candidate up-sampling (KVNET(if_upsample_d=True), Refine.py:44-49), the host side: the model's state dict against
the reference's (tests/golden/rnet_dup_d32.npz, tests/gen_rnet_dup_golden.py), the per-level candidate widths, the embedded weights
against the float64 module graph, the up-sampled candidates, the training call's argument check and the new entries' declarations."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_rnet_dup_golden as gd
from conftest import ROOT
from neuralrgbd_amd import _lib, misc, nets, synth


def _kvnet(upsample=True, D=None):
    import neuralrgbd_amd
    cam, d_candi = gd.setup()
    if D is not None:
        d_candi = np.linspace(gd.DUP["d_min"], gd.DUP["d_max"], D)
    return neuralrgbd_amd.KVNET(64, cam, d_candi, gd.DUP["sigma"], 64, None, if_refined=True, refineNet_name="DPV", t_win_r=gd.DUP["r"],
                                if_upsample_d=upsample), cam, d_candi


def test_state_dict_keys_and_shapes_equal_the_reference():
    g = np.load(gd.PATH)
    sd = _kvnet()[0].state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == gd.state_dict_lines(g)
    D = gd.DUP["D"]
    assert tuple(sd["r_net.conv2_2.weight"].shape) == (4 * D, 4 * D, 3, 3)
    assert tuple(sd["r_net.trans_conv1.0.weight"].shape) == (2 * D + 32, 4 * D, 4, 4)


def test_levels():
    up = lambda D: nets.DPVUpsampleNet(64, 32, 3, D=D, upsample_D=True)
    assert up(32)._levels() == ((32, 64), (64, 64), (128, 128))
    assert up(64)._levels() == ((64, 64), (128, 128), (256, 256))
    for D in (16, 128, 200):
        assert up(D)._levels() is None and up(D)._widths() is None
    assert up(32)._widths() is None and up(64)._widths() is None          # the 5-tuple describes nets without up-sampling only
    for D, Dp in ((16, 64), (64, 64), (100, 128), (128, 128)):
        net = nets.DPVUpsampleNet(64, 32, 3, D=D)
        assert net._levels() == ((D, Dp),) * 3 and net._widths() == (D, Dp, 64, 32, 3)
    assert nets.DPVUpsampleNet(64, 32, 3, D=200)._levels() is None
    assert nets.DPVUpsampleNet(32, 32, 3, D=64, upsample_D=True)._levels() is None      # another feature width


@pytest.mark.parametrize("D", [32, 64])
def test_embedded_weights_reproduce_the_float64_module_graph(D):
    """DPVUpsampleNet._embedded with per-level padding: the re-indexed weights, evaluated with plain torch convolutions on the padded
    channel layout of each level [D_l real | Dp_l - D_l zero | image features], reproduce the module graph (Refine.py:79-107)."""
    torch.manual_seed(0)
    net = nets.DPVUpsampleNet(64, 32, 3, D=D, upsample_D=True).double()
    net.load_state_dict({k: v.double() for k, v in synth.seeded_state_dict(net, 5).items()})
    for m in net.modules():
        if getattr(m, "bias", None) is not None:
            torch.nn.init.normal_(m.bias, 0, 0.1)
    lv = net._levels()
    h, w = 6, 8
    dpv = torch.softmax(torch.randn(1, D, h, w, dtype=torch.float64), 1)
    feats = [torch.randn(1, 64, h, w, dtype=torch.float64), torch.randn(1, 32, 2 * h, 2 * w, dtype=torch.float64),
             torch.rand(1, 3, 4 * h, 4 * w, dtype=torch.float64)]
    with torch.no_grad():
        want = net(dpv, feats)                                   # the CPU module graph
        e = net._embedded()
        pad = lambda x, f, l: torch.cat((x, x.new_zeros(1, lv[l][1] - x.shape[1], *x.shape[2:]), f), 1)
        cl = lambda x, k: F.leaky_relu(F.conv2d(x, e[k][0], e[k][1], 1, 1), 0.01)
        tl = lambda x, k: F.leaky_relu(F.conv_transpose2d(x, e[k][0], e[k][1], 2, 1), 0.01)
        x = cl(cl(pad(dpv, feats[0], 0), "conv0"), "conv0_1")
        assert x.shape[1] == lv[0][1] + 64 and bool((x[:, lv[0][0]:lv[0][1]] == 0).all())
        x = tl(x, "trans_conv0")
        assert x.shape[1] == lv[1][1] == 2 * D
        x = cl(cl(torch.cat((x, feats[1]), 1), "conv1"), "conv1_1")
        x = tl(x, "trans_conv1")
        assert x.shape[1] == lv[2][1] == 4 * D
        x = cl(cl(torch.cat((x, feats[2]), 1), "conv2"), "conv2_1")
        z = F.conv2d(x, e["conv2_2"][0], e["conv2_2"][1], 1, 1)
        assert float(e["conv2_2"][1].min()) > -1e29              # the last level is not padded: no -1e30 bias
        got = torch.log_softmax(z, 1)
    assert got.shape == want.shape == (1, 4 * D, 4 * h, 4 * w)
    assert (got - want).abs().max().item() < 1e-9


def test_d_candi_up4_is_the_loaders_linspace():
    for d in (np.linspace(0.1, 5.0, 32), np.linspace(1.0, 60.0, 64), np.array([0.5, 0.7, 1.3, 4.0])):
        up = misc.d_candi_up4(d)
        assert up.shape == (4 * len(d),) and np.array_equal(up, np.linspace(d.min(), d.max(), len(d) * 4))


def test_training_flag_and_model_must_agree():
    from neuralrgbd_amd.train_step import TrainGraph, train
    plain, cam, d_candi = _kvnet(upsample=False)
    dup, _, _ = _kvnet(upsample=True)
    opt = torch.optim.SGD(plain.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="refine_dup"):
        train(1, plain, opt, 2, d_candi, [{}], [[{}]], torch.zeros(1, 4, 4, 4), None, [cam], refine_dup=True)
    with pytest.raises(ValueError, match="refine_dup"):
        train(1, dup, opt, 2, d_candi, [{}], [[{}]], torch.zeros(1, 4, 4, 4), None, [cam])
    with pytest.raises(ValueError, match="refine_dup"):
        TrainGraph(plain, opt, 2, d_candi, cam, refine_dup=True)
    with pytest.raises(ValueError, match="refine_dup"):
        TrainGraph(dup, opt, 2, d_candi, cam)
    with pytest.raises(NotImplementedError):
        train(1, dup, opt, 2, d_candi, [{}], [[{}]], torch.zeros(1, 4, 4, 4), None, [cam], refine_dup=True, loss_type="L1")


def test_training_path_widths_of_the_upsampling_net():
    """The module path under autograd at the widths of a 64-candidate up-sampling net: the 259-wide full-resolution layers run 272 / 272
    (four 64-column groups + 3 columns on conv_few), conv2_1 reads the 272 wide tensor, conv1 (160 -> 160) is two groups and a 32-column
    tail, and the data gradient of trans_conv1 (its four phases as one 160 -> 1024 layer) has the same tail."""
    from neuralrgbd_amd.autograd import Conv2dCL, _padded_widths
    assert _padded_widths(259, 259, 1, True) == (272, 272)
    assert Conv2dCL._rnet_plan(272, 272, 1, 259) == (256, ("few", 3))
    assert _padded_widths(272, 256, 1, True, real=(259, 256)) == (272, 256)
    assert Conv2dCL._rnet_plan(272, 256, 1, 256) == (256, None) and Conv2dCL._rnet_plan(256, 272, 1, 259) == (256, ("few", 3))
    assert _padded_widths(160, 160, 1, True) == (160, 160) and Conv2dCL._rnet_plan(160, 160, 1) == (128, ("half", 32))
    assert _padded_widths(160, 1024, 1, True) == (160, 1024) and Conv2dCL._rnet_plan(1024, 160, 1, 160) == (128, ("half", 32))
    assert _padded_widths(131, 131, 1, True) == (144, 144)                     # from 32 candidates: the widths of a 128-candidate net


def test_lba_stream_refuses_an_upsampling_model():
    from neuralrgbd_amd import camera, lba_step
    model, _, d_candi = _kvnet()
    cams = [camera.scannet_intrinsics(gd.DUP["W"] // k, gd.DUP["H"] // k) for k in (4, 2, 1)]
    with pytest.raises(_lib.NrgbdError, match="if_upsample_d"):
        lba_step.LBADepthStream(model, cams, d_candi, 2, 1, [np.eye(4)] * 8)


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "nrgbd.h")).read()
    for new, old in (("nrgbd_depth_regress_rows", "nrgbd_depth_regress"), ("nrgbd_export_depth_u16_rows", "nrgbd_export_depth_u16")):
        assert new + "(" in header
        assert _lib.SIGNATURES[new] == _lib.SIGNATURES[old]
    assert "Refine.py:44-49" in header and "Refine.py:104" in header and "misc.py:532-548" in header
    assert header.count('#define NRGBD_INTERFACE_VERSION "0.10"') == 1
