"""warp_volume (csrc/warpvol.hip: warp_volume_kernel and warp_volume_cl16_kernel<false|true>) held element by element against the
exact-position float64 comparator of tests/warp_exact.py: |got - exact| <= bound on the warped channels (the bound is derived there
from the arithmetic), the reference and belief channels bit-exact, an element without a valid tap exactly 0.  The fast kernel must in
addition equal the general kernel bit for bit on every family: the test of the "same bits" claim of div_pair / div_by_const
(common.hpp) at denominators of 1e-10 and of either sign.  tests/test_warp_exact_host.py checks the comparator and the families
without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import warp_exact as wx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRIDS = [(7, 9, 1), (20, 36, 5), (33, 65, 8)]      # h*w below / above one 256-thread workgroup, never a multiple of it; D in {1, 5, 8}
_worst = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _texels(case, V, offset):
    """[V + 1, h, w, 68] texel tensor (sources, then the reference) with the RGB word at channels offset .. offset + 2; the other
    channels hold noise that must never reach the output."""
    _, Cs, h, w = case["src"].shape
    rng = np.random.RandomState(5)
    tex = rng.standard_normal((V + 1, h, w, 68)).astype(np.float32) * 100
    tex[:V, :, :, offset:offset + Cs] = case["src"][:V].transpose(0, 2, 3, 1)
    tex[V, :, :, offset:offset + Cs] = case["ref"].transpose(1, 2, 0)
    return _dev(tex)


def _warp(case, align, V=None, layout="planar", with_ref=True, with_bv=True, channels_last=False, offset=64):
    """One ops.warp_volume call on the first V views of a case -> numpy, always returned planar [channels, D, h, w].
    layouts: "planar" contiguous [V,Cs,h,w]; "texel" channels offset.. of a 68-wide NHWC tensor; "strided" a planar source
    inside a larger buffer (row pitch w + 3, plane pitch (h + 2)(w + 3) + 5)."""
    from neuralrgbd_amd import ops
    nV, Cs, h, w = case["src"].shape
    V = nV if V is None else V
    keep = None
    if layout == "planar":
        src, ss = _dev(case["src"][:V]), (Cs * h * w, h * w, w, 1)
        ref, rs = _dev(case["ref"]), (h * w, w, 1)
    elif layout == "texel":
        keep = _texels(case, V, offset)
        src, ss = keep[:V, :, :, offset:], (h * w * 68, 1, w * 68, 68)
        ref, rs = keep[V, :, :, offset:], (1, w * 68, 68)
    elif layout == "strided":
        pitch, plane = w + 3, (h + 2) * (w + 3) + 5
        buf = torch.full(((V * Cs + Cs) * plane + 7,), 1e6, dtype=torch.float32, device=DEV)
        both = np.concatenate([case["src"][:V].reshape(V * Cs, h, w), case["ref"]])
        for c in range(V * Cs + Cs):
            buf[7 + c * plane:7 + c * plane + h * pitch].view(h, pitch)[:, :w] = _dev(both[c])
        keep = buf
        src, ss = buf[7:], (Cs * plane, plane, pitch, 1)
        ref, rs = buf[7 + V * Cs * plane:], (plane, pitch, 1)
    else:
        raise ValueError(layout)
    out = ops.warp_volume(src, ss, ref if with_ref else None, rs if with_ref else None, _dev(case["KR"][:V]), _dev(case["Kt"][:V]),
                          _dev(case["rays"]), _dev(case["d_candi"]), case["cx"], case["cy"], V, Cs, h, w,
                          bv_cur=_dev(case["bv_cur"]) if with_bv else None, bv_pred=_dev(case["bv_pred"]) if with_bv else None,
                          align_corners=align, channels_last=channels_last)
    torch.cuda.synchronize()
    n_ch = V * Cs + (Cs if with_ref else 0) + (1 if with_bv else 0)
    D = len(case["d_candi"])
    assert tuple(out.shape) == ((D, h, w, n_ch) if channels_last else (n_ch, D, h, w))
    out = out.permute(3, 0, 1, 2) if channels_last else out
    return out.cpu().numpy()


def _compare(name, kernel, got, case, align, V=None, with_ref=True, with_bv=True):
    want, bound = wx.assemble(case, align, V, with_ref, with_bv)
    ratio, at, beyond = wx.worst_ratio(got, want, bound)
    nwarp = want.shape[0] - (case["src"].shape[1] if with_ref else 0) - (1 if with_bv else 0)
    exact_tail = np.array_equal(got[nwarp:].astype(np.float64), want[nwarp:])
    print("[parity] warp_volume %-7s %-40s worst error / bound %.3f at %s, %d beyond" % (kernel, name, ratio, at, beyond))
    _worst[kernel] = max(_worst.get(kernel, 0.0), ratio)
    assert beyond == 0 and exact_tail, name
    return ratio


# ---- the K-Net fast kernel -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("family", wx.FAMILIES)
@pytest.mark.parametrize("h,w,D", GRIDS + [wx.BORDER_POW2 + (5,)])
def test_fast_kernel_vs_comparator_and_general_kernel(h, w, D, family, align):
    """warp_volume_cl16_kernel<align>: V = 4, Cs = 3, the RGB word of a 68-wide texel tensor, channels-last output.  Against the
    comparator, and bit for bit against warp_volume_kernel (planar source, same output layout): on_plane (denominator 1e-10 on
    whole planes) and behind (negative denominators) are where div_pair could part from the IEEE division."""
    case = wx.make_case(h, w, D, 4, 3, family)
    fast = _warp(case, align, layout="texel", channels_last=True)
    name = "%s %dx%dx%d align=%d" % (family, h, w, D, align)
    _compare(name, "cl16<%d>" % align, fast, case, align)
    general = _warp(case, align, layout="planar", channels_last=True)
    _compare(name, "general", general, case, align)
    differ = int((fast.view(np.int32) != general.view(np.int32)).sum())
    assert differ == 0, "%s: %d elements of the fast kernel differ in bits from the general kernel" % (name, differ)


# ---- the general kernel: every channel assembly, planar and channels-last ------------------------------------------------------

GENERAL = [  # V, Cs, ref, bv, align, family, (h, w, D)
    (1, 1, False, False, False, "large", GRIDS[0]),
    (1, 3, True, False, True, "border", GRIDS[1]),
    (2, 4, False, True, False, "behind", GRIDS[1]),        # bv without ref
    (2, 1, True, True, True, "on_plane", GRIDS[2]),
    (4, 3, True, True, True, "large", GRIDS[1]),
    (4, 3, False, False, False, "border", GRIDS[2]),        # V = 4 without ref / bv: not the fast kernel's assembly
    (4, 3, True, False, False, "on_plane", GRIDS[1]),       # 3V + 3
    (4, 3, False, True, True, "behind", GRIDS[0]),          # 3V + 1
    (5, 3, True, True, False, "behind", GRIDS[2]),          # V != 4 with the full assembly
    (5, 4, True, True, True, "border", wx.BORDER_POW2 + (5,)),
    (5, 1, False, True, False, "on_plane", GRIDS[0]),
    (2, 3, True, True, False, "large", GRIDS[2]),
    (1, 4, True, True, False, "border", wx.BORDER_POW2 + (8,)),
    (4, 4, True, True, True, "on_plane", GRIDS[2]),
]


@pytest.mark.parametrize("V,Cs,ref,bv,align,family,grid", GENERAL)
def test_general_kernel_planar_and_channels_last(V, Cs, ref, bv, align, family, grid):
    h, w, D = grid
    case = wx.make_case(h, w, D, 5, Cs, family)
    name = "%s %dx%dx%d V%d Cs%d ref%d bv%d align=%d" % (family, h, w, D, V, Cs, ref, bv, align)
    planar = _warp(case, align, V, "planar", ref, bv, channels_last=False)
    _compare(name, "general", planar, case, align, V, ref, bv)
    cl = _warp(case, align, V, "planar", ref, bv, channels_last=True)
    assert np.array_equal(cl.view(np.int32), planar.view(np.int32)), name + ": channels-last differs from planar"


# ---- dispatch ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("family", ["on_plane", "large"])
def test_misaligned_word_falls_back_to_the_general_kernel(family, align):
    """The same V = 4 inputs with the RGB word at channel 65 of the texel: the source pointer is 4 bytes past a 16-byte boundary, so
    a 16-byte load would be misaligned; the call must take warp_volume_kernel and give identical values."""
    h, w, D = GRIDS[1]
    case = wx.make_case(h, w, D, 4, 3, family)
    aligned = _warp(case, align, layout="texel", channels_last=True, offset=64)
    shifted = _warp(case, align, layout="texel", channels_last=True, offset=65)
    _compare("%s offset 65 align=%d" % (family, align), "general", shifted, case, align)
    assert np.array_equal(shifted.view(np.int32), aligned.view(np.int32))


@pytest.mark.parametrize("channels_last", [False, True])
def test_non_contiguous_planar_source_through_strides(channels_last):
    h, w, D = GRIDS[1]
    case = wx.make_case(h, w, D, 4, 3, "large")
    got = _warp(case, False, layout="strided", channels_last=channels_last)
    _compare("strided planar cl=%d" % channels_last, "general", got, case, False)
    assert np.array_equal(got.view(np.int32), _warp(case, False, layout="planar").view(np.int32))


def test_python_surface_align_corners():
    """homography.warp_img_feats_v3(..., align_corners=True) on the project's own camera, against the comparator."""
    from neuralrgbd_amd import camera, homography
    h, w, D = GRIDS[1]
    V, Cs = 3, 3
    case = wx.make_case(h, w, D, V, Cs, "large")
    cam = camera.scannet_intrinsics(w, h)
    assert np.array_equal(cam["intrinsic_M_cuda"].numpy(), case["K"])
    maps = [_dev(case["src"][v:v + 1]) for v in range(V)]
    Rs = [_dev(case["poses"][v, :3, :3]) for v in range(V)]
    ts = [_dev(case["poses"][v, :3, 3]) for v in range(V)]
    views = homography.warp_img_feats_v3(maps, case["d_candi"], Rs, ts, cam, align_corners=True)
    assert len(views) == V and tuple(views[0].shape) == (Cs, D, h, w)
    got = torch.cat(list(views), 0).cpu().numpy()
    _compare("warp_img_feats_v3 align=1", "general", got, case, True, V, with_ref=False, with_bv=False)


def test_argument_checks():
    from neuralrgbd_amd import _lib
    lib = _lib.load()
    x = torch.zeros(4096, device=DEV)
    p = ctypes.c_void_p(x.data_ptr())

    def call(src=p, bv_cur=None, bv_pred=None, V=1, Cs=1, D=1, h=2, w=2):
        return lib.nrgbd_warp_volume(src, 4, 4, 2, 1, None, 0, 0, 0, p, p, p, p, 1.0, 1.0, 0, bv_cur, bv_pred, p, V, Cs, D, h, w, 0, None)

    assert call(V=17) == -2
    assert call(D=65536) == -2
    assert call(Cs=0) == -2
    assert call(bv_cur=p) == -1 and call(bv_pred=p) == -1
    assert call(src=None) == -1
    torch.cuda.synchronize()


def test_two_calls_give_equal_bits():
    h, w, D = GRIDS[2]
    case = wx.make_case(h, w, D, 4, 3, "large")
    for layout, cl in (("texel", True), ("planar", False)):
        a, b = _warp(case, True, layout=layout, channels_last=cl), _warp(case, True, layout=layout, channels_last=cl)
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_report_worst_fraction_of_the_bound():
    """Last in the file: the worst observed fraction of the bound per kernel over the tests above."""
    for kernel in sorted(_worst):
        print("[parity] warp_volume %-8s worst error / bound over this file: %.3f" % (kernel, _worst[kernel]))
    assert all(v <= 1.0 for v in _worst.values())
