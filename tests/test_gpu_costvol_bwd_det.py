"""The bit-reproducible cost-volume backward (csrc/costvol_bwd_det.hip; ops.costvol_bwd(..., deterministic=True)).

  parity      every element of g_ref and g_src within 1 x the bound of the exact-position float64 comparator
              (tests/costvol_bwd_exact.py: the bound the atomic kernels are held to, valid for any summation order), on the
              shape lists, geometry families and contents of tests/test_gpu_costvol_bwd.py;
  bits        the same bits on every run: through ops, through the raw C entry with NaN-filled workspace and outputs, on a
              non-default stream;
  views       nothing couples the views in g_src: view v of a joint call equals a V = 1 call on view v alone, bit for bit;
  wiring      PlaneSweepCost follows neuralrgbd_amd.autograd.deterministic().
"""
import ctypes

import numpy as np
import pytest
import torch

import costvol_bwd_exact as cx
import costvol_bwd_gpu
from costvol_bwd_gpu import DEV, LDS_SHAPES, _compare, _nchw, _upload
from neuralrgbd_amd import ops

pytestmark = pytest.mark.gpu


def _run(case, dist, align, stream=None):
    return costvol_bwd_gpu._run(case, dist, align, deterministic=True, stream=stream)


def _run_raw_from_nan(case, dist, align):
    """The C entry itself, workspace and both outputs pre-filled with NaN."""
    from neuralrgbd_amd import _lib
    lib = _lib.load()
    V, C, h, w = case["src"].shape
    D, Cp = len(case["d_candi"]), ops.padded_channels(C)
    tex, KR, Kt, rays, d, g = _upload(case)
    n = ctypes.c_size_t(0)
    assert lib.nrgbd_costvol_bwd_det_workspace(V, Cp, D, h, w, ctypes.byref(n)) == 0
    assert n.value == 12 * V * Cp * h * w
    work = torch.full((n.value // 4,), float("nan"), device=DEV)
    g_ref = torch.full((h, w, Cp), float("nan"), device=DEV)
    g_src = torch.full((V, h, w, Cp), float("nan"), device=DEV)
    ref_t, src_t = tex[V].contiguous(), tex[:V].contiguous()
    rc = lib.nrgbd_costvol_bwd_det(ref_t.data_ptr(), src_t.data_ptr(), KR.data_ptr(), Kt.data_ptr(), rays.data_ptr(), d.data_ptr(),
                                   case["cx"], case["cy"], case["sigma"], ops.DIST[dist], int(align), g.data_ptr(), g_ref.data_ptr(),
                                   g_src.data_ptr(), V, C, Cp, D, h, w, work.data_ptr(), n.value, None)
    assert rc == 0
    torch.cuda.synchronize()
    return _nchw(g_ref, g_src)


def _check(case, dist, align, label=None):
    V, C, h, w = case["src"].shape
    got_ref, got_src = _run(case, dist, align)
    name = "%s %dx%dx%d V%d C%d" % (label or case["key"][5], h, w, len(case["d_candi"]), V, C)
    return _compare(name, case, dist, align, got_ref, got_src, "costvol_bwd_det"), got_ref, got_src


# ---- parity at 1 x bound -------------------------------------------------------------------------------------------------------

LARGE_SHAPES = [
    (96, 128, 4, 1, 6, "small"),
    (97, 131, 4, 4, 67, "small"),
    (96, 128, 9, 4, 67, "driver"),
    (97, 131, 9, 1, 6, "large"),
    (97, 131, 33, 4, 6, "driver"),
    (96, 128, 33, 4, 67, "small"),
    (96, 128, 64, 1, 67, "driver"),
    (97, 131, 64, 4, 67, "driver"),
]


@pytest.mark.parametrize("dist", ["L2", "L1"])
@pytest.mark.parametrize("h,w,D,V,C,family", LDS_SHAPES)
def test_det_shapes_of_the_lds_kernel(h, w, D, V, C, family, dist):
    _check(cx.make_case(h, w, D, V, C, family), dist, False)


@pytest.mark.parametrize("dist", ["L2", "L1"])
@pytest.mark.parametrize("h,w,D,V,C,family", LARGE_SHAPES)
def test_det_shapes_of_the_global_kernel(h, w, D, V, C, family, dist):
    _check(cx.make_case(h, w, D, V, C, family), dist, False)


@pytest.mark.parametrize("dist", ["L2", "L1"])
@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("family", cx.FAMILIES)
@pytest.mark.parametrize("shape", ["lds", "global"])
def test_det_geometry_families(shape, family, align, dist):
    h, w, D, V, C = cx.FAMILY_SHAPE_LDS if shape == "lds" else cx.FAMILY_SHAPE_GLOBAL
    _check(cx.make_case(h, w, D, V, C, family), dist, align)


@pytest.mark.parametrize("dist", ["L2", "L1"])
@pytest.mark.parametrize("content,gmode", [("relu", "normal"), ("relu", "blocks"), ("normal", "blocks"), ("relu", "alternate")])
@pytest.mark.parametrize("shape", ["lds", "global"])
def test_det_dead_channels_and_zero_g(shape, content, gmode, dist):
    h, w, D, V, C = cx.FAMILY_SHAPE_LDS if shape == "lds" else cx.FAMILY_SHAPE_GLOBAL
    case = cx.make_case(h, w, D, V, C, "small", content, gmode)
    ex, got_ref, got_src = _check(case, dist, False, "%s/%s" % (content, gmode))
    if content == "relu":
        dead = [1, C - 1]
        assert (ex["g_ref"][dead] == 0).all() and (ex["g_src"][:, dead] == 0).all()
        assert (got_ref[dead] == 0).all() and (got_src[:, dead] == 0).all()
        assert np.abs(got_ref[0]).max() > 0 and np.abs(got_src[:, 0]).max() > 0
    if gmode != "normal":
        only_zero_g = (ex["reach_src"] > 0) & (ex["n_src"] == 0)        # texels whose every sample has g == 0
        if gmode == "blocks":
            assert only_zero_g.sum() > 0
        assert (got_src[np.broadcast_to(only_zero_g[:, None], got_src.shape)] == 0).all()
        assert (got_ref[:, ex["n_ref"] == 0] == 0).all() and ((ex["n_ref"] == 0).sum() > 0) == (gmode == "blocks")


# ---- the same bits on every run ------------------------------------------------------------------------------------------------

BIT_CASES = [("driver", (64, 96, 64, 4, 67)), ("scatter", cx.FAMILY_SHAPE_LDS), ("zoom_far", cx.FAMILY_SHAPE_LDS),
             ("driver", (96, 128, 9, 4, 67))]


@pytest.mark.parametrize("dist", ["L2", "L1"])
@pytest.mark.parametrize("family,shape", BIT_CASES)
def test_det_three_runs_same_bits(family, shape, dist):
    """ops on the current stream, the raw C entry on the null stream with NaN-filled workspace and outputs, ops on a stream of its
    own: three launches with different buffers, different previous contents and different queues."""
    h, w, D, V, C = shape
    case = cx.make_case(h, w, D, V, C, family)
    a_ref, a_src = _run(case, dist, False)
    b_ref, b_src = _run_raw_from_nan(case, dist, False)
    c_ref, c_src = _run(case, dist, False, stream=torch.cuda.Stream())
    assert np.isfinite(b_ref).all() and np.isfinite(b_src).all()
    assert np.abs(a_src).max() > 0 and np.abs(a_ref).max() > 0
    for name, x, y in (("g_ref raw/NaN", a_ref, b_ref), ("g_src raw/NaN", a_src, b_src), ("g_ref stream", a_ref, c_ref),
                       ("g_src stream", a_src, c_src)):
        diff = int((x.view(np.uint32) != y.view(np.uint32)).sum())
        print("[bits] costvol_bwd_det %s %s %s: %d of %d elements differ" % (family, shape, name, diff, x.size))
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name


def test_det_views_are_independent_in_g_src():
    h, w, D, V, C = 33, 47, 16, 4, 67
    case = cx.make_case(h, w, D, V, C, "large")
    _, joint = _run(case, "L2", False)
    for v in range(V):
        one = dict(case, src=case["src"][v:v + 1], KR=case["KR"][v:v + 1], Kt=case["Kt"][v:v + 1])
        _, alone = _run(one, "L2", False)
        assert np.abs(alone).max() > 0
        assert np.array_equal(joint[v].view(np.uint32), alone[0].view(np.uint32)), "view %d" % v


# ---- wiring --------------------------------------------------------------------------------------------------------------------

def _plane_sweep_grad(case, tex, KR, Kt, rays, d, g, dist, align):
    from neuralrgbd_amd.autograd import PlaneSweepCost
    C = case["src"].shape[1]
    t = tex.detach().clone().requires_grad_(True)
    cost = PlaneSweepCost.apply(t, KR, Kt, rays, d, case["cx"], case["cy"], case["sigma"], C, dist, align)
    return cost, t


def test_det_autograd_switch_selects_the_kernel_of_the_forward():
    from neuralrgbd_amd import autograd as ag
    h, w, D, V, C = cx.FAMILY_SHAPE_LDS
    case = cx.make_case(h, w, D, V, C, "large")
    tex, KR, Kt, rays, d, g = _upload(case)
    want_ref, want_src = ops.costvol_bwd(tex[V], tex[:V], KR, Kt, rays, d, case["cx"], case["cy"], case["sigma"], C, g, dist="L1",
                                         align_corners=True, deterministic=True)
    assert ag.is_deterministic() is False
    with ag.deterministic():
        assert ag.is_deterministic() is True
        cost, t = _plane_sweep_grad(case, tex, KR, Kt, rays, d, g, "L1", True)
    # the backward runs OUTSIDE the context: it follows the forward it belongs to
    assert ag.is_deterministic() is False
    (cost * g).sum().backward()
    assert torch.equal(t.grad[:V], want_src) and torch.equal(t.grad[V], want_ref)
    # outside the context: the atomic kernels, within the bound
    cost, t = _plane_sweep_grad(case, tex, KR, Kt, rays, d, g, "L1", True)
    (cost * g).sum().backward()
    grad = t.grad.permute(0, 3, 1, 2).cpu().numpy()
    _compare("PlaneSweepCost, switch off", case, "L1", True, grad[V], grad[:V], "costvol_bwd_det")
    # a forward recorded with the switch off keeps the atomic kernels even if the backward runs under the switch
    cost, t = _plane_sweep_grad(case, tex, KR, Kt, rays, d, g, "L1", True)
    with ag.deterministic():
        (cost * g).sum().backward()
    grad = t.grad.permute(0, 3, 1, 2).cpu().numpy()
    _compare("PlaneSweepCost, forward off / backward on", case, "L1", True, grad[V], grad[:V], "costvol_bwd_det")
    # restored after an exception too
    with pytest.raises(RuntimeError):
        with ag.deterministic():
            raise RuntimeError("x")
    assert ag.is_deterministic() is False


def test_det_workspace_contract():
    from neuralrgbd_amd import _lib
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    assert lib.nrgbd_costvol_bwd_det_workspace(4, 68, 64, 64, 96, ctypes.byref(n)) == 0 and n.value == 12 * 4 * 68 * 64 * 96
    assert lib.nrgbd_costvol_bwd_det_workspace(4, 68, 64, 192, 256, ctypes.byref(n)) == 0 and n.value == 12 * 4 * 68 * 192 * 256
    assert lib.nrgbd_costvol_bwd_det_workspace(4, 67, 64, 64, 96, ctypes.byref(n)) == -2
    assert lib.nrgbd_costvol_bwd_det_workspace(4, 68, 64, 64, 96, None) == -1
    assert lib.nrgbd_costvol_bwd_det_workspace(1, 4, 256, 2048, 2048, ctypes.byref(n)) == -2       # h w D = 2^30: no headroom
    case = cx.make_case(9, 11, 6, 2, 3, "small")
    tex, KR, Kt, rays, d, g = _upload(case)
    V, C, h, w, D, Cp = 2, 3, 9, 11, 6, 4
    g_ref, g_src = torch.zeros(h, w, Cp, device=DEV), torch.zeros(V, h, w, Cp, device=DEV)
    work = torch.zeros(12 * V * Cp * h * w // 4, device=DEV)
    ref_t, src_t = tex[V].contiguous(), tex[:V].contiguous()

    def call(work_ptr, nbytes, dist=0):
        return lib.nrgbd_costvol_bwd_det(ref_t.data_ptr(), src_t.data_ptr(), KR.data_ptr(), Kt.data_ptr(), rays.data_ptr(), d.data_ptr(),
                                         case["cx"], case["cy"], case["sigma"], dist, 0, g.data_ptr(), g_ref.data_ptr(), g_src.data_ptr(),
                                         V, C, Cp, D, h, w, work_ptr, nbytes, None)
    full = 12 * V * Cp * h * w
    assert call(None, full) == -1                      # always needs its workspace
    assert call(work.data_ptr(), full - 1) == -2
    assert call(work.data_ptr() + 4, full) == -3
    assert call(work.data_ptr(), full, dist=2) == -4
    assert call(work.data_ptr(), full) == 0
    torch.cuda.synchronize()
