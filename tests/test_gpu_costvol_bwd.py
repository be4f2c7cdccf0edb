"""Cost-volume backward (csrc/costvol_bwd.hip: the LDS-scatter kernel + its fixed-order reduce, and the global-atomic kernel) held
element by element against the exact-position float64 comparator of tests/costvol_bwd_exact.py: |got - exact| <= bound on g_ref and
g_src, with the bound derived there from the arithmetic (never from what the kernels give).  tests/test_costvol_bwd_host.py checks
the comparator itself and the populations of the input families without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import costvol_bwd_exact as cx
from costvol_bwd_gpu import DEV, LDS_SHAPES, _compare, _nchw, _run, _upload
from neuralrgbd_amd import ops

pytestmark = pytest.mark.gpu


def _kernel_path(V, Cp, D, h, w):
    """("lds", depth slices) or ("global", 0), read from the library's own workspace query (the global-atomic kernel's slice count
    is internal to the launcher: its ragged coverage rests on the D values of test_global_kernel_shapes)."""
    from neuralrgbd_amd import _lib
    n = ctypes.c_size_t(0)
    assert _lib.load().nrgbd_costvol_bwd_workspace(V, Cp, D, h, w, ctypes.byref(n)) == 0
    if n.value == 0:
        return "global", 0
    per_slice = 2 * V * (Cp // 4) * h * w * 16
    assert n.value % per_slice == 0
    return "lds", n.value // per_slice


def _check(case, dist, align, kernel, label=None, slices=None):
    V, C, h, w = case["src"].shape
    D = len(case["d_candi"])
    path, n = _kernel_path(V, ops.padded_channels(C), D, h, w)
    assert path == kernel, "%dx%dx%d V=%d C=%d takes the %s kernel, the case is meant for the %s kernel" % (h, w, D, V, C, path, kernel)
    if slices is not None:
        assert n == slices
    got_ref, got_src = _run(case, dist, align)
    name = "%s %dx%dx%d V%d C%d %s/%d" % (label or case["key"][5], h, w, D, V, C, path, n)
    return _compare(name, case, dist, align, got_ref, got_src, "costvol_bwd"), got_ref, got_src


# ---- kernel paths ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dist", ["L2", "L1"])
@pytest.mark.parametrize("h,w,D,V,C,family", LDS_SHAPES)
def test_lds_kernel_shapes(h, w, D, V, C, family, dist):
    _check(cx.make_case(h, w, D, V, C, family), dist, False, "lds")


@pytest.mark.parametrize("dist", ["L2", "L1"])
@pytest.mark.parametrize("rule", ["ragged_last", "empty_slices"])
@pytest.mark.parametrize("h,w,V,C", [(33, 47, 4, 67), (9, 11, 2, 4)])
def test_lds_kernel_ragged_slices(h, w, V, C, rule, dist):
    """D chosen from the device's own slice count kc: 7 kc + 1 leaves a shorter last slice (per = 8: ..., the last holds 8 - (kc - 1)
    or fewer); kc + 1 makes per = 2, so about half of the slices start at or beyond D and must write zeros."""
    Cp = ops.padded_channels(C)
    _, kc = _kernel_path(V, Cp, 64, h, w)
    D = 7 * kc + 1 if rule == "ragged_last" else kc + 1
    per = -(-D // kc)
    print("[inputs] %dx%d V=%d C=%d: %d slices on this device, %s D = %d, per = %d, %d slices start beyond D, last holds %d"
          % (h, w, V, C, kc, rule, D, per, sum(1 for s in range(kc) if s * per >= D), D - per * ((D - 1) // per)))
    if kc > 1:
        assert D % kc != 0
    if rule == "empty_slices" and kc > 2:
        assert (kc - 1) * per >= D
    _check(cx.make_case(h, w, D, V, C, "driver"), dist, False, "lds", rule, slices=min(kc, D))


@pytest.mark.parametrize("dist", ["L2", "L1"])
@pytest.mark.parametrize("h,w,D,V,C,family", [
    # the launcher cuts D >= 8 into 2 and D >= 32 into 4 slices of ceil(D / slices) candidates (costvol_bwd.hip); the comments
    # name what each D is there for
    (96, 128, 4, 1, 6, "small"),       # kchunks 1 (the shape of the earlier test)
    (97, 131, 4, 4, 67, "small"),      # kchunks 1, g_ref accumulated over views by atomics, hw no multiple of 64
    (96, 128, 9, 4, 67, "driver"),     # kchunks 2, slices of 5 / 4
    (97, 131, 9, 1, 6, "large"),
    (97, 131, 33, 4, 6, "driver"),     # kchunks 4, slices of 9 / 9 / 9 / 6
    (96, 128, 33, 4, 67, "small"),
    (96, 128, 64, 1, 67, "driver"),    # kchunks 4, 16 each
    (97, 131, 64, 4, 67, "driver"),
])
def test_global_kernel_shapes(h, w, D, V, C, family, dist):
    _check(cx.make_case(h, w, D, V, C, family), dist, False, "global")


# ---- geometry families, both kernels, both align_corners values ---------------------------------------------------------------

@pytest.mark.parametrize("dist", ["L2", "L1"])
@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("family", cx.FAMILIES)
@pytest.mark.parametrize("kernel", ["lds", "global"])
def test_geometry_families(kernel, family, align, dist):
    h, w, D, V, C = cx.FAMILY_SHAPE_LDS if kernel == "lds" else cx.FAMILY_SHAPE_GLOBAL
    _check(cx.make_case(h, w, D, V, C, family), dist, align, kernel)


# ---- contents: dead channels, exact zeros in g_cost ---------------------------------------------------------------------------

@pytest.mark.parametrize("dist", ["L2", "L1"])
@pytest.mark.parametrize("content,gmode", [("relu", "normal"), ("relu", "blocks"), ("normal", "blocks"), ("relu", "alternate")])
@pytest.mark.parametrize("kernel", ["lds", "global"])
def test_dead_channels_and_zero_g(kernel, content, gmode, dist):
    h, w, D, V, C = cx.FAMILY_SHAPE_LDS if kernel == "lds" else cx.FAMILY_SHAPE_GLOBAL
    case = cx.make_case(h, w, D, V, C, "small", content, gmode)
    ex, got_ref, got_src = _check(case, dist, False, kernel, "%s/%s" % (content, gmode))
    if content == "relu":
        # post-activation features: both dead channels (zero in the reference and in every source) get exactly zero gradient:
        # under L1 sign(0) is 0 (torch.abs's convention), under L2 2 * 0 * g
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


# ---- every output element is written, whatever the buffers held ---------------------------------------------------------------

@pytest.mark.parametrize("C", [3, 5, 67])
@pytest.mark.parametrize("kernel,h,w,D,V,dist", [("lds", 12, 20, 6, 2, "L2"), ("global", 96, 128, 9, 2, "L1")])
def test_outputs_fully_overwritten_from_nan(kernel, h, w, D, V, dist, C):
    """The C-ABI entry with both outputs and the workspace pre-filled with NaN (ops.costvol_bwd hands it torch.empty_like): every
    element finite afterwards, the padding lanes exactly 0, the values within the bound."""
    from neuralrgbd_amd import _lib
    lib = _lib.load()
    case = cx.make_case(h, w, D, V, C, "large")
    Cp = ops.padded_channels(C)
    path, _ = _kernel_path(V, Cp, D, h, w)
    assert path == kernel
    tex, KR, Kt, rays, d, g = _upload(case)
    n = ctypes.c_size_t(0)
    assert lib.nrgbd_costvol_bwd_workspace(V, Cp, D, h, w, ctypes.byref(n)) == 0
    work = torch.full((max(n.value, 16) // 4,), float("nan"), device=DEV)
    g_ref = torch.full((h, w, Cp), float("nan"), device=DEV)
    g_src = torch.full((V, h, w, Cp), float("nan"), device=DEV)
    ref_t, src_t = tex[V].contiguous(), tex[:V].contiguous()
    rc = lib.nrgbd_costvol_bwd(ref_t.data_ptr(), src_t.data_ptr(), KR.data_ptr(), Kt.data_ptr(), rays.data_ptr(), d.data_ptr(),
                               case["cx"], case["cy"], case["sigma"], ops.DIST[dist], 0, g.data_ptr(), g_ref.data_ptr(), g_src.data_ptr(),
                               V, C, Cp, D, h, w, work.data_ptr() if n.value else None, n.value, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isfinite(g_ref).all() and torch.isfinite(g_src).all()
    assert (g_ref[..., C:] == 0).all() and (g_src[..., C:] == 0).all()
    _compare("NaN-filled buffers %dx%dx%d V%d C%d %s" % (h, w, D, V, C, kernel), case, dist, False, *_nchw(g_ref, g_src), "costvol_bwd")


# ---- reproducibility, as far as it holds --------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,h,w,D,V,C,family", [("lds", 64, 96, 16, 2, 67, "small"), ("global", 96, 128, 9, 4, 67, "driver")])
def test_two_runs(kernel, h, w, D, V, C, family):
    """g_src goes through LDS or global atomics and the global kernel's g_ref through global atomics: order dependent, so two runs
    agree within twice the bound.  The LDS path's g_ref (register accumulation, reduce in index order) is the same bit for bit."""
    case = cx.make_case(h, w, D, V, C, family)
    assert _kernel_path(V, ops.padded_channels(C), D, h, w)[0] == kernel
    a_ref, a_src = _run(case, "L2", False)
    b_ref, b_src = _run(case, "L2", False)
    ex = cx.exact_case(case, "L2", False)
    if kernel == "lds":
        assert np.array_equal(a_ref, b_ref)
    d_ref, d_src = np.abs(a_ref[:C].astype(np.float64) - b_ref[:C]), np.abs(a_src[:, :C].astype(np.float64) - b_src[:, :C])
    print("[parity] costvol_bwd two runs %s: %d g_ref / %d g_src elements differ, largest difference / (2 bound) %.3f / %.3f"
          % (kernel, (d_ref > 0).sum(), (d_src > 0).sum(), (d_ref / np.maximum(2 * ex["bound_ref"], 1e-300)).max(),
             (d_src / np.maximum(2 * ex["bound_src"], 1e-300)).max()))
    assert (d_ref <= 2 * ex["bound_ref"]).all() and (d_src <= 2 * ex["bound_src"]).all()


def test_autograd_wrapper_passes_dist_and_align_corners():
    """PlaneSweepCost with dist = L1 and align_corners = True: the forward equals ops.costvol bit for bit, the backward is within
    the bound of the comparator run with the same two arguments."""
    from neuralrgbd_amd.autograd import PlaneSweepCost
    h, w, D, V, C = cx.FAMILY_SHAPE_LDS
    case = cx.make_case(h, w, D, V, C, "large")
    tex, KR, Kt, rays, d, g = _upload(case)
    tex.requires_grad_(True)
    cost = PlaneSweepCost.apply(tex, KR, Kt, rays, d, case["cx"], case["cy"], case["sigma"], C, "L1", True)
    (cost * g).sum().backward()
    want, _ = ops.costvol(tex.detach()[V], tex.detach()[:V], KR, Kt, rays, d, case["cx"], case["cy"], case["sigma"], C, dist="L1",
                          align_corners=True)
    other, _ = ops.costvol(tex.detach()[V], tex.detach()[:V], KR, Kt, rays, d, case["cx"], case["cy"], case["sigma"], C, dist="L1",
                           align_corners=False)
    assert torch.equal(cost.detach(), want) and not torch.equal(want, other)
    grad = tex.grad.permute(0, 3, 1, 2).cpu().numpy()
    _compare("PlaneSweepCost", case, "L1", True, grad[V], grad[:V], "costvol_bwd")
