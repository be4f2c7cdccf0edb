"""warp_volume's comparator (tests/warp_exact.py) held against independent witnesses on the CPU: float64 F.grid_sample on the same
positions, the oracle's fp32 warp, and the populations its input families claim."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import warp_exact as wx
from oracle import cpu_oracle as co

SHAPE = (13, 17, 6, 4, 3)            # h, w, D, V, Cs of the witness cases
POP_SHAPE = (20, 36, 8, 4, 3)        # the K-Net fast kernel's test shape


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("family", wx.FAMILIES)
def test_comparator_vs_float64_grid_sample(family, align):
    """Zero-padded bilinear interpolation is continuous in the position, so positions on exact integers are no obstacle."""
    h, w, D, V, Cs = SHAPE
    case = wx.make_case(h, w, D, V, Cs, family, seed=3)
    ex = wx.exact_warp(case, align)
    ix, iy = wx.positions(case, align)
    ix, iy = torch.from_numpy(ix).double(), torch.from_numpy(iy).double()
    if align:
        gx, gy = 2 * ix / (w - 1) - 1, 2 * iy / (h - 1) - 1
    else:
        gx, gy = (2 * ix + 1) / w - 1, (2 * iy + 1) / h - 1
    src = torch.from_numpy(case["src"]).double()
    texel = float(np.abs(case["src"]).max())
    worst = 0.0
    for v in range(V):
        want = F.grid_sample(src[v:v + 1].expand(D, Cs, h, w), torch.stack((gx[v], gy[v]), -1), mode="bilinear",
                             padding_mode="zeros", align_corners=align).permute(1, 0, 2, 3).numpy()
        # positions of ~1e12 texels (on_plane) lose the float64 grid's digits, not the comparator's: both say "outside"
        worst = max(worst, float(np.abs(ex["warped"][v] - want).max()))
    print("[parity] warp comparator vs float64 grid_sample %-8s align=%d: %.2e of %.2f" % (family, align, worst, texel))
    assert texel > 1.0 and worst <= 1e-9 * texel
    assert np.isfinite(ex["warped"]).all() and np.isfinite(ex["bound"]).all() and (ex["bound"] >= 0).all()
    assert (ex["warped"][np.broadcast_to(ex["nvalid"][:, None] == 0, ex["warped"].shape)] == 0).all()


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("family", wx.FAMILIES)
def test_comparator_vs_oracle_warp_volume(family, align):
    h, w, D, V, Cs = SHAPE
    case = wx.make_case(h, w, D, V, Cs, family, seed=3)
    ex = wx.exact_warp(case, align)
    got = co.warp_volume(case["src"], case["KR"], case["Kt"], case["rays"], case["d_candi"], case["cx"], case["cy"], align)
    ratio, at, beyond = wx.worst_ratio(got, ex["warped"], ex["bound"])
    print("[parity] oracle warp_volume vs comparator %-8s align=%d: worst error / bound %.3f at %s" % (family, align, ratio, at))
    assert beyond == 0
    vol, bnd = wx.assemble(case, align, V=2, with_ref=True, with_bv=True)
    assert vol.shape == (2 * Cs + Cs + 1, D, h, w) and (bnd[2 * Cs:] == 0).all()
    assert np.array_equal(vol[-1], (case["bv_cur"] - case["bv_pred"]).astype(np.float64))


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("family", wx.FAMILIES)
def test_family_contains_what_it_claims(family, align):
    h, w, D, V, Cs = POP_SHAPE
    case = wx.make_case(h, w, D, V, Cs, family)
    pop = wx.population(case, align)
    n = pop["samples"]
    print("[inputs] warp %-8s align=%d: %s" % (family, align, {k: v for k, v in pop.items() if not callable(v)}))
    assert n == V * D * h * w
    if family == "small":
        assert pop["behind"] == 0 and pop["wholly_outside"] < 0.1 * n and pop["planes_at_min_den"] == 0
    if family == "large":
        assert pop["partly_outside"] > 0.005 * n and pop["wholly_outside"] > 0.1 * n
    if family == "behind":
        assert 0.05 * n < pop["behind"] < 0.9 * n and pop["behind_in_image"] > 0.02 * n
    if family == "zoom_far":
        assert pop["behind"] == 0 and pop["wholly_outside"] < 0.1 * n
    if family == "on_plane":
        den = wx.denominators(case)
        for v in range(V):
            k = wx.on_plane_k(D, v)
            assert (den[v, k] == np.float32(1e-10)).all()
            assert (den[v, :k] < 0).all() and (den[v, k + 1:] > 0).all()           # P_z changes sign across the candidates
        assert pop["planes_at_min_den"] == V and pop["behind"] > 0.2 * n
        ix, iy = wx.positions(case, align)
        assert np.isfinite(ix).all() and np.isfinite(iy).all()
        assert float(np.abs(ix[0, wx.on_plane_k(D, 0)]).max()) > 1e9             # the quotient by 1e-10
    if family == "border":
        assert pop["behind"] == 0 and pop["partly_outside"] > 0.04 * n
        _border_values(case, pop, align, near_only=(-1, 0))


def _border_values(case, pop, align, near_only=()):
    """Whole columns (rows) of positions on each listed value; the values of `near_only` within 8 ulps of 1 instead (see warp_exact)."""
    h, w = case["src"].shape[2:]
    ix, iy = wx.positions(case, align)
    for size, other, at, pos, axis in ((w, h, pop["at_x"], ix, "x"), (h, w, pop["at_y"], iy, "y")):
        targets = (0, size - 1) if align else (-1, -0.5, 0, size - 1, size - 0.5, size)   # align: u = 0 and u = size only
        for val in targets:
            if val in near_only and not align:
                near = int((np.abs(pos - np.float32(val)) <= 8 * 2.0 ** -23).sum())
                assert near >= other, "no line of sample positions next to %s = %s" % (axis, val)
            else:
                assert at(val) >= other, "no line of sample positions at %s = %s" % (axis, val)


@pytest.mark.parametrize("align", [False, True])
def test_border_family_on_the_power_of_two_grid(align):
    h, w = wx.BORDER_POW2
    case = wx.make_case(h, w, 5, 4, 3, "border")
    _border_values(case, wx.population(case, align), align)


@pytest.mark.parametrize("D", [1, 5])
def test_families_at_the_small_depth_counts(D):
    """The GPU tests also run D = 1 and 5: the on_plane plane exists there too, and border keeps its whole-texel candidate d = 1."""
    case = wx.make_case(7, 9, D, 4, 3, "on_plane")
    assert wx.population(case)["planes_at_min_den"] == 4
    case = wx.make_case(7, 9, D, 4, 3, "border")
    assert 1.0 in case["d_candi"]
    pop = wx.population(case)
    assert pop["at_x"](8) >= 7 and pop["at_x"](9) >= 7 and pop["at_y"](6) >= 9 and pop["at_y"](7) >= 9
