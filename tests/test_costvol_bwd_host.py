"""The cost-volume backward's comparator (tests/costvol_bwd_exact.py) held against independent witnesses on the CPU: float64
autograd through F.grid_sample on the same positions, the oracle's forward cost, and the populations its input families claim."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import costvol_bwd_exact as cx
from oracle import cpu_oracle as co


def _autograd_grads(case, dist, align):
    """float64 autograd of sum(cost * g) through F.grid_sample fed the comparator's fp32 positions as a float64 grid."""
    V, C, h, w = case["src"].shape
    D = len(case["d_candi"])
    ix, iy = co.sweep_positions(case["KR"], case["Kt"], case["rays"], case["d_candi"], case["cx"], case["cy"], h, w, align)
    ix, iy = torch.from_numpy(ix).double(), torch.from_numpy(iy).double()
    if align:
        gx, gy = 2 * ix / (w - 1) - 1, 2 * iy / (h - 1) - 1
    else:
        gx, gy = (2 * ix + 1) / w - 1, (2 * iy + 1) / h - 1
    ref = torch.from_numpy(case["ref"]).double().requires_grad_(True)
    src = torch.from_numpy(case["src"]).double().requires_grad_(True)
    g = torch.from_numpy(case["g_cost"]).double()
    cost = torch.zeros(D, h, w, dtype=torch.float64)
    for v in range(V):
        warped = F.grid_sample(src[v:v + 1].expand(D, C, h, w), torch.stack((gx[v], gy[v]), -1), mode="bilinear",
                               padding_mode="zeros", align_corners=align)
        diff = warped - ref.unsqueeze(0)
        cost = cost + (diff.pow(2) if dist == "L2" else diff.abs()).sum(1) / case["sigma"]
    (cost * g).sum().backward()
    return ref.grad.numpy(), src.grad.numpy(), cost.detach().numpy()


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("dist", ["L2", "L1"])
@pytest.mark.parametrize("family,content,gmode", [("small", "normal", "normal"), ("large", "relu", "blocks"),
                                                  ("behind", "normal", "alternate"), ("zoom_far", "normal", "normal")])
def test_exact_grads_vs_float64_autograd(family, content, gmode, dist, align):
    case = cx.make_case(13, 17, 12, 3, 6, family, content, gmode, seed=2)
    ex = cx.exact_grads(case["ref"], case["src"], case["KR"], case["Kt"], case["rays"], case["d_candi"], case["cx"], case["cy"],
                        case["sigma"], case["g_cost"], dist, align)
    want_ref, want_src, _ = _autograd_grads(case, dist, align)
    scale = max(np.abs(want_ref).max(), np.abs(want_src).max())
    assert scale > 0.1
    e_ref, e_src = np.abs(ex["g_ref"] - want_ref).max(), np.abs(ex["g_src"] - want_src).max()
    print("[parity] comparator vs float64 autograd %s %s align=%d: %.2e / %.2e of %.2f" % (family, dist, align, e_ref, e_src, scale))
    assert e_ref <= 1e-10 * scale and e_src <= 1e-10 * scale
    # the bound is finite, non-negative, and zero only where nothing lands
    for b, n in ((ex["bound_ref"], ex["n_ref"][None]), (ex["bound_src"], ex["n_src"][:, None])):
        assert np.isfinite(b).all() and (b >= 0).all() and (b[np.broadcast_to(n == 0, b.shape)] == 0).all()


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("dist", ["L2", "L1"])
def test_positions_consistent_with_oracle_costvol(dist, align):
    for family in ("small", "large", "behind"):
        case = cx.make_case(13, 17, 12, 3, 6, family, seed=2)
        want = co.costvol(case["ref"], case["src"], case["KR"], case["Kt"], case["rays"], case["d_candi"], case["cx"], case["cy"],
                          case["sigma"], dist, align)
        got, bound = cx.exact_cost(case, dist, align)
        ratio = np.abs(got - want) / np.maximum(bound, 1e-300)
        print("[parity] float64 cost from sweep_positions vs oracle %s %s align=%d: worst error / bound %.3f" % (family, dist, align, ratio.max()))
        assert (np.abs(got - want) <= bound).all() and np.abs(want).max() > 1.0
        _, _, cost64 = _autograd_grads(case, dist, align)
        assert np.abs(cost64 - got).max() <= 1e-10 * np.abs(got).max()


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("family", cx.FAMILIES)
def test_family_contains_what_it_claims(family, align):
    h, w, D, V, C = cx.FAMILY_SHAPE_LDS
    case = cx.make_case(h, w, D, V, C, family)
    pop = cx.population(case, align)
    print("[inputs] %-9s align=%d: %s" % (family, align, pop))
    n = pop["samples"]
    assert n == V * D * h * w and pop["g_zero"] == 0
    if family in ("small", "driver"):
        assert pop["behind"] == 0 and pop["wholly_outside"] < 0.1 * n and pop["runs_ge4"] > 0
    if family == "large":
        assert pop["partly_outside"] > 0.005 * n and pop["wholly_outside"] > 0.1 * n
    if family == "behind":
        assert pop["behind"] > 0.05 * n and pop["behind"] < 0.9 * n
        assert pop["behind_in_image"] > 0.02 * n      # mirrored points do land on valid taps
    if family == "zoom_far":
        assert pop["runs_ge4"] > V * h * w and pop["longest_run"] >= 16 and pop["behind"] == 0
    if family == "scatter":
        assert pop["longest_run"] == 1 and pop["same_cell_share"] == 0.0 and pop["wholly_outside"] < 0.5 * n


@pytest.mark.parametrize("family", cx.FAMILIES)
def test_tie_share_of_every_family(family):
    """The tie term may not hide a wrong sign rule: at most TIE_CAP of the contributing L1 elements are ties."""
    h, w, D, V, C = cx.FAMILY_SHAPE_LDS
    for content, gmode in (("normal", "normal"), ("relu", "blocks"), ("relu", "alternate")):
        case = cx.make_case(h, w, D, V, C, family, content, gmode)
        for align in (False, True):
            ex = cx.exact_case(case, "L1", align)
            share = ex["ties"] / max(1, ex["elements"])
            print("[inputs] %-9s %-6s %-9s align=%d: %d ties of %d L1 elements (%.1e)" % (family, content, gmode, align, ex["ties"],
                                                                                         ex["elements"], share))
            assert ex["elements"] > 0 and share <= cx.TIE_CAP


def test_contents_contain_what_they_claim():
    h, w, D, V, C = cx.FAMILY_SHAPE_LDS
    relu = cx.make_case(h, w, D, V, C, "small", "relu", "blocks")
    assert (relu["ref"][[1, C - 1]] == 0).all() and (relu["src"][:, [1, C - 1]] == 0).all()
    live = [c for c in range(C) if c not in (1, C - 1)]
    assert (relu["ref"][live] > 0).mean() > 0.3 and (relu["ref"][live] == 0).mean() > 0.3
    g = relu["g_cost"]
    assert (g[D // 4:D // 2] == 0).all() and (g[:, h // 4:h // 2, w // 3:2 * w // 3] == 0).all() and (g != 0).mean() > 0.5
    alt = cx.make_case(h, w, D, V, C, "small", "normal", "alternate")["g_cost"]
    assert (alt[::2] == 0).all() and (alt[1::2] != 0).all()
    for dist in ("L2", "L1"):
        ex = cx.exact_case(relu, dist, False)
        # dead channels: exactly zero gradient and a zero bound; texels reached only through zeroed g exist and are exactly zero
        assert (ex["g_ref"][[1, C - 1]] == 0).all() and (ex["g_src"][:, [1, C - 1]] == 0).all()
        if dist == "L1":
            assert (ex["bound_ref"][[1, C - 1]] == 0).all() and (ex["bound_src"][:, [1, C - 1]] == 0).all()
        only_zero_g = (ex["reach_src"] > 0) & (ex["n_src"] == 0)
        assert only_zero_g.sum() > 0 and (ex["g_src"][np.broadcast_to(only_zero_g[:, None], ex["g_src"].shape)] == 0).all()
        assert (ex["bound_src"][np.broadcast_to(only_zero_g[:, None], ex["g_src"].shape)] == 0).all()
