"""The persistent Winograd kernel (csrc/wino_pc.hip, conv_wino_pc_kernel) where a workgroup WALKS: more tiles than CUs, so that every
workgroup hands at least one tile over to a next one — the producers' next-tile book and its owner bits, the consumers' weight ring
wrapping into the next tile's stream, the A-operand prefetch of the next tile's first points, the FIRST-stage accumulator reset, the
register-set parity of the odd forms, the change between the interior and the edge epilogue — in every instantiation family: the
four (KD, DIL, HALF) families with their four (residual, materialise) forms, the four R-Net forms, the deconv form; and the input
forms of wino_dw4.hip on its 280-tile grid.  (The odd 3-D first layer walks in tests/test_gpu_knet.py.)

The grids come from tests/wino_walk.py, the host mirror of the tile list, for this device's CU count, and every test asserts from
the mirror that its launch walks (wino_walk.preconditions): conditions, not measurements.  Two oracles per case:
  (a) float64 on the host, prologue included, computed from the fp32 operands;
  (b) 2-D, R-Net and deconv forms: the same operands one sample per launch — fewer tiles than CUs, no workgroup walks, the regime of
      the other test files — concatenated: a tile's arithmetic does not depend on which workgroup computes it or at which iteration,
      so y, the materialised input and the statistics rows are equal bit for bit.
Every form runs twice with equal bits.

Bounds.  Plain, R-Net and deconv forms: the project's 2e-5 max(1, |y|max).  Fused forms: the kernel rounds its prologue to fp32, the
float64 reference does not; what that costs is measured on the reference side (fp32 prologue -> float64 convolution, minus the
all-float64 result, max over the tensor; _reference()["cost"], recomputed in every run) and the bound is the plain bound + twice
that.  Measured on the host at the grids of 256 CUs, as  cost / plain bound / bound  per activation kind:
  family (N)        x_ss+ReLU                          + res_ss+ReLU                      + identity residual
  64 -> 64 (10)     2.445e-07 / 1.258e-04 / 1.263e-04  3.882e-07 / 1.852e-04 / 1.860e-04  3.427e-07 / 1.782e-04 / 1.789e-04
  128 -> 128 (5)    3.391e-07 / 1.856e-04 / 1.863e-04  5.657e-07 / 2.595e-04 / 2.607e-04  4.541e-07 / 2.934e-04 / 2.943e-04
  ... dilation 2    3.369e-07 / 1.732e-04 / 1.739e-04  5.335e-07 / 2.405e-04 / 2.415e-04  4.361e-07 / 2.528e-04 / 2.536e-04
  HALF 32 -> 32     2.264e-07 / 1.260e-04 / 1.264e-04  4.302e-07 / 1.491e-04 / 1.500e-04  3.309e-07 / 1.861e-04 / 1.867e-04
  kd = 3 (D 21)     3.246e-07 / 1.727e-04 / 1.734e-04  5.851e-07 / 2.576e-04 / 2.588e-04  4.569e-07 / 2.639e-04 / 2.648e-04
  wino_dw4          ReLU 9.945e-07 / 1.107e-03 / 1.109e-03; no ReLU 1.326e-06 / 1.538e-03 / 1.540e-03 (plain bound 4e-5 max(1, |y|max))
(the plain bounds are 2e-5 |y|max with |y|max between 6.3 and 14.7: rounding the prologue costs well under a hundredth of them).
Materialised input: elementwise 4 * 2^-24 * (|x s| + |t| + |r rs| + |rt|): at most three roundings (two FMAs and the addition),
each below 2^-24 of that sum.
Statistics rows against float64: the plain tests' allclose(rtol 1e-5, atol 1e-3; HALF, two rows per tile: atol 2e-3) for the plain
forms; a statistics error is linear in the error of y, so the fused forms get both tolerances times (fused bound / plain bound)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import wino_walk as ww

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H2, W2 = 50, 120          # 2-D plane: 7 x 8 tiles, the last row and the last column cross the edge; 56 tiles per sample
H3, W3 = 38, 70           # kd = 3 plane: 5 x 5 tiles.  Not 30 x 70: with 20 tiles per slice the XCD eighths end exactly at the ends
                          # of the tile rows and no walk ever goes from an edge tile to an interior one (test_wino_walk_host.py)
EPS = 2.0 ** -24

FAMILIES = {"64": (64, 64, 1), "128": (128, 128, 1), "dil2": (128, 128, 2), "half": (32, 32, 1)}      # (Cin, Cout, dilation)
# form -> (activation kind, materialise).  Fused forms use x_ss + ReLU; the residual once with res_ss + ReLU, once as identity
FORMS = {"plain": ("plain", False), "res_ss": ("res_ss", False), "res_id": ("res_id", False), "mat": ("ss", True),
         "res_ss+mat": ("res_ss", True), "res_id+mat": ("res_id", True)}
KINDS = ["plain", "res_ss", "res_id", "ss"]


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _walking_grid(ncg, kd, dil, H, W, ncu=None):
    """N (depth for kd = 3) of the launch, with the preconditions asserted: they fail loudly if a change stops exercising the walk."""
    ncu = ncu or _ncu()
    N = ww.grid_for(ncu, ncg, kd, dil, H, W)
    pre = ww.preconditions(ncu, N, H, W, ncg, kd, dil)
    assert all(pre.values()), (ncu, N, pre)
    return N


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ----------------------------------------------------------------------------- operands and float64 references (host, computed once)
@functools.lru_cache(maxsize=1)
def _operands(fam, N, kd):
    """fp32 operands on the host, channels-last: x, r [N,H,W,Cin]; (scale, shift) tables; w."""
    Cin, Cout, dil = FAMILIES[fam]
    H, W = (H3, W3) if kd == 3 else (H2, W2)
    seed = 1000 * kd + Cin + dil
    w = _randn(Cout, Cin, *((3, 3, 3) if kd == 3 else (3, 3)), seed=seed + 4, scale=0.08 if Cin == 32 else 0.05)
    return {"x": _randn(N, H, W, Cin, seed=seed), "r": _randn(N, H, W, Cin, seed=seed + 1), "ss": _randn(Cin, 2, seed=seed + 2),
            "rs": _randn(Cin, 2, seed=seed + 3), "w": w}


def _activated(op, kind, dtype):
    """The convolution's input of an activation kind in `dtype`, from the fp32 operands; and the materialise bound (float64)."""
    x, r, ss, rs = (op[k].to(dtype) for k in ("x", "r", "ss", "rs"))
    if kind == "plain":
        return x, None
    xs, t = x * ss[:, 0], ss[:, 1]
    act = torch.relu(xs + t)
    mag = xs.abs() + t.abs()
    if kind == "res_ss":
        act = act + torch.relu(r * rs[:, 0] + rs[:, 1])
        mag = mag + (r * rs[:, 0]).abs() + rs[:, 1].abs()
    elif kind == "res_id":
        act = act + r
        mag = mag + r.abs()
    return act, 4.0 * EPS * mag


def _conv64(act, w, kd, dil):
    """channels-last activated input (any dtype) -> float64 convolution, channels-last."""
    a = act.double()
    if kd == 3:
        return F.conv3d(a.permute(3, 0, 1, 2)[None], w.double(), padding=1)[0].permute(1, 2, 3, 0).contiguous()
    return F.conv2d(a.permute(0, 3, 1, 2), w.double(), padding=dil, dilation=dil).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=1)
def _reference(fam, kind, N, kd):
    """float64 reference of one (family, activation kind): activated input, its materialise bound, y; cost = what rounding the prologue
    to fp32 costs in y (0 for the plain kind); bound = plain bound + 2 cost."""
    op = _operands(fam, N, kd)
    dil = FAMILIES[fam][2]
    act, matbound = _activated(op, kind, torch.float64)
    want = _conv64(act, op["w"], kd, dil)
    cost = 0.0 if kind == "plain" else (_conv64(_activated(op, kind, torch.float32)[0], op["w"], kd, dil) - want).abs().max().item()
    plain = 2e-5 * max(1.0, want.abs().max().item())
    return {"act": act, "matbound": matbound, "want": want, "cost": cost, "plain_bound": plain, "bound": plain + 2.0 * cost}


def _check_stats(stats, want, Cout, half, factor, tag):
    s = stats.double().sum(1).cpu()
    red = tuple(range(want.dim() - 1))
    atol = (2e-3 if half else 1e-3) * factor
    assert torch.allclose(s[:Cout], want.sum(red), rtol=1e-5 * factor, atol=atol), tag
    assert torch.allclose(s[Cout:], (want ** 2).sum(red), rtol=1e-5 * factor, atol=atol), tag


def _run_pc(op, fam, form, kd, sl=None):
    """One launch of nrgbd_conv_wino_f32 in a prologue form on the operands (sl: a sample slice) -> (y, stats, mat)."""
    from neuralrgbd_amd import ops
    Cin, Cout, dil = FAMILIES[fam]
    kind, mat = FORMS[form]
    sl = sl if sl is not None else slice(None)
    kw = {}
    if kind != "plain":
        kw.update(x_ss=op["ss_d"], x_relu=True)
    if kind == "res_ss":
        kw.update(res=op["r_d"][sl], res_ss=op["rs_d"], res_relu=True)
    elif kind == "res_id":
        kw.update(res=op["r_d"][sl])
    return ops.conv_wino(op["x_d"][sl], op["wp"], Cout, kd, dil, materialize=mat, **kw)


@functools.lru_cache(maxsize=1)
def _device_operands(fam, N, kd):
    from neuralrgbd_amd import ops
    op = dict(_operands(fam, N, kd))
    for k in ("x", "r", "ss", "rs"):
        op[k + "_d"] = op[k].to(DEV)
    wd = op["w"].to(DEV)
    op["wp"] = ops.conv_wino_pack32(wd) if FAMILIES[fam][1] == 32 else ops.conv_wino_pack(wd)
    return op


def _check_pc_form(fam, form, kd):
    Cin, Cout, dil = FAMILIES[fam]
    half = Cout == 32
    ncg = (Cout + 63) // 64
    H, W = (H3, W3) if kd == 3 else (H2, W2)
    N = _walking_grid(ncg, kd, dil, H, W)
    kind, mat_on = FORMS[form]
    ref = _reference(fam, kind, N, kd)
    op = _device_operands(fam, N, kd)
    tag = "%s %s kd%d N%d" % (fam, form, kd, N)
    y, stats, mat = _run_pc(op, fam, form, kd)
    rows = ww.spatial_tiles(N, H, W, dil)
    assert stats.shape == (2 * Cout, 2 * rows if half else rows) and rows * ncg > _ncu()
    # (a) float64
    err = (y.double().cpu() - ref["want"]).abs().max().item()
    emat = -1.0
    if mat_on:
        dm = (mat.double().cpu() - ref["act"]).abs()
        emat = dm.max().item()
    print("[parity] conv_wino_pc walk %s: max|dy vs fp64| %.3e (plain bound %.3e, fp32-prologue cost %.3e, bound %.3e; |y|max %.2f) max|dmat| %.3e"
          % (tag, err, ref["plain_bound"], ref["cost"], ref["bound"], ref["want"].abs().max().item(), emat))
    assert err < ref["bound"], tag
    if mat_on:
        assert bool((dm <= ref["matbound"]).all()), tag
    _check_stats(stats, ref["want"], Cout, half, ref["bound"] / ref["plain_bound"], tag)
    # twice, equal bits
    y2, stats2, mat2 = _run_pc(op, fam, form, kd)
    assert _same_bits(y, y2) and _same_bits(stats, stats2) and (not mat_on or _same_bits(mat, mat2)), tag
    if kd == 3:
        return
    # (b) one sample per launch: one tile per workgroup
    assert ww.launch_tiles(1, H, W, ncg, dil) <= _ncu()
    parts = [_run_pc(op, fam, form, kd, slice(i, i + 1)) for i in range(N)]
    assert _same_bits(y, torch.cat([p[0] for p in parts], 0)), tag
    assert _same_bits(stats, torch.cat([p[1] for p in parts], 1)), tag
    if mat_on:
        assert _same_bits(mat, torch.cat([p[2] for p in parts], 0)), tag


@pytest.mark.parametrize("fam,form", [(f, k) for f in FAMILIES for k in sorted(FORMS, key=lambda k: KINDS.index(FORMS[k][0]))])
def test_2d_forms_where_every_workgroup_walks(fam, form):
    """nrgbd_conv_wino_f32, kd = 1: (Cin, Cout, dilation) = (64, 64, 1), (128, 128, 1), (128, 128, 2), HALF (32, 32, 1), each plain, residual
    only, materialise only, residual + materialise (the residual with res_ss + ReLU and as identity) on the 50 x 120 plane, N from the
    mirror (256 CUs: 10 / 5 / 5 / 10 samples = 560 / 560 / 640 / 560 tiles, walks of 2 and 3 tiles).  Oracles (a) and (b) of the file's
    docstring, statistics rows included.  Fused bound = plain bound + 2 x the measured fp32-prologue cost: measured 2.3e-07 .. 5.7e-07
    against plain bounds of 1.26e-04 .. 2.93e-04, i.e. bounds of 1.263e-04 .. 2.943e-04 (the table in the file's docstring)."""
    _check_pc_form(fam, form, 1)


@pytest.mark.parametrize("form", sorted(FORMS, key=lambda k: KINDS.index(FORMS[k][0])))
def test_3d_forms_where_every_workgroup_walks(form):
    """nrgbd_conv_wino_f32, kd = 3, 64 -> 64, the same prologue forms on a D x 38 x 70 grid (256 CUs: D = 21, 525 tiles, depth fastest:
    every hand-over goes on to another slice).  Oracle (a) and equal bits of two runs; a launch per slice is another operation.  Fused
    bounds (measured cost 3.2e-07 .. 5.9e-07): 1.734e-04 (x_ss + ReLU), 2.588e-04 (+ res_ss + ReLU), 2.648e-04 (+ identity residual)."""
    _check_pc_form("64", form, 3)


# ----------------------------------------------------------------------------- R-Net forms (EPI = 1)
@pytest.mark.parametrize("name,Cin,cout,cout_valid,ycoff,ldy,lrelu", [
    ("even full", 96, 64, 50, 8, 80, True),
    ("even HALF", 96, 32, 32, 8, 48, False),
    ("odd HALF", 80, 32, 3, 64, 96, True),
    ("odd full", 80, 64, 64, 0, 96, False),
])
def test_rnet_forms_where_every_workgroup_walks(name, Cin, cout, cout_valid, ycoff, ldy, lrelu):
    """nrgbd_conv_wino_rnet_ex_f32 into a wider buffer at a column offset (sentinel elsewhere): even and odd stage counts, the 64- and
    the 32-column kernel; vs F.conv2d + bias (+ LeakyReLU) in float64 at 2e-5 max(1, |y|max), and bit-equal to a launch per sample."""
    from neuralrgbd_amd import ops
    N = _walking_grid(1, 1, 1, H2, W2)
    x = _randn(N, H2, W2, Cin, seed=31 + Cin)
    w = _randn(cout_valid, Cin, 3, 3, seed=32 + cout, scale=0.05)
    b = _randn(cout_valid, seed=33, scale=0.2)
    want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), 1, 1)
    want = (F.leaky_relu(want, 0.01) if lrelu else want).permute(0, 2, 3, 1)
    wp = torch.zeros(cout, Cin, 3, 3)
    wp[:cout_valid] = w
    bp = torch.zeros(cout)
    bp[:cout_valid] = b
    xd, bd = x.to(DEV), bp.to(DEV)
    stream = ops.conv_wino_pack32(wp.to(DEV)) if cout == 32 else ops.conv_wino_pack(wp.to(DEV))

    def run(sl):
        out = torch.full((xd[sl].shape[0], H2, W2, ldy), 7.0, device=DEV)
        return ops.conv_wino_rnet(xd[sl], stream, cout, bias=bd, lrelu=lrelu, out=out, ycoff=ycoff, cout_valid=cout_valid)
    out = run(slice(None))
    err = (out[..., ycoff:ycoff + cout_valid].double().cpu() - want).abs().max().item()
    bound = 2e-5 * max(1.0, want.abs().max().item())
    print("[parity] R-Net Winograd walk, %s N%d %dx%d %d->%d (%d valid at %d of %d) lrelu=%d: max|d vs fp64|=%.3e (bound %.3e)"
          % (name, N, H2, W2, Cin, cout, cout_valid, ycoff, ldy, lrelu, err, bound))
    assert err < bound
    assert bool((out[..., :ycoff] == 7.0).all()) and bool((out[..., ycoff + cout_valid:] == 7.0).all())   # nothing else touched
    assert _same_bits(out, run(slice(None)))
    assert ww.launch_tiles(1, H2, W2, 1) <= _ncu()
    assert _same_bits(out, torch.cat([run(slice(i, i + 1)) for i in range(N)], 0))


# ----------------------------------------------------------------------------- deconv form (EPI = 2)
@pytest.mark.parametrize("Cin,ldy", [(96, 80), (128, 96)])
def test_deconv_form_where_every_workgroup_walks(Cin, ldy):
    """nrgbd_conv_wino_rnet_deconv_f32 into NaN-filled [N, 2H, 2W, ldy]: four phases per tile row, so the list is 4 x 56 per sample (256
    CUs: N = 3, 672 tiles, walks of 2 and 3; the phase is constant along a walk on this device: DESIGN.md).  vs F.conv_transpose2d + bias
    + LeakyReLU in float64 at 2e-5 max(1, |y|max); columns beyond 64 stay NaN; bit-equal to the unmasked evaluation + pixel shuffle and
    to a launch per sample."""
    from neuralrgbd_amd import ops
    N = _walking_grid(4, 1, 1, H2, W2)
    x = _randn(N, H2, W2, Cin, seed=61 + Cin)
    w = _randn(Cin, 64, 4, 4, seed=62, scale=0.05)
    b = _randn(64, seed=63, scale=0.1)
    want = F.leaky_relu(F.conv_transpose2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), 2, 1), 0.01).permute(0, 2, 3, 1)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    stream = ops.conv_wino_pack(ops.deconv_phase_weights(wd))
    masked_stream = ops.conv_wino_rnet_deconv_pack(stream, Cin)

    def run(sl):
        n = xd[sl].shape[0]
        return ops.conv_wino_rnet_deconv(xd[sl], masked_stream, torch.full((n, 2 * H2, 2 * W2, ldy), float("nan"), device=DEV), bias=bd,
                                         ycoff=0, cout_valid=64)
    got = run(slice(None))
    assert bool(torch.isfinite(got[..., :64]).all()) and bool(torch.isnan(got[..., 64:]).all())
    err = (got[..., :64].double().cpu() - want).abs().max().item()
    bound = 2e-5 * max(1.0, want.abs().max().item())
    print("[parity] deconv walk N%d %dx%d %d->64 into %d: max|d vs fp64|=%.3e (bound %.3e)" % (N, H2, W2, Cin, ldy, err, bound))
    assert err < bound
    y4 = ops.conv_wino_rnet(xd, stream, 256, bias=bd.repeat(4), lrelu=True)               # unmasked: the R-Net form, four column groups
    unmasked = y4.reshape(N, H2, W2, 2, 2, 64).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H2, 2 * W2, 64)
    assert _same_bits(got[..., :64], unmasked)
    assert _same_bits(got, run(slice(None)))
    assert ww.launch_tiles(1, H2, W2, 4) <= _ncu()
    assert _same_bits(got, torch.cat([run(slice(i, i + 1)) for i in range(N)], 0))


# ----------------------------------------------------------------------------- wino_dw4.hip's input forms on its walking grid
@functools.lru_cache(maxsize=1)
def _dw4_case():
    D, H, W, C = 16, 40, 224, 64
    x = _randn(D, H, W, C, seed=33, scale=3.0)
    w = _randn(C, C, 3, 3, 3, seed=34, scale=0.05)
    ss = _randn(C, 2, seed=35)
    out = {"x": x, "w": w, "ss": ss}
    for relu in (False, True):
        def act(dtype):
            a = x.to(dtype) * ss[:, 0].to(dtype) + ss[:, 1].to(dtype)
            return torch.relu(a) if relu else a
        want = _conv64(act(torch.float64), w, 3, 1)
        cost = (_conv64(act(torch.float32), w, 3, 1) - want).abs().max().item()
        plain = 4e-5 * max(1.0, want.abs().max().item())
        out[relu] = {"want": want, "cost": cost, "plain_bound": plain, "bound": plain + 2.0 * cost}
    return out


@pytest.mark.parametrize("relu", [False, True])
def test_dw4_input_forms_where_a_workgroup_walks(relu):
    """wino_dw4.hip at (16, 40, 224), the 280-tile grid of test_conv_wino_dw4_plain_vs_torch: act(x * s + t) with and without ReLU vs
    float64 — the plain test's bound 4e-5 max(1, |y|max) + twice the measured cost of rounding the prologue to fp32 —, statistics rows,
    two runs with equal bits; the clamped-FMA ReLU bit-equal to its plain form.  Measured cost / bound: 1.326e-06 / 1.540e-03 without
    ReLU, 9.945e-07 / 1.109e-03 with it."""
    from neuralrgbd_amd import ops
    import math
    D, H, W, C = 16, 40, 224, 64
    tiles = (D // 4) * (H // 8) * (W // 16)
    assert 0 < _ncu() < tiles == 280, (_ncu(), tiles)        # fails if the walk is no longer exercised
    c = _dw4_case()
    ref = c[relu]
    xd, ssd, wd = c["x"].to(DEV), c["ss"].to(DEV), c["w"].to(DEV)
    wp = ops.conv_wino_dw4_pack(wd)
    y, st = ops.conv_wino_dw4(xd, wp, C, x_ss=ssd, x_relu=relu)
    err = (y.double().cpu() - ref["want"]).abs().max().item()
    print("[parity] conv_wino_dw4 walk %dx%dx%d x_ss relu=%d: max|d vs fp64| %.3e (plain bound %.3e, fp32-prologue cost %.3e, bound %.3e)"
          % (D, H, W, relu, err, ref["plain_bound"], ref["cost"], ref["bound"]))
    assert err < ref["bound"]
    f = ref["bound"] / ref["plain_bound"]
    s = st.double().sum(1).cpu()
    assert torch.allclose(s[:C], ref["want"].sum((0, 1, 2)), rtol=1e-5 * f, atol=2e-3 * f)
    assert torch.allclose(s[C:], (ref["want"] ** 2).sum((0, 1, 2)), rtol=1e-5 * f, atol=2e-3 * f)
    y2, st2 = ops.conv_wino_dw4(xd, wp, C, x_ss=ssd, x_relu=relu)
    assert _same_bits(y, y2) and _same_bits(st, st2)
    if relu:
        act_max = torch.relu(c["x"] * c["ss"][:, 0] + c["ss"][:, 1]).max().item()
        for k in (math.floor(math.log2(act_max)) + 1, 14):
            y1, st1 = ops.conv_wino_dw4(xd, ops.conv_wino_dw4_pack(wd * 2.0 ** k), C, x_ss=ssd, x_relu=True, x_unit=2.0 ** -k)
            assert _same_bits(y, y1) and _same_bits(st, st1), k
