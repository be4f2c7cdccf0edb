"""Host-side checks of the colour carried through the TSDF volume: the four C entries (declared, bound, exported, every refusal without
a GPU and in the documented order), the fp32 restatement of tests/tsdf_color_ref.py against the float64 one on tsdf_ref's families and
grids (flips capped: a condition on the inputs; values inside the bounds derived in tsdf_color_ref's header), the closed forms (an
affine colour field, a constant-colour image), fusion.to_uint8 and save_ply with colours, and the Python refusals.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tsdf_color_ref as cref
import tsdf_raycast_ref as rc
import tsdf_ref as ref
from conftest import ROOT
from neuralrgbd_amd import _lib, fusion, ops

U = ref.U
FLIP_CAP = 1e-3                 # of the touched voxels, per case: the cap tests/test_tsdf_host.py uses
ENTRIES = {"nrgbd_tsdf_integrate_color_f32": 35, "nrgbd_tsdf_extract_points_color": 18, "nrgbd_tsdf_extract_mesh_color": 20,
           "nrgbd_tsdf_raycast_color_f32": 26}
COLOURLESS = {"nrgbd_tsdf_integrate_color_f32": ("nrgbd_tsdf_integrate_f32", 9), "nrgbd_tsdf_extract_points_color": ("nrgbd_tsdf_extract_points", 2),
              "nrgbd_tsdf_extract_mesh_color": ("nrgbd_tsdf_extract_mesh", 2), "nrgbd_tsdf_raycast_color_f32": ("nrgbd_tsdf_raycast_f32", 2)}


# ---- 1. the C entries
def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nrgbd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES.items():
        decl = re.search(r"\bint %s\((.*?)\);" % name, code, flags=re.S).group(1)
        assert decl.count(",") + 1 == len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name)
        assert re.search(r"%s\b[^.]*— no counterpart in the reference" % name, header), name
        assert name in header[:header.index("#define NRGBD_INTERFACE_VERSION")]       # named in the list at the top
        plain, more = COLOURLESS[name]
        assert nargs == len(_lib.SIGNATURES[plain][1]) + more                           # the colourless entry's arguments plus the colour's
    assert header.count('#define NRGBD_INTERFACE_VERSION "0.10"') == 1                 # no entry changed or disappeared


E_NULL, E_SHAPE, E_ALIGN, E_ARG = -1, -2, -3, -4
P = ctypes.c_void_p(64)                     # never dereferenced: every call below is refused before anything touches the device
NAN, INF = float("nan"), float("inf")


def test_integrate_color_refuses_bad_arguments_without_a_gpu():
    fn = _lib.load().nrgbd_tsdf_integrate_color_f32
    pose = (ctypes.c_float * 12)(*np.eye(4, dtype=np.float32)[:3].reshape(-1))

    def call(null=None, X=8, Y=6, Z=4, H=5, W=7, vs=.05, trunc=.15, d_near=0., d_far=INF, w_max=64., box=None, Hc=9, Wc=11,
             Kc=(40., 40., 5.5, 4.5), affine=(1., 1., 1., 0., 0., 0.)):
        ca = (ctypes.c_float * 6)(*affine)
        host = {3: ctypes.cast(pose, ctypes.c_void_p), 6: ctypes.cast(ca, ctypes.c_void_p)}
        ptr = [None if i == null else host.get(i, P) for i in range(7)]       # tsdf, weight, depth, pose, color, image, affine
        cbox = None if box is None else (ctypes.c_int * 6)(*box)
        return fn(ptr[0], ptr[1], ptr[4], X, Y, Z, 0., 0., 0., vs, ptr[2], None, 0., None, H, W, ptr[3], 30., 30., 3.5, 2.5, trunc, d_near,
                  d_far, w_max, cbox, ptr[5], Hc, Wc, Kc[0], Kc[1], Kc[2], Kc[3], ptr[6], None)
    for i in range(7):
        assert call(null=i) == E_NULL, i
    for kw in (dict(X=0), dict(Y=-1), dict(Z=0), dict(H=0), dict(W=-3), dict(X=2 ** 16, Y=2 ** 15, Z=2), dict(X=2 ** 31 - 1, Y=2, Z=1),
               dict(X=2 ** 16, Y=2 ** 16, Z=2 ** 16), dict(box=(-1, 0, 0, 8, 6, 4)), dict(box=(0, 0, 0, 9, 6, 4)), dict(box=(0, 0, 0, 8, 7, 4)),
               dict(box=(0, 0, 0, 8, 6, 5)), dict(box=(3, 0, 0, 3, 6, 4)), dict(box=(0, 4, 0, 8, 2, 4)), dict(box=(0, 0, 4, 8, 6, 4)),
               dict(Hc=0), dict(Wc=0), dict(Hc=-2), dict(Wc=-1)):
        assert call(**kw) == E_SHAPE, kw
    bad = lambda seq, i, v: tuple(v if j == i else x for j, x in enumerate(seq))
    args = [dict(vs=0.), dict(vs=-1.), dict(vs=NAN), dict(vs=INF), dict(trunc=0.), dict(trunc=NAN), dict(trunc=INF), dict(w_max=0.),
            dict(w_max=-2.), dict(w_max=NAN), dict(w_max=INF), dict(d_near=1., d_far=1.), dict(d_near=2., d_far=1.), dict(d_near=NAN),
            dict(d_far=NAN)]
    args += [dict(Kc=bad((40., 40., 5.5, 4.5), i, v)) for i in range(4) for v in (NAN, INF, -INF)]
    args += [dict(affine=bad((1., 1., 1., 0., 0., 0.), i, v)) for i in range(6) for v in (NAN, INF)]
    for kw in args:
        assert call(**kw) == E_ARG, kw
    # the order of the checks: NULL, then shape (the grid, H W, Hc Wc, the box), then argument (the colourless ones, then the colour's)
    assert call(null=4, X=0, vs=0.) == E_NULL and call(null=6, Hc=0) == E_NULL and call(X=0, vs=0.) == E_SHAPE
    assert call(Hc=0, vs=0.) == E_SHAPE and call(box=(0, 0, 0, 9, 6, 4), affine=(NAN,) * 6) == E_SHAPE
    assert call(Wc=0, Kc=(NAN,) * 4) == E_SHAPE and call(vs=0., Kc=(NAN,) * 4) == E_ARG
    assert call(X=2 ** 16, Y=2 ** 15, Z=1, affine=bad((1.,) * 6, 5, NAN)) == E_ARG       # exactly 2^31 voxels is a grid


def test_extract_color_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    V = _lib.TSDF_EXTRACT_VOXELS

    def points(null=None, X=8, Y=6, Z=4, vs=.05, w_min=1., bytes_=16, cap=10, ws_ptr=P, counts_ptr=P):
        ptr = [None if i == null else P for i in range(7)]          # tsdf, weight, color, workspace, points, colors, counts
        ptr[3] = ptr[3] and ws_ptr
        ptr[6] = ptr[6] and counts_ptr
        return lib.nrgbd_tsdf_extract_points_color(ptr[0], ptr[1], ptr[2], X, Y, Z, 0., 0., 0., vs, w_min, ptr[3], bytes_, ptr[4], ptr[5], cap,
                                                   ptr[6], None)

    def mesh(null=None, X=8, Y=6, Z=4, vs=.05, w_min=1., bytes_=2 ** 20, vcap=10, fcap=10, ws_ptr=P, counts_ptr=P):
        ptr = [None if i == null else P for i in range(8)]          # tsdf, weight, color, workspace, vertices, colors, faces, counts
        ptr[3] = ptr[3] and ws_ptr
        ptr[7] = ptr[7] and counts_ptr
        return lib.nrgbd_tsdf_extract_mesh_color(ptr[0], ptr[1], ptr[2], X, Y, Z, 0., 0., 0., vs, w_min, ptr[3], bytes_, ptr[4], ptr[5], vcap,
                                                 ptr[6], fcap, ptr[7], None)
    for i in range(7):
        assert points(null=i) == E_NULL, i
    for i in range(8):
        assert mesh(null=i) == E_NULL, i
    # colors (and points / vertices / faces) may be NULL only when their capacity is 0; then the call goes on to the next check
    assert points(null=5, cap=0, vs=0.) == E_ARG and points(null=4, cap=0, vs=0.) == E_ARG and points(null=2, cap=0) == E_NULL
    assert mesh(null=5, vcap=0, vs=0.) == E_ARG and mesh(null=6, fcap=0, vs=0.) == E_ARG and mesh(null=2, vcap=0, fcap=0) == E_NULL
    for kw in (dict(X=0), dict(Z=-1), dict(X=2 ** 16, Y=2 ** 15, Z=2, bytes_=2 ** 40), dict(cap=-1), dict(bytes_=15), dict(X=V + 1, Y=1, Z=1, bytes_=16)):
        assert points(**kw) == E_SHAPE, kw
    for kw in (dict(X=0), dict(Z=-1), dict(X=2 ** 16, Y=2 ** 15, Z=1, bytes_=2 ** 40), dict(vcap=-1), dict(fcap=-1),
               dict(bytes_=ops.tsdf_mesh_workspace(8, 6, 4) - 1)):
        assert mesh(**kw) == E_SHAPE, kw
    for fn in (points, mesh):
        for kw in (dict(vs=0.), dict(vs=NAN), dict(vs=INF), dict(w_min=NAN)):
            assert fn(**kw) == E_ARG, kw
        assert fn(ws_ptr=ctypes.c_void_p(68)) == E_ALIGN and fn(counts_ptr=ctypes.c_void_p(36)) == E_ALIGN
        # the order of the checks: NULL, shape, argument, alignment
        assert fn(null=2, X=0, vs=0.) == E_NULL and fn(X=0, vs=0.) == E_SHAPE and fn(vs=0., ws_ptr=ctypes.c_void_p(68)) == E_ARG


def test_raycast_color_refuses_bad_arguments_without_a_gpu():
    fn = _lib.load().nrgbd_tsdf_raycast_color_f32
    eye = np.eye(4, dtype=np.float32)[:3].reshape(-1)

    def call(null=None, X=8, Y=6, Z=4, H=5, W=7, vs=.05, fx=30., fy=30., d_near=0., d_far=INF, w_min=1., step=.05, pose=eye,
             centre=(0., 0., 0.), normal=P):
        cp, cc = (ctypes.c_float * 12)(*pose), (ctypes.c_float * 3)(*centre)
        host = (P, P, ctypes.cast(cp, ctypes.c_void_p), ctypes.cast(cc, ctypes.c_void_p), P, P, P)
        ptr = [None if i == null else p for i, p in enumerate(host)]            # tsdf, weight, pose, centre, depth, color, rgb
        return fn(ptr[0], ptr[1], ptr[5], X, Y, Z, 0., 0., 0., vs, ptr[2], ptr[3], fx, fy, 3.5, 2.5, H, W, d_near, d_far, w_min, step, ptr[4],
                  normal, ptr[6], None)
    for i in range(7):
        assert call(null=i) == E_NULL, i
    for kw in (dict(X=0), dict(Y=-1), dict(Z=0), dict(H=0), dict(W=-3), dict(X=2 ** 16, Y=2 ** 15, Z=2), dict(X=2 ** 31 - 1, Y=2, Z=1),
               dict(X=2 ** 16, Y=2 ** 16, Z=2 ** 16), dict(H=16385), dict(W=16385)):
        assert call(**kw) == E_SHAPE, kw
    bad = lambda i, v: tuple(v if j == i else x for j, x in enumerate(eye))
    for kw in (dict(vs=0.), dict(vs=-1.), dict(vs=NAN), dict(vs=INF), dict(step=0.), dict(step=-.1), dict(step=NAN), dict(step=INF),
               dict(fx=0.), dict(fx=NAN), dict(fx=INF), dict(fy=-1.), dict(fy=NAN), dict(fy=INF), dict(d_near=1., d_far=1.),
               dict(d_near=2., d_far=1.), dict(d_near=NAN), dict(d_far=NAN), dict(w_min=NAN), dict(pose=bad(0, NAN)), dict(pose=bad(7, INF)),
               dict(pose=bad(11, -INF)), dict(centre=(0., NAN, 0.)), dict(centre=(INF, 0., 0.))):
        assert call(**kw) == E_ARG, kw
    assert call(null=5, X=0, vs=0.) == E_NULL and call(null=6, H=0) == E_NULL and call(X=0, vs=0.) == E_SHAPE
    assert call(H=16385, pose=bad(3, NAN)) == E_SHAPE and call(normal=None, w_min=NAN) == E_ARG      # normal may be NULL


# ---- 2. fp32 against float64
def _compare(family, dims, size, variant):
    """-> (touched, flips, colour flips that are not geometry's, worst |C32 - C64| / bound) over the views of a case."""
    case = ref.make_case(family, dims, size)
    shape = dims[::-1]
    Kc = cref.color_K(case, variant)
    m = max(abs(a) + abs(b) for a, b in zip(*cref.AFFINE))                               # the images lie in [0, 1)
    agree = np.ones(shape, bool)
    bound_C = np.zeros(shape)
    C32, W32, C64, W64 = np.zeros((3,) + shape, np.float32), np.zeros(shape, np.float32), np.zeros((3,) + shape), np.zeros(shape)
    T32, T64 = np.zeros(shape, np.float32), np.zeros(shape)
    touched = flips = extra = 0
    for v in range(len(case["views"])):
        image = cref.make_image(family, dims, size, variant, v)
        a = cref.observe(np.float32, case, v, image, Kc, cref.AFFINE)
        b = cref.observe(np.float64, case, v, image, Kc, cref.AFFINE)
        geometry = (a["ok"] != b["ok"]) | (a["ok"] & b["ok"] & (a["pix"] != b["pix"]))
        colour = a["ok"] & b["ok"] & (a["cpix"] != b["cpix"])
        flip = geometry | colour
        touched += int(a["ok"].sum())
        flips += int(flip.sum())
        extra += int((colour & ~geometry).sum())
        agree &= ~flip
        both = a["fin"] & b["fin"] & ~flip
        assert np.array_equal((a["fin"] & ~flip), (b["fin"] & ~flip))                    # the same pixel: the same finiteness
        dc = np.abs(a["c"].astype(np.float64) - b["c"])
        assert (dc[:, both] <= 2 * U * m).all(), (family, dims, size, variant, v)        # e(c) = 2 u m
        bound_C = np.where(both, np.maximum(bound_C, 2 * U * m) + 8 * U * m, bound_C)
        C32, C64 = cref.integrate(np.float32, C32, W32, a), cref.integrate(np.float64, C64, W64, b)
        T32, W32 = ref.integrate(np.float32, T32, W32, a, case["w_max"])
        T64, W64 = ref.integrate(np.float64, T64, W64, b, case["w_max"])
    dC = np.abs(C32.astype(np.float64) - C64)
    assert (dC[:, agree] <= bound_C[agree][None]).all(), (family, dims, size, variant)
    worst = float((dC[:, agree] / np.maximum(bound_C[agree][None], 1e-300)).max()) if agree.any() and bound_C[agree].any() else 0.0
    return touched, flips, extra, worst


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_fp32_colour_against_float64_on_every_family_and_grid(family):
    total = 0
    for dims in ref.GRIDS:
        for size in cref.DEPTH_SIZES:
            for variant in cref.VARIANTS:
                touched, flips, extra, worst = _compare(family, dims, size, variant)
                if dims == ref.PLANE_GRID and size == ref.PLANE_SIZE:
                    print("[tsdf colour] %s %s: %d touched, %d flips (%d colour-only), worst |C32 - C64| / bound %.3f"
                          % (family, variant, touched, flips, extra, worst))
                assert flips <= FLIP_CAP * touched, (family, dims, size, variant, flips, touched)
                assert worst <= 1.0
                if variant in ("same", "one"):
                    assert extra == 0, (family, dims, size, variant)                     # uc is u, bit for bit (one pixel: nothing to flip)
                total += touched
    assert total > 0 or family == "behind"


def test_colour_image_at_the_depth_size_projects_bit_identically():
    for family in ("front", "edge", "inside"):
        case = ref.make_case(family, ref.PLANE_GRID, ref.PLANE_SIZE)
        for v in range(len(case["views"])):
            o = cref.observe(np.float32, case, v, cref.make_image(family, ref.PLANE_GRID, ref.PLANE_SIZE, "same", v), case["K"])
            assert o["ok"].any() and np.array_equal(o["cpix"][o["ok"]], o["pix"][o["ok"]])     # no clamp bites inside the map either


@pytest.mark.parametrize("family", ["front", "inside", "side", "edge"])
def test_fp32_extraction_lerp_against_float64(family):
    """On the stored fp32 volume (the same on both sides: e(C) = 0 and e(q) = 2 u |q| — the difference and the quotient round once
    each): |col32 - col64| <= (e(q) + 3 u) |Cb - Ca| + u m."""
    n = 0
    for dims in ref.GRIDS:
        T, Wt, C = cref.fused(family, dims, ref.PLANE_SIZE, "x4")[-1]
        c32 = cref.extract(np.float32, T, Wt, C, 1.0)
        c64, q, d = cref.extract(np.float64, T, Wt, C, 1.0, with_q=True)
        assert len(c32) == len(c64) == len(ref.extract(np.float32, T, Wt, (0, 0, 0), 0.05, 1.0))
        if not len(c64):
            continue
        m = float(np.abs(C).max())
        bound = 1.01 * ((2 * U * np.abs(q)[:, None] + 3 * U) * d + U * m)
        assert (np.abs(c32.astype(np.float64) - c64) <= bound).all(), (family, dims)
        assert (q >= 0).all() and (q <= 1).all()
        n += len(c64)
    assert n > 100


# ---- 3. closed forms
COEF = ((1, 2, 0, -1), (0, 0, 3, 1), (5, -1, 1, 2))                 # c_j = k0 + k1 ix + k2 iy + k3 iz


def _affine_at(points, origin, vs):
    g = (np.asarray(points, np.float64) - np.asarray(origin, np.float64)) / vs          # lattice coordinates
    return np.stack([k[0] + k[1] * g[:, 0] + k[2] * g[:, 1] + k[3] * g[:, 2] for k in COEF], axis=1)


def test_an_affine_colour_field_comes_back_at_the_vertices_and_at_the_hits():
    dims, vs, origin, trunc = (24, 20, 16), 0.0625, (-0.75, -0.625, 0.75), 0.1875       # powers of two: lattice coordinates are exact
    X, Y, Z = dims
    normal = -np.array([0.1, -0.15, 1.0]) / np.linalg.norm([0.1, -0.15, 1.0])         # T > 0, free space, on the camera's side
    T, Wt = rc.linear_field(dims, origin, vs, trunc, normal, -1.2, np.float32)
    C = cref.affine_field(dims, COEF)
    m = float(np.abs(C).max())
    # vertices: the point is o + vs (i + q), the colour C(a) + q (C(b) - C(a)) with the same q: the function at the point up to the
    # roundings of the two (3 u m for the colour, 2 u |p| / vs |k| for the point's own coordinates, which the function then scales)
    pts = ref.extract(np.float32, T, Wt, origin, vs, 1.0)
    cols = cref.extract(np.float32, T, Wt, C, 1.0)
    assert len(pts) == len(cols) > 300
    slope = max(sum(abs(c) for c in k[1:]) for k in COEF)
    bound = 3 * U * m + slope * 2 * U * float(np.abs(pts).max() + 1) / vs
    assert np.abs(cols.astype(np.float64) - _affine_at(pts, origin, vs)).max() <= bound
    # the ray cast: the trilinear interpolant of an affine field is the field; seven lerps in three levels round three times each on
    # values of at most m (15 u m), and the hit point p carries 2 u |p| of its own
    view = {"size": (33, 65), "extM": np.eye(4), "K": rc.render_K(33, 65), "depth_range": (0.1, 3.0), "w_min": 1.0, "step": None}
    case = {"origin": origin, "vs": vs}
    want = rc.cast(np.float32, case, (T, Wt), view)
    rgb, p, ok, rows = cref.raycast(np.float32, want, Wt, C, origin, vs, view["extM"], view["K"], view["size"], 1.0)
    assert ok.sum() > 300 and ok.all()
    g = np.stack([np.asarray(a, np.float64) for a in p], axis=1)
    exact = np.stack([k[0] + k[1] * g[:, 0] + k[2] * g[:, 1] + k[3] * g[:, 2] for k in COEF], axis=0)
    got = rgb.reshape(3, -1)[:, rows].astype(np.float64)
    assert np.abs(got - exact).max() <= 15 * U * m + slope * 2 * U * float(np.abs(g).max())
    assert not rgb.reshape(3, -1)[:, ~want["hit"].reshape(-1)].any()


def test_a_constant_colour_image_gives_that_constant():
    """Wt = 0: C' = (0 * 0 + c * w) / (0 + w) = c exactly with w = 1 (the clean plane scene: no weight map).  With Wt = k observations
    behind it the update rounds the sum and the quotient, 2 u c, and inherits k / (k + 1) of what was there: after six views at most
    6 u c, which stays within 2 u for c <= 0.3."""
    family, dims, size = "front", ref.PLANE_GRID, ref.PLANE_SIZE
    case = ref.make_case(family, dims, size, True)
    const = np.float32([0.3, 0.1, 0.2])
    image = np.broadcast_to(const[:, None, None], (3,) + size).copy()
    shape = dims[::-1]
    T, Wt, C = np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.zeros((3,) + shape, np.float32)
    first = 0
    for v in range(len(case["views"])):
        obs = cref.observe(np.float32, case, v, image, case["K"])
        fresh = obs["fin"] & (Wt == 0)
        C = cref.integrate(np.float32, C, Wt, obs)
        assert (C[:, fresh] == const[:, None]).all()
        first += int(fresh.sum())
        T, Wt = ref.integrate(np.float32, T, Wt, obs, case["w_max"])
        seen = Wt > 0
        assert (np.abs(C[:, seen].astype(np.float64) - const[:, None].astype(np.float64)) <= 2 * U).all() and not C[:, ~seen].any()
    assert first > 1000 and Wt.max() == 6.0


# ---- 4. to_uint8 and save_ply
def test_to_uint8():
    half = np.float32(0.5) / np.float32(255)
    x = np.array([0.0, 1.0, -0.2, 1.7, half, np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(0)), np.nan, np.inf, -np.inf,
                  0.25, 254.5 / 255], np.float32)
    want = np.rint(np.clip(np.where(np.isnan(x), 0, x), 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8)
    assert list(want[:4]) == [0, 255, 0, 255] and want[5] == 1 and want[6] == 0 and list(want[7:11]) == [0, 255, 0, 64]       # a NaN is 0
    assert want[4] == (0 if half * np.float32(255) <= 0.5 else 1)                       # 0.5 ties to even: 0
    got = fusion.to_uint8(x)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    t = fusion.to_uint8(torch.from_numpy(x))
    assert t.dtype == torch.uint8 and np.array_equal(t.numpy(), want)
    every = np.arange(256, dtype=np.float32) / np.float32(255)
    assert np.array_equal(fusion.to_uint8(every), np.arange(256)) and np.array_equal(fusion.to_uint8(torch.from_numpy(every)).numpy(), np.arange(256))
    assert fusion.to_uint8(np.zeros((4, 3), np.float32)).shape == (4, 3)


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    nf = ([int(ln.split()[-1]) for ln in lines if ln.startswith("element face")] or [0])[0]
    props = [ln.split()[1:] for ln in lines if ln.startswith("property") and "list" not in ln]
    coloured = [p[1] for p in props] == ["x", "y", "z", "red", "green", "blue"]
    assert coloured or [p[1] for p in props] == ["x", "y", "z"]
    if "binary_little_endian" in lines[1]:
        vt = np.dtype([("p", "<f4", (3,))] + ([("c", "u1", (3,))] if coloured else []))
        v = np.frombuffer(body, vt, nv)
        f = np.frombuffer(body, np.dtype([("n", "u1"), ("v", "<i4", (3,))]), nf, offset=nv * vt.itemsize)
        assert len(body) == nv * vt.itemsize + nf * 13 and (f["n"] == 3).all()
        return v["p"], (v["c"] if coloured else None), f["v"]
    rows = body.decode("ascii").split("\n")
    assert rows[nv + nf:] == [""]
    vals = [r.split() for r in rows[:nv]]
    pts = np.array([[float(x) for x in r[:3]] for r in vals], np.float32).reshape(-1, 3)
    cols = np.array([[int(x) for x in r[3:]] for r in vals], np.uint8).reshape(-1, 3) if coloured else None
    faces = np.array([[int(x) for x in r.split()[1:]] for r in rows[nv:nv + nf]], np.int32).reshape(-1, 3)
    return pts, cols, faces


def _save_ply_before_colour(path, points, faces=None, binary=False):
    """The bytes the writer produced before it took colours (the format its docstring fixes), written out independently."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    head = "ply\nformat %s 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % (
        "binary_little_endian" if binary else "ascii", len(p))
    if faces is not None:
        head += "element face %d\nproperty list uchar int vertex_indices\n" % len(faces)
    head += "end_header\n"
    out = head.encode("ascii")
    if binary:
        out += p.astype("<f4").tobytes()
        for tri in (faces if faces is not None else ()):
            out += b"\x03" + np.asarray(tri, "<i4").tobytes()
    else:
        out += "".join("%.9g %.9g %.9g\n" % tuple(r) for r in p).encode("ascii")
        out += "".join("3 %d %d %d\n" % tuple(t) for t in (faces if faces is not None else ())).encode("ascii")
    open(path, "wb").write(out)


def test_save_ply_with_and_without_colours(tmp_path):
    rng = np.random.RandomState(4)
    pts = np.concatenate([rng.randn(40, 3).astype(np.float32) * 3, [[0.0, -0.0, 1e-30], [np.float32(1) / 3, 1e20, -7.25]]]).astype(np.float32)
    faces = rng.randint(0, len(pts), size=(25, 3)).astype(np.int32)
    cols = rng.rand(len(pts), 3).astype(np.float32) * 1.4 - 0.2                         # beyond [0, 1] on both sides
    u8 = fusion.to_uint8(cols)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    for binary in (False, True):
        for f in (None, faces):
            for c in (cols, torch.from_numpy(cols), u8, torch.from_numpy(u8)):
                assert fusion.save_ply(a, torch.from_numpy(pts), faces=f, binary=binary, colors=c) == len(pts)
                gp, gc, gf = _read_ply(a)
                assert np.array_equal(gp.view(np.int32), pts.view(np.int32)) and np.array_equal(gc, u8), (binary, type(c))
                assert np.array_equal(gf, faces if f is not None else np.zeros((0, 3), np.int32))
            # without colours: the bytes of the writer as it was
            fusion.save_ply(a, pts, faces=f, binary=binary)
            _save_ply_before_colour(b, pts, f, binary)
            assert open(a, "rb").read() == open(b, "rb").read(), (binary, f is None)
    assert fusion.save_ply(a, np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.float32)) == 0
    with pytest.raises(ValueError):
        fusion.save_ply(a, pts, colors=cols[:-1])
    with pytest.raises(ValueError):
        fusion.save_ply(a, pts, colors=np.zeros((len(pts), 3), np.int32))


# ---- 5. the Python surface
def test_python_refusals():
    import gen_dgf_golden as gg
    import neuralrgbd_amd
    K = (30., 30., 3.5, 2.5)
    d = torch.ones(5, 7)
    img = torch.zeros(3, 5, 7)
    col = fusion.TSDFVolume((4, 3, 2), .05, (0, 0, 0), device="cpu", color=True)
    plain = fusion.TSDFVolume((4, 3, 2), .05, (0, 0, 0), device="cpu")
    assert tuple(col._buf.shape) == (5, 2, 3, 4) and tuple(col.color.shape) == (3, 2, 3, 4) and plain.color is None
    assert col.tsdf.data_ptr() == col._buf.data_ptr() and col.color.data_ptr() == col._buf[2].data_ptr() and tuple(plain._buf.shape) == (2, 2, 3, 4)
    col._buf.fill_(1.0)
    col.reset()
    assert not col._buf.any()
    with pytest.raises(ValueError, match="colour"):                  # a colour volume without an image: the weight would go out of step
        col.integrate(d, np.eye(4), K, cull=False)
    with pytest.raises(ValueError, match="colour"):
        plain.integrate(d, np.eye(4), K, cull=False, color=img)
    with pytest.raises(ValueError):
        plain.integrate(d, np.eye(4), K, cull=False, color_affine=((1, 1, 1), (0, 0, 0)))
    for bad in (torch.zeros(3, 5, 7, dtype=torch.float64), np.zeros((3, 5, 7), np.float32)):
        with pytest.raises(TypeError):
            col.integrate(d, np.eye(4), K, cull=False, color=bad)
    for bad in (torch.zeros(5, 7), torch.zeros(1, 5, 7), torch.zeros(4, 5, 7), torch.zeros(3, 0, 7), torch.zeros(3, 7, 5).transpose(1, 2),
                torch.zeros(3, 5, 7, device="meta")):
        with pytest.raises(ValueError):
            col.integrate(d, np.eye(4), K, cull=False, color=bad)
    with pytest.raises(ValueError, match="color_intrinsics"):         # another size beside plain intrinsics: nothing to default to
        col.integrate(d, np.eye(4), K, cull=False, color=torch.zeros(3, 10, 14))
    with pytest.raises(_lib.NrgbdError):                            # everything in order: it reaches the wrapper, which refuses host tensors
        col.integrate(d, np.eye(4), K, cull=False, color=img)
    with pytest.raises(_lib.NrgbdError):
        col.integrate(d, np.eye(4), {"hfov": 60., "vfov": 45.}, cull=False, color=torch.zeros(3, 10, 14))
    for call in (lambda: plain.points(colors=True), lambda: plain.mesh(colors=True), lambda: plain.raycast(np.eye(4), K, (5, 7), color=True)):
        with pytest.raises(ValueError, match="no colour"):
            call()
    T, Wt = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4)
    with pytest.raises(_lib.NrgbdError):
        ops.tsdf_integrate_color(T, Wt, torch.zeros(3, 2, 3, 4), (0, 0, 0), .05, d, np.eye(4), K, .15, img, K)
    with pytest.raises(ValueError):
        ops.tsdf_raycast(T, Wt, (0, 0, 0), .05, np.eye(4), K, (5, 7), (0., 3.), rgb=True)
    # the stream
    cam, d_candi = gg.model_setup()
    mdl = gg.MODEL
    model = neuralrgbd_amd.KVNET(64, cam, d_candi, mdl["sigma"], 64, None, if_refined=True, refineNet_name="DPV", t_win_r=mdl["r"])
    with pytest.raises(ValueError, match="color=True takes a volume with colour"):
        fusion.FusionVideoStream(model, cam, d_candi, plain, t_win_r=mdl["r"], color=True, device="cpu")
    with pytest.raises(ValueError, match="color=False takes a volume without colour"):
        fusion.FusionVideoStream(model, cam, d_candi, col, t_win_r=mdl["r"], device="cpu")
    fs = fusion.FusionVideoStream(model, cam, d_candi, col, t_win_r=mdl["r"], color=True, device="cpu")
    assert fs.color and fs.volume is col and neuralrgbd_amd.to_uint8 is fusion.to_uint8


def test_the_ring_still_holds_the_frame_that_is_fused():
    """Frame i lies in slot i mod R, R = 2 r + 1.  The frame fused after push n (counted from 0) is n - r, or n - r - 1 with
    pipeline=True, and flush() hands out n - r after the last push n: at most r + 1 pushes behind the newest, and the slots written
    since then are those of frames ref + 1 .. n, none of which is congruent to ref mod R."""
    from neuralrgbd_amd import video
    for r in (1, 2, 3):
        R = 2 * r + 1
        for n_pushed in range(R, 4 * R):
            _, ref_slot, ref_index = video.window_slots(n_pushed, r)
            newest = n_pushed - 1
            assert ref_index == newest - r and ref_slot == ref_index % R
            for fused in (ref_index, ref_index - 1):                 # as it comes out, and one push late (pipeline=True)
                written_since = {i % R for i in range(fused + 1, newest + 1)}
                assert newest - fused <= r + 1 < R and fused % R not in written_since
