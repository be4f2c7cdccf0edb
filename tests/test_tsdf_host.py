"""Host-side checks of the TSDF fusion: the fp32 restatement of tests/tsdf_ref.py against the float64 one on every input of
tests/test_gpu_tsdf.py (flips capped: a condition on the inputs; values inside the bound derived in tsdf_ref), the float64 surface of
the plane scene, fusion.frustum_box, the three C entries (declared, bound, exported, every refusal without a GPU and in a fixed order),
the wrappers' refusals and save_ply.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tsdf_ref as ref
from conftest import ROOT
from neuralrgbd_amd import _lib, fusion, ops

ENTRIES = {"nrgbd_tsdf_integrate_f32": 26, "nrgbd_tsdf_extract_workspace": 3, "nrgbd_tsdf_extract_points": 16}
FLIP_CAP = 1e-3                 # of the touched voxels, per case
CASES = ref.all_cases() + [("front", ref.PLANE_GRID, ref.PLANE_SIZE, True)]


# ---- 1. fp32 against float64 on the GPU tests' inputs
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_fp32_chain_against_float64_on_every_gpu_input(family):
    for key in (c for c in CASES if c[0] == family):
        case = ref.make_case(*key)
        shape = case["dims"][::-1]
        flips = touched = 0
        agree = np.ones(shape, bool)
        bound_T = np.zeros(shape)
        T32, W32, T64, W64 = np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.zeros(shape), np.zeros(shape)
        worst_t = 0.0
        for v in range(len(case["views"])):
            a, b = ref.observe(np.float32, case, v), ref.observe(np.float64, case, v, bound=True)
            flip = (a["ok"] != b["ok"]) | (a["ok"] & b["ok"] & (a["pix"] != b["pix"]))
            flips += int(flip.sum())
            touched += int(a["ok"].sum())
            agree &= ~flip
            both = a["ok"] & b["ok"] & ~flip
            dt = np.abs(a["t"].astype(np.float64) - b["t"])
            assert np.isfinite(b["bound"]).all() and b["bound"].max() <= 5e-5          # not vacuous: t lives in [-1, 1]
            assert (dt[both] <= b["bound"][both]).all(), key
            assert np.array_equal(a["w"][both].astype(np.float64), b["w"][both])        # the weight is a value read, not computed
            worst_t = max(worst_t, float(dt[both].max()) if both.any() else 0.0)
            bound_T = np.where(both, np.maximum(bound_T, b["bound"]) + 8 * ref.U, bound_T)
            T32, W32 = ref.integrate(np.float32, T32, W32, a, case["w_max"])
            T64, W64 = ref.integrate(np.float64, T64, W64, b, case["w_max"])
        dT = np.abs(T32.astype(np.float64) - T64)
        if key[1:] == (ref.PLANE_GRID, ref.PLANE_SIZE) or flips:
            print("[tsdf] %s: %d touched, %d flips, max |t32 - t64| %.2e, max |T32 - T64| %.2e (bound %.2e)"
                  % (key, touched, flips, worst_t, dT[agree].max(), bound_T.max()))
        assert flips <= FLIP_CAP * touched, key
        assert (dT[agree] <= bound_T[agree]).all(), key
        if family == "behind":
            assert touched == 0                                                         # nothing in front of the camera
        if key[1] == ref.PLANE_GRID and key[2] == ref.PLANE_SIZE and family in ("front", "inside", "side", "edge"):
            assert touched > 1000, key                                                  # the case is not empty


def test_views_cover_the_options_and_the_seeded_values():
    case = ref.make_case("front", ref.PLANE_GRID, ref.PLANE_SIZE)
    assert [(v["gate"] is not None, v["wmap"] is not None) for v in case["views"]] == [(False, False), (True, True), (False, True),
                                                                                      (True, False), (False, True), (True, True)]
    lo, hi = (np.float32(x) for x in case["depth_range"])
    for v in case["views"]:
        d = v["depth"]
        for x in (0.0, -1.0, np.inf, lo, hi, np.nextafter(lo, np.float32(4)), np.nextafter(hi, np.float32(0))):
            assert (d == np.float32(x)).any()
        assert np.isnan(d).any()
    g, w = case["views"][1]["gate"], case["views"][1]["wmap"]
    thr = np.float32(ref.GATE_THR)
    assert (g == thr).any() and (g == np.nextafter(thr, np.float32(0))).any() and (g == np.nextafter(thr, np.float32(-9))).any()
    assert np.isnan(g).any() and np.isnan(w).any() and (w == 0).any() and (w < 0).any() and np.isinf(w).any()
    # w_max = 3 binds over six views
    assert ref.fused("front", ref.PLANE_GRID, ref.PLANE_SIZE)[-1][1].max() == 3.0
    assert ref.fused("front", ref.PLANE_GRID, ref.PLANE_SIZE, "float32", True)[-1][1].max() == 6.0


def test_edge_case_lands_on_the_pixel_borders_exactly():
    """edge: with power-of-two intrinsics and spacing the chain is exact on the slice z = 0.5 (and on z = 1), so fp32 and float64 agree
    to the bit there and u, v take the values 0, W and H."""
    case = ref.make_case("edge", ref.PLANE_GRID, ref.PLANE_SIZE)
    a, b = ref.observe(np.float32, case, 0), ref.observe(np.float64, case, 0)
    assert np.array_equal(a["ok"][0], b["ok"][0]) and np.array_equal(a["t"][0].astype(np.float64), b["t"][0]) and a["ok"][0].any()
    X = case["dims"][0]
    xw = case["origin"][0] + case["vs"] * np.arange(X)
    u = 32.0 * (xw / 0.5) + 32.0
    assert 0.0 in u and 64.0 in u and a["pix"][0][:, u == 64.0].max() == -1 and a["pix"][0][:, u == 0.0].max() >= 0
    yw = case["origin"][1] + case["vs"] * np.arange(case["dims"][1])
    v = 32.0 * (yw / 0.5) + 24.0
    assert 0.0 in v and 48.0 in v and a["pix"][0][v == 48.0].max() == -1 and a["pix"][0][v == 0.0].max() >= 0


# ---- 2. the surface of the plane scene in float64
def test_float64_surface_of_the_plane_scene_lies_on_the_plane():
    case = ref.make_case("front", ref.PLANE_GRID, ref.PLANE_SIZE, True)
    T, Wt = ref.fused("front", ref.PLANE_GRID, ref.PLANE_SIZE, "float64", True)[-1]
    pts = ref.extract(np.float64, T, Wt, case["origin"], case["vs"], 1.0)
    dist = ref.plane_distance(pts, case["vs"])
    print("[tsdf] plane scene: %d points, worst distance %.3f voxel" % (len(pts), dist.max()))
    assert len(pts) > 1000 and dist.max() <= 0.25
    # a hand-made volume: one crossing per axis at a known place, in (linear index, axis) order
    T = np.full((2, 2, 2), 0.5, np.float32)
    T[0, 0, 0] = -0.5
    pts = ref.extract(np.float64, T, np.ones_like(T), (1.0, 2.0, 3.0), 0.5, 1.0)
    assert np.array_equal(pts, [[1.25, 2.0, 3.0], [1.0, 2.25, 3.0], [1.0, 2.0, 3.25]])


# ---- 3. frustum_box
class _Vol:
    def __init__(self, case):
        self.dims, self.origin, self.voxel_size = case["dims"], case["origin"], case["vs"]


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_frustum_box_holds_every_touched_voxel(family):
    for key in (c for c in CASES if c[0] == family):
        case = ref.make_case(*key)
        X, Y, Z = case["dims"]
        for i, view in enumerate(case["views"]):
            ok = ref.observe(np.float32, case, i)["ok"]
            box = fusion.frustum_box(view["extM"], case["K"], case["size"], case["depth_range"][1] + case["trunc"], _Vol(case))
            if family == "behind":
                assert box is None and not ok.any()
                continue
            if box is None:
                assert not ok.any(), key
                continue
            x0, y0, z0, x1, y1, z1 = box
            assert 0 <= x0 < x1 <= X and 0 <= y0 < y1 <= Y and 0 <= z0 < z1 <= Z
            inside = np.zeros(ok.shape, bool)
            inside[z0:z1, y0:y1, x0:x1] = True
            assert not (ok & ~inside).any(), key
            if family in ("side", "inside") and case["dims"] == ref.PLANE_GRID:       # the grids that extend beyond what the camera sees
                assert (x1 - x0) * (y1 - y0) * (z1 - z0) < X * Y * Z, key
            # the same bits with and without the box
            assert np.array_equal(ref.observe(np.float32, case, i, box=box)["ok"], ok)


def test_frustum_box_special_poses():
    case = ref.make_case("front", ref.PLANE_GRID, ref.PLANE_SIZE)
    vol, m = _Vol(case), case["views"][0]["extM"]
    assert fusion.frustum_box(m, case["K"], case["size"], float("inf"), vol) == (0, 0, 0) + case["dims"]
    assert fusion.frustum_box(np.full((4, 4), np.nan), case["K"], case["size"], 3.0, vol) is None
    assert fusion.frustum_box(np.zeros((4, 4)), case["K"], case["size"], 3.0, vol) == (0, 0, 0) + case["dims"]       # singular: no culling
    with pytest.raises(ValueError):
        fusion.frustum_box(np.eye(3), case["K"], case["size"], 3.0, vol)
    K = fusion.intrinsics_at({"hfov": 90.0, "vfov": 90.0}, 48, 64)
    assert np.allclose(K, (32.0, 24.0, 32.0, 24.0))


# ---- 4. the C entries
def _header():
    return open(os.path.join(ROOT, "include", "nrgbd.h")).read()


def test_entries_are_declared_bound_and_exported():
    header = _header()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES.items():
        decl = re.search(r"\b(?:int|long) %s\((.*?)\);" % name, code, flags=re.S).group(1)
        assert decl.count(",") + 1 == len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name)
        assert re.search(r"%s — no counterpart in the reference" % name, header), name
    assert header.count('#define NRGBD_INTERFACE_VERSION "0.10"') == 1
    assert b"0.10" in _lib.load().nrgbd_version()
    assert _lib.TSDF_EXTRACT_VOXELS == int(re.search(r"#define NRGBD_TSDF_EXTRACT_VOXELS (\d+)", header).group(1))
    assert _lib.TSDF_SCAN_PASS == int(re.search(r"#define NRGBD_TSDF_SCAN_PASS (\d+)", header).group(1))


E_NULL, E_SHAPE, E_ALIGN, E_ARG = -1, -2, -3, -4
P = ctypes.c_void_p(64)                     # never dereferenced: every call below is refused before anything touches the device
NAN, INF = float("nan"), float("inf")


def test_integrate_refuses_bad_arguments_without_a_gpu():
    fn = _lib.load().nrgbd_tsdf_integrate_f32
    pose = (ctypes.c_float * 12)(*np.eye(4, dtype=np.float32)[:3].reshape(-1))

    def call(null=None, X=8, Y=6, Z=4, H=5, W=7, vs=.05, trunc=.15, d_near=0., d_far=INF, w_max=64., box=None):
        ptr = [None if i == null else P for i in range(3)] + [None if null == 3 else ctypes.cast(pose, ctypes.c_void_p)]
        cbox = None if box is None else (ctypes.c_int * 6)(*box)
        return fn(ptr[0], ptr[1], X, Y, Z, 0., 0., 0., vs, ptr[2], None, 0., None, H, W, ptr[3], 30., 30., 3.5, 2.5, trunc, d_near, d_far,
                  w_max, cbox, None)
    for i in range(4):                                              # tsdf, weight, depth, pose
        assert call(null=i) == E_NULL
    for kw in (dict(X=0), dict(Y=-1), dict(Z=0), dict(H=0), dict(W=-3), dict(X=2 ** 16, Y=2 ** 15, Z=2), dict(X=2 ** 31 - 1, Y=2, Z=1),
               dict(X=2 ** 16, Y=2 ** 16, Z=2 ** 16), dict(box=(-1, 0, 0, 8, 6, 4)), dict(box=(0, 0, 0, 9, 6, 4)), dict(box=(0, 0, 0, 8, 7, 4)),
               dict(box=(0, 0, 0, 8, 6, 5)), dict(box=(3, 0, 0, 3, 6, 4)), dict(box=(0, 4, 0, 8, 2, 4)), dict(box=(0, 0, 4, 8, 6, 4))):
        assert call(**kw) == E_SHAPE, kw
    for kw in (dict(vs=0.), dict(vs=-1.), dict(vs=NAN), dict(vs=INF), dict(trunc=0.), dict(trunc=NAN), dict(trunc=INF), dict(w_max=0.),
               dict(w_max=-2.), dict(w_max=NAN), dict(w_max=INF), dict(d_near=1., d_far=1.), dict(d_near=2., d_far=1.), dict(d_near=NAN),
               dict(d_far=NAN)):
        assert call(**kw) == E_ARG, kw
    # the order of the checks: NULL, then shape, then argument
    assert call(null=0, X=0, vs=0.) == E_NULL and call(X=0, vs=0.) == E_SHAPE and call(box=(0, 0, 0, 9, 6, 4), trunc=0.) == E_SHAPE
    assert call(X=2 ** 16, Y=2 ** 15, Z=1, vs=0.) == E_ARG          # exactly 2^31 voxels is a grid


def test_extract_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    ws, fn = lib.nrgbd_tsdf_extract_workspace, lib.nrgbd_tsdf_extract_points
    V = _lib.TSDF_EXTRACT_VOXELS
    assert ws(1, 1, 1) == 16 and ws(V, 1, 1) == 16 and ws(V + 1, 1, 1) == 32 and ws(256, 256, 256) == 2 ** 24 // V * 16
    assert ws(2 ** 16, 2 ** 15, 1) == 2 ** 31 // V * 16
    for dims in ((0, 1, 1), (1, -1, 1), (1, 1, 0), (2 ** 16, 2 ** 15, 2), (2 ** 31 - 1, 2, 1)):
        assert ws(*dims) == E_SHAPE, dims

    def call(null=None, X=8, Y=6, Z=4, vs=.05, w_min=1., bytes_=16, cap=10, ws_ptr=P, counts_ptr=P):
        ptr = [None if i == null else P for i in range(5)]          # tsdf, weight, workspace, points, counts
        if ptr[2] is not None:
            ptr[2] = ws_ptr
        if ptr[4] is not None:
            ptr[4] = counts_ptr
        return fn(ptr[0], ptr[1], X, Y, Z, 0., 0., 0., vs, w_min, ptr[2], bytes_, ptr[3], cap, ptr[4], None)
    for i in range(5):
        assert call(null=i) == E_NULL
    for kw in (dict(X=0), dict(Z=-1), dict(X=2 ** 16, Y=2 ** 15, Z=2, bytes_=2 ** 40), dict(cap=-1), dict(bytes_=15),
               dict(X=V + 1, Y=1, Z=1, bytes_=16)):
        assert call(**kw) == E_SHAPE, kw
    for kw in (dict(vs=0.), dict(vs=NAN), dict(vs=INF), dict(w_min=NAN)):
        assert call(**kw) == E_ARG, kw
    assert call(ws_ptr=ctypes.c_void_p(68)) == E_ALIGN and call(counts_ptr=ctypes.c_void_p(36)) == E_ALIGN
    # the order of the checks: NULL, shape, argument, alignment
    assert call(null=0, X=0, vs=0.) == E_NULL and call(X=0, vs=0.) == E_SHAPE and call(vs=0., ws_ptr=ctypes.c_void_p(68)) == E_ARG


# ---- 5. the wrappers and the stream
def test_ops_refuse_host_tensors_and_what_python_can_see():
    T, Wt, d = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4), torch.ones(5, 7)
    with pytest.raises(_lib.NrgbdError):
        ops.tsdf_integrate(T, Wt, (0, 0, 0), .05, d, np.eye(4), (30., 30., 3.5, 2.5), .15)
    with pytest.raises(_lib.NrgbdError):
        ops.tsdf_extract_points(T, Wt, (0, 0, 0), .05, 1., torch.zeros(2, dtype=torch.int64), None, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(TypeError):
        ops.tsdf_integrate(np.zeros((2, 3, 4), np.float32), Wt, (0, 0, 0), .05, d, np.eye(4), (30., 30., 3.5, 2.5), .15)
    assert ops.tsdf_extract_workspace(4, 3, 2) == 16
    with pytest.raises(_lib.NrgbdError, match="code -2"):
        ops.tsdf_extract_workspace(0, 3, 2)
    with pytest.raises(ValueError):
        fusion.TSDFVolume((4, 0, 2), .05, (0, 0, 0), device="cpu")
    with pytest.raises(ValueError):
        fusion.TSDFVolume((4, 3, 2), 0., (0, 0, 0), device="cpu")
    with pytest.raises(ValueError):
        fusion.TSDFVolume((2 ** 16, 2 ** 15, 2), .05, (0, 0, 0), device="cpu")
    vol = fusion.TSDFVolume((4, 3, 2), .05, (0, 0, 0), device="cpu")
    assert vol.device == torch.device("cpu") == vol.tsdf.device
    assert vol.trunc == pytest.approx(.15) and vol.w_max == 64. and tuple(vol.tsdf.shape) == (2, 3, 4) == tuple(vol.weight.shape)
    with pytest.raises(_lib.NrgbdError):
        vol.integrate(d, np.eye(4), (30., 30., 3.5, 2.5), cull=False)
    with pytest.raises(ValueError):
        vol.integrate(d, np.eye(4), (30., 30., 3.5, 2.5), gate=d)


def test_fusion_stream_refuses_a_dgf_model_by_name():
    import gen_dgf_golden as gg
    import neuralrgbd_amd
    cam, d_candi = gg.model_setup()
    m = gg.MODEL
    model = neuralrgbd_amd.KVNET(64, cam, d_candi, m["sigma"], 64, None, if_refined=True, refineNet_name="DGF", t_win_r=m["r"])
    vol = fusion.TSDFVolume((4, 3, 2), .05, (0, 0, 0), device="cpu")
    with pytest.raises(_lib.NrgbdError, match="FusionVideoStream: refineNet_name='DGF'"):
        fusion.FusionVideoStream(model, cam, d_candi, vol, t_win_r=m["r"])
    plain = neuralrgbd_amd.KVNET(64, cam, d_candi, m["sigma"], 64, None, if_refined=True, refineNet_name="DPV", t_win_r=m["r"])
    for kw in (dict(source="raw"), dict(weight="depth"), dict(conf_threshold=1.0), dict(conf_threshold=-0.1)):
        with pytest.raises(ValueError):
            fusion.FusionVideoStream(plain, cam, d_candi, vol, t_win_r=m["r"], **kw)
    for name in ("TSDFVolume", "FusionVideoStream", "fuse_sequence", "frustum_box", "intrinsics_at", "save_ply"):
        assert getattr(neuralrgbd_amd, name) is getattr(fusion, name)


def test_save_ply_round_trip(tmp_path):
    rng = np.random.RandomState(3)
    pts = np.concatenate([rng.randn(50, 3).astype(np.float32) * 3, [[0.0, -0.0, 1e-30], [np.float32(1) / 3, 1e20, -7.25]]]).astype(np.float32)
    path = str(tmp_path / "points.ply")
    assert fusion.save_ply(path, torch.from_numpy(pts)) == len(pts)
    lines = open(path).read().split("\n")
    assert lines[:3] == ["ply", "format ascii 1.0", "element vertex %d" % len(pts)] and lines[6] == "end_header"
    back = np.array([[float(x) for x in ln.split()] for ln in lines[7:7 + len(pts)]], dtype=np.float32)
    assert np.array_equal(back, pts) and lines[7 + len(pts):] == [""]
    assert fusion.save_ply(path, np.zeros((0, 3), np.float32)) == 0
