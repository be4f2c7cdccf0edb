"""Host-side checks of the TSDF ray cast (csrc/tsdf_raycast.hip): the restatement of tests/tsdf_raycast_ref.py in fp32 against float64
and against closed forms, the mutants each gate has to catch, the conditions on the inputs of tests/test_gpu_tsdf_raycast.py (no hit
flips between fp32 and float64 on any of them), the C entry (declared, bound, exported, every refusal without a GPU and in the
documented order) and the refusals of the Python surface.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tsdf_raycast_ref as rc
import tsdf_ref as ref
from conftest import ROOT
from neuralrgbd_amd import _lib, fusion, ops, synth

PLANE_VIEWS = ((48, 64), (7, 9), (17, 33))
RANGE = (0.3, 3.0)
GATE_VOXELS = 0.25              # the gate tsdf_ref's surface points use
N_FREE, OFFSET_FREE = -ref.PLANE_N, -ref.PLANE_OFFSET         # the plane with its normal towards the cameras (free space: n . x > offset)


def _held_out_poses():
    rng = np.random.RandomState(rc.HELD_OUT)
    return [synth.random_pose(rng, 0.08, 0.15) for _ in range(3)]


def _agreement(a, b):
    """(hit / miss flips, hits at different samples, the pixels that hit at the same sample) of an fp32 and a float64 cast."""
    both = a["hit"] & b["hit"]
    same = both & (a["k"] == b["k"])
    return int((a["hit"] != b["hit"]).sum()), int((both & ~same).sum()), same


def _inside_bound(a, b, same, slack=0.0):
    d = np.abs(a["depth"].astype(np.float64) - b["depth"])
    return bool((d[same] <= b["bound"][same] + slack).all()), float(d[same].max()) if same.any() else 0.0


# ---- 1. the plane scene
@pytest.mark.parametrize("pose", range(3))
def test_plane_scene_fp32_against_float64_and_the_closed_form(pose):
    """Measured over the 9 pose / size cases: 0 flips, 0 hits at different samples, max |d32 - d64| 4.1e-7 m against a bound whose
    median is 2e-5 to 7e-5 m (smallest 1.9e-5; it grows without limit where Tp - T is small), max |d64 - plane| 0.050 voxel (mean 0.007),
    2,356 to 3,018 hits of 3,072 pixels at 48 x 64."""
    case = ref.make_case("front", ref.PLANE_GRID, ref.PLANE_SIZE, True)
    vol = ref.fused("front", ref.PLANE_GRID, ref.PLANE_SIZE, "float32", True)[-1]
    m = _held_out_poses()[pose]
    for size in PLANE_VIEWS:
        view = {"size": size, "extM": m, "K": rc.render_K(*size), "depth_range": RANGE, "w_min": 1.0, "step": None}
        a, b = rc.cast(np.float32, case, vol, view), rc.cast(np.float64, case, vol, view, bound=True)
        flips, moved, same = _agreement(a, b)
        hits = int(b["hit"].sum())
        ok, worst = _inside_bound(a, b, same)
        plane = (np.abs(b["depth"] - ref.plane_depth(m, view["K"], *size)) / case["vs"])[b["hit"]]
        print("[raycast] pose %d %s: %d of %d hit, %d flips, %d moved, max |d32 - d64| %.2e (bound: median %.2e), plane %.3f voxel (mean %.3f)"
              % (pose, size, hits, size[0] * size[1], flips, moved, worst, np.median(b["bound"][same]), plane.max(), plane.mean()))
        assert flips == 0 and moved == 0                            # conditions on the inputs
        assert 2 * hits >= size[0] * size[1]                        # not vacuous
        assert plane.max() <= GATE_VOXELS
        assert ok and np.median(b["bound"][same]) <= 1e-4           # inside the bound, and the bound says something (2e-3 voxel)
        shaded = a["hit"] & (np.abs(a["normal"]).sum(0) > 0)
        assert shaded.sum() >= 0.9 * a["hit"].sum() and (a["normal"][2][shaded] < 0).all()      # towards the camera
        assert np.abs(np.linalg.norm(a["normal"][:, shaded].astype(np.float64), axis=0) - 1).max() <= 1e-6


# ---- 2. conditions on the inputs of the GPU tests
def _check_gpu_input(name, case, vol, view):
    a, b = rc.cast(np.float32, case, vol, view), rc.cast(np.float64, case, vol, view, bound=True)
    flips, moved, same = _agreement(a, b)
    assert flips == 0 and moved == 0, (name, view["size"], flips, moved)
    assert _inside_bound(a, b, same)[0], (name, view["size"])
    return int(a["hit"].sum())


@pytest.mark.parametrize("family", rc.RENDER_FAMILIES)
def test_no_hit_flips_between_fp32_and_float64_on_any_gpu_input(family):
    hits = 0
    for grid in rc.RENDER_GRIDS:
        case, vol, views = rc.render_views(family, grid)
        n = sum(_check_gpu_input((family, grid), case, vol, v) for v in views)
        if grid == (1, 1, 1):
            assert n == 0                                           # no cell
        hits += n
    assert hits > 100, family
    for name, fam, view in rc.special_views():
        if fam == family:
            n = _check_gpu_input(name, ref.make_case(fam, ref.PLANE_GRID, ref.PLANE_SIZE), ref.fused(fam, ref.PLANE_GRID, ref.PLANE_SIZE)[-1], view)
            assert (n == 0) == (name == "away"), name
    if family == "front":
        case, vol, views = rc.parameter_views()
        n = {name: _check_gpu_input(name, case, vol, v) for name, v in views}
        assert n["w_min=4"] == 0 and n["range=(0.3, 1.2)"] == 0 and n["range=(2.2, 3.0)"] == 0                 # above every weight; cut off
        assert 0 < n["range=(0.3, 1.55)"] < n["w_min=1"] and 0 < n["range=(1.65, 3.0)"] < n["w_min=1"]         # partly cut off
        assert 0 < n["w_min=3"] < n["w_min=1"] <= n["w_min=0.5"] and n["range=(0.0, inf)"] == n["step=vs"] == n["w_min=1"]


def test_axis_views_take_the_zero_direction_branch():
    """The identity pose with the principal point on a pixel centre: the centre column has gd_x == 0 and the centre row gd_y == 0; from
    beside the grid those rays miss by that rule alone while their neighbours hit."""
    views = {name: (fam, v) for name, fam, v in rc.special_views()}
    case, vol = ref.make_case("edge", ref.PLANE_GRID, ref.PLANE_SIZE), ref.fused("edge", ref.PLANE_GRID, ref.PLANE_SIZE)[-1]
    a = rc.cast(np.float32, case, vol, views["axis"][1])
    assert a["hit"][:, 32].sum() > 20 and a["hit"][24, :].sum() > 20
    b = rc.cast(np.float32, case, vol, views["axis_beside"][1])
    assert not b["hit"][:, 32].any() and b["hit"][:, 33:].any()
    assert (rc.camera_centre(np.float32(views["on_face"][1]["extM"][:3])) == np.float32([0, 0, 0.5])).all() and case["origin"][2] == 0.5


# ---- 3. the exact field
def _linear_case(dtype):
    case = ref.make_case("front", ref.PLANE_GRID, ref.PLANE_SIZE, True)
    return case, rc.linear_field(case["dims"], case["origin"], case["vs"], case["trunc"], N_FREE, OFFSET_FREE, dtype)


@pytest.mark.parametrize("pose", range(3))
def test_exact_field_depth_and_normals(pose):
    """Trilinear interpolation and the interpolation along the ray are exact on a linear field.  Measured: the float64 restatement
    meets the analytic depth to 8.9e-16 m and R n to 4.2e-15 on every hit of the three poses (2,540 to 3,072 of 3,072 pixels), far
    inside the 1e-9 m / 1e-6 gates; fp32 on the fp32-rounded field: 4.0e-7 m against a bound of median 2.0e-5 m."""
    case, field = _linear_case(np.float64)
    m, size = _held_out_poses()[pose], ref.PLANE_SIZE
    view = {"size": size, "extM": m, "K": rc.render_K(*size), "depth_range": RANGE, "w_min": 1.0, "step": None}
    want = rc.plane_depth64(m, view["K"], *size, N_FREE, OFFSET_FREE)
    b = rc.cast(np.float64, case, field, view)
    h = b["hit"]
    # unclamped: a corner of a cell differs from the value inside it by at most sum_a |n_a| vs / trunc
    reach = np.abs(N_FREE).sum() * case["vs"] / case["trunc"]
    assert np.maximum(np.abs(b["Tp"]), np.abs(b["T"]))[h].max() + reach < 1
    err = np.abs(b["depth"] - want)[h]
    n_cam = np.float32(m[:3, :3]).astype(np.float64) @ N_FREE
    n_err = np.abs(b["normal"] - n_cam[:, None, None]).max(0)[h]
    print("[raycast] exact field, pose %d: %d hits, depth within %.2e m, normals within %.2e" % (pose, h.sum(), err.max(), n_err.max()))
    assert 2 * h.sum() >= h.size and err.max() <= 1e-9 and n_err.max() <= 1e-6
    # fp32 on the fp32-rounded field: the corners carry an input error of at most u
    field32 = tuple(f.astype(np.float32) for f in field)
    a, b32 = rc.cast(np.float32, case, field32, view), rc.cast(np.float64, case, field32, view, bound=True, e_in=rc.U)
    flips, moved, same = _agreement(a, b32)
    assert flips == 0 and moved == 0
    assert (np.abs(a["depth"] - want)[same] <= b32["bound"][same] + 1e-9).all() and np.median(b32["bound"][same]) <= 1e-4


# ---- 4. mutants: each has to leave its gate on at least 1 % of the hit pixels
def _plane_view(pose=0):
    m, size = _held_out_poses()[pose], ref.PLANE_SIZE
    return {"size": size, "extM": m, "K": rc.render_K(*size), "depth_range": RANGE, "w_min": 1.0, "step": None}


def test_mutant_without_the_half_pixel_leaves_the_exact_field_gate():
    case, field = _linear_case(np.float64)
    view = _plane_view()
    want = rc.plane_depth64(view["extM"], view["K"], *view["size"], N_FREE, OFFSET_FREE)
    b = rc.cast(np.float64, case, field, view, mutant="half")
    assert (np.abs(b["depth"] - want)[b["hit"]] > 1e-9).mean() >= 0.01


def test_mutant_with_the_normal_reversed_leaves_the_normal_gate():
    case, field = _linear_case(np.float64)
    view = _plane_view()
    b = rc.cast(np.float64, case, field, view, mutant="normal_sign")
    n_cam = np.float32(view["extM"][:3, :3]).astype(np.float64) @ N_FREE
    assert (np.abs(b["normal"] - n_cam[:, None, None]).max(0)[b["hit"]] > 1e-6).mean() >= 0.01


def test_mutant_with_strict_crossing_runs_through_a_zero_plateau():
    """T_prev >= 0 and T < 0 in place of T_prev > 0 and T <= 0: where the field is exactly 0 over several cells the crossing is the
    first sample that reads 0 (q = 1), at most one step behind the plateau's face; the mutant runs on to its far side."""
    case = ref.make_case("front", ref.PLANE_GRID, ref.PLANE_SIZE, True)
    X, Y, Z = case["dims"]
    face, thick = 16, 4
    T = np.full((Z, Y, X), 0.5)
    T[face:face + thick + 1] = 0.0
    T[face + thick + 1:] = -0.5
    field = (T, np.ones_like(T))
    view = _plane_view()
    zs = float(np.float32(case["origin"][2])) + float(np.float32(case["vs"])) * face
    p = np.float32(view["extM"][:3]).astype(np.float64)
    fx, fy, cx, cy = view["K"]
    H, W = view["size"]
    dz = p[0, 2] * ((np.arange(W) + .5 - cx) / fx)[None, :] + p[1, 2] * ((np.arange(H) + .5 - cy) / fy)[:, None] + p[2, 2]
    cz = float(rc.camera_centre(p)[2])
    for mutant, leaves in ((None, False), ("strict", True)):
        b = rc.cast(np.float64, case, field, view, mutant=mutant)
        z_hit = (cz + b["depth"] * dz)[b["hit"]]
        outside = (z_hit < zs - 1e-9) | (z_hit > zs + case["vs"])
        assert b["hit"].sum() > 1000 and ((outside.mean() >= 0.01) if leaves else not outside.any()), mutant


def test_mutant_with_the_lerps_in_another_order_changes_bits_on_a_sphere():
    """z, then y, then x is the same interpolant with other roundings: what tells them apart is the bit comparison of the GPU test.
    The bracketing values differ on most hits; the fp32 depth, where z_prev absorbs most of it, still on more than 1 %."""
    case = ref.make_case("front", ref.PLANE_GRID, ref.PLANE_SIZE, True)
    field = rc.sphere_field(case["dims"], case["origin"], case["vs"], case["trunc"], (0.0, 0.0, 1.8), 0.5)
    view = _plane_view()
    for dtype in (np.float64, np.float32):
        a, b = rc.cast(dtype, case, field, view), rc.cast(dtype, case, field, view, mutant="zyx")
        h = a["hit"]
        assert h.sum() > 500 and np.array_equal(h, b["hit"])
        assert ((a["T"] != b["T"]) | (a["Tp"] != b["Tp"]))[h].mean() >= 0.5
        if dtype is np.float32:
            assert (a["depth"] != b["depth"])[h].mean() >= 0.01
        assert np.abs(a["depth"].astype(np.float64) - b["depth"])[h].max() <= 1e-6          # and nothing else differs


def test_mutant_with_one_corner_deciding_validity_sees_through_holes():
    """Validity from corner (0,0,0) alone interpolates with unobserved corners (T = 0, W = 0) at the rim of every hole of the volume
    fused from the seeded maps: hits where there are none, and other depths."""
    case = ref.make_case("front", ref.PLANE_GRID, ref.PLANE_SIZE)
    vol = ref.fused("front", ref.PLANE_GRID, ref.PLANE_SIZE)[-1]
    view = _plane_view()
    a, b = rc.cast(np.float64, case, vol, view), rc.cast(np.float64, case, vol, view, mutant="one_corner")
    differ = (a["hit"] != b["hit"]) | (a["depth"] != b["depth"])
    assert a["hit"].sum() > 1000 and differ.sum() >= 0.01 * a["hit"].sum()


# ---- 5. the C entry
E_NULL, E_SHAPE, E_ARG = -1, -2, -4
P = ctypes.c_void_p(64)                     # never dereferenced: every call below is refused before anything touches the device
NAN, INF = float("nan"), float("inf")
NARGS = 24


def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nrgbd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint nrgbd_tsdf_raycast_f32\((.*?)\);", code, flags=re.S).group(1)
    assert decl.count(",") + 1 == len(_lib.SIGNATURES["nrgbd_tsdf_raycast_f32"][1]) == NARGS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "nrgbd_tsdf_raycast_f32")
    assert re.search(r"nrgbd_tsdf_raycast_f32 — no counterpart in the reference", header)
    assert "nrgbd_tsdf_raycast_f32" in header[:header.index("#define NRGBD_INTERFACE_VERSION")]          # named in the list at the top
    assert header.count('#define NRGBD_INTERFACE_VERSION "0.10"') == 1
    for name in ("MAX_STEPS", "TILE", "MAX_SIDE"):
        assert getattr(_lib, "TSDF_RAYCAST_" + name) == int(re.search(r"#define NRGBD_TSDF_RAYCAST_%s (\d+)" % name, header).group(1))
    assert _lib.TSDF_RAYCAST_MAX_STEPS == rc.MAX_STEPS == 65536 and ops.TSDF_RAYCAST_TILE == 16


def test_entry_refuses_bad_arguments_without_a_gpu():
    fn = _lib.load().nrgbd_tsdf_raycast_f32
    eye = np.eye(4, dtype=np.float32)[:3].reshape(-1)

    def call(null=None, X=8, Y=6, Z=4, H=5, W=7, vs=.05, fx=30., fy=30., d_near=0., d_far=INF, w_min=1., step=.05, pose=eye,
             centre=(0., 0., 0.), normal=P):
        cp, cc = (ctypes.c_float * 12)(*pose), (ctypes.c_float * 3)(*centre)
        ptr = [None if i == null else p for i, p in enumerate((P, P, ctypes.cast(cp, ctypes.c_void_p), ctypes.cast(cc, ctypes.c_void_p), P))]
        return fn(ptr[0], ptr[1], X, Y, Z, 0., 0., 0., vs, ptr[2], ptr[3], fx, fy, 3.5, 2.5, H, W, d_near, d_far, w_min, step, ptr[4], normal, None)
    for i in range(5):                                              # tsdf, weight, pose, centre, depth
        assert call(null=i) == E_NULL
    for kw in (dict(X=0), dict(Y=-1), dict(Z=0), dict(H=0), dict(W=-3), dict(X=2 ** 16, Y=2 ** 15, Z=2), dict(X=2 ** 31 - 1, Y=2, Z=1),
               dict(X=2 ** 16, Y=2 ** 16, Z=2 ** 16), dict(H=16385), dict(W=16385)):
        assert call(**kw) == E_SHAPE, kw
    bad = lambda i, v: tuple(v if j == i else x for j, x in enumerate(eye))
    for kw in (dict(vs=0.), dict(vs=-1.), dict(vs=NAN), dict(vs=INF), dict(step=0.), dict(step=-.1), dict(step=NAN), dict(step=INF),
               dict(fx=0.), dict(fx=NAN), dict(fx=INF), dict(fy=-1.), dict(fy=NAN), dict(fy=INF), dict(d_near=1., d_far=1.),
               dict(d_near=2., d_far=1.), dict(d_near=NAN), dict(d_far=NAN), dict(w_min=NAN), dict(pose=bad(0, NAN)), dict(pose=bad(7, INF)),
               dict(pose=bad(11, -INF)), dict(centre=(0., NAN, 0.)), dict(centre=(INF, 0., 0.))):
        assert call(**kw) == E_ARG, kw
    # the order of the checks: NULL, then shape, then argument
    assert call(null=4, X=0, vs=0.) == E_NULL and call(X=0, vs=0.) == E_SHAPE and call(H=16385, pose=bad(3, NAN)) == E_SHAPE
    assert call(X=2 ** 16, Y=2 ** 15, Z=1, step=0.) == E_ARG and call(H=16384, W=16384, fx=0.) == E_ARG      # the largest grid and map
    assert call(normal=None, w_min=NAN) == E_ARG                    # normal may be NULL


# ---- 6. the Python surface
def test_python_surface_refusals():
    import neuralrgbd_amd
    T, Wt = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4)
    K = (30., 30., 3.5, 2.5)
    with pytest.raises(_lib.NrgbdError):
        ops.tsdf_raycast(T, Wt, (0, 0, 0), .05, np.eye(4), K, (5, 7), (0., 3.))
    with pytest.raises(TypeError):
        ops.tsdf_raycast(np.zeros((2, 3, 4), np.float32), Wt, (0, 0, 0), .05, np.eye(4), K, (5, 7), (0., 3.))
    vol = fusion.TSDFVolume((4, 3, 2), .05, (0, 0, 0), device="cpu")
    with pytest.raises(_lib.NrgbdError):
        vol.raycast(np.eye(4), K, (5, 7))
    with pytest.raises(_lib.NrgbdError):
        vol.raycast(np.eye(4), {"hfov": 60., "vfov": 45.}, (5, 7), step=vol.trunc)          # trunc itself is a step
    for kw in (dict(step=1.0001 * vol.trunc), dict(step=0.), dict(step=NAN)):
        with pytest.raises(ValueError, match="step"):
            vol.raycast(np.eye(4), K, (5, 7), **kw)
    nan_pose = np.eye(4)
    nan_pose[1, 3] = NAN
    for m in (nan_pose, np.full((4, 4), INF)):
        with pytest.raises(ValueError, match="not finite"):
            vol.raycast(m, K, (5, 7))
    with pytest.raises(ValueError):
        vol.raycast(np.eye(3), K, (5, 7))
    assert neuralrgbd_amd.shade is fusion.shade
    assert (ops.camera_centre(ref.look_at(synth.rotvec_to_R([0.3, -0.2, 0.1]), (0.25, -1.5, 2.0))) == np.float32([0.25, -1.5, 2.0])).all()
    m = _held_out_poses()[0]
    assert np.array_equal(ops.camera_centre(m), rc.camera_centre(np.float32(m[:3])))


def test_render_before_any_frame_needs_a_pose():
    import gen_dgf_golden as gg
    import neuralrgbd_amd
    cam, d_candi = gg.model_setup()
    mdl = gg.MODEL
    model = neuralrgbd_amd.KVNET(64, cam, d_candi, mdl["sigma"], 64, None, if_refined=True, refineNet_name="DPV", t_win_r=mdl["r"])
    vol = fusion.TSDFVolume((4, 3, 2), .05, (0, 0, 0), device="cpu")
    fs = fusion.FusionVideoStream(model, cam, d_candi, vol, t_win_r=mdl["r"], device="cpu")
    assert fs.last_ext is None
    with pytest.raises(ValueError, match="no frame has been integrated"):
        fs.render()
    with pytest.raises(_lib.NrgbdError):                            # with a pose it reaches the kernel's wrapper, which refuses host tensors
        fs.render(extM=np.eye(4))
    with pytest.raises(ValueError, match="not finite"):
        fs.render(extM=np.full((4, 4), NAN))


def test_shade():
    n = np.zeros((3, 2, 3), np.float32)
    n[2] = [[-1.0, -0.5, 0.0], [0.5, -2.0, -0.25]]
    want = np.array([[255, 128, 0], [0, 255, 64]], np.uint8)
    assert np.array_equal(fusion.shade(n), want) and fusion.shade(n).dtype == np.uint8
    t = fusion.shade(torch.from_numpy(n))
    assert t.dtype == torch.uint8 and np.array_equal(t.numpy(), want)
