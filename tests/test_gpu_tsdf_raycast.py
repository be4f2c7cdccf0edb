"""GPU: the TSDF ray cast (csrc/tsdf_raycast.hip) against the fp32 restatement of tests/tsdf_raycast_ref.py, bit for bit.

Volumes: tsdf_ref.fused(family, grid, PLANE_SIZE)[-1] with their seeded NaN / inf maps (holes) for four families and five grids — no
cell, one cell thick, odd sizes, the plane grid; views on and around the 16 x 16 / 8 x 8 tiles from integration and held-out poses;
a camera inside, outside, looking away, along an axis (gd == 0), beside the grid, on a face; weight thresholds, depth ranges, steps and
the step cap; with and without normals; guard words, outputs off the 16-byte grid, inputs untouched, two runs, hipGraph capture and
replay, out= without an allocation; the round trip integrate -> ray cast on the plane scene and the exact linear field.  The
conditions on these inputs (no hit flips between fp32 and float64) are checked on the host by tests/test_tsdf_raycast_host.py."""
import numpy as np
import pytest
import torch

import tsdf_raycast_ref as rc
import tsdf_ref as ref
from neuralrgbd_amd import _lib, fusion, ops
from test_gpu_tsdf import DEV, Guarded, _bits, _dev, _run_plane, _same_bits

pytestmark = pytest.mark.gpu
FILL = 7.5                      # what the outputs hold before a call: every element is written


def _volume(vol):
    return tuple(_dev(np.ascontiguousarray(a, np.float32)) for a in vol)


def _cast(case, dvol, view, normals=True, shift=0):
    """-> (depth, normal or None) as Guarded arrays, `shift` floats off the 16-byte grid."""
    H, W = view["size"]
    d = Guarded((H, W), shift, init=np.full((H, W), FILL, np.float32))
    n = Guarded((3, H, W), shift, init=np.full((3, H, W), FILL, np.float32)) if normals else None
    got = ops.tsdf_raycast(dvol[0], dvol[1], case["origin"], case["vs"], view["extM"], view["K"], view["size"], view["depth_range"],
                           w_min=view["w_min"], step=view["step"], normals=normals, out=(d.t, n.t) if normals else d.t)
    assert (got[0] if normals else got) is d.t
    return d, n


def _check(case, vol, dvol, view, what, shift=0):
    """Both forms of a view against the restatement; returns the restatement's record."""
    want = rc.cast(np.float32, case, vol, view)
    d, n = _cast(case, dvol, view, True, shift)
    d2, _ = _cast(case, dvol, view, False, (shift + 1) % 4)
    assert _same_bits(d.t, want["depth"]), "%s: depth differs on %d pixels" % (what, (_bits(d.t.cpu().numpy()) != _bits(want["depth"])).sum())
    assert _same_bits(n.t, want["normal"]), "%s: normals differ" % (what,)
    assert _same_bits(d2.t, want["depth"]), "%s: depth without normals differs" % (what,)
    assert d.intact() and n.intact() and d2.intact(), what
    assert _same_bits(dvol[0], vol[0]) and _same_bits(dvol[1], vol[1]), "%s: the volume was written" % (what,)
    return want


# ---- 1. every family, grid and view size
@pytest.mark.parametrize("grid", rc.RENDER_GRIDS, ids=str)
@pytest.mark.parametrize("family", rc.RENDER_FAMILIES)
def test_raycast_equals_the_restatement(family, grid):
    case, vol, views = rc.render_views(family, grid)
    dvol = _volume(vol)
    hits = 0
    for j, view in enumerate(views):
        want = _check(case, vol, dvol, view, "%s %s %s" % (family, grid, view["size"]), shift=j % 4)
        hits += int(want["hit"].sum())
    if grid == (1, 1, 1):
        assert hits == 0
    if grid == ref.PLANE_GRID and family != "side":
        assert hits > 300, (family, hits)


# ---- 2. poses
@pytest.mark.parametrize("name", [v[0] for v in rc.special_views()])
def test_special_poses(name):
    family, view = {v[0]: v[1:] for v in rc.special_views()}[name]
    case, vol = ref.make_case(family, ref.PLANE_GRID, ref.PLANE_SIZE), ref.fused(family, ref.PLANE_GRID, ref.PLANE_SIZE)[-1]
    want = _check(case, vol, _volume(vol), view, name)
    if name == "away":
        assert not want["hit"].any() and not want["depth"].any() and not want["normal"].any()      # zeros were written everywhere
    else:
        assert want["hit"].sum() > 100
    if name == "axis_beside":
        assert not want["hit"][:, 32].any() and want["hit"][:, 33:].any()


# ---- 3. parameters
def test_weight_thresholds_depth_ranges_and_steps():
    case, vol, views = rc.parameter_views()
    dvol = _volume(vol)
    hits = {name: int(_check(case, vol, dvol, view, name)["hit"].sum()) for name, view in views}
    assert hits["w_min=4"] == 0 and hits["range=(0.3, 1.2)"] == 0 and 0 < hits["w_min=3"] < hits["w_min=1"]
    assert 0 < hits["range=(0.3, 1.55)"] < hits["step=vs"] and 0 < hits["range=(1.65, 3.0)"] < hits["step=vs"]


def test_a_ray_that_reaches_the_step_cap_misses():
    grid = (5, 4, 3)
    case, vol, views = rc.render_views("front", grid)
    view = views[2]                                                 # 16 x 16, an integration pose
    usual = rc.cast(np.float32, case, vol, view)
    tiny = dict(view, step=1e-7)                                    # 65536 steps cover 6.6 mm of a path of centimetres
    want = _check(case, vol, _volume(vol), tiny, "step cap")
    assert usual["hit"].sum() > 0 and want["capped"] > 0 and want["hit"].sum() < usual["hit"].sum()


# ---- 4. the standard checks on one view
def _plane_inputs():
    case, vol, views = rc.parameter_views()
    return case, vol, _volume(vol), dict(views)["w_min=1"]


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_outputs_off_the_16_byte_grid(shift):
    case, vol, dvol, view = _plane_inputs()
    _check(case, vol, dvol, view, "shift %d" % shift, shift=shift)


def test_two_runs_are_bit_identical_and_out_allocates_nothing():
    case, vol, dvol, view = _plane_inputs()
    H, W = view["size"]
    args = (dvol[0], dvol[1], case["origin"], case["vs"], view["extM"], view["K"], view["size"], view["depth_range"])
    a = ops.tsdf_raycast(*args, normals=True)
    b = ops.tsdf_raycast(*args, normals=True)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert tuple(a[0].shape) == (H, W) and tuple(a[1].shape) == (3, H, W) and a[0].any()
    out = (torch.empty_like(a[0]), torch.empty_like(a[1]))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    got = ops.tsdf_raycast(*args, normals=True, out=out)
    only_depth = ops.tsdf_raycast(*args, out=out[0])
    assert torch.cuda.memory_allocated() == before
    assert got[0] is out[0] and got[1] is out[1] and only_depth is out[0] and torch.equal(out[0].view(torch.int32), a[0].view(torch.int32))
    with pytest.raises(ValueError):
        ops.tsdf_raycast(*args, out=out[0][:, :-1])
    with pytest.raises(ValueError):
        ops.tsdf_raycast(*args, normals=True, out=(out[0], out[1][:2]))
    with pytest.raises(_lib.NrgbdError, match="code -4"):
        ops.tsdf_raycast(*args, step=0.0)
    with pytest.raises(ValueError):
        ops.tsdf_raycast(*args[:6], (0, 4), view["depth_range"])
    torch.cuda.synchronize()
    assert torch.equal(out[0].view(torch.int32), a[0].view(torch.int32))                  # the refused calls wrote nothing


def test_graph_capture_and_replay_equals_eager():
    from neuralrgbd_amd.distributed import graph_capture_mode
    case, vol, dvol, view = _plane_inputs()
    args = (dvol[0], dvol[1], case["origin"], case["vs"], view["extM"], view["K"], view["size"], view["depth_range"])
    eager = ops.tsdf_raycast(*args, normals=True)
    out = (torch.full_like(eager[0], FILL), torch.full_like(eager[1], FILL))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=graph_capture_mode()):
        ops.tsdf_raycast(*args, normals=True, out=out)
    assert bool((out[0] == FILL).all())                             # a capture executes nothing
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0].view(torch.int32), eager[0].view(torch.int32)) and torch.equal(out[1].view(torch.int32), eager[1].view(torch.int32))


# ---- 5. the round trip and the exact field
def test_round_trip_integrate_then_raycast_on_the_plane_scene():
    case, dev_vol = _run_plane(True)
    vol = ref.fused("front", ref.PLANE_GRID, ref.PLANE_SIZE, "float32", True)[-1]
    assert _same_bits(dev_vol.tsdf, vol[0]) and _same_bits(dev_vol.weight, vol[1])
    size = ref.PLANE_SIZE
    view = {"size": size, "extM": rc.held_out(case["views"][0]["extM"]), "K": rc.render_K(*size), "depth_range": (0.3, 3.0), "w_min": 1.0,
            "step": None}
    want = rc.cast(np.float32, case, vol, view)
    depth, normal = dev_vol.raycast(view["extM"], view["K"], size, depth_range=view["depth_range"], normals=True)
    assert _same_bits(depth, want["depth"]) and _same_bits(normal, want["normal"])
    hit = want["hit"]
    off = (np.abs(depth.cpu().numpy().astype(np.float64) - ref.plane_depth(view["extM"], view["K"], *size)) / case["vs"])[hit]
    print("[raycast] round trip on the GPU: %d of %d pixels hit, worst distance to the plane %.3f voxel" % (hit.sum(), hit.size, off.max()))
    assert 2 * hit.sum() >= hit.size and off.max() <= 0.25
    # the dict form of the intrinsics and the default step
    again = dev_vol.raycast(view["extM"], {"hfov": 2 * np.degrees(np.arctan(size[1] / 2 / view["K"][0])),
                                           "vfov": 2 * np.degrees(np.arctan(size[0] / 2 / view["K"][1]))}, size, depth_range=view["depth_range"])
    assert (again != 0).sum() >= 0.9 * hit.sum()
    shaded = fusion.shade(normal)
    assert shaded.dtype == torch.uint8 and tuple(shaded.shape) == size and bool((shaded[torch.from_numpy(hit).to(DEV)] > 0).float().mean() > 0.9)


def test_exact_field_depth_inside_the_derived_bound():
    case = ref.make_case("front", ref.PLANE_GRID, ref.PLANE_SIZE, True)
    n, offset = -ref.PLANE_N, -ref.PLANE_OFFSET
    field = tuple(f.astype(np.float32) for f in rc.linear_field(case["dims"], case["origin"], case["vs"], case["trunc"], n, offset))
    size = ref.PLANE_SIZE
    view = {"size": size, "extM": rc.held_out(case["views"][0]["extM"]), "K": rc.render_K(*size), "depth_range": (0.3, 3.0), "w_min": 1.0,
            "step": None}
    want = _check(case, field, _volume(field), view, "exact field")
    b = rc.cast(np.float64, case, field, view, bound=True, e_in=rc.U)       # the corners carry the rounding of the field to fp32
    same = want["hit"] & b["hit"] & (want["k"] == b["k"])
    assert np.array_equal(want["hit"], b["hit"]) and same.sum() == want["hit"].sum() and 2 * same.sum() >= same.size
    err = np.abs(want["depth"].astype(np.float64) - rc.plane_depth64(view["extM"], view["K"], *size, n, offset))
    print("[raycast] exact field on the GPU: %d hits, max |depth - analytic| %.2e m (bound: median %.2e)"
          % (same.sum(), err[same].max(), np.median(b["bound"][same])))
    assert (err[same] <= b["bound"][same] + 1e-9).all() and np.median(b["bound"][same]) <= 1e-4
    n_cam = np.float32(view["extM"][:3, :3]).astype(np.float64) @ n
    # a gradient component carries at most ~10 u (two rounded corners, the difference, three lerps) against |g| = vs / trunc = 1 / 3:
    # 1.8e-6 relative, three components and the rotation on top: under 1e-5
    assert np.abs(want["normal"][:, same] - n_cam[:, None]).max() <= 1e-5
