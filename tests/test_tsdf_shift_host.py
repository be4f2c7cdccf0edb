"""Host-side checks of the moving TSDF volume (csrc/tsdf_shift.hip, fusion.TSDFVolume.shift, fusion.follow_shift): the triangle
partition the one-voxel rim is there for, on the fused volumes of tests/tsdf_ref.py; the mutants of the rule each gate has to catch,
with the numpy restatement standing in for the device; composition of two shifts; the window equivalence — a small volume that follows
the camera holds, bit for bit, what a static volume over the same views holds in its window, and hands out what that one holds outside;
follow_shift; the origin after many shifts; the C entry (declared, bound, exported, every refusal without a GPU and in the documented
order).  No GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import tsdf_mesh_ref as mref
import tsdf_ref as ref
import tsdf_shift_ref as sr
from conftest import ROOT
from neuralrgbd_amd import _lib, fusion, ops

E_NULL, E_SHAPE, E_ARG = -1, -2, -4
NAME = "nrgbd_tsdf_shift_f32"
W_MIN = 0.5


def _same_bits(a, b):
    return np.array_equal(sr.bits(a), sr.bits(b))


# ---- 1. the partition
@pytest.mark.parametrize("family", sr.PARTITION_FAMILIES)
def test_spill_and_live_meshes_partition_the_old_mesh(family):
    old, origin, vs = sr.fused_planes(family, ref.PLANE_GRID)
    total = 0
    for s in sr.SHIFTS:
        n = sr.partition(old, origin, vs, s, W_MIN)
        print("[shift] %s %s: triangles old %d = spill %d + live %d" % (family, s, n["old"], n["spill"], n["live"]))
        assert n["old"] == n["spill"] + n["live"] and n["subset"], (family, s)
        dst = sr.shift(old, s)[0]
        direct = sr.window(old, s)
        assert _same_bits(dst, direct)
        want = mref.mesh(direct[0], direct[1], sr.new_origin(origin, vs, s), vs, W_MIN)
        assert _same_bits(n["meshes"][2][0], want[0]) and np.array_equal(n["meshes"][2][1], want[1])
        if s == (0, 0, 0):
            assert n["spill"] == 0 and n["live"] == n["old"]
        if s in ((48, 0, 0), (47, 0, 0)):
            assert n["live"] == 0 and n["spill"] == n["old"]        # one retained column (or none) holds no cell
        total += n["old"]
    assert total > 0, "the fixture has a surface"


@pytest.mark.parametrize("dims", [(67, 5, 3), (5, 4, 3)])
@pytest.mark.parametrize("family", sr.PARTITION_FAMILIES)
def test_partition_on_the_small_grids(family, dims):
    old, origin, vs = sr.fused_planes(family, dims)
    for s in ((4, 0, 0), (-8, 0, 0), (0, 2, 0), (0, 0, -1), (3, -1, 1), (-1, -1, -1), (1, 0, 0), (dims[0] - 1, 0, 0), (dims[0], 0, 0), (0, 0, 0)):
        n = sr.partition(old, origin, vs, s, W_MIN)
        assert n["ok"], (family, dims, s, n["old"], n["spill"], n["live"])


# ---- 2. the mutants: each is caught by the partition or by the bit gates (the restatement stands in for the device)
# (a dst buffer that keeps its garbage — NaNs — has no weight there either: the partition is blind to it, like to the colour planes;
# and a shift by -s is a shift too — its spill and live parts partition the old mesh just as well: the bit gates alone again)
PARTITION_CATCHES = {"rim_dropped", "rim_two_thick", "rim_wrong_face"}


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_every_mutant_is_caught(mutant):
    old, origin, vs = sr.fused_planes("front", ref.PLANE_GRID)
    colour = np.concatenate([old, sr.pattern(3, ref.PLANE_GRID, 9)])            # a colour volume: the fused planes and three more
    shifts = [s for s in sr.SHIFTS if s != (0, 0, 0)]
    by_partition = sum(not sr.partition(old, origin, vs, s, W_MIN, mutant)["ok"] for s in shifts)
    by_bits = 0
    for s in shifts:
        want, got = sr.shift(colour, s, spill=True), sr.shift(colour, s, spill=True, mutant=mutant)
        by_bits += not (_same_bits(want[0], got[0]) and _same_bits(want[1], got[1]))
    print("[shift] mutant %s: caught by the partition on %d, by the bit gates on %d of %d shifts" % (mutant, by_partition, by_bits, len(shifts)))
    assert by_bits > 0
    assert (by_partition > 0) == (mutant in PARTITION_CATCHES)      # the colour planes take no part in a mesh: the bit gates alone


# ---- 3. composition
@pytest.mark.parametrize("a,b", [((4, 0, 0), (8, 0, 0)), ((3, -2, 1), (-5, 1, 1)), ((-8, 0, 0), (8, 0, 0)), ((1, 1, 1), (0, 0, 0)),
                                 ((40, 0, 0), (10, 0, 0))])
def test_two_shifts_compose_where_both_sources_stayed_inside(a, b):
    src = sr.pattern(5, (48, 10, 9), 3)
    ab = tuple(x + y for x, y in zip(a, b))
    two = sr.shift(sr.shift(src, a)[0], b)[0]
    one = sr.shift(src, ab)[0]
    Z, Y, X = src.shape[1:]
    iz, iy, ix = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    ins = lambda s: ((ix + s[0] >= 0) & (ix + s[0] < X) & (iy + s[1] >= 0) & (iy + s[1] < Y) & (iz + s[2] >= 0) & (iz + s[2] < Z))
    both = ins(b) & ins(ab)
    assert _same_bits(two[:, both], one[:, both])
    assert not sr.bits(two[:, ~ins(b)]).any()                       # what passed outside in between came back empty
    assert both.any() or max(abs(v) for v in ab) >= 48


# ---- 4. the window equivalence
def test_a_window_that_follows_the_camera_equals_the_static_volume():
    sc = sr.window_scenario()
    X, Y, Z = sr.WINDOW_DIMS
    static = np.zeros((2,) + sr.STATIC_DIMS[::-1], np.float32)
    live = np.zeros((2, Z, Y, X), np.float32)
    off, spills, touched = 0, [], 0
    for extM, depth, at in sc["views"]:
        if at != off:
            assert at - off == sr.WINDOW_STEP
            live, spill = sr.shift(live, (at - off, 0, 0), spill=True)
            spills.append((off, spill))
            off = at
        origin = sr.new_origin(sr.WINDOW_ORIGIN, sr.VS, (off, 0, 0))
        box = sr.unclipped_box(extM, origin, sr.WINDOW_DIMS)        # the condition: the view touches nothing outside the window
        assert min(box[:3]) >= 0 and all(b <= n for b, n in zip(box[3:], sr.WINDOW_DIMS)), (box, off)
        obs = sr.window_observe(sr.WINDOW_DIMS, origin, extM, depth)
        touched += int(obs["ok"].sum())
        live = np.stack(ref.integrate(np.float32, live[0], live[1], obs, 64.0))
        static = np.stack(ref.integrate(np.float32, static[0], static[1], sr.window_observe(sr.STATIC_DIMS, sr.WINDOW_ORIGIN, extM, depth), 64.0))
    print("[shift] window: %d voxel updates over %d views, %d voxels with weight in the last window" % (touched, len(sc["views"]), (live[1] > 0).sum()))
    assert len(spills) == 8 and touched > 50 * len(sc["views"])
    for at, spill in spills:                                        # what left is what the static volume still holds there
        assert _same_bits(spill[:, :, :, :sr.WINDOW_STEP], static[:, :, :, at:at + sr.WINDOW_STEP])
        assert (spill[1, :, :, :sr.WINDOW_STEP] > 0).any()
    assert _same_bits(live, static[:, :, :, off:off + X]) and (live[1] > 0).sum() > 100


# ---- 5. follow_shift
def _vol(dims=(64, 48, 32), origin=(-3.2, -2.4, 0.0), vs=0.1):
    return types.SimpleNamespace(dims=dims, origin=origin, voxel_size=vs)


def _camera_at(centre, R=np.eye(3)):
    return ref.look_at(R, centre)


def test_follow_shift_hand_cases():
    vol = _vol()
    # the grid's centre is at lattice (31.5, 23.5, 15.5) = world (-0.05, -0.05, 1.55); the camera looks along +z, focus 1.55 m ahead
    centre = np.array([-0.05, -0.05, 0.0])
    f = lambda d, **kw: fusion.follow_shift(_camera_at(centre + np.asarray(d, float)), vol, 1.55, **kw)
    assert f((0, 0, 0)) == (0, 0, 0)
    assert f((1.5, 0, 0)) == (0, 0, 0) and f((-1.5, 0, 0)) == (0, 0, 0)             # 15 voxels: inside the margin of 16
    assert f((1.7, 0, 0)) == (16, 0, 0) and f((-1.7, 0, 0)) == (-16, 0, 0)          # 17 voxels: past it, the nearest multiple of 8
    assert f((2.1, 0, 0)) == (24, 0, 0) and f((3.0, 0, 0)) == (32, 0, 0)
    assert f((0, 1.3, 0)) == (0, 16, 0) and f((0, -1.3, 0)) == (0, -16, 0) and f((0, 1.1, 0)) == (0, 0, 0)        # margin 12
    assert f((0, 0, 0.9)) == (0, 0, 8) and f((0, 0, -0.9)) == (0, 0, -8) and f((0, 0, 0.7)) == (0, 0, 0)          # margin 8
    assert f((1.7, -1.3, 2.1)) == (16, -16, 24)
    assert f((1.7, 0, 0), step=4) == (16, 0, 0) and f((2.0, 0, 0), step=12) == (24, 0, 0) and f((1.7, 0, 0), step=12) == (12, 0, 0)
    assert f((0.8, 0, 0), margin=0.1) == (8, 0, 0) and f((0.6, 0, 0), margin=0.1) == (0, 0, 0)
    for s in (f((2.63, -1.91, 0.97), step=4), f((-2.63, 1.91, -0.97), step=16)):
        assert all(isinstance(v, int) for v in s)
    assert all(v % 16 == 0 for v in f((-2.63, 1.91, -0.97), step=16)) and all(v % 4 == 0 for v in f((2.63, -1.91, 0.97), step=4))
    # the optical axis, not world z: a camera that looks along +x with the focus 1.7 m ahead
    Ry = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])        # rows: the camera's axes in the world; z axis = world +x
    assert fusion.follow_shift(_camera_at(np.array([-0.05, -0.05, 1.55]), Ry), vol, 1.7) == (16, 0, 0)
    # a shifted volume is asked from where it is now
    moved = _vol(origin=(-3.2 + 1.6, -2.4, 0.0))
    assert fusion.follow_shift(_camera_at(centre + np.array([1.7, 0, 0])), moved, 1.55) == (0, 0, 0)
    # [3,4] and tensors are poses too
    assert fusion.follow_shift(torch.from_numpy(_camera_at(centre + np.array([1.7, 0, 0]))[:3]), vol, 1.55) == (16, 0, 0)


def test_follow_shift_non_finite_pose_and_refusals():
    vol = _vol()
    for bad in (float("nan"), float("inf")):
        m = np.eye(4)
        m[0, 3] = bad
        assert fusion.follow_shift(m, vol, 1.0) == (0, 0, 0)
        m = np.eye(4)
        m[1, 1] = bad
        assert fusion.follow_shift(m, vol, 1.0) == (0, 0, 0)
    assert fusion.follow_shift(np.zeros((4, 4)), vol, 1.0) == (0, 0, 0)         # singular: nothing to follow
    for kw in (dict(step=0), dict(step=-8), dict(step=6), dict(step=8.5), dict(step=True), dict(margin=0.0), dict(margin=0.5),
               dict(margin=-0.1), dict(margin=float("nan"))):
        with pytest.raises(ValueError):
            fusion.follow_shift(np.eye(4), vol, 1.0, **kw)
    for d in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            fusion.follow_shift(np.eye(4), vol, d)
    with pytest.raises(ValueError):
        fusion.follow_shift(np.eye(3), vol, 1.0)


# ---- 6. TSDFVolume.shift's bookkeeping, with the restatement in the launch's place
@pytest.fixture
def host_shift(monkeypatch):
    calls = []

    def fake(src, dst, shift, spill=False):
        d, a = sr.shift(src.numpy(), shift, spill=spill, dst_before=dst.numpy())
        dst.copy_(torch.from_numpy(d.view(np.int32)).view(torch.float32))
        src.copy_(torch.from_numpy(a.view(np.int32)).view(torch.float32))
        calls.append(tuple(shift))
    monkeypatch.setattr(ops, "tsdf_shift", fake)
    return calls


def test_origin_after_a_thousand_alternating_shifts(host_shift):
    vs, origin0 = 0.02, (-2.56, 0.1, 1.0 / 3.0)
    vol = fusion.TSDFVolume((4, 3, 3), vs, origin0, device="cpu")
    rng = np.random.RandomState(0)
    for i in range(1000):
        s = tuple(int(v) for v in rng.randint(-9, 10, 3) * (1 if i % 2 else -1))
        before = vol.offset
        assert vol.shift(s) is None
        assert vol.offset == tuple(o + v for o, v in zip(before, s))
        assert vol.origin == tuple(o + vs * k for o, k in zip(origin0, vol.offset))      # exactly, as Python floats
    assert 990 < len(host_shift) <= 1000 and (0, 0, 0) not in host_shift and vol.offset != (0, 0, 0)       # a zero shift launches nothing
    back = tuple(-o for o in vol.offset)
    vol.shift(back)
    assert vol.offset == (0, 0, 0) and vol.origin == origin0


def test_shift_swaps_the_buffers_and_a_spill_goes_stale(host_shift):
    vol = fusion.TSDFVolume((8, 5, 4), 0.5, (1.0, 2.0, 3.0), trunc=1.0, w_max=7.0, device="cpu", color=True)
    assert vol._spare is None and vol.offset == (0, 0, 0)
    assert vol.shift((0, 0, 0)) is None and vol.shift((0, 0, 0), spill=True) is None and vol._spare is None and host_shift == []
    start = sr.pattern(5, (8, 5, 4), 1)
    vol._buf.copy_(torch.from_numpy(start.view(np.int32)).view(torch.float32))
    first, tsdf_before = vol._buf, vol.tsdf
    spill = vol.shift((4, -1, 0), spill=True)
    want_dst, want_src = sr.shift(start, (4, -1, 0), spill=True)
    assert vol._buf is not first and vol._spare is first and vol.offset == (4, -1, 0) and vol.origin == (3.0, 1.5, 3.0)
    assert vol.tsdf.data_ptr() == vol._buf[0].data_ptr() and vol.weight.data_ptr() == vol._buf[1].data_ptr()
    assert vol.color.data_ptr() == vol._buf[2].data_ptr() and tuple(vol.color.shape) == (3, 4, 5, 8)
    assert _same_bits(vol._buf.numpy(), want_dst)
    assert tsdf_before.data_ptr() == spill.tsdf.data_ptr()          # a tensor fetched before the shift is the spill buffer afterwards
    assert isinstance(spill, fusion.TSDFVolume) and spill.origin == (1.0, 2.0, 3.0) and spill.dims == vol.dims
    assert (spill.voxel_size, spill.trunc, spill.w_max) == (0.5, 1.0, 7.0) and spill.color is not None and spill._buf is first
    assert _same_bits(spill._buf.numpy(), want_src)
    spill._live("points")                                           # valid until the parent's next shift
    assert vol.shift((-4, 0, 0)) is None                            # reuses the buffer: no third one
    assert vol._buf is first and vol.offset == (0, -1, 0)
    for call in (lambda: spill.points(), lambda: spill.mesh(), lambda: spill.raycast(np.eye(4), (5., 5., 3., 2.), (4, 6)),
                 lambda: spill.shift((1, 0, 0)), lambda: spill.reset()):
        with pytest.raises(ValueError, match="stale"):
            call()
    for bad in ((1, 2), (1.5, 0, 0), "abc", 3):
        with pytest.raises(ValueError):
            vol.shift(bad)


# ---- 7. the C entry
def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nrgbd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint %s\((.*?)\);" % NAME, code, flags=re.S).group(1)
    assert decl.count(",") + 1 == len(_lib.SIGNATURES[NAME][1]) == 11
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert re.search(r"%s — no counterpart in the reference" % NAME, header)
    assert NAME in header[:header.index("#define NRGBD_INTERFACE_VERSION")]               # named in the list at the top
    assert header.count('#define NRGBD_INTERFACE_VERSION "0.10"') == 1                     # no entry changed or disappeared
    assert ops.version().startswith("nrgbd_hip 0.10 ")


P, Q = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)          # non-NULL addresses: every refusal comes before anything touches the device


def test_refuses_bad_arguments_without_a_gpu():
    fn = _lib.load().nrgbd_tsdf_shift_f32

    def call(src=P, dst=Q, planes=2, X=8, Y=4, Z=2, s=(4, 0, 0), spill=0):
        return fn(src, dst, planes, X, Y, Z, s[0], s[1], s[2], spill, None)
    for kw in (dict(src=None), dict(dst=None), dict(src=None, dst=None)):
        assert call(**kw) == E_NULL, kw
    for kw in (dict(planes=0), dict(planes=1), dict(planes=3), dict(planes=4), dict(planes=6), dict(planes=-2), dict(X=0), dict(Y=-1),
               dict(Z=0), dict(X=1 << 16, Y=1 << 16, Z=1), dict(X=1 << 11, Y=1 << 11, Z=(1 << 9) + 1)):
        assert call(**kw) == E_SHAPE, kw
    n = 8 * 4 * 2 * 4                                               # bytes of one plane
    at = lambda a: ctypes.c_void_p(a)
    for kw in (dict(dst=P), dict(dst=at((1 << 20) + 4)), dict(dst=at((1 << 20) + 2 * n - 4)), dict(dst=at((1 << 20) - 2 * n + 4)),
               dict(planes=5, dst=at((1 << 20) + 5 * n - 4)), dict(dst=P, s=(0, 0, 0)), dict(dst=P, s=(1 << 30, -(1 << 31), 7), spill=1)):
        assert call(**kw) == E_ARG, kw
    # the order: NULL, shape, argument
    assert call(src=None, planes=3, dst=None) == E_NULL and call(dst=None, X=0) == E_NULL
    assert call(planes=3, dst=P) == E_SHAPE and call(X=0, dst=P) == E_SHAPE


def test_the_wrapper_checks_before_it_calls():
    """ops.tsdf_shift needs CUDA tensors: a host tensor is refused by name, with no fallback."""
    a, b = torch.zeros(2, 3, 4, 8), torch.zeros(2, 3, 4, 8)
    with pytest.raises(_lib.NrgbdError, match="src"):
        ops.tsdf_shift(a, b, (4, 0, 0))
    with pytest.raises(TypeError):
        ops.tsdf_shift(a.numpy(), b, (4, 0, 0))
