"""GPU: the TSDF kernels (csrc/tsdf.hip) against the fp32 restatement of tests/tsdf_ref.py, bit for bit.

Integration: every (family, grid, map size) of tsdf_ref.all_cases() after every view, with and without the frustum box, between guard
words, inputs untouched; sub-boxes whose x range starts and ends off the 16-byte groups; a volume that is not 16-byte aligned (the
element form at X % 4 == 0); two runs; hipGraph capture and replay.  Extraction: points, order and (found, written) against the
restatement on hand-made volumes, an empty one, one crossing, capacities around N with guard rows, a grid whose count records need
more than one pass of the scan workgroup, and the plane scene (whose points lie on the plane)."""
import numpy as np
import pytest
import torch

import tsdf_ref as ref
from neuralrgbd_amd import _lib, fusion, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.5
GUARD = 64                      # floats in front of and behind a guarded array (a multiple of 4: the array stays 16-byte aligned)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(got, want):
    return np.array_equal(_bits(got.cpu().numpy() if isinstance(got, torch.Tensor) else got), _bits(want))


class Guarded:
    """A [Z,Y,X] fp32 array of zeros between sentinel words; `shift` floats off the 16-byte grid."""

    def __init__(self, shape, shift=0, init=None):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD + 4,), SENTINEL, device=DEV)
        self.lo = GUARD + shift
        self.t = self.buf[self.lo:self.lo + self.n].view(*shape)
        if init is None:
            self.t.zero_()
        else:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init, np.float32)))

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:self.lo] == SENTINEL).all()) and bool((b[self.lo + self.n:] == SENTINEL).all())


def _dev(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def _view_inputs(view):
    return _dev(view["depth"]), _dev(view["gate"]), _dev(view["wmap"])


def _untouched(dev, host):
    return all(h is None or _same_bits(d, h) for d, h in zip(dev, host))


def _integrate_raw(T, Wt, case, view, maps, box=None):
    ops.tsdf_integrate(T, Wt, case["origin"], case["vs"], maps[0], view["extM"], case["K"], case["trunc"], case["depth_range"],
                       case["w_max"], gate=maps[1], gate_thr=view["gate_thr"] or 0.0, wmap=maps[2], box=box)


# ---- 1. integration ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", ref.GRIDS, ids=str)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_integrate_equals_the_restatement_after_every_view(family, dims):
    X, Y, Z = dims
    for size in ref.SIZES:
        case = ref.make_case(family, dims, size)
        want = ref.fused(family, dims, size)
        vol = fusion.TSDFVolume(dims, case["vs"], case["origin"], trunc=case["trunc"], w_max=case["w_max"], device=DEV)      # cull=True
        cT, cW = Guarded((Z, Y, X)), Guarded((Z, Y, X))
        vol.tsdf, vol.weight = cT.t, cW.t                                                                                 # between guard words too
        gT, gW = Guarded((Z, Y, X)), Guarded((Z, Y, X))                                                                   # the whole grid
        launched = 0
        for i, view in enumerate(case["views"]):
            maps = _view_inputs(view)
            launched += bool(vol.integrate(maps[0], view["extM"], case["K"], gate=maps[1], gate_thr=view["gate_thr"], weight=maps[2],
                                           depth_range=case["depth_range"], cull=True))
            _integrate_raw(gT.t, gW.t, case, view, maps)
            what = "%s %s %s view %d" % (family, dims, size, i)
            assert _same_bits(gT.t, want[i][0]) and _same_bits(gW.t, want[i][1]), what
            assert _same_bits(vol.tsdf, want[i][0]) and _same_bits(vol.weight, want[i][1]), what + " (cull)"
            assert _untouched(maps, (view["depth"], view["gate"], view["wmap"])), what
        assert gT.intact() and gW.intact() and cT.intact() and cW.intact()
        if family == "behind":
            assert launched == 0 and not vol.weight.any()


BOXES = {(48, 40, 36): [(1, 0, 0, 48, 40, 36), (2, 3, 1, 47, 39, 35), (3, 0, 0, 5, 40, 36), (21, 18, 10, 22, 22, 30), (7, 0, 0, 8, 40, 36),
                        (22, 19, 15, 27, 21, 25), (9, 20, 18, 43, 21, 24)],
         (64, 3, 2): [(1, 0, 0, 63, 3, 2), (3, 1, 1, 62, 2, 2), (7, 0, 0, 13, 3, 2)],
         (67, 5, 3): [(1, 1, 0, 66, 4, 3)]}


@pytest.mark.parametrize("dims", sorted(BOXES), ids=str)
def test_sub_boxes_off_the_16_byte_groups(dims):
    X, Y, Z = dims
    family = "front" if dims == ref.PLANE_GRID else "edge"
    case = ref.make_case(family, dims, ref.PLANE_SIZE)
    hits = 0
    for i in (0, 1):
        view = case["views"][i]
        maps = _view_inputs(view)
        start = ref.fused(family, dims, ref.PLANE_SIZE)[0] if i else (np.zeros((Z, Y, X), np.float32),) * 2
        for box in BOXES[dims]:
            obs = ref.observe(np.float32, case, i, box=box)
            wT, wW = ref.integrate(np.float32, start[0], start[1], obs, case["w_max"])
            hits += bool(obs["ok"].any())
            gT, gW = Guarded((Z, Y, X), init=start[0]), Guarded((Z, Y, X), init=start[1])
            _integrate_raw(gT.t, gW.t, case, view, maps, box=box)
            assert _same_bits(gT.t, wT) and _same_bits(gW.t, wW), (dims, box)
            assert gT.intact() and gW.intact()
    assert hits >= len(BOXES[dims])                                 # most boxes hold voxels that are updated
    with pytest.raises(_lib.NrgbdError, match="code -2"):
        _integrate_raw(gT.t, gW.t, case, view, maps, box=(0, 0, 0, X + 1, Y, Z))
    with pytest.raises(_lib.NrgbdError, match="code -4"):
        ops.tsdf_integrate(gT.t, gW.t, case["origin"], 0.0, maps[0], view["extM"], case["K"], case["trunc"])
    with pytest.raises(TypeError):
        ops.tsdf_integrate(gT.t.double(), gW.t, case["origin"], case["vs"], maps[0], view["extM"], case["K"], case["trunc"])
    with pytest.raises(ValueError):
        ops.tsdf_integrate(gT.t, gW.t, case["origin"], case["vs"], maps[0][:, :-1], view["extM"], case["K"], case["trunc"])
    torch.cuda.synchronize()
    assert _same_bits(gT.t, wT) and _same_bits(gW.t, wW)            # the refused calls wrote nothing


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_unaligned_volume_takes_the_element_form(shift):
    dims = (64, 3, 2)
    X, Y, Z = dims
    case, want = ref.make_case("edge", dims, ref.PLANE_SIZE), ref.fused("edge", dims, ref.PLANE_SIZE)
    gT, gW = Guarded((Z, Y, X), shift), Guarded((Z, Y, X), shift if shift != 2 else 0)      # shift 2: only one of the two is off the grid
    for i, view in enumerate(case["views"]):
        _integrate_raw(gT.t, gW.t, case, view, _view_inputs(view))
        assert _same_bits(gT.t, want[i][0]) and _same_bits(gW.t, want[i][1])
    assert gT.intact() and gW.intact() and want[-1][1].any()


def _run_plane(clean):
    case = ref.make_case("front", ref.PLANE_GRID, ref.PLANE_SIZE, clean)
    vol = fusion.TSDFVolume(case["dims"], case["vs"], case["origin"], trunc=case["trunc"], w_max=case["w_max"], device=DEV)
    for view in case["views"]:
        maps = _view_inputs(view)
        vol.integrate(maps[0], view["extM"], case["K"], gate=maps[1], gate_thr=view["gate_thr"], weight=maps[2], depth_range=case["depth_range"])
    return case, vol


def test_two_runs_are_bit_identical_and_reset_empties_the_volume():
    _, a = _run_plane(False)
    _, b = _run_plane(False)
    assert torch.equal(a.tsdf.view(torch.int32), b.tsdf.view(torch.int32)) and torch.equal(a.weight.view(torch.int32), b.weight.view(torch.int32))
    assert a.weight.any()
    a.reset()
    assert not a.weight.any() and not a.tsdf.any()


def test_graph_capture_and_two_replays_equal_two_eager_calls():
    from neuralrgbd_amd.distributed import graph_capture_mode
    dims = ref.PLANE_GRID
    X, Y, Z = dims
    case = ref.make_case("front", dims, ref.PLANE_SIZE)
    view = case["views"][1]                                         # gate and weight map
    maps = _view_inputs(view)
    eT, eW = torch.zeros(Z, Y, X, device=DEV), torch.zeros(Z, Y, X, device=DEV)
    for _ in range(2):
        _integrate_raw(eT, eW, case, view, maps)
    gT, gW = torch.zeros(Z, Y, X, device=DEV), torch.zeros(Z, Y, X, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=graph_capture_mode()):
        _integrate_raw(gT, gW, case, view, maps)
    assert not gW.any()                                             # a capture executes nothing
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gT.view(torch.int32), eT.view(torch.int32)) and torch.equal(gW.view(torch.int32), eW.view(torch.int32))
    assert eW.any() and float(eW.max()) <= case["w_max"]


# ---- 2. extraction ----------------------------------------------------------------------------------------------------------------

PAD_ROWS = 8


def _extract(T, Wt, origin, vs, w_min, capacity):
    """-> (rows written [written,3] numpy, found, written); checks the guard rows behind the written ones."""
    Z, Y, X = T.shape
    tT = T if isinstance(T, torch.Tensor) else _dev(np.ascontiguousarray(T, np.float32))
    tW = Wt if isinstance(Wt, torch.Tensor) else _dev(np.ascontiguousarray(Wt, np.float32))
    ws = torch.empty(ops.tsdf_extract_workspace(X, Y, Z) // 8, dtype=torch.int64, device=DEV)
    buf = torch.full((capacity + PAD_ROWS, 3), SENTINEL, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    ops.tsdf_extract_points(tT, tW, origin, vs, w_min, ws, buf[:capacity] if capacity else None, counts)
    found, written = (int(v) for v in counts.cpu())
    rows = buf.cpu().numpy()
    assert (rows[written:] == SENTINEL).all(), "a row behind the %d written ones was touched (capacity %d)" % (written, capacity)
    return rows[:written], found, written


def _check_extract(T, Wt, origin, vs, w_min, capacities=None):
    want = ref.extract(np.float32, T, Wt, origin, vs, w_min)
    N = len(want)
    for cap in (capacities if capacities is not None else sorted({0, max(N - 1, 0), N, N + 1})):
        got, found, written = _extract(T, Wt, origin, vs, w_min, cap)
        assert (found, written) == (N, min(N, cap)), (found, written, N, cap)
        assert np.array_equal(_bits(got), _bits(want[:written])), "points or their order differ (capacity %d of %d)" % (cap, N)
    return want


T_VALUES = np.array([0.0, -0.0, 1.0, -1.0, np.nan, 0.5, -0.5, 0.99999994, -0.99999994, 0.25, -0.125, 1e-30, -1e-30, 2.0,
                     1e-40, -3e-41, 1e-45, -1e-45], np.float32)                       # the last four are subnormal
W_VALUES = np.array([0.0, 0.5, 0.99999994, 1.0, 2.0, 64.0, np.nan, np.inf], np.float32)


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (3, 5, 2), (4, 3, 3), (5, 4, 3), (67, 5, 3), (33, 32, 2)], ids=str)
def test_extract_on_hand_made_volumes(dims):
    X, Y, Z = dims
    total = 0
    for seed in range(4):
        rng = np.random.RandomState(50 + seed)
        T = rng.choice(T_VALUES, size=(Z, Y, X))
        Wt = rng.choice(W_VALUES, size=(Z, Y, X), p=[.05, .05, .05, .4, .2, .15, .05, .05])
        total += len(_check_extract(T, Wt, (0.3, -1.7, 2.0), 0.05, 1.0))
    if min(dims) > 1:
        assert total > 10
        # the last index of every axis takes part as `a` along the other two axes and never looks beyond the grid
        T = np.full((Z, Y, X), 0.5, np.float32)
        T[-1, -1, -1] = -0.5
        want = _check_extract(T, np.ones_like(T), (0.0, 0.0, 0.0), 1.0, 1.0)
        assert len(want) == 3 and np.array_equal(want, [[X - 1.5, Y - 1, Z - 1], [X - 1, Y - 1.5, Z - 1], [X - 1, Y - 1, Z - 1.5]][::-1])


def test_extract_empty_volume_one_crossing_and_signed_zero():
    Z, Y, X = 3, 4, 5
    zero = np.zeros((Z, Y, X), np.float32)
    for Wt in (zero, np.ones_like(zero)):                           # a fresh volume; T = 0 everywhere with weight: no sign change
        got, found, written = _extract(zero, Wt, (0, 0, 0), 0.05, 1.0, 4)
        assert (found, written, len(got)) == (0, 0, 0)
    T = np.full((Z, Y, X), 0.5, np.float32)
    T[1, 2, 3], T[1, 2, 4] = 0.25, -0.75
    Wt = np.zeros_like(T)
    Wt[1, 2, 3] = Wt[1, 2, 4] = 1.0                                 # every other neighbour is below w_min
    want = _check_extract(T, Wt, (1.0, 2.0, 3.0), 0.5, 1.0)
    assert np.array_equal(want, [[1.0 + 0.5 * 3.25, 3.0, 3.5]])
    # T = 0 counts as positive, -0.0 too: (T < 0) is false for both
    T = np.array([[[0.0, -0.5, -0.0, -0.5, 0.0, 0.0, -0.0]]], np.float32)
    want = _check_extract(T, np.ones_like(T), (0.0, 0.0, 0.0), 1.0, 1.0)
    assert np.array_equal(want[:, 0], [0.0, 2.0, 2.0, 4.0])
    # subnormal values on either side and a subnormal quotient: the kernel's division keeps denormals, as numpy's does
    sub = np.float32(1e-40)
    T = np.array([[[sub, -sub, 3 * sub, -0.5, sub, -1e-45, 1e-45]]], np.float32)
    want = _check_extract(T, np.ones_like(T), (0.0, 0.0, 0.0), 1.0, 1.0)
    assert len(want) == 6 and want[0, 0] == 0.5 and want[1, 0] == 1.25 and want[5, 0] == 5.5
    got, _, _ = _extract(np.array([[[sub, -0.5]]], np.float32), np.ones((1, 1, 2), np.float32), (0.0, 0.0, 0.0), 1.0, 1.0, 1)
    assert got[0, 0] == sub / (sub + np.float32(0.5)) and 0 < got[0, 0] < 1.2e-38       # the point's x is itself subnormal
    # sub-w_min weights on either side, |T| = 1 on either side, NaN
    for a, b, wa, wb in ((0.5, -0.5, 0.5, 1.0), (0.5, -0.5, 1.0, 0.5), (1.0, -0.5, 1, 1), (0.5, -1.0, 1, 1), (np.nan, -0.5, 1, 1),
                         (0.5, -0.5, np.nan, 1)):
        got, found, _ = _extract(np.array([[[a, b]]], np.float32), np.array([[[wa, wb]]], np.float32), (0, 0, 0), 1.0, 1.0, 2)
        assert found == 0, (a, b, wa, wb)


def test_extract_with_more_count_records_than_one_scan_pass():
    V, PASS = _lib.TSDF_EXTRACT_VOXELS, _lib.TSDF_SCAN_PASS
    X = Y = 128
    Z = PASS * V // (X * Y) + 1                                     # the first Z whose records exceed one pass of the scan workgroup
    records = -(-X * Y * Z // V)
    assert records > PASS and records % PASS != 0 and (X * Y * (Z - 1)) // V <= PASS
    rng = np.random.RandomState(11)
    T = np.full((Z, Y, X), 0.5, np.float32)
    T.reshape(-1)[rng.choice(T.size, T.size // 500, replace=False)] = -0.5
    iz, iy, ix = np.meshgrid(np.arange(2), np.arange(Y), np.arange(X), indexing="ij")
    T[:2] = np.where((ix + iy + iz) % 2 == 0, 0.25, -0.75)          # workgroups in which every voxel has its three crossings
    T[-1, -1, -4:] = [-0.5, 0.5, -0.5, 0.5]                         # crossings in the last, partial pass
    Wt = np.ones_like(T)
    Wt.reshape(-1)[rng.choice(T.size, T.size // 100, replace=False)] = 0.5
    N = len(ref.extract(np.float32, T, Wt, (-3.2, -3.2, 0.1), 0.05, 1.0))
    assert N > 3 * V
    _check_extract(T, Wt, (-3.2, -3.2, 0.1), 0.05, 1.0, capacities=(N, N - 1, 2 * V + 1))


def test_plane_scene_points_lie_on_the_plane():
    case, vol = _run_plane(True)
    want_T, want_W = ref.fused("front", ref.PLANE_GRID, ref.PLANE_SIZE, "float32", True)[-1]
    assert _same_bits(vol.tsdf, want_T) and _same_bits(vol.weight, want_W)
    want = ref.extract(np.float32, want_T, want_W, case["origin"], case["vs"], 1.0)
    pts, found = vol.points(w_min=1.0)
    assert found == len(want) == len(pts) > 1000 and np.array_equal(_bits(pts.cpu().numpy()), _bits(want))
    dist = ref.plane_distance(pts.cpu().numpy(), case["vs"])
    print("[tsdf] plane scene on the GPU: %d points, worst distance %.3f voxel" % (found, dist.max()))
    assert dist.max() <= 0.25
    few, found2 = vol.points(w_min=1.0, capacity=100)
    assert found2 == found and torch.equal(few, pts[:100])
    more, _ = vol.points(w_min=1.0, capacity=found + 5)
    assert torch.equal(more, pts)
    none, found3 = vol.points(w_min=7.0)                            # six views: no voxel has that weight
    assert found3 == 0 and tuple(none.shape) == (0, 3)
    _check_extract(vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), case["origin"], case["vs"], 2.0)
