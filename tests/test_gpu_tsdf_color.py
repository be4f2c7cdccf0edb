"""GPU: the colour carried through the TSDF volume (nrgbd_tsdf_integrate_color_f32, nrgbd_tsdf_extract_points_color,
nrgbd_tsdf_extract_mesh_color) against the fp32 restatement of tests/tsdf_color_ref.py, bit for bit.

Integration: every family of tsdf_ref on six grids after every view, depth maps 7 x 9 and 48 x 64, colour images at the depth size, at
4 x it, at an unrelated size whose intrinsics push projections onto the clamp and at 1 x 1, with a NaN and an inf pixel and a non-trivial
affine, between guard words; tsdf and weight also against the colourless entry; sub-boxes off the 16-byte groups; a colour buffer off
the 16-byte grid (the element form); two runs; hipGraph capture and replay.  Extraction: the colours of the points and of the mesh's
vertices on hand-made volumes, on one with more count records than a scan pass, at capacities around the count with guard rows, and
points / vertices / faces against the colourless calls."""
import numpy as np
import pytest
import torch

import tsdf_color_ref as cref
import tsdf_ref as ref
from neuralrgbd_amd import _lib, fusion, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.5
GUARD = 64                      # floats in front of and behind a guarded array (a multiple of 4: the array stays 16-byte aligned)
GRIDS = ((1, 1, 1), (3, 5, 2), (5, 4, 3), (64, 3, 2), (67, 5, 3), (48, 40, 36))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(got, want):
    return np.array_equal(_bits(got.cpu().numpy() if isinstance(got, torch.Tensor) else got), _bits(want))


class Guarded:
    """An fp32 array of zeros (or `init`) between sentinel words; `shift` floats off the 16-byte grid."""

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
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _integrate(T, Wt, C, case, view, image, Kc, affine=cref.AFFINE, box=None):
    v = case["views"][view]
    ops.tsdf_integrate_color(T, Wt, C, case["origin"], case["vs"], _dev(v["depth"]), v["extM"], case["K"], case["trunc"], image, Kc, affine,
                             case["depth_range"], case["w_max"], gate=_dev(v["gate"]), gate_thr=v["gate_thr"] or 0.0, wmap=_dev(v["wmap"]),
                             box=box)


def _integrate_plain(T, Wt, case, view):
    v = case["views"][view]
    ops.tsdf_integrate(T, Wt, case["origin"], case["vs"], _dev(v["depth"]), v["extM"], case["K"], case["trunc"], case["depth_range"],
                       case["w_max"], gate=_dev(v["gate"]), gate_thr=v["gate_thr"] or 0.0, wmap=_dev(v["wmap"]))


# ---- 1. integration ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", GRIDS, ids=str)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_integrate_color_equals_the_restatement_after_every_view(family, dims):
    X, Y, Z = dims
    for size in cref.DEPTH_SIZES:
        case = ref.make_case(family, dims, size)
        pT, pW = torch.zeros(Z, Y, X, device=DEV), torch.zeros(Z, Y, X, device=DEV)
        plain = []
        for i in range(len(case["views"])):
            _integrate_plain(pT, pW, case, i)
            plain.append((pT.clone(), pW.clone()))
        for variant in cref.VARIANTS:
            want = cref.fused(family, dims, size, variant)
            Kc = cref.color_K(case, variant)
            gT, gW, gC = Guarded((Z, Y, X)), Guarded((Z, Y, X)), Guarded((3, Z, Y, X))
            for i in range(len(case["views"])):
                host = cref.make_image(family, dims, size, variant, i)
                image = _dev(host)
                _integrate(gT.t, gW.t, gC.t, case, i, image, Kc)
                what = "%s %s %s %s view %d" % (family, dims, size, variant, i)
                assert _same_bits(gC.t, want[i][2]), what + ": colour"
                assert _same_bits(gT.t, want[i][0]) and _same_bits(gW.t, want[i][1]), what
                assert torch.equal(gT.t.view(torch.int32), plain[i][0].view(torch.int32)), what + ": tsdf against the colourless entry"
                assert torch.equal(gW.t.view(torch.int32), plain[i][1].view(torch.int32)), what + ": weight against the colourless entry"
                assert _same_bits(image, host), what + ": the image was written"
            assert gT.intact() and gW.intact() and gC.intact()


def test_the_inputs_reach_the_clamp_the_specials_and_every_channel():
    """Not vacuous: on the plane grid the unrelated image size clamps part of the projections on either side, a voxel meets the NaN and
    the inf pixel (its colour keeps its bits while its distance is updated), and the colour volume is neither empty nor grey."""
    family, dims, size = "front", ref.PLANE_GRID, ref.PLANE_SIZE
    case = ref.make_case(family, dims, size)
    obs = cref.observe(np.float32, case, 0, cref.make_image(family, dims, size, "odd", 0), cref.color_K(case, "odd"), cref.AFFINE)
    Hc, Wc = cref.image_size("odd", size)
    uc = obs["uc"][obs["ok"]]
    assert (uc == 0).any() and (uc == Wc - 1).any() and ((uc > 0) & (uc < Wc - 1)).any()
    skipped = 0
    for variant in ("same", "x4", "odd"):
        for i in range(len(case["views"])):
            o = cref.observe(np.float32, case, i, cref.make_image(family, dims, size, variant, i), cref.color_K(case, variant), cref.AFFINE)
            skipped += int((o["ok"] & ~o["fin"]).sum())
    assert skipped > 0
    C = cref.fused(family, dims, size, "same")[-1][2]
    assert all(np.unique(C[j]).size > 100 for j in range(3)) and not np.array_equal(C[0], C[1])
    # the kernel: a voxel that met a special pixel keeps its colour bits and takes the distance update
    X, Y, Z = dims
    img = np.full((3,) + size, 0.25, np.float32)
    img[1] = np.nan
    seed = np.random.RandomState(5).rand(3, Z, Y, X).astype(np.float32)
    gT, gW, gC = Guarded((Z, Y, X)), Guarded((Z, Y, X)), Guarded((3, Z, Y, X), init=seed)
    _integrate(gT.t, gW.t, gC.t, case, 0, _dev(img), case["K"])
    assert _same_bits(gC.t, seed) and _same_bits(gW.t, ref.fused(family, dims, size)[0][1]) and bool(gW.t.any())
    assert gC.intact()


def test_the_default_affine_is_the_identity():
    family, dims, size, variant = "front", (67, 5, 3), (7, 9), "x4"
    X, Y, Z = dims
    case, want = ref.make_case(family, dims, size), cref.fused(family, dims, size, variant, "float32", False)
    gT, gW, gC = Guarded((Z, Y, X)), Guarded((Z, Y, X)), Guarded((3, Z, Y, X))
    for i in range(len(case["views"])):
        _integrate(gT.t, gW.t, gC.t, case, i, _dev(cref.make_image(family, dims, size, variant, i)), cref.color_K(case, variant), affine=None)
        assert _same_bits(gC.t, want[i][2]) and _same_bits(gT.t, want[i][0]) and _same_bits(gW.t, want[i][1])
    assert gC.intact() and want[-1][2].any() and not np.array_equal(want[-1][2], cref.fused(family, dims, size, variant)[-1][2])


BOXES = {(48, 40, 36): [(1, 0, 0, 48, 40, 36), (2, 3, 1, 47, 39, 35), (3, 0, 0, 5, 40, 36), (21, 18, 10, 22, 22, 30), (7, 0, 0, 8, 40, 36),
                        (22, 19, 15, 27, 21, 25), (9, 20, 18, 43, 21, 24)],
         (64, 3, 2): [(1, 0, 0, 63, 3, 2), (3, 1, 1, 62, 2, 2), (7, 0, 0, 13, 3, 2)],
         (67, 5, 3): [(1, 1, 0, 66, 4, 3)]}


@pytest.mark.parametrize("dims", sorted(BOXES), ids=str)
def test_sub_boxes_off_the_16_byte_groups(dims):
    X, Y, Z = dims
    family = "front" if dims == ref.PLANE_GRID else "edge"
    size, variant = ref.PLANE_SIZE, "x4"
    case = ref.make_case(family, dims, size)
    Kc = cref.color_K(case, variant)
    hits = 0
    for i in (0, 1):
        host = cref.make_image(family, dims, size, variant, i)
        image = _dev(host)
        start = cref.fused(family, dims, size, variant)[0] if i else (np.zeros((Z, Y, X), np.float32),) * 2 + (np.zeros((3, Z, Y, X), np.float32),)
        for box in BOXES[dims]:
            obs = cref.observe(np.float32, case, i, host, Kc, cref.AFFINE, box=box)
            wC = cref.integrate(np.float32, start[2], start[1], obs)
            wT, wW = ref.integrate(np.float32, start[0], start[1], obs, case["w_max"])
            hits += bool(obs["fin"].any())
            gT, gW, gC = Guarded((Z, Y, X), init=start[0]), Guarded((Z, Y, X), init=start[1]), Guarded((3, Z, Y, X), init=start[2])
            _integrate(gT.t, gW.t, gC.t, case, i, image, Kc, box=box)
            assert _same_bits(gC.t, wC) and _same_bits(gT.t, wT) and _same_bits(gW.t, wW), (dims, box)
            assert gT.intact() and gW.intact() and gC.intact()
    assert hits >= len(BOXES[dims])


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_a_colour_buffer_off_the_16_byte_grid_takes_the_element_form(shift):
    dims, size, variant = (64, 3, 2), ref.PLANE_SIZE, "same"
    X, Y, Z = dims
    case, want = ref.make_case("edge", dims, size), cref.fused("edge", dims, size, variant)
    gT, gW, gC = Guarded((Z, Y, X)), Guarded((Z, Y, X)), Guarded((3, Z, Y, X), shift)        # tsdf and weight stay on the grid
    for i in range(len(case["views"])):
        _integrate(gT.t, gW.t, gC.t, case, i, _dev(cref.make_image("edge", dims, size, variant, i)), cref.color_K(case, variant))
        assert _same_bits(gC.t, want[i][2]) and _same_bits(gT.t, want[i][0]) and _same_bits(gW.t, want[i][1])
    assert gT.intact() and gW.intact() and gC.intact() and want[-1][2].any()


def _run_plane(variant="x4"):
    family, dims, size = "front", ref.PLANE_GRID, ref.PLANE_SIZE
    case = ref.make_case(family, dims, size)
    vol = fusion.TSDFVolume(dims, case["vs"], case["origin"], trunc=case["trunc"], w_max=case["w_max"], device=DEV, color=True)
    for i, v in enumerate(case["views"]):
        vol.integrate(_dev(v["depth"]), v["extM"], case["K"], gate=_dev(v["gate"]), gate_thr=v["gate_thr"], weight=_dev(v["wmap"]),
                      depth_range=case["depth_range"], color=_dev(cref.make_image(family, dims, size, variant, i)),
                      color_intrinsics=cref.color_K(case, variant), color_affine=cref.AFFINE)
    return case, vol


def test_the_volume_object_two_runs_and_reset():
    case, a = _run_plane()
    _, b = _run_plane()
    want = cref.fused("front", ref.PLANE_GRID, ref.PLANE_SIZE, "x4")[-1]
    assert _same_bits(a.tsdf, want[0]) and _same_bits(a.weight, want[1]) and _same_bits(a.color, want[2])      # frustum culling: the same bits
    assert torch.equal(a._buf.view(torch.int32), b._buf.view(torch.int32)) and tuple(a._buf.shape) == (5,) + ref.PLANE_GRID[::-1]
    assert a.color.data_ptr() == a._buf[2].data_ptr() and bool(a.color.any())
    a.reset()
    assert not a._buf.any()
    v = case["views"][0]
    with pytest.raises(ValueError):
        a.integrate(_dev(v["depth"]), v["extM"], case["K"])
    plain = fusion.TSDFVolume((4, 4, 4), 0.05, (0, 0, 0), device=DEV)
    with pytest.raises(ValueError):
        plain.integrate(_dev(v["depth"]), v["extM"], case["K"], color=torch.zeros((3,) + ref.PLANE_SIZE, device=DEV))
    with pytest.raises(ValueError):
        plain.points(colors=True)
    torch.cuda.synchronize()
    assert not a._buf.any() and not plain._buf.any()


def test_graph_capture_and_two_replays_equal_two_eager_calls():
    from neuralrgbd_amd.distributed import graph_capture_mode
    family, dims, size, variant = "front", ref.PLANE_GRID, ref.PLANE_SIZE, "x4"
    X, Y, Z = dims
    case = ref.make_case(family, dims, size)
    image, Kc = _dev(cref.make_image(family, dims, size, variant, 1, False)), cref.color_K(case, variant)
    v = case["views"][1]
    maps = (_dev(v["depth"]), _dev(v["gate"]), _dev(v["wmap"]))

    def run(buf):
        ops.tsdf_integrate_color(buf[0], buf[1], buf[2:], case["origin"], case["vs"], maps[0], v["extM"], case["K"], case["trunc"], image, Kc,
                                 cref.AFFINE, case["depth_range"], case["w_max"], gate=maps[1], gate_thr=v["gate_thr"], wmap=maps[2])
    eager, graphed = torch.zeros(5, Z, Y, X, device=DEV), torch.zeros(5, Z, Y, X, device=DEV)
    for _ in range(2):
        run(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=graph_capture_mode()):
        run(graphed)
    assert not graphed.any()                                        # a capture executes nothing
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.view(torch.int32), eager.view(torch.int32)) and bool(eager[2:].any())


# ---- 2. extraction ----------------------------------------------------------------------------------------------------------------

PAD_ROWS = 8
T_VALUES = np.array([0.0, -0.0, 1.0, -1.0, np.nan, 0.5, -0.5, 0.99999994, -0.99999994, 0.25, -0.125, 1e-30, -1e-30, 2.0,
                     1e-40, -3e-41], np.float32)
W_VALUES = np.array([0.0, 0.5, 0.99999994, 1.0, 2.0, 64.0, np.nan, np.inf], np.float32)


def _capacities(N):
    return sorted({0, 1, max(N - 1, 0), N, N + 5})


def _check_points(T, Wt, C, origin, vs, w_min, capacities=None):
    """points_color at every capacity: colours against the restatement, points against the colourless entry, guard rows."""
    Z, Y, X = T.shape
    want_p = ref.extract(np.float32, T, Wt, origin, vs, w_min)
    want_c = cref.extract(np.float32, T, Wt, C, w_min)
    N = len(want_p)
    assert len(want_c) == N
    tT, tW, tC = _dev(T), _dev(Wt), _dev(C)
    ws = torch.empty(ops.tsdf_extract_workspace(X, Y, Z) // 8, dtype=torch.int64, device=DEV)
    for cap in (_capacities(N) if capacities is None else capacities):
        pts, cols = torch.full((cap + PAD_ROWS, 3), SENTINEL, device=DEV), torch.full((cap + PAD_ROWS, 3), SENTINEL, device=DEV)
        plain = torch.full((cap + PAD_ROWS, 3), SENTINEL, device=DEV)
        counts, counts0 = torch.full((2,), -7, dtype=torch.int64, device=DEV), torch.full((2,), -7, dtype=torch.int64, device=DEV)
        ops.tsdf_extract_points(tT, tW, origin, vs, w_min, ws, pts[:cap] if cap else None, counts, color=tC, colors=cols[:cap] if cap else None)
        ops.tsdf_extract_points(tT, tW, origin, vs, w_min, ws, plain[:cap] if cap else None, counts0)
        found, written = (int(v) for v in counts.cpu())
        assert (found, written) == (N, min(N, cap)) and torch.equal(counts, counts0), (found, written, N, cap)
        assert torch.equal(pts.view(torch.int32), plain.view(torch.int32)), "the points differ from the colourless entry's (capacity %d)" % cap
        assert np.array_equal(_bits(pts[:written].cpu().numpy()), _bits(want_p[:written]))
        rows = cols.cpu().numpy()
        assert (rows[written:] == SENTINEL).all(), "a colour row behind the %d written ones was touched (capacity %d)" % (written, cap)
        assert np.array_equal(_bits(rows[:written]), _bits(want_c[:written])), "colours differ (capacity %d of %d)" % (cap, N)
    return want_c


def _check_mesh(T, Wt, C, origin, vs, w_min):
    Z, Y, X = T.shape
    want_c = cref.extract(np.float32, T, Wt, C, w_min)
    N = len(want_c)
    tT, tW, tC = _dev(T), _dev(Wt), _dev(C)
    ws = torch.empty((ops.tsdf_mesh_workspace(X, Y, Z) + 7) // 8, dtype=torch.int64, device=DEV)
    counts, counts0 = torch.full((4,), -7, dtype=torch.int64, device=DEV), torch.full((4,), -7, dtype=torch.int64, device=DEV)
    ops.tsdf_extract_mesh(tT, tW, origin, vs, w_min, ws, None, None, counts0)
    F = int(counts0[2])
    for cap in _capacities(N):
        v, c = torch.full((cap + PAD_ROWS, 3), SENTINEL, device=DEV), torch.full((cap + PAD_ROWS, 3), SENTINEL, device=DEV)
        v0 = torch.full((cap + PAD_ROWS, 3), SENTINEL, device=DEV)
        f, f0 = torch.full((F + PAD_ROWS, 3), -9, dtype=torch.int32, device=DEV), torch.full((F + PAD_ROWS, 3), -9, dtype=torch.int32, device=DEV)
        ops.tsdf_extract_mesh(tT, tW, origin, vs, w_min, ws, v[:cap] if cap else None, f[:F] if F else None, counts, color=tC,
                              colors=c[:cap] if cap else None)
        ops.tsdf_extract_mesh(tT, tW, origin, vs, w_min, ws, v0[:cap] if cap else None, f0[:F] if F else None, counts0)
        assert torch.equal(counts, counts0) and int(counts[0]) == N and int(counts[1]) == min(N, cap) and int(counts[3]) == F
        assert torch.equal(v.view(torch.int32), v0.view(torch.int32)) and torch.equal(f, f0)
        rows = c.cpu().numpy()
        written = min(N, cap)
        assert (rows[written:] == SENTINEL).all() and np.array_equal(_bits(rows[:written]), _bits(want_c[:written])), cap
    return N, F


@pytest.mark.parametrize("dims", [(2, 1, 1), (1, 2, 1), (1, 1, 2), (4, 3, 3), (67, 5, 3), (33, 32, 2)], ids=str)
def test_extracted_colours_on_hand_made_volumes(dims):
    X, Y, Z = dims
    total = faces = 0
    for seed in range(3):
        rng = np.random.RandomState(80 + seed)
        T = rng.choice(T_VALUES, size=(Z, Y, X))
        Wt = rng.choice(W_VALUES, size=(Z, Y, X), p=[.05, .05, .05, .4, .2, .15, .05, .05])
        C = (rng.rand(3, Z, Y, X) * 2 - 0.5).astype(np.float32)
        total += len(_check_points(T, Wt, C, (0.3, -1.7, 2.0), 0.05, 1.0))
        n, f = _check_mesh(T, Wt, C, (0.3, -1.7, 2.0), 0.05, 1.0)
        faces += f
    # one crossing per axis at a known place
    T = np.full((Z, Y, X), 0.5, np.float32)
    T[0, 0, 0] = -0.25                                              # q = 1/3 towards every neighbour
    C = cref.affine_field(dims, ((1, 2, 0, 0), (0, 0, 4, 0), (3, 0, 0, -2)))
    got = _check_points(T, np.ones_like(T), C, (0.0, 0.0, 0.0), 1.0, 1.0)
    assert len(got) == sum(n > 1 for n in dims)
    if min(dims) > 1:
        assert total > 10 and len(got) == 3
    if X * Y * Z > 500:                                             # random holes leave the small grids without a valid cell
        assert faces > 0


def test_extracted_colours_with_more_count_records_than_one_scan_pass():
    V, PASS = _lib.TSDF_EXTRACT_VOXELS, _lib.TSDF_SCAN_PASS
    X = Y = 128
    Z = PASS * V // (X * Y) + 1
    assert -(-X * Y * Z // V) > PASS
    rng = np.random.RandomState(12)
    T = np.full((Z, Y, X), 0.5, np.float32)
    T.reshape(-1)[rng.choice(T.size, T.size // 500, replace=False)] = -0.5
    T[-1, -1, -4:] = [-0.5, 0.5, -0.5, 0.5]                         # crossings in the last, partial pass
    Wt = np.ones_like(T)
    C = rng.rand(3, Z, Y, X).astype(np.float32)
    N = len(ref.extract(np.float32, T, Wt, (-3.2, -3.2, 0.1), 0.05, 1.0))
    assert N > 3 * V
    _check_points(T, Wt, C, (-3.2, -3.2, 0.1), 0.05, 1.0, capacities=(N, N - 1, 2 * V + 1))


def test_volume_points_and_mesh_return_the_colours():
    case, vol = _run_plane()
    want = cref.fused("front", ref.PLANE_GRID, ref.PLANE_SIZE, "x4")[-1]
    want_c = cref.extract(np.float32, want[0], want[1], want[2], 1.0)
    pts0, found0 = vol.points()
    pts, cols, found = vol.points(colors=True)
    assert found == found0 == len(want_c) > 100 and torch.equal(pts, pts0) and _same_bits(cols, want_c)
    v0, f0, n0 = vol.mesh()
    v, f, c, n = vol.mesh(colors=True)
    assert n == n0 and torch.equal(v, v0) and torch.equal(f, f0) and torch.equal(v, pts) and _same_bits(c, want_c) and len(f) > 100
    few, cfew, _ = vol.points(capacity=10, colors=True)
    assert torch.equal(few, pts[:10]) and torch.equal(cfew.view(torch.int32), cols[:10].view(torch.int32))
    v5, f5, c5, _ = vol.mesh(capacity=(found + 5, 7), colors=True)
    assert torch.equal(c5.view(torch.int32), cols.view(torch.int32)) and torch.equal(f5, f[:7])
