"""GPU: the TSDF mesh extraction (csrc/tsdf_mesh.hip) against the numpy restatement tests/tsdf_mesh_ref.py: vertices bit for bit,
faces equal, counts, guard rows behind both outputs, and in every case the vertices against ops.tsdf_extract_points on the same volume.
Hand-made volumes (special values, X off the groups of four, partial last workgroups, cells across workgroups) at capacities around the
counts, dense sign fields with a checkerboard slab, grids whose count records need more than one pass of the scan workgroup, the fused
plane scene through TSDFVolume.mesh, two runs, hipGraph capture and replay."""
import numpy as np
import pytest
import torch

import tsdf_mesh_ref as mref
import tsdf_ref as ref
from neuralrgbd_amd import _lib, fusion, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.5
FACE_SENTINEL = -77
PAD_ROWS = 8

T_VALUES = np.array([0.0, -0.0, 1.0, -1.0, np.nan, 0.5, -0.5, 0.99999994, -0.99999994, 0.25, -0.125, 1e-30, -1e-30, 2.0,
                     1e-40, -3e-41, 1e-45, -1e-45], np.float32)                       # the last four are subnormal
T_BAD = np.isnan(T_VALUES) | (np.abs(T_VALUES) >= 1)                                  # 1, -1, NaN, 2: a corner that fails
T_P = np.where(T_BAD, 0.02, 0.92 / (~T_BAD).sum())
W_VALUES = np.array([0.0, 0.5, 0.99999994, 1.0, 2.0, 64.0, np.nan, np.inf], np.float32)
W_P = [.02, .02, .02, .5, .2, .2, .02, .02]
ORIGIN, VS = (0.3, -1.7, 2.0), 0.05


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _mesh(tT, tW, origin, vs, w_min, vcap, fcap):
    """-> (vertex rows written, face rows written, counts); checks the guard rows behind both."""
    Z, Y, X = tT.shape
    ws = torch.empty(ops.tsdf_mesh_workspace(X, Y, Z) // 8 + 1, dtype=torch.int64, device=DEV)
    vbuf = torch.full((vcap + PAD_ROWS, 3), SENTINEL, device=DEV)
    fbuf = torch.full((fcap + PAD_ROWS, 3), FACE_SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    ops.tsdf_extract_mesh(tT, tW, origin, vs, w_min, ws, vbuf[:vcap] if vcap else None, fbuf[:fcap] if fcap else None, counts)
    c = tuple(int(v) for v in counts.cpu())
    v, f = vbuf.cpu().numpy(), fbuf.cpu().numpy()
    assert (v[c[1]:] == SENTINEL).all(), "a vertex row behind the %d written ones was touched (capacity %d)" % (c[1], vcap)
    assert (f[c[3]:] == FACE_SENTINEL).all(), "a face row behind the %d written ones was touched (capacity %d)" % (c[3], fcap)
    return v[:c[1]], f[:c[3]], c


def _points(tT, tW, origin, vs, w_min, capacity):
    Z, Y, X = tT.shape
    ws = torch.empty(ops.tsdf_extract_workspace(X, Y, Z) // 8, dtype=torch.int64, device=DEV)
    out = torch.empty((max(capacity, 1), 3), device=DEV)
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    ops.tsdf_extract_points(tT, tW, origin, vs, w_min, ws, out[:capacity] if capacity else None, counts)
    assert int(counts[0]) == capacity
    return out[:capacity].cpu().numpy()


def _check_mesh(T, Wt, origin=ORIGIN, vs=VS, w_min=1.0, capacities=None):
    want_v, want_f = mref.mesh(T, Wt, origin, vs, w_min)
    N, M = len(want_v), len(want_f)
    tT, tW = _dev(T), _dev(Wt)
    assert np.array_equal(_bits(_points(tT, tW, origin, vs, w_min, N)), _bits(want_v))
    if capacities is None:
        capacities = [(a, b) for a in sorted({0, max(N - 1, 0), N, N + 1}) for b in sorted({0, max(M - 1, 0), M, M + 1})]
    for vcap, fcap in capacities:
        v, f, c = _mesh(tT, tW, origin, vs, w_min, vcap, fcap)
        assert c == (N, min(N, vcap), M, min(M, fcap)), (c, N, M, vcap, fcap)
        assert np.array_equal(_bits(v), _bits(want_v[:c[1]])), "vertices or their order differ (capacity %d of %d)" % (vcap, N)
        assert np.array_equal(f, want_f[:c[3]]), "faces or their order differ (capacities %d, %d of %d, %d)" % (vcap, fcap, N, M)
    return want_v, want_f


# ---- 1. hand-made volumes
@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 2, 2), (3, 5, 2), (5, 4, 3), (67, 5, 3), (33, 32, 2), (37, 29, 5)], ids=str)
def test_mesh_on_hand_made_volumes(dims):
    X, Y, Z = dims
    faces = 0
    for seed in range(4):
        rng = np.random.RandomState(70 + seed)
        T = rng.choice(T_VALUES, size=(Z, Y, X), p=T_P)
        Wt = rng.choice(W_VALUES, size=(Z, Y, X), p=W_P)
        faces += len(_check_mesh(T, Wt)[1])
    if X * Y * Z > 100:
        assert faces > 50
    if min(dims) > 1:
        # the last cell: its triangle's vertices are the crossings of three different voxels of the last rows and slices
        T = np.full((Z, Y, X), 0.5, np.float32)
        T[-1, -1, -1] = -0.5
        v, f = _check_mesh(T, np.ones_like(T), (0.0, 0.0, 0.0), 1.0, 1.0)
        assert len(v) == 3 and len(f) == 1 and sorted(f[0]) == [0, 1, 2]
        n = mref.normals(v, f)[0][0]
        assert (n < 0).all()                                        # away from the inside corner at the far end
    else:
        assert faces == 0


def test_exact_zeros_special_values_and_w_min():
    T = np.full((2, 2, 2), -0.5, np.float32)
    T[0, 0, 0] = 0.0
    v, f = _check_mesh(T, np.ones_like(T), (1.0, 2.0, 3.0), 0.5, 1.0)
    assert len(f) == 1 and np.array_equal(v, [[1.0, 2.0, 3.0]] * 3)             # coincident vertices, the triangle is kept
    rng = np.random.RandomState(5)
    T = rng.uniform(-0.99, 0.99, size=(4, 6, 9)).astype(np.float32)
    Wt = rng.choice([1.0, 2.0, 3.0], size=T.shape).astype(np.float32)
    counts = [len(_check_mesh(T, Wt, w_min=w, capacities=[(10 ** 4, 10 ** 4)])[1]) for w in (1.0, 2.0, 3.0, 4.0)]
    assert counts[0] > counts[1] > counts[2] >= counts[3] == 0                      # a higher w_min only removes cells
    for bad in (np.nan, 1.0, -1.0):                                                 # one bad corner in the middle
        T1 = T.copy()
        T1[2, 3, 4] = bad
        _check_mesh(T1, np.ones_like(T1))


# ---- 2. dense sign fields
def test_dense_random_signs_and_a_checkerboard_slab():
    X, Y, Z = 21, 18, 10
    rng = np.random.RandomState(9)
    T = (rng.uniform(0.05, 0.95, size=(Z, Y, X)) * rng.choice([-1.0, 1.0], size=(Z, Y, X))).astype(np.float32)
    iz, iy, ix = np.meshgrid(np.arange(3), np.arange(Y), np.arange(X), indexing="ij")
    T[4:7] = np.where((ix + iy + iz) % 2 == 0, 0.25, -0.75)                        # cases 0x69 / 0x96: four triangles, every edge a vertex
    Wt = np.ones_like(T)
    v, f = _check_mesh(T, Wt)
    cells = (X - 1) * (Y - 1) * (Z - 1)
    assert len(f) > 2 * cells                                                       # most cells emit
    case = mref.cell_cases(T, Wt, 1.0)
    assert set(np.unique(case[4:6])) == {0x69, 0x96} and (mref.COUNT[[0x69, 0x96]] == 4).all()
    # all the outer lattice points outside: a closed manifold, every vertex referenced
    T[0] = T[-1] = T[:, 0] = T[:, -1] = T[:, :, 0] = T[:, :, -1] = 0.5
    v, f = _check_mesh(T, Wt, capacities=[(10 ** 5, 10 ** 5)])
    assert mref.closed_manifold(f) and np.array_equal(np.unique(f), np.arange(len(v)))


# ---- 3. more count records than one pass of the scan workgroup
@pytest.mark.parametrize("extra", [1, 2])
def test_mesh_with_more_count_records_than_one_scan_pass(extra):
    """Z = PASS V / 128^2 + 1 is the first grid whose records exceed one pass; its last, partial pass holds the last slice alone, whose
    voxels own crossings but no cells (iz + 1 < Z fails), so that pass scans vertex counts and zero triangle counts.  With one more
    slice the partial pass owns cells: triangles in the first and in the last partial pass."""
    V, PASS = _lib.TSDF_EXTRACT_VOXELS, _lib.TSDF_SCAN_PASS
    X = Y = 128
    Z = PASS * V // (X * Y) + extra
    records = -(-X * Y * Z // V)
    assert records > PASS and records % PASS != 0 and (X * Y * (Z - extra)) // V <= PASS
    rng = np.random.RandomState(11)
    T = np.full((Z, Y, X), 0.5, np.float32)
    T.reshape(-1)[rng.choice(T.size, T.size // 500, replace=False)] = -0.5
    iz, iy, ix = np.meshgrid(np.arange(2), np.arange(Y), np.arange(X), indexing="ij")
    T[:2] = np.where((ix + iy + iz) % 2 == 0, 0.25, -0.75)          # workgroups in which every cell has four triangles
    T[-1, -1, -4:] = [-0.5, 0.5, -0.5, 0.5]                         # crossings in the last records
    T[-2:, 40:44, 50:54] = -0.5                                     # and cells around them
    Wt = np.ones_like(T)
    Wt.reshape(-1)[rng.choice(T.size, T.size // 100, replace=False)] = 0.5
    origin = (-3.2, -3.2, 0.1)
    want_v, want_f = mref.mesh(T, Wt, origin, VS, 1.0)
    N, M = len(want_v), len(want_f)
    assert N > 3 * V and M > 4 * V
    case = mref.cell_cases(T, Wt, 1.0)
    per_cell = np.where(case > 0, mref.COUNT[np.maximum(case, 0)], 0)
    in_last = int(per_cell[PASS * V // (X * Y):].sum())             # the slices whose voxels lie in the records of the last pass
    assert (in_last > 0) == (extra == 2)
    _check_mesh(T, Wt, origin, VS, 1.0, capacities=[(N, M), (N - 1, M - 1), (2 * V + 1, 3 * V + 1)])


# ---- 4. the fused plane scene through TSDFVolume.mesh
def _run_plane():
    case = ref.make_case("front", ref.PLANE_GRID, ref.PLANE_SIZE, True)
    vol = fusion.TSDFVolume(case["dims"], case["vs"], case["origin"], trunc=case["trunc"], w_max=case["w_max"], device=DEV)
    for view in case["views"]:
        vol.integrate(torch.from_numpy(view["depth"]).to(DEV), view["extM"], case["K"], depth_range=case["depth_range"])
    return case, vol


def test_plane_scene_mesh():
    case, vol = _run_plane()
    want_T, want_W = ref.fused("front", ref.PLANE_GRID, ref.PLANE_SIZE, "float32", True)[-1]
    assert np.array_equal(_bits(vol.tsdf.cpu().numpy()), _bits(want_T)) and np.array_equal(_bits(vol.weight.cpu().numpy()), _bits(want_W))
    want_v, want_f = mref.mesh(want_T, want_W, case["origin"], case["vs"], 1.0)
    v, f, (nv, nf) = vol.mesh(w_min=1.0)
    assert f.dtype == torch.int32 and v.dtype == torch.float32
    assert (nv, nf) == (len(want_v), len(want_f)) == (len(v), len(f)) and nf > 1000
    assert np.array_equal(_bits(v.cpu().numpy()), _bits(want_v)) and np.array_equal(f.cpu().numpy(), want_f)
    pts, found = vol.points(w_min=1.0)
    assert found == nv and torch.equal(pts.view(torch.int32), v.view(torch.int32))
    n, _ = mref.normals(want_v, want_f)
    cos = -(n @ ref.PLANE_N) / np.maximum(np.linalg.norm(n, axis=1), 1e-300)      # free space is the camera's side: -PLANE_N
    print("[tsdf mesh] plane scene on the GPU: %d vertices, %d triangles, worst cosine to the free-space normal %.3f" % (nv, nf, cos.min()))
    assert (cos > 0).all()
    fv, ff, found2 = vol.mesh(w_min=1.0, capacity=(100, 50))
    assert found2 == (nv, nf) and torch.equal(fv, v[:100]) and torch.equal(ff, f[:50])
    mv, mf, _ = vol.mesh(w_min=1.0, capacity=(nv + 5, nf + 5))
    assert torch.equal(mv, v) and torch.equal(mf, f)
    ev, ef, found3 = vol.mesh(w_min=7.0)                            # six views: no voxel has that weight
    assert found3 == (0, 0) and tuple(ev.shape) == (0, 3) == tuple(ef.shape)
    _check_mesh(want_T, want_W, case["origin"], case["vs"], 2.0, capacities=[(nv, nf)])


# ---- 5. determinism and capture
def test_two_runs_and_graph_replays_give_the_same_bits():
    from neuralrgbd_amd.distributed import graph_capture_mode
    rng = np.random.RandomState(21)
    X, Y, Z = 37, 29, 5
    T = rng.uniform(-0.99, 0.99, size=(Z, Y, X)).astype(np.float32)
    Wt = rng.choice([0.5, 1.0, 2.0], size=T.shape, p=[.05, .5, .45]).astype(np.float32)
    want_v, want_f = mref.mesh(T, Wt, ORIGIN, VS, 1.0)
    N, M = len(want_v), len(want_f)
    tT, tW = _dev(T), _dev(Wt)
    a, b = _mesh(tT, tW, ORIGIN, VS, 1.0, N, M), _mesh(tT, tW, ORIGIN, VS, 1.0, N, M)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2] == (N, N, M, M) and M > 1000
    ws = torch.empty(ops.tsdf_mesh_workspace(X, Y, Z) // 8 + 1, dtype=torch.int64, device=DEV)
    vbuf = torch.full((N + PAD_ROWS, 3), SENTINEL, device=DEV)
    fbuf = torch.full((M + PAD_ROWS, 3), FACE_SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=graph_capture_mode()):
        ops.tsdf_extract_mesh(tT, tW, ORIGIN, VS, 1.0, ws, vbuf[:N], fbuf[:M], counts)
    assert int(counts[0]) == -7 and bool((fbuf == FACE_SENTINEL).all())             # a capture executes nothing
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert tuple(int(c) for c in counts.cpu()) == (N, N, M, M)
        assert np.array_equal(_bits(vbuf[:N].cpu().numpy()), _bits(a[0])) and np.array_equal(fbuf[:M].cpu().numpy(), a[1])
        assert bool((vbuf[N:] == SENTINEL).all()) and bool((fbuf[M:] == FACE_SENTINEL).all())
        vbuf[:N].fill_(SENTINEL)
        fbuf[:M].fill_(FACE_SENTINEL)
        counts.fill_(-7)
