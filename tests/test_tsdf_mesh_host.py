"""Host-side checks of the TSDF mesh extraction: the case table (tools/gen_mc_table.py against the committed header and against the
rule's properties, restated here independently of the generator's own helpers), the numpy restatement tests/tsdf_mesh_ref.py on
random sign fields (closed manifold), a sphere (Euler characteristic 2, outward winding), invalid corners, exact zeros and
degenerate grids, fusion.save_ply, and the two C entries (declared, bound, exported, every refusal without a GPU, in a fixed order).
No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tsdf_mesh_ref as mref
import tsdf_ref as ref
from conftest import ROOT
from neuralrgbd_amd import _lib, fusion, ops

gen = mref.gen
ENTRIES = {"nrgbd_tsdf_mesh_workspace": 3, "nrgbd_tsdf_extract_mesh": 18}


# ---- 1. the table -----------------------------------------------------------------------------------------------------------------
def _edge_ends(e):
    """The two corners of edge e as coordinates, from the numbering written in the header (not from the generator)."""
    a, p, q = e >> 2, e & 1, (e >> 1) & 1
    lo = {0: (0, p, q), 1: (p, 0, q), 2: (p, q, 0)}[a]
    hi = tuple(v + (1 if k == a else 0) for k, v in enumerate(lo))
    return lo, hi


def _inside(case, c):
    return (case >> (c[0] + 2 * c[1] + 4 * c[2])) & 1


def _changing(case, e):
    lo, hi = _edge_ends(e)
    return _inside(case, lo) != _inside(case, hi)


def _common_faces(a, b):
    ends = _edge_ends(a) + _edge_ends(b)
    return [(d, s) for d in range(3) for s in (0, 1) if all(c[d] == s for c in ends)]


def test_generator_output_is_the_committed_header():
    assert open(gen.HEADER).read() == gen.render()
    header = open(gen.HEADER).read()
    rows = re.findall(r"^    \{([^}]*)\},  // (\d+)$", header, flags=re.M)
    assert [int(n) for _, n in rows] == list(range(256))
    for (body, _), tris in zip(rows, mref.TABLE):
        flat = [int(v) for v in body.split(",")]
        assert len(flat) == 16 and flat == [e for t in tris for e in t] + [-1] * (16 - 3 * len(tris))
    counts = [int(v) for v in re.search(r"kMcCount\[256\] = \{(.*?)\};", header, flags=re.S).group(1).replace("\n", " ").split(",") if v.strip()]
    assert counts == [len(t) for t in mref.TABLE]
    assert "not MC33" in header and "cx + 2 cy + 4 cz" in header


def test_table_properties():
    tab = mref.TABLE
    assert len(tab) == 256 and tab[0] == [] and tab[255] == []
    assert sum(len(t) for t in tab) == 820 and max(len(t) for t in tab) == 5
    for case, tris in enumerate(tab):
        changing = {e for e in range(12) if _changing(case, e)}
        used = set()
        for t in tris:
            assert len(set(t)) == 3 and set(t) <= changing, (case, t)
            used |= set(t)
        assert used == changing, case                               # every sign-changing edge carries a vertex of the case's mesh
        for t in tris:
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                for d, s in _common_faces(a, b):
                    # a mesh edge inside a cube face must be that face's segment: the face has two sign changes (then a and b are
                    # them), or four, and then a and b meet in an INSIDE corner
                    face_edges = [e for e in range(12) if all(c[d] == s for c in _edge_ends(e))]
                    n_changing = sum(_changing(case, e) for e in face_edges)
                    shared = set(_edge_ends(a)) & set(_edge_ends(b))
                    assert n_changing == 2 or (n_changing == 4 and len(shared) == 1 and _inside(case, next(iter(shared)))), (case, a, b)
        # within the cell every directed mesh edge occurs once; the ones without a partner are face segments
        d = mref.directed_edges(np.array(tris).reshape(-1, 3))
        assert len({tuple(x) for x in d}) == len(d)
        for a, b in d:
            if not ((d[:, 0] == b) & (d[:, 1] == a)).any():
                assert _common_faces(a, b), (case, a, b)


def test_single_corner_winds_towards_free_space():
    T = np.full((2, 2, 2), 0.5, np.float32)
    T[0, 0, 0] = -0.5
    v, f = mref.mesh(T, np.ones_like(T), (0, 0, 0), 1.0, 1.0)
    assert len(v) == 3 and f.tolist() == [[0, 1, 2]]
    n, _ = mref.normals(v, f)
    assert (n[0] > 0).all()                                         # towards (1, 1, 1): positive T
    v, f = mref.mesh(-T, np.ones_like(T), (0, 0, 0), 1.0, 1.0)      # the complement: the same vertices, the opposite side
    n, _ = mref.normals(v, f)
    assert len(f) == 1 and (n[0] < 0).all()


# ---- 2. closed manifold on random fields, a sphere
def _random_field(seed):
    rng = np.random.RandomState(seed)
    T = np.full((7, 8, 9), 0.5, np.float32)                         # [Z,Y,X] of the 9 x 8 x 7 grid
    T[1:-1, 1:-1, 1:-1] = rng.uniform(-0.99, 0.99, size=(5, 6, 7)).astype(np.float32)
    return T


@pytest.mark.parametrize("seed", range(5))
def test_random_sign_field_gives_a_closed_manifold(seed):
    T = _random_field(seed)
    v, f = mref.mesh(T, np.ones_like(T), (0.3, -1.7, 2.0), 0.05, 1.0)
    assert len(f) > 300
    assert mref.closed_manifold(f)
    assert np.array_equal(np.unique(f), np.arange(len(v)))          # every vertex is referenced
    assert mref.euler(len(v), f) % 2 == 0
    assert np.array_equal(v.view(np.int32), ref.extract(np.float32, T, np.ones_like(T), (0.3, -1.7, 2.0), 0.05, 1.0).view(np.int32))


def test_naive_apex_would_fail_the_manifold_test():
    """The apex rule is load-bearing: fans from the lowest edge put diagonals into cube faces and break the manifold on these fields."""
    saved = mref.TRI.copy()
    try:
        for case in range(256):
            tris = [(L[0], L[i], L[i + 1]) for L in gen.loops(case) for i in range(1, len(L) - 1)]
            mref.TRI[case] = -1
            if tris:
                mref.TRI[case, :len(tris)] = tris
        bad = 0
        for seed in range(5):
            T = _random_field(seed)
            bad += not mref.closed_manifold(mref.mesh(T, np.ones_like(T), (0, 0, 0), 1.0, 1.0)[1])
        assert bad > 0
    finally:
        mref.TRI[:] = saved


def test_sphere_is_closed_with_euler_2_and_outward_normals():
    c = np.array([7.3, 7.6, 7.45])
    iz, iy, ix = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    r = np.sqrt((ix - c[0]) ** 2 + (iy - c[1]) ** 2 + (iz - c[2]) ** 2)
    T = np.clip((r - 5.2) / 3, -0.99, 0.99).astype(np.float32)
    v, f = mref.mesh(T, np.ones_like(T), (0, 0, 0), 1.0, 1.0)
    assert len(f) > 500 and mref.closed_manifold(f) and mref.euler(len(v), f) == 2
    n, centroid = mref.normals(v, f)
    assert ((n * (centroid - c)).sum(axis=1) > 0).all()
    assert np.abs(np.linalg.norm(v - c, axis=1) - 5.2).max() < 0.1


# ---- 3. validity, zeros, degenerate grids
def _face_points(T, Wt, w_min=1.0):
    v, f = mref.mesh(T, Wt, (0, 0, 0), 1.0, w_min)
    case = mref.cell_cases(T, Wt, w_min)
    n = np.where(case >= 0, mref.COUNT[np.maximum(case, 0)], 0).reshape(-1)
    cell = np.repeat(np.arange(n.size), n)                          # the cell of every face (cells in ascending order)
    assert len(cell) == len(f)
    return v[f], cell, case


@pytest.mark.parametrize("what", ["weight", "one", "minus_one", "nan", "nan_weight"])
def test_an_invalid_corner_removes_exactly_the_cells_that_contain_it(what):
    T = _random_field(1)
    Wt = np.ones_like(T)
    Z, Y, X = T.shape
    tri0, cell0, case0 = _face_points(T, Wt)
    removed = 0
    for (z, y, x) in ((3, 4, 5), (1, 1, 1), (0, 3, 2), (6, 7, 8)):
        T1, W1 = T.copy(), Wt.copy()
        if what == "weight":
            W1[z, y, x] = 0.99999994
        elif what == "nan_weight":
            W1[z, y, x] = np.nan
        else:
            T1[z, y, x] = {"one": 1.0, "minus_one": -1.0, "nan": np.nan}[what]
        tri1, cell1, case1 = _face_points(T1, W1)
        cz, cy, cx = np.unravel_index(np.arange(case0.size), case0.shape)
        holds = ((cz == z) | (cz == z - 1)) & ((cy == y) | (cy == y - 1)) & ((cx == x) | (cx == x - 1))
        assert np.array_equal(case1.reshape(-1) == -1, holds) and np.array_equal(case1.reshape(-1)[~holds], case0.reshape(-1)[~holds])
        keep = ~holds[cell0]
        removed += int((~keep).sum())
        assert np.array_equal(tri1.view(np.int32), tri0[keep].view(np.int32)) and np.array_equal(cell1, cell0[keep])
        v1 = mref.mesh(T1, W1, (0, 0, 0), 1.0, 1.0)[0]
        assert np.array_equal(v1.view(np.int32), ref.extract(np.float32, T1, W1, (0, 0, 0), 1.0, 1.0).view(np.int32))
    assert removed > 10                                             # the corners chosen do carry triangles


def test_exact_zero_gives_coincident_vertices_and_keeps_the_triangle():
    T = np.full((2, 2, 2), -0.5, np.float32)
    T[0, 0, 0] = 0.0                                                # outside (T < 0 is false), q = 0 / (0 - T_b) = 0 on its three edges
    v, f = mref.mesh(T, np.ones_like(T), (1.0, 2.0, 3.0), 0.5, 1.0)
    assert len(v) == 3 and f.shape == (1, 3) and sorted(f[0]) == [0, 1, 2]
    assert np.array_equal(v, [[1.0, 2.0, 3.0]] * 3)
    assert not mref.normals(v, f)[0].any()                          # zero area, kept
    T[0, 0, 0] = -0.0                                               # -0.0 is outside as well
    assert mref.mesh(T, np.ones_like(T), (1.0, 2.0, 3.0), 0.5, 1.0)[1].shape == (1, 3)


@pytest.mark.parametrize("dims", [(1, 1, 1), (6, 1, 1), (1, 5, 4), (5, 1, 4), (5, 4, 1)], ids=str)
def test_degenerate_grids_have_vertices_but_no_faces(dims):
    X, Y, Z = dims
    T = np.random.RandomState(2).uniform(-0.9, 0.9, size=(Z, Y, X)).astype(np.float32)
    v, f = mref.mesh(T, np.ones_like(T), (0, 0, 0), 1.0, 1.0)
    assert f.shape == (0, 3) and f.dtype == np.int32
    assert (len(v) > 0) == (max(dims) > 1)


# ---- 4. save_ply
def _old_save_ply(path, p):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(p))
        for x, y, z in p:
            f.write("%.9g %.9g %.9g\n" % (x, y, z))


def _parse_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply"
    nv = int(re.search(r"element vertex (\d+)", head.decode()).group(1))
    m = re.search(r"element face (\d+)\nproperty list uchar int vertex_indices\n", head.decode())
    nf = int(m.group(1)) if m else None
    if lines[1] == "format ascii 1.0":
        rows = body.decode("ascii").split("\n")
        assert rows[-1] == ""
        v = np.array([[float(x) for x in r.split()] for r in rows[:nv]], np.float32).reshape(-1, 3)
        f = None
        if nf is not None:
            f = np.array([[int(x) for x in r.split()] for r in rows[nv:nv + nf]], np.int64).reshape(-1, 4)
            assert (f[:, 0] == 3).all() and len(rows) == nv + nf + 1
            f = f[:, 1:].astype(np.int32)
        return v, f
    assert lines[1] == "format binary_little_endian 1.0"
    v = np.frombuffer(body[:12 * nv], "<f4").reshape(-1, 3)
    f = None
    rest = body[12 * nv:]
    if nf is not None:
        rec = np.frombuffer(rest, np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        assert len(rec) == nf and (rec["n"] == 3).all()
        f = rec["v"].astype(np.int32)
    else:
        assert rest == b""
    return v, f


def test_save_ply_defaults_write_the_same_bytes_and_faces_round_trip(tmp_path):
    rng = np.random.RandomState(3)
    pts = np.concatenate([rng.randn(50, 3).astype(np.float32) * 3, [[0.0, -0.0, 1e-30], [np.float32(1) / 3, 1e20, -7.25]]]).astype(np.float32)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    _old_save_ply(a, pts)
    assert fusion.save_ply(b, torch.from_numpy(pts)) == len(pts)
    assert open(a, "rb").read() == open(b, "rb").read()
    T = _random_field(0)
    v, f = mref.mesh(T, np.ones_like(T), (0.3, -1.7, 2.0), 0.05, 1.0)
    for binary in (False, True):
        for faces in (f, torch.from_numpy(f), None, f[:0]):
            if faces is None and not binary:
                continue
            assert fusion.save_ply(b, v, faces=faces, binary=binary) == len(v)
            gv, gf = _parse_ply(b)
            assert np.array_equal(gv.view(np.int32), v.view(np.int32))
            if faces is None:
                assert gf is None
            else:
                assert gf.shape == (len(faces), 3) and np.array_equal(gf, np.asarray(faces))
    assert fusion.save_ply(b, np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32), binary=True) == 0
    with pytest.raises(ValueError):
        fusion.save_ply(b, v[:5], faces=f)                          # rows beyond the points


# ---- 5. the C entries
def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nrgbd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES.items():
        decl = re.search(r"\b(?:int|long) %s\((.*?)\);" % name, code, flags=re.S).group(1)
        assert decl.count(",") + 1 == len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name)
        assert re.search(r"%s — no counterpart in the reference" % name, header), name
        assert name in header[:header.index("#define NRGBD_INTERFACE_VERSION")]       # named in the list at the top


E_NULL, E_SHAPE, E_ALIGN, E_ARG = -1, -2, -3, -4
P = ctypes.c_void_p(64)                     # never dereferenced: every call below is refused before anything touches the device
NAN, INF = float("nan"), float("inf")


def test_mesh_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    ws, fn = lib.nrgbd_tsdf_mesh_workspace, lib.nrgbd_tsdf_extract_mesh
    V = _lib.TSDF_EXTRACT_VOXELS
    assert ws(1, 1, 1) == 24 + 4 and ws(V, 1, 1) == 24 + 4 * V and ws(V + 1, 1, 1) == 48 + 4 * (V + 1)
    assert ws(8, 6, 4) == 24 + 4 * 192 and ws(256, 256, 256) == 2 ** 24 // V * 24 + 4 * 2 ** 24
    most = (2 ** 31 - 1) // 3                                        # 715827882 = 2 * 3 * 119304647 voxels is the largest grid
    assert ws(most, 1, 1) == -(-most // V) * 24 + 4 * most and ws(2, most // 2, 1) > 0
    for dims in ((0, 1, 1), (1, -1, 1), (1, 1, 0), (most + 1, 1, 1), (2 ** 10, 2 ** 10, 2 ** 10), (2 ** 16, 2 ** 15, 1), (2 ** 16, 2 ** 16, 2 ** 16)):
        assert ws(*dims) == E_SHAPE, dims

    def call(null=None, X=8, Y=6, Z=4, vs=.05, w_min=1., bytes_=24 + 4 * 192, vcap=10, fcap=10, ws_ptr=P, counts_ptr=P):
        ptr = [None if i == null else P for i in range(6)]          # tsdf, weight, workspace, vertices, faces, counts
        if ptr[2] is not None:
            ptr[2] = ws_ptr
        if ptr[5] is not None:
            ptr[5] = counts_ptr
        return fn(ptr[0], ptr[1], X, Y, Z, 0., 0., 0., vs, w_min, ptr[2], bytes_, ptr[3], vcap, ptr[4], fcap, ptr[5], None)
    for i in range(6):
        assert call(null=i) == E_NULL
    for kw in (dict(X=0), dict(Z=-1), dict(X=2 ** 10, Y=2 ** 10, Z=2 ** 10, bytes_=2 ** 40), dict(X=most + 1, Y=1, Z=1, bytes_=2 ** 40),
               dict(vcap=-1), dict(fcap=-1), dict(bytes_=24 + 4 * 192 - 1), dict(X=V + 1, Y=1, Z=1, bytes_=24 + 4 * (V + 1))):
        assert call(**kw) == E_SHAPE, kw
    for kw in (dict(vs=0.), dict(vs=NAN), dict(vs=INF), dict(vs=-1.), dict(w_min=NAN)):
        assert call(**kw) == E_ARG, kw
    assert call(ws_ptr=ctypes.c_void_p(68)) == E_ALIGN and call(counts_ptr=ctypes.c_void_p(36)) == E_ALIGN
    # the order of the checks: NULL, shape, argument, alignment
    assert call(null=0, X=0, vs=0.) == E_NULL and call(X=0, vs=0.) == E_SHAPE and call(vs=0., ws_ptr=ctypes.c_void_p(68)) == E_ARG
    assert call(fcap=-1, vs=0.) == E_SHAPE and call(null=4, X=0) == E_NULL and call(null=4, fcap=-1) == E_SHAPE     # NULL faces: only above 0


def test_ops_and_volume_refuse_what_python_can_see():
    T, Wt = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4)
    c4, ws = torch.zeros(4, dtype=torch.int64), torch.zeros(64, dtype=torch.int64)
    with pytest.raises(_lib.NrgbdError):
        ops.tsdf_extract_mesh(T, Wt, (0, 0, 0), .05, 1., ws, None, None, c4)       # host tensors: no CPU path
    assert ops.tsdf_mesh_workspace(4, 3, 2) == 24 + 4 * 24
    with pytest.raises(_lib.NrgbdError, match="code -2"):
        ops.tsdf_mesh_workspace(0, 3, 2)
    with pytest.raises(_lib.NrgbdError, match="code -2"):
        ops.tsdf_mesh_workspace(1024, 1024, 1024)
    with pytest.raises(TypeError):
        ops.tsdf_extract_mesh(np.zeros((2, 3, 4), np.float32), Wt, (0, 0, 0), .05, 1., ws, None, None, c4)
    import neuralrgbd_amd
    assert hasattr(neuralrgbd_amd.TSDFVolume, "mesh") and hasattr(neuralrgbd_amd.FusionVideoStream, "mesh")
    vol = fusion.TSDFVolume((4, 3, 2), .05, (0, 0, 0), device="cpu")
    with pytest.raises(_lib.NrgbdError):
        vol.mesh()
    with pytest.raises(_lib.NrgbdError):
        vol.mesh(capacity=(3, 2))
