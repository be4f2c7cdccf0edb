"""Comparator of the TSDF mesh extraction (csrc/tsdf_mesh.hip; include/nrgbd.h, nrgbd_tsdf_extract_mesh): the numpy restatement the
GPU must equal exactly, and the mesh checks the host and GPU tests share.

Vertices are tsdf_ref.extract's.  A face holds the rows of its vertices in that sequence: the crossing flags [Z,Y,X,3] in (linear voxel
index, axis) order give every (voxel, axis) its row by a running count.  Cells and the table lookup are vectorised; the table is the
generator's (tools/gen_mc_table.py), the same data the committed header holds."""
import os
import sys

import numpy as np

import tsdf_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_mc_table as gen  # noqa: E402

TABLE = gen.table()                                                 # [256] lists of (e0, e1, e2)
MAX_TRI = max(len(t) for t in TABLE)
TRI = np.full((256, MAX_TRI, 3), -1, np.int64)
for _case, _tris in enumerate(TABLE):
    if _tris:
        TRI[_case, :len(_tris)] = _tris
COUNT = np.array([len(t) for t in TABLE])
# edge -> (offset of the owning voxel (dx, dy, dz), axis)
EDGE_VOXEL = np.array([gen.edge_low_corner(e) for e in range(12)])
EDGE_AXIS = np.arange(12) >> 2


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def crossing_rows(tsdf, weight, w_min):
    """([Z,Y,X,3] int64: the row of crossing (voxel, axis) in the vertex sequence, -1 where there is none; the number of crossings)."""
    T, Wt = _f32(tsdf), _f32(weight)
    with np.errstate(all="ignore"):
        side = (Wt >= np.float32(w_min)) & (np.abs(T) < 1)
    neg = T < 0
    cross = np.zeros(T.shape + (3,), bool)
    for k in range(3):
        ax = 2 - k
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[ax], b[ax] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        cross[a + (k,)] = side[a] & side[b] & (neg[a] != neg[b])
    flat = cross.reshape(-1)
    rows = np.where(flat, np.cumsum(flat) - 1, -1).reshape(cross.shape)
    return rows, int(flat.sum())


def cell_cases(tsdf, weight, w_min):
    """[Z-1,Y-1,X-1] int64: the case of every cell, -1 where a corner fails W >= w_min && |T| < 1."""
    T, Wt = _f32(tsdf), _f32(weight)
    Z, Y, X = T.shape
    with np.errstate(all="ignore"):
        side = (Wt >= np.float32(w_min)) & (np.abs(T) < 1)
    neg = T < 0
    case = np.zeros((Z - 1, Y - 1, X - 1), np.int64)
    valid = np.ones(case.shape, bool)
    for c in range(8):
        cx, cy, cz = c & 1, (c >> 1) & 1, c >> 2
        sl = (slice(cz, Z - 1 + cz), slice(cy, Y - 1 + cy), slice(cx, X - 1 + cx))
        case |= neg[sl].astype(np.int64) << c
        valid &= side[sl]
    return np.where(valid, case, -1)


def mesh(tsdf, weight, origin, vs, w_min):
    """-> (vertices [N,3] fp32, faces [M,3] int32): what nrgbd_tsdf_extract_mesh writes with capacities >= (N, M)."""
    tsdf, weight = _f32(tsdf), _f32(weight)
    vertices = tsdf_ref.extract(np.float32, tsdf, weight, origin, vs, w_min)
    rows, n = crossing_rows(tsdf, weight, w_min)
    assert n == len(vertices)
    Z, Y, X = tsdf.shape
    if min(X, Y, Z) < 2:
        return vertices, np.zeros((0, 3), np.int32)
    case = cell_cases(tsdf, weight, w_min)
    iz, iy, ix = np.nonzero(case > 0)                               # C order: ascending linear index of the lowest corner
    c = case[iz, iy, ix]
    keep = COUNT[c] > 0
    iz, iy, ix, c = iz[keep], iy[keep], ix[keep], c[keep]
    tri = TRI[c]                                                    # [cells, MAX_TRI, 3] edges
    used = tri[:, :, 0] >= 0
    e = np.where(tri >= 0, tri, 0)
    off = EDGE_VOXEL[e]                                             # [cells, MAX_TRI, 3, 3]
    r = rows[iz[:, None, None] + off[..., 2], iy[:, None, None] + off[..., 1], ix[:, None, None] + off[..., 0], EDGE_AXIS[e]]
    faces = r[used]                                                 # cell-major, table order inside a cell
    assert (faces >= 0).all(), "a valid cell's sign-changing edge is a crossing"
    return vertices, faces.astype(np.int32)


# ---- mesh checks ------------------------------------------------------------------------------------------------------------------

def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def closed_manifold(faces):
    """Every directed edge (a, b) occurs exactly once and (b, a) exactly once."""
    d = directed_edges(faces)
    if len(d) == 0:
        return True
    key = d[:, 0] * (d.max() + 1) + d[:, 1]
    rev = d[:, 1] * (d.max() + 1) + d[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    return bool((cnt == 1).all()) and np.array_equal(uniq, np.unique(rev)) and not (d[:, 0] == d[:, 1]).any()


def euler(n_vertices, faces):
    d = directed_edges(faces)
    und = np.unique(np.sort(d, axis=1), axis=0)
    return n_vertices - len(und) + len(faces)


def normals(vertices, faces):
    """Right-hand geometric normals (not normalised) and centroids, float64."""
    p = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p.mean(axis=1)
