"""Comparator of the moving TSDF volume (csrc/tsdf_shift.hip; include/nrgbd.h, nrgbd_tsdf_shift_f32): the numpy restatement of the
documented rule — the moved copy, the zero fill, the spill mask with the one-voxel rim — written from the rule, per axis, on int32 bit
patterns (nothing here touches a value as a float, so NaN payloads and signed zeros survive as they must on the device); the mutants
of the rule the host suite has to catch; the triangle partition the rim is there for; and the window-equivalence scenario the host and
the GPU tests share."""
import functools
import types

import numpy as np

import tsdf_mesh_ref as mref
import tsdf_ref as ref
from neuralrgbd_amd import fusion

SHIFTS = ((4, 0, 0), (-8, 0, 0), (0, 5, 0), (0, 0, -7), (12, -6, 3), (-1, -1, -1), (47, 0, 0), (48, 0, 0), (0, 0, 0), (20, 20, 18))
PARTITION_FAMILIES = ("inside", "front", "edge")
MUTANTS = ("rim_dropped", "rim_two_thick", "rim_wrong_face", "sign_flipped", "colour_zeroed", "no_zero_fill")
GARBAGE = np.int32(0x7FC00ABC)                                      # what a dst buffer holds before the launch (a NaN with a payload)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def _axis_masks(n, s, rim_thick=1, wrong_face=False):
    """Per old index j along one axis of n voxels shifted by s: (leaving [n], rim [n]) as the header states them."""
    j = np.arange(n)
    leaving = (j < s) if s > 0 else (j >= n + s) if s < 0 else np.zeros(n, bool)
    new = j - s                                                     # the index the voxel has after the shift
    if wrong_face:                                                  # the mutant: the rim on the face that trails the motion
        rim = (new >= n - rim_thick) if s > 0 else (new < rim_thick) if s < 0 else np.zeros(n, bool)
    else:
        rim = (new < rim_thick) if s > 0 else (new >= n - rim_thick) if s < 0 else np.zeros(n, bool)
    return leaving, rim & ~leaving


def masks(dims, shift, rim_thick=1, wrong_face=False):
    """([Z,Y,X] leaving, [Z,Y,X] rim) of the OLD voxels: a voxel leaves when it leaves along some axis; a retained voxel is on the rim
    when it is on the rim along some axis."""
    per = [_axis_masks(n, s, rim_thick, wrong_face) for n, s in zip(dims, shift)]
    grid = lambda k: (per[0][k][None, None, :], per[1][k][None, :, None], per[2][k][:, None, None])
    lx, ly, lz = grid(0)
    leaving = lx | ly | lz
    rx, ry, rz = grid(1)
    return leaving, (rx | ry | rz) & ~leaving


def shift(src, s, spill=False, dst_before=None, mutant=None):
    """nrgbd_tsdf_shift_f32 on a [P,Z,Y,X] fp32 array: -> (dst, src afterwards), new fp32 arrays.  dst_before: what dst held (default:
    GARBAGE in every word) — the rule overwrites all of it."""
    assert mutant is None or mutant in MUTANTS
    a = bits(src)
    P, Z, Y, X = a.shape
    s = tuple(int(v) for v in s)
    move = tuple(-v for v in s) if mutant == "sign_flipped" else s
    dst = np.full(a.shape, GARBAGE, np.int32) if dst_before is None else bits(dst_before).copy()
    if mutant != "no_zero_fill":
        dst[:] = 0
    lo = [max(0, -m) for m in move]                                 # the dst indices i whose source i + s lies in the grid, per axis
    hi = [min(n, n - m) for n, m in zip((X, Y, Z), move)]
    if all(l < h for l, h in zip(lo, hi)):
        d = tuple(slice(l, h) for l, h in zip(lo, hi))
        f = tuple(slice(l + m, h + m) for l, h, m in zip(lo, hi, move))
        dst[:, d[2], d[1], d[0]] = a[:, f[2], f[1], f[0]]
    after = a.copy()
    if spill:
        leaving, rim = masks((X, Y, Z), move, rim_thick=2 if mutant == "rim_two_thick" else 1, wrong_face=mutant == "rim_wrong_face")
        if mutant == "rim_dropped":
            rim = np.zeros_like(rim)
        clear = ~leaving & ~rim
        after[:2, clear] = 0
        if mutant == "colour_zeroed":
            after[2:, clear] = 0
    return dst.view(np.float32), after.view(np.float32)


def window(src, s):
    """The moved copy built directly, one voxel at a time by its definition dst[i] = src[i + s] (the yardstick of `shift`'s slices)."""
    a = bits(src)
    P, Z, Y, X = a.shape
    iz, iy, ix = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    jx, jy, jz = ix + s[0], iy + s[1], iz + s[2]
    inside = (jx >= 0) & (jx < X) & (jy >= 0) & (jy < Y) & (jz >= 0) & (jz < Z)
    out = np.zeros_like(a)
    out[:, inside] = a[:, jz[inside], jy[inside], jx[inside]]
    return out.view(np.float32)


def new_origin(origin, vs, s):
    return tuple(float(o) + float(vs) * int(k) for o, k in zip(origin, s))


# ---- the partition the rim is there for ---------------------------------------------------------------------------------------------

def triangles(vertices, faces):
    """[M] rows of nine fp32 bit patterns (as bytes): a triangle as its three corner positions."""
    t = bits(np.asarray(vertices, np.float32)[np.asarray(faces, np.int64)].reshape(len(faces), 9))
    return np.ascontiguousarray(t).view(np.dtype((np.void, 36))).reshape(-1)


def partition(old, origin, vs, s, w_min, mutant=None):
    """The old volume's mesh against the spill's and the live volume's: -> dict(old, spill, live triangle counts, subset: every spill
    triangle is bit for bit a triangle of the old mesh, ok: the counts add up and subset)."""
    dst, after = shift(old, s, spill=True, mutant=mutant)
    m_old = mref.mesh(old[0], old[1], origin, vs, w_min)
    m_spill = mref.mesh(after[0], after[1], origin, vs, w_min)
    m_live = mref.mesh(dst[0], dst[1], new_origin(origin, vs, s), vs, w_min)
    subset = bool(np.isin(triangles(*m_spill), triangles(*m_old)).all())
    n = dict(old=len(m_old[1]), spill=len(m_spill[1]), live=len(m_live[1]), subset=subset)
    n["ok"] = subset and n["old"] == n["spill"] + n["live"]
    n["meshes"] = (m_old, m_spill, m_live)
    return n


@functools.lru_cache(maxsize=None)
def fused_planes(family, dims):
    """The fused volume of tsdf_ref's case as [2,Z,Y,X] fp32 with the case (origin, vs)."""
    size = ref.SIZES[0]
    T, W = ref.fused(family, dims, size)[-1]
    case = ref.make_case(family, dims, size)
    return np.stack([T, W]).astype(np.float32), case["origin"], case["vs"]


def pattern(planes, dims, seed=0):
    """A recognisable [P,Z,Y,X] fp32 pattern — every word of every plane differs — with NaNs (quiet and signalling payloads), +-inf,
    -0.0, +0.0 and denormals seeded into every plane."""
    X, Y, Z = dims
    n = X * Y * Z
    rng = np.random.RandomState(100 + seed)
    a = (np.arange(planes * n, dtype=np.float32) * np.float32(0.25) + np.float32(1)).reshape(planes, n)
    special = np.array([0x7FC12345, 0xFFC00001 - (1 << 32), 0x7F800001, 0x7F800000, 0xFF800000 - (1 << 32), 0x80000000 - (1 << 32), 0,
                        0x00000001, 0x807FFFFF - (1 << 32)], np.int64).astype(np.int32)
    b = a.view(np.int32)
    for p in range(planes):
        k = min(n, max(len(special), n // 8))
        at = rng.choice(n, k, replace=False)
        b[p, at] = special[(np.arange(k) + p) % len(special)]
    return b.view(np.float32).reshape(planes, Z, Y, X)


# ---- the window scenario: a small volume that follows a camera against a static one over the same views -----------------------------

VS = 2.0 ** -5                                                      # a dyadic lattice: ox + vs ix is exact wherever the origin sits
WINDOW_DIMS, STATIC_DIMS, WINDOW_STEP = (32, 24, 24), (96, 24, 24), 8
WINDOW_ORIGIN = (-16 * VS, -12 * VS, 8 * VS)
WINDOW_K, WINDOW_SIZE = (64.0, 64.0, 16.0, 12.0), (24, 32)
WINDOW_TRUNC, WINDOW_RANGE = 3 * VS, (0.05, 0.4)


@functools.lru_cache(maxsize=None)
def window_scenario():
    """-> dict(views=[(extM, depth, offset the window has when the view is integrated)], ...).  The camera looks along +z from two
    voxels inside the grid's near face, starts 8 voxels from its low x face and translates along +x by 1.7 voxels a view; the window moves by WINDOW_STEP once the camera is more
    than 20 voxels from its low face."""
    rng = np.random.RandomState(5)
    H, W = WINDOW_SIZE
    views, off = [], 0
    for i in range(42):
        gx = 8.0 + 1.7 * i                                         # the camera's lattice x in the static grid
        centre = np.array([WINDOW_ORIGIN[0] + VS * gx, WINDOW_ORIGIN[1] + VS * 11.6, WINDOW_ORIGIN[2] + VS * 2.0])
        extM = ref.look_at(np.eye(3), centre)
        while gx - off > 20:
            off += WINDOW_STEP
        depth = (0.22 + 0.1 * rng.rand(H, W)).astype(np.float32)
        views.append((extM, depth, off))
    assert off == STATIC_DIMS[0] - WINDOW_DIMS[0]
    return dict(views=views)


def unclipped_box(extM, origin, dims):
    """fusion.frustum_box without the clip to the grid: the box in a grid grown by 2^12 voxels on every side, moved back."""
    big = 1 << 12
    vol = types.SimpleNamespace(dims=tuple(n + 2 * big for n in dims), origin=tuple(o - VS * big for o in origin), voxel_size=VS)
    box = fusion.frustum_box(extM, WINDOW_K, WINDOW_SIZE, WINDOW_RANGE[1] + WINDOW_TRUNC, vol)
    return tuple(b - big for b in box)


def window_observe(dims, origin, extM, depth):
    return ref.chain(np.float32, dims, origin, VS, np.float32(extM[:3, :4]), WINDOW_K, depth, WINDOW_TRUNC, WINDOW_RANGE[0], WINDOW_RANGE[1])
