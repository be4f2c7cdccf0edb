"""Comparator of the paged TSDF volume (csrc/tsdf_page.hip; include/nrgbd.h, nrgbd_tsdf_blocks_gather_f32 / _scatter_f32;
fusion.BlockStore, TSDFVolume.shift(store=...), fusion.paged_extract): numpy restatements of the documented rules on int32 bit patterns
— the block gather with its flag, the scatter, the paged shift (tsdf_shift_ref.shift plus the store logic, with a plain dict as the
store), the tile assembly of the world —, the one-voxel-at-a-time definitions they are checked against, the mutants the host suite has
to catch, the origin lists the GPU test uses, and the out-and-back window scenario the host and the GPU tests share."""
import functools

import numpy as np

import tsdf_mesh_ref as mref
import tsdf_shift_ref as sr

B = 8                                                               # NRGBD_TSDF_BLOCK
MUTANTS = ("flag_ignores_colour", "minus_zero_is_empty", "no_clipping", "xz_swapped", "take_keeps", "sets_swapped")
KERNEL_MUTANTS = MUTANTS[:4]                                        # of gather / scatter; the last two are of the store logic


def _clip(o, n):
    """Along one axis: (block slice, grid slice) of the part of block [o, o + 8) inside [0, n), or None."""
    lo, hi = max(o, 0), min(o + B, n)
    return None if lo >= hi else (slice(lo - o, hi - o), slice(lo, hi))


def gather(vol, origins, mutant=None):
    """nrgbd_tsdf_blocks_gather_f32 on a [P,Z,Y,X] fp32 array: -> (blocks [n,P,8,8,8] fp32, nonempty [n] int32)."""
    assert mutant is None or mutant in KERNEL_MUTANTS
    a = sr.bits(vol)
    P, Z, Y, X = a.shape
    origins = np.asarray(origins, np.int64).reshape(-1, 3)
    out = np.zeros((len(origins), P, B, B, B), np.int32)
    flags = np.zeros(len(origins), np.int32)
    for b, (ox, oy, oz) in enumerate(origins):
        if mutant == "no_clipping":                                 # indices wrap round the grid instead of reading +0.0
            iz, iy, ix = np.meshgrid(np.arange(oz, oz + B) % Z, np.arange(oy, oy + B) % Y, np.arange(ox, ox + B) % X, indexing="ij")
            out[b] = a[:, iz, iy, ix]
            inside = out[b]
        else:
            cx, cy, cz = _clip(int(ox), X), _clip(int(oy), Y), _clip(int(oz), Z)
            if cx is None or cy is None or cz is None:
                continue
            out[b][:, cz[0], cy[0], cx[0]] = a[:, cz[1], cy[1], cx[1]]
            inside = out[b][:, cz[0], cy[0], cx[0]]
        seen = inside[:2] if mutant == "flag_ignores_colour" else inside
        if mutant == "minus_zero_is_empty":
            seen = seen & np.int32(0x7FFFFFFF)
        flags[b] = int(seen.any())
        if mutant == "xz_swapped":
            out[b] = out[b].transpose(0, 3, 2, 1)
    return out.view(np.float32), flags


def scatter(vol, origins, blocks, mutant=None):
    """nrgbd_tsdf_blocks_scatter_f32: -> the [P,Z,Y,X] fp32 array afterwards (a new array)."""
    assert mutant is None or mutant in KERNEL_MUTANTS
    a = sr.bits(vol).copy()
    P, Z, Y, X = a.shape
    blk = sr.bits(blocks)
    for b, (ox, oy, oz) in enumerate(np.asarray(origins, np.int64).reshape(-1, 3)):
        src = blk[b].transpose(0, 3, 2, 1) if mutant == "xz_swapped" else blk[b]
        if mutant == "no_clipping":
            iz, iy, ix = np.meshgrid(np.arange(oz, oz + B) % Z, np.arange(oy, oy + B) % Y, np.arange(ox, ox + B) % X, indexing="ij")
            a[:, iz, iy, ix] = src
            continue
        cx, cy, cz = _clip(int(ox), X), _clip(int(oy), Y), _clip(int(oz), Z)
        if cx is None or cy is None or cz is None:
            continue
        a[:, cz[1], cy[1], cx[1]] = src[:, cz[0], cy[0], cx[0]]
    return a.view(np.float32)


def gather_by_definition(vol, origins):
    """blocks[b][p][k][j][i] = vol[p][oz+k][oy+j][ox+i] where that voxel lies in the grid, +0.0 where not; the flag: any in-grid word
    with a non-zero bit pattern.  One voxel at a time."""
    a = sr.bits(vol)
    P, Z, Y, X = a.shape
    origins = np.asarray(origins, np.int64).reshape(-1, 3)
    out = np.zeros((len(origins), P, B, B, B), np.int32)
    flags = np.zeros(len(origins), np.int32)
    for b, (ox, oy, oz) in enumerate(origins):
        for k in range(B):
            for j in range(B):
                for i in range(B):
                    x, y, z = ox + i, oy + j, oz + k
                    if 0 <= x < X and 0 <= y < Y and 0 <= z < Z:
                        out[b, :, k, j, i] = a[:, z, y, x]
                        if (a[:, z, y, x] != 0).any():
                            flags[b] = 1
    return out.view(np.float32), flags


def scatter_by_definition(vol, origins, blocks):
    a = sr.bits(vol).copy()
    P, Z, Y, X = a.shape
    blk = sr.bits(blocks)
    for b, (ox, oy, oz) in enumerate(np.asarray(origins, np.int64).reshape(-1, 3)):
        for k in range(B):
            for j in range(B):
                for i in range(B):
                    x, y, z = ox + i, oy + j, oz + k
                    if 0 <= x < X and 0 <= y < Y and 0 <= z < Z:
                        a[:, z, y, x] = blk[b, :, k, j, i]
    return a.view(np.float32)


def overlap_in_grid(a, b, dims):
    """Two blocks share a voxel of the grid."""
    return all(max(p, q, 0) < min(p + B, q + B, n) for p, q, n in zip(a, b, dims))


def cases(dims):
    """-> [(name, origins [n,3] int64)] for a dims = (X, Y, Z) grid with X >= 11 and Y, Z >= 8: the lists of the GPU test and of the
    host comparison.  (0, 0, 0) and (8, 0, 0) are the blocks `prepared` empties: an aligned interior block that is all zero, and one
    that is zero except a -0.0 in the last plane; ox = 4 is aligned to 4 but not to 8, ox = 3 to nothing; a block half outside each
    of the six faces (-4 and dim - 4), each alone and, in `mixed`, together with the others as far as they do not overlap inside
    the grid (scatter's contract) and with blocks wholly outside; n = 1 and n = 0."""
    X, Y, Z = dims
    far = [(X, 0, 0), (-8, 0, 0), (0, -8, Z), (1 << 30, -(1 << 30), 3), (X + 5, Y + 1, -9)]
    faces = [(-4, 0, 0), (X - 4, 0, 0), (0, -4, 0), (0, Y - 4, 0), (0, 0, -4), (0, 0, Z - 4)]
    mixed = []
    for o in [(3, 1, 0), far[0]] + faces[::-1] + far[1:] + [(4, 0, 0), (0, 0, 0), (8, 0, 0), (-4, -4, -4), (X - 4, Y - 4, Z - 4)]:
        if not any(overlap_in_grid(o, q, dims) for q in mixed):
            mixed.append(o)
    lists = [("prepared", [(0, 0, 0), (8, 0, 0)]), ("ox4", [(4, 0, 0)] + far), ("ox3", [(3, 1, 0), far[0]])]
    lists += [("face%d" % k, [o]) for k, o in enumerate(faces)]
    lists += [("corners", [(-4, -4, -4), (X - 4, Y - 4, Z - 4)] if min(dims) >= 12 else [(-4, -4, -4)]), ("outside", far), ("mixed", mixed),
              ("one", [(X - 5, Y - 6, Z - 7)]), ("none", [])]
    return [(name, np.asarray(o, np.int64).reshape(-1, 3)) for name, o in lists]


def prepared(planes, dims, seed=0):
    """tsdf_shift_ref.pattern with the in-grid part of the block at (0, 0, 0) zeroed — an all-zero block — and that of the block at
    (8, 0, 0) zero except one -0.0 in the last plane (a colour plane of a colour volume)."""
    assert dims[0] >= 11 and min(dims[1:]) >= 8
    vol = sr.bits(sr.pattern(planes, dims, seed)).copy()
    vol[:, :B, :B, :2 * B] = 0
    vol[planes - 1, 3, 5, B + 2] = np.int32(-2 ** 31)
    return vol.view(np.float32)


# ---- the paged shift: tsdf_shift_ref.shift plus the store logic, the store a plain dict ------------------------------------------------

def window_keys(offset, dims):
    """The set of world block indices of the window [offset, offset + dims): both multiples of 8."""
    assert all(v % B == 0 for v in tuple(offset) + tuple(dims))
    r = [range(o // B, (o + n) // B) for o, n in zip(offset, dims)]
    return {(x, y, z) for z in r[2] for y in r[1] for x in r[0]}


def paged_shift(live, offset, s, store, mutant=None):
    """TSDFVolume.shift(s, store=...) on a [P,Z,Y,X] array at `offset`: -> (the array afterwards, the new offset, counts: dict(out,
    dropped, in)).  `store`: a dict {(bx, by, bz): [P,8,8,8] fp32}, modified in place."""
    assert mutant is None or mutant in MUTANTS
    P, Z, Y, X = live.shape
    dims = (X, Y, Z)
    new_offset = tuple(o + v for o, v in zip(offset, s))
    moved = sr.shift(live, s)[0]
    old_keys, new_keys = window_keys(offset, dims), window_keys(new_offset, dims)
    leaving, entering = sorted(old_keys - new_keys), sorted(new_keys - old_keys)
    if mutant == "sets_swapped":
        leaving, entering = entering, leaving
    kernel = mutant if mutant in KERNEL_MUTANTS else None
    blocks, flags = gather(live, [tuple(B * k - o for k, o in zip(key, offset)) for key in leaving], kernel)
    found = [key for key in entering if key in store]
    if found:
        data = np.stack([store[key] for key in found])
        moved = scatter(moved, [tuple(B * k - o for k, o in zip(key, new_offset)) for key in found], data, kernel)
        if mutant != "take_keeps":
            for key in found:
                del store[key]
    kept = 0
    for key, blk, flag in zip(leaving, blocks, flags):
        if flag:
            if mutant != "take_keeps":
                assert key not in store, key
            store[key] = blk.copy()
            kept += 1
    return moved, new_offset, dict(out=kept, dropped=len(leaving) - kept, **{"in": len(found)})


def world(live, offset, store, bounds=None):
    """The live window and the store laid out as one array: -> (the [P,Z,Y,X] fp32 array over the voxel bounds of both — or over
    bounds = (lo, hi), which must hold them —, its low corner (x, y, z) in world voxels).  +0.0 where neither holds a voxel."""
    P, Z, Y, X = live.shape
    lo = np.array(offset, np.int64)
    hi = lo + (X, Y, Z)
    for key in store:
        lo, hi = np.minimum(lo, B * np.array(key)), np.maximum(hi, B * np.array(key) + B)
    if bounds is not None:
        assert (np.array(bounds[0]) <= lo).all() and (np.array(bounds[1]) >= hi).all()
        lo, hi = np.array(bounds[0], np.int64), np.array(bounds[1], np.int64)
    out = np.zeros((P,) + tuple(int(v) for v in (hi - lo)[::-1]), np.int32)
    at = lambda o, n: tuple(slice(int(o[k] - lo[k]), int(o[k] - lo[k]) + n[k]) for k in (2, 1, 0))
    out[(slice(None),) + at(offset, (X, Y, Z))] = sr.bits(live)
    for key, blk in store.items():
        out[(slice(None),) + at(B * np.array(key), (B, B, B))] = sr.bits(blk)
    return out.view(np.float32), tuple(int(v) for v in lo)


# ---- the tile assembly of fusion.paged_extract -----------------------------------------------------------------------------------------

def tile_starts(lo, hi, dims):
    """Per axis the tile origins: lo, lo + (dims - 1), ... while a cell is left."""
    return [list(range(lo[k], max(hi[k] - 1, lo[k] + 1), max(dims[k] - 1, 1))) for k in range(3)]


def tiles(live, offset, store, dims):
    """-> [(tile origin (x, y, z) in world voxels, the assembled [P,Z,Y,X] tile)] in ascending (z, y, x) order, the tiles no block
    touches left out: every block of the live window and of the store that touches the tile, clipped to it."""
    P = live.shape[0]
    X, Y, Z = live.shape[3], live.shape[2], live.shape[1]
    lo = np.array(offset, np.int64)
    hi = lo + (X, Y, Z)
    for key in store:
        lo, hi = np.minimum(lo, B * np.array(key)), np.maximum(hi, B * np.array(key) + B)
    every = dict(store)
    for key in window_keys(offset, (X, Y, Z)):
        o = tuple(B * k - f for k, f in zip(key, offset))
        every[key] = live[:, o[2]:o[2] + B, o[1]:o[1] + B, o[0]:o[0] + B]
    out = []
    starts = tile_starts([int(v) for v in lo], [int(v) for v in hi], dims)
    for tz in starts[2]:
        for ty in starts[1]:
            for tx in starts[0]:
                t = (tx, ty, tz)
                keys = [key for key in sorted(every) if all(B * k + B > a and B * k < a + n for k, a, n in zip(key, t, dims))]
                if not keys:
                    continue
                tile = np.zeros((P, dims[2], dims[1], dims[0]), np.float32)
                tile = scatter(tile, [tuple(B * k - a for k, a in zip(key, t)) for key in keys], np.stack([every[key] for key in keys]))
                out.append((t, tile))
    return out


def tiled_mesh(parts, origin0, vs, w_min):
    """The tiles' meshes concatenated as fusion.paged_extract does: -> (vertices, faces, [per-tile (vertices, faces)])."""
    meshes = [mref.mesh(tile[0], tile[1], sr.new_origin(origin0, vs, t), vs, w_min) for t, tile in parts]
    base = np.cumsum([0] + [len(m[0]) for m in meshes[:-1]])
    if not meshes:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), []
    return (np.concatenate([m[0] for m in meshes]).astype(np.float32),
            np.concatenate([np.asarray(m[1], np.int64) + b for m, b in zip(meshes, base)]).astype(np.int32), meshes)


def sorted_triangles(vertices, faces):
    """[m,9] fp32: every triangle as its three corner positions, the triangles in lexicographic order — what two meshes of one surface
    with different vertex numbering are compared by."""
    t = np.asarray(vertices, np.float32)[np.asarray(faces, np.int64)].reshape(len(faces), 9)
    return t[np.lexsort(t.T[::-1])]


# ---- the out-and-back window scenario --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def out_and_back():
    """tsdf_shift_ref.window_scenario's camera carried out and back: view index 0..41, then 41..0 — 84 views.  The window moves by +8
    once gx - off > 20, and by -8 once gx - off < 12 while off > 0.  -> [(extM, depth, the window's x offset at the view)]."""
    import tsdf_ref as ref
    rng = np.random.RandomState(11)
    H, W = sr.WINDOW_SIZE
    views, off = [], 0
    for i in list(range(42)) + list(range(41, -1, -1)):
        gx = 8.0 + 1.7 * i
        centre = np.array([sr.WINDOW_ORIGIN[0] + sr.VS * gx, sr.WINDOW_ORIGIN[1] + sr.VS * 11.6, sr.WINDOW_ORIGIN[2] + sr.VS * 2.0])
        extM = ref.look_at(np.eye(3), centre)
        while gx - off > 20:
            off += sr.WINDOW_STEP
        while gx - off < 12 and off > 0:
            off -= sr.WINDOW_STEP
        depth = (0.22 + 0.1 * rng.rand(H, W)).astype(np.float32)
        views.append((extM, depth, off))
    return views


SCENARIO_COUNTS = dict(shifts=16, out=29, dropped=115, **{"in": 16}, left=13)


@functools.lru_cache(maxsize=None)
def out_and_back_host(mutant=None):
    """The scenario in numpy: -> dict(live, off, store, static, counts, boxes_ok).  Read-only: shared between tests."""
    import tsdf_ref as ref
    X, Y, Z = sr.WINDOW_DIMS
    static = np.zeros((2,) + sr.STATIC_DIMS[::-1], np.float32)
    live = np.zeros((2, Z, Y, X), np.float32)
    store, off = {}, 0
    counts = dict(shifts=0, out=0, dropped=0, **{"in": 0})
    boxes_ok = True
    for extM, depth, at in out_and_back():
        while at != off:                                            # one block step at a time, as the scenario states it
            step = sr.WINDOW_STEP if at > off else -sr.WINDOW_STEP
            live, (off, _, _), c = paged_shift(live, (off, 0, 0), (step, 0, 0), store, mutant)
            counts["shifts"] += 1
            for k, v in c.items():
                counts[k] += v
        origin = sr.new_origin(sr.WINDOW_ORIGIN, sr.VS, (off, 0, 0))
        box = sr.unclipped_box(extM, origin, sr.WINDOW_DIMS)
        boxes_ok = boxes_ok and min(box[:3]) >= 0 and all(b <= n for b, n in zip(box[3:], sr.WINDOW_DIMS))
        live = np.stack(ref.integrate(np.float32, live[0], live[1], sr.window_observe(sr.WINDOW_DIMS, origin, extM, depth), 64.0))
        static = np.stack(ref.integrate(np.float32, static[0], static[1],
                                        sr.window_observe(sr.STATIC_DIMS, sr.WINDOW_ORIGIN, extM, depth), 64.0))
    counts["left"] = len(store)
    for a in (live, static):
        a.setflags(write=False)
    return dict(live=live, off=off, store=store, static=static, counts=counts, boxes_ok=boxes_ok)
