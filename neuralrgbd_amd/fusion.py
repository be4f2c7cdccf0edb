"""On-device TSDF fusion: the depth and confidence maps of a trajectory accumulated in the world frame.

The reference stops at the maps (test_utils/export_res.py writes them to files); nothing in it accumulates them.  Here a depth frame
costs one launch (ops.tsdf_integrate) that updates a dense truncated-signed-distance volume on the device, and the surface is read out
as points by a deterministic compaction (ops.tsdf_extract_points): fp32 throughout, no atomics, the same bits in every run.  The
conventions (lattice, projection, update rule, crossings) are written out in include/nrgbd.h.

  * `TSDFVolume`: the volume, `integrate` (one launch, nothing allocated, nothing synchronised) and `points`;
  * `frustum_box`: the voxel box a camera can touch, in float64 on the host — `integrate(cull=True)` launches over it alone;
  * `FusionVideoStream`: a video.VideoDepthStream that integrates the map of every frame that comes out, with the extrinsic that was
    pushed with that frame;
  * `TSDFVolume.raycast` / `FusionVideoStream.render`: the volume seen from any camera — depth and normals, one launch
    (ops.tsdf_raycast); `shade` turns the normals into a viewable image;
  * `TSDFVolume.mesh` / `FusionVideoStream.mesh`: the surface as an indexed triangle mesh (ops.tsdf_extract_mesh): the vertices are
    `points()`'s, the triangles come from a 256-case table and wind towards free space; `save_ply` writes it (ASCII or binary);
  * colour: `TSDFVolume(color=True)` carries three colour planes that share the TSDF's weight; `integrate(color=image)` averages the
    frame's pixels into them in the same launch (ops.tsdf_integrate_color), `points(colors=True)`, `mesh(colors=True)` and
    `raycast(color=True)` read them out, and `FusionVideoStream(color=True)` fuses every frame's own picture from its ring slot;
    `to_uint8` and `save_ply(colors=...)` write them;
  * tracking: `TSDFVolume.track` registers a depth frame against the volume from a pose guess (tracking.FrameTracker: ray casts and
    point-to-plane Gauss-Newton iterations on the device, ops.icp_terms / ops.icp_update), and `FusionVideoStream(track=True)`
    integrates every map at its tracked pose instead of the pushed one;
  * pose corrections: `TSDFVolume.deintegrate` takes a fused frame out of the volume again and `TSDFVolume.reintegrate` moves it to a
    corrected pose in one launch (ops.tsdf_reintegrate: BundleFusion's re-integration); `FusionVideoStream(history=N)` keeps the maps
    of the last N frames for it — `repose`, `retrack`;
  * multi-view consistency: `filter_depth` cross-checks a depth map against other views' maps in one launch (ops.depth_consistency:
    a pixel stays where enough views see the same surface at the same depth) and `FusionVideoStream(history=N, consistency=k)` does
    it for every frame against the held ones before the frame is tracked and fused: the flying pixels of a depth expectation at a
    discontinuity never enter the volume.  Not built: deferred two-sided filtering (with the frames that arrive later), a fused
    depth averaged over the agreeing views, a free-space-violation count, sources of another size or intrinsics, and scoring the
    filtered set in evaluate.EvalVideoStream;
  * the moving volume: `TSDFVolume.shift` moves the grid by whole voxels in one launch (ops.tsdf_shift: what stays keeps its bits,
    what enters is empty, what leaves is handed out as a spill volume), `follow_shift` says when and by how much from a camera pose,
    and `FusionVideoStream(follow=distance)` keeps the volume around the camera's focus, extracts every spill (`chunks`) and
    stitches them with the live mesh (`world_mesh`, `world_points`) — the scheme of Kintinuous and large-scale KinFu.  Not built:
    exact `repose` of frames integrated before a shift (it would clip the removal to the region that has existed since), circular
    addressing in place of the copy, a sparse block volume;
  * paging: `TSDFVolume.shift(store=BlockStore)` keeps what leaves as 8^3 voxel blocks on the host (ops.tsdf_blocks_gather) and puts
    back, bit for bit, what the store holds of the region that enters (ops.tsdf_blocks_scatter), so a camera that returns finds the
    model it left; `paged_extract` reads the whole world — live window and store — as one mesh or point set, tile by tile, and
    `FusionVideoStream(follow_spill="page")` does both for a stream.  Not built: compressed or device-resident blocks, prefetch ahead
    of the motion, exact `repose` across shifts;
  * `fuse_sequence`, `save_ply`.
"""
import math
import typing

import numpy as np
import torch

from . import misc, ops
from . import homography as warp_homo
from .evaluate import GtRing
from .video import VideoDepthStream


def intrinsics_at(cam_intrinsics, H, W):
    """(fx, fy, cx, cy) of an H x W map from the dict's fields of view, as camera.make_cam_intrinsics forms them (the principal point at
    the centre; pixel x covers [x, x + 1))."""
    fx = (W / 2.0) / math.tan(math.radians(cam_intrinsics["hfov"] / 2.0))
    fy = (H / 2.0) / math.tan(math.radians(cam_intrinsics["vfov"] / 2.0))
    return fx, fy, W / 2.0, H / 2.0


def _indexed(device):
    """(type, index) of a device, "cuda" without an index standing for the current one."""
    d = torch.device(device)
    return d.type, (torch.cuda.current_device() if d.type == "cuda" and d.index is None else d.index)


def _host_matrix(extM, who):
    if isinstance(extM, torch.Tensor):
        extM = extM.detach().cpu().numpy()
    m = np.asarray(extM, dtype=np.float64)
    if m.shape not in ((3, 4), (4, 4)):
        raise ValueError("%s: extM is a [3,4] or [4,4] world-to-camera matrix, got %s" % (who, m.shape))
    return m


def frustum_box(extM, intrinsics, size, depth_max, volume):
    """The half-open voxel box (x0, y0, z0, x1, y1, z1) of `volume` that a camera at extM (world -> camera) can touch out to z-depth
    `depth_max` (d_far + trunc): the index box of the camera centre and of the four corners of the pixel rectangle [0, W] x [0, H] at
    that depth — the convex hull of every lattice point the kernel can update —, widened by one voxel and clipped to the grid.  float64
    on the host.  None when the clipped box is empty (or the pose is not finite): nothing to launch; the whole grid when depth_max is
    infinite."""
    dims = volume.dims
    m = _host_matrix(extM, "frustum_box")
    if not math.isfinite(float(m.sum())) or math.isnan(depth_max):  # a NaN or infinite entry makes the sum NaN or infinite
        return None
    if math.isinf(depth_max):
        return (0, 0, 0) + tuple(dims)
    fx, fy, cx, cy = (float(k) for k in intrinsics)
    H, W = size
    x0, x1, y0, y1 = -cx / fx * depth_max, (W - cx) / fx * depth_max, -cy / fy * depth_max, (H - cy) / fy * depth_max
    cam = np.array([[0.0, 0.0, 0.0], [x0, y0, depth_max], [x0, y1, depth_max], [x1, y0, depth_max], [x1, y1, depth_max]])
    try:
        world = np.linalg.solve(m[:3, :3], (cam - m[:3, 3]).T).tolist()      # [3][5]: one solve for the five points
    except np.linalg.LinAlgError:                                   # not a rigid motion: nothing to cull by
        return (0, 0, 0) + tuple(dims)
    lo_hi = []
    for k in range(3):
        a = [(x - volume.origin[k]) / volume.voxel_size for x in world[k]]
        lo, hi = min(a), max(a)
        if not (math.isfinite(lo) and math.isfinite(hi)):
            return (0, 0, 0) + tuple(dims)
        lo = max(int(math.floor(lo)) - 1, 0)
        hi = min(int(math.ceil(hi)) + 2, dims[k])                   # half-open: the last index + 1, + 1 for the margin
        if lo >= hi:
            return None
        lo_hi.append((lo, hi))
    return tuple(v[0] for v in lo_hi) + tuple(v[1] for v in lo_hi)


def follow_shift(extM, volume, distance, margin=0.25, step=8):
    """The shift (sx, sy, sz) in whole voxels that brings `volume` back around a camera at extM (host world -> camera): float64 on
    the host, nothing launched.  The focus point is the camera centre plus `distance` metres along the optical axis, in world
    coordinates; g is its lattice coordinate (focus - origin) / voxel_size and c = (dims - 1) / 2 the grid's centre.  Along each axis
    the shift is step * round((g_k - c_k) / step) where |g_k - c_k| > margin * dims_k (Python's round: a tie goes to the even
    multiple), and 0 otherwise: the volume stays put while the focus is inside the middle 2 margin of the grid, and moves by whole
    steps that re-centre it when it is not.  step: a positive multiple of 4, so that an x shift keeps the shift kernel's 16-byte
    source loads; 0 < margin < 0.5; distance finite.  distance, margin and step are parameters, not measurements: where the fused
    surface lies in front of the camera, and how often the volume may move.  A non-finite or singular pose gives (0, 0, 0)."""
    distance, margin = float(distance), float(margin)
    if not math.isfinite(distance):
        raise ValueError("follow_shift: distance must be finite, got %r" % (distance,))
    if not 0 < margin < 0.5:
        raise ValueError("follow_shift: margin %r is not in (0, 0.5)" % (margin,))
    if isinstance(step, bool) or int(step) != step or step <= 0 or int(step) % 4:
        raise ValueError("follow_shift: step is a positive multiple of 4 voxels (the 16-byte source path), got %r" % (step,))
    step = int(step)
    m = _host_matrix(extM, "follow_shift")
    if not np.isfinite(m).all():
        return (0, 0, 0)
    try:
        focus = np.linalg.solve(m[:3, :3], np.array([0.0, 0.0, distance]) - m[:3, 3])
    except np.linalg.LinAlgError:
        return (0, 0, 0)
    out = []
    for k in range(3):
        off = (float(focus[k]) - volume.origin[k]) / volume.voxel_size - (volume.dims[k] - 1) / 2.0
        if not math.isfinite(off):
            return (0, 0, 0)
        out.append(step * int(round(off / step)) if abs(off) > margin * volume.dims[k] else 0)
    return tuple(out)


BLOCK = ops.TSDF_BLOCK                                              # voxels along the edge of a paged block


def _block_keys(keys):
    """Block indices as an int64 array [n,3]."""
    k = np.asarray(list(keys) if not isinstance(keys, np.ndarray) else keys, dtype=np.int64)
    return k.reshape(-1, 3)


class BlockStore:
    """What a paged volume keeps on the host: a dict from the world block index (bx, by, bz) — any integers, negative ones too; the
    block covers the world voxels 8 b .. 8 b + 7 of the volume's construction lattice — to the block's [planes,8,8,8] fp32 words,
    indexed (plane, z, y, x).  Pure numpy: no GPU is needed to fill, query, save or load one.  `n_put`, `n_dropped` and `n_taken`
    count, over the store's life, the blocks `put` kept, the all-zero ones it dropped and the ones `take` handed back."""

    def __init__(self, planes, block=BLOCK):
        if planes not in (2, 5):
            raise ValueError("BlockStore: planes is 2 (tsdf, weight) or 5 (with r, g, b), got %r" % (planes,))
        if block != BLOCK:
            raise ValueError("BlockStore: blocks are %d voxels wide (NRGBD_TSDF_BLOCK), got %r" % (BLOCK, block))
        self.planes, self.block = int(planes), BLOCK
        self._blocks = {}
        self.n_put = self.n_dropped = self.n_taken = 0

    def _shape(self):
        return (self.planes,) + (self.block,) * 3

    def put(self, keys, data, nonempty=None):
        """keys [n,3] block indices, data [n,planes,8,8,8] fp32, nonempty [n] (ops.tsdf_blocks_gather's flags; None: every block
        counts): the flagged blocks are copied in, the others — +0.0 throughout, what an entering region holds anyway — dropped.
        A key the store already holds is refused (ValueError) before anything is stored: a block is paged out once before it is
        paged in again.  Returns the number of blocks kept."""
        keys = _block_keys(keys)
        data = np.asarray(data)
        if data.dtype != np.float32 or tuple(data.shape) != (len(keys),) + self._shape():
            raise ValueError("BlockStore.put: data is fp32 [%d,%s], got %s %s" % (len(keys), ",".join(str(n) for n in self._shape()),
                                                                                  data.dtype, data.shape))
        flags = np.ones(len(keys), bool) if nonempty is None else np.asarray(nonempty).reshape(-1) != 0
        if len(flags) != len(keys):
            raise ValueError("BlockStore.put: %d flags for %d blocks" % (len(flags), len(keys)))
        rows = np.flatnonzero(flags)
        kept = list(zip(map(tuple, keys[rows].tolist()), rows.tolist()))
        names = [k for k, _ in kept]
        if len(set(names)) != len(names) or any(k in self._blocks for k in names):
            raise ValueError("BlockStore.put: a block is already in the store (%s)"
                             % ([k for k in names if k in self._blocks or names.count(k) > 1][:4],))
        for k, b in kept:
            self._blocks[k] = data[b].copy()
        self.n_put += len(kept)
        self.n_dropped += len(keys) - len(kept)
        return len(kept)

    def get(self, keys):
        """(found [m,3] int64, data [m,planes,8,8,8] fp32): the blocks of `keys` the store holds, in `keys`' order, copied."""
        found = [k for k in map(tuple, _block_keys(keys).tolist()) if k in self._blocks]
        data = np.empty((len(found),) + self._shape(), np.float32)
        for b, k in enumerate(found):
            data[b] = self._blocks[k]
        return np.asarray(found, dtype=np.int64).reshape(-1, 3), data

    def take(self, keys):
        """`get`, and the blocks it returns leave the store."""
        found, data = self.get(keys)
        for k in map(tuple, found.tolist()):
            del self._blocks[k]
        self.n_taken += len(found)
        return found, data

    def keys(self):
        """The block indices held, as a sorted list of (bx, by, bz)."""
        return sorted(self._blocks)

    def __len__(self):
        return len(self._blocks)

    def __contains__(self, key):
        return tuple(int(v) for v in key) in self._blocks

    @property
    def nbytes(self):
        return len(self._blocks) * self.planes * self.block ** 3 * 4

    def bounds(self):
        """((bx0, by0, bz0), (bx1, by1, bz1)): the half-open box of block indices held; None for an empty store."""
        if not self._blocks:
            return None
        k = np.asarray(list(self._blocks), dtype=np.int64)
        return tuple(int(v) for v in k.min(axis=0)), tuple(int(v) + 1 for v in k.max(axis=0))

    def clear(self):
        self._blocks.clear()

    def save(self, path):
        """One .npz: the keys [n,3] int64 in sorted order, the blocks [n,planes,8,8,8] as their int32 bit patterns, planes and the
        block width.  `load` gives every word back bit for bit (NaN payloads included)."""
        found, data = self.get(self.keys())
        with open(path, "wb") as f:
            np.savez(f, keys=found, bits=data.view(np.int32), planes=np.int64(self.planes), block=np.int64(self.block))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            out = cls(int(z["planes"]), int(z["block"]))
            out.put(z["keys"], np.ascontiguousarray(z["bits"]).view(np.float32))
        out.n_put = 0                                               # the counters count paging, not loading
        return out


def _window_blocks(offset, dims):
    """The world block indices of the window [offset, offset + dims) — both multiples of 8 —: (lo [3], hi [3]) half-open."""
    lo = np.asarray(offset, dtype=np.int64) // BLOCK
    return lo, lo + np.asarray(dims, dtype=np.int64) // BLOCK


def _box_keys(lo, hi):
    """Every block index of the half-open box, [n,3] int64 in ascending (z, y, x) order."""
    if any(h <= l for l, h in zip(lo, hi)):
        return np.zeros((0, 3), np.int64)
    z, y, x = np.meshgrid(*(np.arange(lo[k], hi[k], dtype=np.int64) for k in (2, 1, 0)), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


def _outside(keys, lo, hi):
    """The rows of keys [n,3] that do not lie in the half-open box."""
    return keys[~((keys >= lo) & (keys < hi)).all(axis=1)]


def _in_calls(entry, buf, origins, blocks, *flags):
    """ops.tsdf_blocks_gather / _scatter over any number of blocks: calls of at most NRGBD_TSDF_MAX_BLOCKS."""
    for at in range(0, len(origins), ops.TSDF_MAX_BLOCKS):
        part = slice(at, min(len(origins), at + ops.TSDF_MAX_BLOCKS))
        entry(buf, origins[part], blocks[part], *(f[part] for f in flags))


class _Staging:
    """Device staging for paged blocks — [capacity,planes,8,8,8] fp32 and the int32 flags —, allocated once and grown only when a
    call needs more; on a GPU also the pinned host mirror the blocks are read back through."""

    def __init__(self, planes, device):
        self.planes, self.device = planes, device
        self.blocks = self.flags = self._host = None

    def need(self, n):
        if self.blocks is None or self.blocks.shape[0] < n:
            self.blocks = torch.empty((n, self.planes) + (BLOCK,) * 3, dtype=torch.float32, device=self.device)
            self.flags = torch.empty(n, dtype=torch.int32, device=self.device)
            self._host = None
        return self.blocks, self.flags

    def to_host(self, n):
        """(blocks [n,...], flags [n]) as numpy arrays, views of buffers the next call overwrites; the one synchronisation."""
        if self.device.type != "cuda":
            return self.blocks[:n].numpy(), self.flags[:n].numpy()
        if self._host is None:
            self._host = (torch.empty(self.blocks.shape, dtype=torch.float32, pin_memory=True),
                          torch.empty(self.flags.shape, dtype=torch.int32, pin_memory=True))
        for h, d in zip(self._host, (self.blocks, self.flags)):
            h[:n].copy_(d[:n], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self._host[0][:n].numpy(), self._host[1][:n].numpy()


class TSDFVolume:
    """A dense TSDF volume on the device: `tsdf` and `weight`, fp32 [Z,Y,X]; lattice point (ix, iy, iz) lies at
    origin + voxel_size (ix, iy, iz).  color=True: also `color`, fp32 [3,Z,Y,X] (r, g, b), the running average of the colours of
    exactly the observations that updated a voxel's distance, with the same weights (one buffer [5,Z,Y,X] holds all of it)."""

    def __init__(self, dims, voxel_size, origin, trunc=None, w_max=64., device=None, color=False):
        self.dims = tuple(int(n) for n in dims)
        if len(self.dims) != 3 or min(self.dims) <= 0 or self.dims[0] * self.dims[1] * self.dims[2] > 2 ** 31:
            raise ValueError("TSDFVolume: dims = (X, Y, Z), positive, at most 2^31 voxels; got %s" % (dims,))
        self.voxel_size = float(voxel_size)
        self.origin = tuple(float(o) for o in origin)
        self.trunc = 3.0 * self.voxel_size if trunc is None else float(trunc)
        self.w_max = float(w_max)
        if len(self.origin) != 3 or not all(math.isfinite(o) for o in self.origin):
            raise ValueError("TSDFVolume: origin takes three finite values, got %s" % (origin,))
        for v, nm in ((self.voxel_size, "voxel_size"), (self.trunc, "trunc"), (self.w_max, "w_max")):
            if not (v > 0 and math.isfinite(v)):
                raise ValueError("TSDFVolume: %s must be positive and finite, got %s" % (nm, v))
        X, Y, Z = self.dims
        self._buf = torch.zeros((5 if color else 2, Z, Y, X), dtype=torch.float32,
                                device=torch.device(device if device is not None else "cuda"))
        self.device = self._buf.device                              # with its index: "cuda" names the current device
        self._origin0 = self.origin                                 # the construction origin: `origin` is always formed from it
        self.offset = (0, 0, 0)                                     # the cumulative shift in voxels (shift)
        self._spare = None                                          # the second buffer, allocated at the first shift
        self._generation = 0                                        # counts the shifts: a spill volume is valid for one
        self._parent = None                                         # a spill volume: (the volume it came from, its generation then)
        self._page_out = self._page_in = None                       # block staging, allocated at the first shift with a store
        self._page_scratch = None                                   # paged_extract's tile volume, allocated at its first call
        self._point(self._buf)
        self._scratch()

    def _point(self, buf):
        self._buf = buf
        self.tsdf, self.weight = buf[0], buf[1]
        self.color = buf[2:5] if buf.shape[0] == 5 else None

    def _scratch(self):
        self._counts = torch.zeros(2, dtype=torch.int64, device=self.device)
        self._workspace = None
        self._mesh_counts = self._mesh_workspace = None
        self._trackers = {}

    def _live(self, who):
        """The one check of a spill volume's validity: its buffer is the parent's spare, which the parent's next shift overwrites."""
        if self._parent is not None and self._parent[0]._generation != self._parent[1]:
            raise ValueError("TSDFVolume.%s: this spill volume is stale — the volume it came from has shifted again and reused its "
                             "buffer (extract a spill before the next shift)" % who)

    def reset(self):
        """An empty volume again (asynchronous); `offset` and `origin` stay where the shifts have put them."""
        self._live("reset")
        self._buf.zero_()

    def shift(self, voxels, spill=False, store=None):
        """The volume moved by voxels = (sx, sy, sz) whole voxels, one launch (ops.tsdf_shift): `offset` grows by it, `origin` becomes
        origin0 + voxel_size * offset (formed in float64 from the construction origin: rounding does not accumulate over many
        shifts), the voxels that stay keep their bits at their new indices, the region that enters is empty, and what leaves is gone
        — or, with spill=True, returned: a TSDFVolume at the OLD origin (the same voxel size, trunc, w_max and colour) that holds the
        leaving voxels and a one-voxel rim of the retained ones on the faces that face the motion, everything else at weight 0, so
        that its mesh() is exactly the old mesh's triangles with a corner that left and the live volume's mesh the rest: no gap, no
        duplicate.  points(), mesh() and raycast() work on it unchanged.  It is a view of this volume's other buffer, not a copy:
        valid until this volume's next shift, after which its methods raise ValueError.
        The volume keeps two buffers of the same shape and the launch copies from one into the other, then they swap roles: the
        second is allocated at the first shift (the one allocation; a volume that is never shifted never has it).  `tsdf`, `weight`
        and `color` are re-pointed: tensors fetched from these attributes BEFORE a shift are the spill buffer afterwards.
        A zero shift launches nothing and returns None; without spill the result is None.  Synchronises nothing.
        store=BlockStore: the shift is paged.  The volume is seen as 8^3 voxel blocks; the world index of the block at grid voxel o
        is (offset + o) / 8, on the construction lattice, so every dimension, every component of `voxels` and `offset` must be
        multiples of 8, the store's planes the volume's, and spill False (ValueError otherwise).  After the shift launch — the same
        launch, the old buffer intact — the blocks of the old window that are not in the new one are gathered out of the old
        buffer (ops.tsdf_blocks_gather; the set difference of block indices is formed on the host, which also covers a shift past
        the whole grid), whatever the store holds of the blocks of the new window that were not in the old one is taken from it
        and scattered into the new buffer (ops.tsdf_blocks_scatter), and the gathered blocks and their flags are copied to the host
        and `put`: a block that holds nothing but +0.0 is dropped, as an entering region is +0.0 anyway.  Everything runs on the
        current stream; the read-back synchronises once per shift, as the mesh spill does.  The staging tensors are allocated at
        the first such shift and grown only when a larger one needs it.  Returns None.  What the live window and the store hold
        together is then, bit for bit, what an unbounded static volume would hold, as long as no frame updates voxels outside
        the window."""
        self._live("shift")
        try:
            s = tuple(int(v) for v in voxels)
            whole = len(s) == 3 and all(v == w for v, w in zip(s, voxels))
        except (TypeError, ValueError):
            whole = False
        if not whole:
            raise ValueError("TSDFVolume.shift: voxels = (sx, sy, sz), whole voxels; got %r" % (voxels,))
        if store is not None:
            self._paged("shift", store)
            if spill:
                raise ValueError("TSDFVolume.shift: spill=True hands the leaving part out as a volume, store= keeps it as blocks: one of the two")
            if any(v % BLOCK for v in s):
                raise ValueError("TSDFVolume.shift: with a store the shift is whole blocks of %d voxels, got %r" % (BLOCK, s))
        if s == (0, 0, 0):
            return None
        if self._spare is None:
            self._spare = torch.empty_like(self._buf)
        ops.tsdf_shift(self._buf, self._spare, s, spill=spill)
        old_buf, old_origin, old_offset = self._buf, self.origin, self.offset
        self._point(self._spare)
        self._spare = old_buf
        self._generation += 1                                       # whatever spill volume viewed the spare is stale from here
        self.offset = tuple(o + v for o, v in zip(self.offset, s))
        self.origin = tuple(o + self.voxel_size * k for o, k in zip(self._origin0, self.offset))       # Python floats: float64
        if store is not None:
            self._page(store, old_buf, old_offset)
        if not spill:
            return None
        out = object.__new__(TSDFVolume)
        out.dims, out.voxel_size, out.trunc, out.w_max, out.device = self.dims, self.voxel_size, self.trunc, self.w_max, self.device
        out.origin = out._origin0 = old_origin
        out.offset, out._spare, out._generation = (0, 0, 0), None, 0
        out._page_out = out._page_in = out._page_scratch = None
        out._parent = (self, self._generation)
        out._point(old_buf)
        out._scratch()
        return out

    def _paged(self, who, store):
        """The conditions of a paged volume: the store's planes, and the window on the block lattice."""
        if not isinstance(store, BlockStore) or store.planes != self._buf.shape[0]:
            raise ValueError("TSDFVolume.%s: store is a BlockStore of %d planes, got %r" % (who, self._buf.shape[0], getattr(
                store, "planes", store)))
        if any(n % BLOCK for n in self.dims) or any(o % BLOCK for o in self.offset):
            raise ValueError("TSDFVolume.%s: a paged volume's dims %s and offset %s are multiples of %d voxels"
                             % (who, self.dims, self.offset, BLOCK))

    def _page(self, store, old_buf, old_offset):
        """After a shift's launch: the blocks that left, out of the old buffer into `store`; the blocks that entered, out of it."""
        old_lo, old_hi = _window_blocks(old_offset, self.dims)
        new_lo, new_hi = _window_blocks(self.offset, self.dims)
        leaving = _outside(_box_keys(old_lo, old_hi), new_lo, new_hi)
        entering = _outside(_box_keys(new_lo, new_hi), old_lo, old_hi)
        if self._page_out is None:
            self._page_out, self._page_in = _Staging(self._buf.shape[0], self.device), _Staging(self._buf.shape[0], self.device)
        blocks, flags = self._page_out.need(len(leaving))
        _in_calls(ops.tsdf_blocks_gather, old_buf, leaving * BLOCK - np.asarray(old_offset, np.int64), blocks, flags)
        found, data = store.take(entering)
        if len(found):
            staged = self._page_in.need(len(found))[0]
            staged[:len(found)].copy_(torch.from_numpy(data))
            _in_calls(ops.tsdf_blocks_scatter, self._buf, found * BLOCK - np.asarray(self.offset, np.int64), staged)
        store.put(leaving, *self._page_out.to_host(len(leaving)))

    def _frame(self, who, depth, intrinsics, gate, gate_thr, weight, color, color_intrinsics, color_affine):
        """What integrate, deintegrate and reintegrate check and prepare alike: -> (depth [H,W], gate, weight, (fx, fy, cx, cy),
        the colour intrinsics or None)."""
        who = "TSDFVolume." + who
        if (color is None) != (self.color is None):
            raise ValueError("%s: a colour volume is integrated with a colour image (the weight is shared), a volume "
                             "without colour without one" % who)
        if color is None and (color_intrinsics is not None or color_affine is not None):
            raise ValueError("%s: color_intrinsics / color_affine come with color" % who)
        if color is not None:
            if not isinstance(color, torch.Tensor) or color.dtype != torch.float32:
                raise TypeError("%s: color is an fp32 tensor [3,Hc,Wc]" % who)
            if color.dim() != 3 or color.shape[0] != 3 or color.shape[1] < 1 or color.shape[2] < 1:
                raise ValueError("%s: color is [3,Hc,Wc], got %s" % (who, tuple(color.shape),))
            if color.device != self.device or not color.is_contiguous():
                raise ValueError("%s: color must be contiguous and on %s" % (who, self.device,))
        if depth.dim() == 3 and depth.shape[0] == 1:
            depth = depth[0]
            gate = gate if gate is None else gate.view(depth.shape)
            weight = weight if weight is None else weight.view(depth.shape)
        if depth.dim() != 2:
            raise ValueError("%s: depth is [H,W], got %s" % (who, tuple(depth.shape),))
        H, W = depth.shape
        if color is not None and color_intrinsics is None:
            if isinstance(intrinsics, dict):
                color_intrinsics = intrinsics_at(intrinsics, color.shape[1], color.shape[2])
            elif tuple(color.shape[1:]) != (H, W):
                raise ValueError("%s: a %d x %d colour image beside a %d x %d depth map needs color_intrinsics"
                                 % (who, color.shape[1], color.shape[2], H, W))
        if isinstance(color_intrinsics, dict):
            color_intrinsics = intrinsics_at(color_intrinsics, color.shape[1], color.shape[2])
        if isinstance(intrinsics, dict):
            intrinsics = intrinsics_at(intrinsics, H, W)
        if color is not None and color_intrinsics is None:
            color_intrinsics = intrinsics
        if (gate is None) != (gate_thr is None):
            raise ValueError("%s: gate and gate_thr come together" % who)
        return depth, gate, weight, intrinsics, color_intrinsics

    def integrate(self, depth, extM, intrinsics, gate=None, gate_thr=None, weight=None, depth_range=(0., float("inf")), cull=True,
                  color=None, color_intrinsics=None, color_affine=None):
        """One depth frame: depth [H,W] (or [1,H,W]) CUDA fp32 z-depth in metres; extM: the host [4,4] world -> camera matrix
        (VideoDepthStream.push's), used as float32(extM[:3,:4]); intrinsics: (fx, fy, cx, cy) at the map's size, or a cam_intrinsics
        dict (intrinsics_at); gate / gate_thr: a pixel counts where gate >= gate_thr; weight: a per-pixel weight map (default 1);
        depth_range = (d_near, d_far]; cull: launch over frustum_box alone (the same bits).  Returns False when the box is empty and
        nothing was launched.  Allocates nothing and synchronises nothing.
        A colour volume takes color: the frame's picture, CUDA fp32 [3,Hc,Wc] at any size (a volume without colour refuses one; a
        colour volume refuses a frame without: the shared weight would go out of step with the colour); color_intrinsics:
        (fx, fy, cx, cy) at that size — by default intrinsics_at when `intrinsics` is a dict, or the depth map's when the sizes are
        equal; color_affine = (a [3], b [3]): a pixel's colour is image * a + b per channel (default a = 1, b = 0)."""
        return self._launch("integrate", depth, None, extM, intrinsics, gate, gate_thr, weight, depth_range, cull, color, color_intrinsics,
                            color_affine, None)

    def _launch(self, who, depth, extM_old, extM_new, intrinsics, gate, gate_thr, weight, depth_range, cull, color, color_intrinsics,
                color_affine, w_floor):
        """The one launch behind integrate (extM_old None: add only), deintegrate (extM_new None: remove only) and reintegrate:
        _frame's checks, the frustum box — the hull of the boxes — of the poses given, and the entry."""
        depth, gate, weight, intrinsics, color_intrinsics = self._frame(who, depth, intrinsics, gate, gate_thr, weight, color,
                                                                        color_intrinsics, color_affine)
        self._live(who)
        removes = extM_old is not None                              # without a pose to remove, the pose to add is required
        old = _host_matrix(extM_old, "TSDFVolume." + who) if removes else None
        new = _host_matrix(extM_new, "TSDFVolume." + who) if extM_new is not None or not removes else None
        kw = dict(depth_range=depth_range, w_max=self.w_max, gate=gate, gate_thr=0.0 if gate_thr is None else gate_thr, wmap=weight, box=None)
        if cull:                                                    # the hull of the boxes: culling is conservative, the same bits
            boxes = [b for b in (frustum_box(m, intrinsics, tuple(depth.shape), float(depth_range[1]) + self.trunc, self)
                                 for m in (old, new) if m is not None) if b is not None]
            if not boxes:
                return False
            kw["box"] = tuple(min(b[k] for b in boxes) for k in range(3)) + tuple(max(b[k] for b in boxes) for k in range(3, 6))
        if removes:
            kw.update(pose_add=new, w_floor=w_floor)
        entry = "tsdf_reintegrate" if removes else "tsdf_integrate"
        planes, colour = (self.tsdf, self.weight), ()
        if color is not None:
            entry, planes, colour = entry + "_color", planes + (self.color,), (color, color_intrinsics, color_affine)
        getattr(ops, entry)(*planes, self.origin, self.voxel_size, depth, old if removes else new, intrinsics, self.trunc, *colour, **kw)
        return True

    def deintegrate(self, depth, extM, intrinsics, gate=None, gate_thr=None, weight=None, depth_range=(0., float("inf")), cull=True,
                    color=None, color_intrinsics=None, color_affine=None, w_floor=1e-3):
        """A frame that `integrate` fused taken out of the volume again, one launch (ops.tsdf_reintegrate): the arguments are
        integrate's — pass what the frame was integrated with — and w_floor >= 0: a voxel whose weight does not stay above it is
        fresh again (0, 0, and colour 0).  An inverse on voxels whose weight never reached w_max; up to rounding, which a voxel whose
        only observation this was does not see: it comes out exactly empty.  Returns False when the frustum box is empty and nothing
        was launched.  Allocates nothing and synchronises nothing."""
        return self._launch("deintegrate", depth, extM, None, intrinsics, gate, gate_thr, weight, depth_range, cull, color,
                            color_intrinsics, color_affine, w_floor)

    def reintegrate(self, depth, extM_old, extM_new, intrinsics, gate=None, gate_thr=None, weight=None, depth_range=(0., float("inf")),
                    cull=True, color=None, color_intrinsics=None, color_affine=None, w_floor=1e-3):
        """A fused frame moved from extM_old to extM_new — what a pose correction needs: deintegrate(extM_old) and integrate(extM_new)
        in ONE launch over the hull of the two frustum boxes, bit for bit what the two calls give, with every plane read and written
        once.  An empty box leaves the other; returns False when both are empty and nothing was launched.  Allocates nothing and
        synchronises nothing."""
        if extM_new is None:
            raise ValueError("TSDFVolume.reintegrate: extM_new is the pose to put the frame back at (deintegrate takes it out alone)")
        return self._launch("reintegrate", depth, extM_old, extM_new, intrinsics, gate, gate_thr, weight, depth_range, cull, color,
                            color_intrinsics, color_affine, w_floor)

    def _need_color(self, who):
        if self.color is None:
            raise ValueError("TSDFVolume.%s: the volume has no colour (TSDFVolume(..., color=True))" % who)
        return self.color

    def points(self, w_min=1., capacity=None, colors=False):
        """The zero crossings between lattice neighbours whose weights are >= w_min, as ([n,3] CUDA fp32 world points in ascending
        (linear voxel index, axis) order, crossings found).  capacity=None: counts first, then writes every point; else the first
        min(found, capacity).  colors=True (a colour volume): (points, colors [n,3] CUDA fp32 — row p the colour of point p, the
        two voxels' colours interpolated at the crossing —, found).  Reads the count back: the one place this object synchronises
        (and allocates)."""
        color = self._need_color("points") if colors else None
        self._live("points")
        if self._workspace is None:
            self._workspace = torch.empty(ops.tsdf_extract_workspace(*self.dims) // 8, dtype=torch.int64, device=self.device)
        args = (self.tsdf, self.weight, self.origin, self.voxel_size, w_min, self._workspace)
        if capacity is None:
            ops.tsdf_extract_points(*args, None, self._counts)
            capacity = int(self._counts[0].item())
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError("TSDFVolume.points: capacity %d" % capacity)
        out = torch.empty((capacity, 3), dtype=torch.float32, device=self.device)
        rgb = torch.empty_like(out) if colors else None
        ops.tsdf_extract_points(*args, out if capacity else None, self._counts, color=color, colors=rgb if capacity else None)
        found, written = (int(v) for v in self._counts.cpu())
        return (out[:written],) + ((rgb[:written],) if colors else ()) + (found,)

    def mesh(self, w_min=1., capacity=None, colors=False):
        """The surface as an indexed triangle mesh: (vertices [n,3] CUDA fp32, faces [m,3] CUDA int32, (vertices found, triangles
        found)).  The vertices are exactly `points(w_min)` in its order; a cell whose eight corners all have weight >= w_min and
        |T| < 1 emits the triangles of its sign case (at most 5, the normal towards free space, ascending cell order); a face holds
        the rows of its vertices in the FULL vertex sequence, whatever the vertex capacity.  capacity=None: counts first, then
        writes everything; capacity=(nv, nf): the first min(found, capacity) rows of either.  colors=True (a colour volume):
        (vertices, faces, colors [n,3] CUDA fp32 — row p the colour of vertex p —, (vertices found, triangles found)).  Reads the
        counts back: like `points`, the one place this object synchronises (and allocates)."""
        color = self._need_color("mesh") if colors else None
        self._live("mesh")
        if self._mesh_workspace is None:
            self._mesh_workspace = torch.empty((ops.tsdf_mesh_workspace(*self.dims) + 7) // 8, dtype=torch.int64, device=self.device)
            self._mesh_counts = torch.zeros(4, dtype=torch.int64, device=self.device)
        args = (self.tsdf, self.weight, self.origin, self.voxel_size, w_min, self._mesh_workspace)
        if capacity is None:
            ops.tsdf_extract_mesh(*args, None, None, self._mesh_counts)
            found = self._mesh_counts.cpu()
            capacity = (int(found[0]), int(found[2]))
        nv, nf = (int(c) for c in capacity)
        if nv < 0 or nf < 0:
            raise ValueError("TSDFVolume.mesh: capacity %s" % (capacity,))
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=self.device)
        faces = torch.empty((nf, 3), dtype=torch.int32, device=self.device)
        rgb = torch.empty_like(vertices) if colors else None
        ops.tsdf_extract_mesh(*args, vertices if nv else None, faces if nf else None, self._mesh_counts, color=color,
                              colors=rgb if nv else None)
        v_found, v_written, f_found, f_written = (int(v) for v in self._mesh_counts.cpu())
        return (vertices[:v_written], faces[:f_written]) + ((rgb[:v_written],) if colors else ()) + ((v_found, f_found),)

    def raycast(self, extM, intrinsics, size, depth_range=(0., float("inf")), w_min=1., step=None, normals=False, out=None, color=False):
        """The volume seen from a camera at extM (host [3,4] or [4,4] world -> camera), one launch (ops.tsdf_raycast): z-depth [H,W] of
        the surface along every pixel's ray, 0 where there is none, and with normals=True (depth, normal [3,H,W]) with the unit normals
        in the camera frame.  intrinsics: (fx, fy, cx, cy) at size = (H, W), or a cam_intrinsics dict (intrinsics_at); depth_range: the
        z-depths searched; w_min: a sample counts where the eight weights around it reach it; step: the sample distance along the ray
        in metres (default voxel_size; above trunc a ray could step over the band); out: tensors to write into (then nothing is
        allocated).  color=True (a colour volume): rgb [3,H,W], the trilinear colour at every hit and (0, 0, 0) where there is none,
        as one more element of the result: (depth, rgb) or (depth, normal, rgb); `out` then takes the same tuple.  Synchronises
        nothing."""
        planes = self._need_color("raycast") if color else None
        self._live("raycast")
        H, W = (int(n) for n in size)
        if isinstance(intrinsics, dict):
            intrinsics = intrinsics_at(intrinsics, H, W)
        m = _host_matrix(extM, "TSDFVolume.raycast")
        if not np.isfinite(m[:3, :4]).all():
            raise ValueError("TSDFVolume.raycast: the pose is not finite")
        step = self.voxel_size if step is None else float(step)
        if not 0 < step <= self.trunc:
            raise ValueError("TSDFVolume.raycast: step %s is not in (0, trunc = %s]: a ray could step over the band" % (step, self.trunc))
        return ops.tsdf_raycast(self.tsdf, self.weight, self.origin, self.voxel_size, m, intrinsics, (H, W), depth_range, w_min=w_min,
                                step=step, normals=normals, out=out, color=planes, rgb=bool(color))

    def track(self, depth, extM_guess, intrinsics, levels=None, image=None, **kw):
        """The pose of a depth frame registered against the volume, from a guess: tracking.FrameTracker(self, depth's size,
        intrinsics, levels, photo).track(depth, extM_guess, image=image, **kw) with photo = an image was given; the tracker is built
        once per (size, intrinsics, levels, photo) and kept — the second call with a size allocates nothing.  image=[3,H,W] (a colour
        volume): the frame's picture, for the photometric term (image_affine, photo_weight, photo_huber go with it in kw).  Returns a
        tracking.TrackResult (extM, ok, flag, log, delta).  Synchronises once, at the end."""
        from .tracking import DEFAULT_LEVELS, FrameTracker
        levels = DEFAULT_LEVELS if levels is None else tuple((int(s), int(n)) for s, n in levels)
        size = tuple(int(n) for n in depth.shape[-2:])
        K = intrinsics_at(intrinsics, *size) if isinstance(intrinsics, dict) else tuple(float(k) for k in intrinsics)
        photo = image is not None
        key = (size, K, levels, photo)
        if key not in self._trackers:
            self._trackers[key] = FrameTracker(self, size, intrinsics, levels, photo=photo)
        return self._trackers[key].track(depth, extM_guess, image=image, **kw)


def to_uint8(rgb):
    """fp32 colours in [0, 1] (a tensor on any device, or an array) -> uint8 of the same shape and kind: rint(clip(c, 0, 1) * 255),
    ties to even; a NaN becomes 0."""
    if isinstance(rgb, torch.Tensor):
        return torch.nan_to_num(rgb, nan=0.0).clamp(0., 1.).mul(255.).round().to(torch.uint8)
    c = np.asarray(rgb, dtype=np.float32)
    return np.rint(np.clip(np.where(np.isnan(c), np.float32(0), c), 0., 1.) * np.float32(255.)).astype(np.uint8)


def shade(normal):
    """[3,H,W] camera-frame normals (TSDFVolume.raycast(normals=True)) -> a uint8 [H,W] Lambert image with the light along the view
    direction: 255 * max(0, -n_z), 0 where there is no surface."""
    if isinstance(normal, torch.Tensor):
        return (-normal[2]).clamp(0., 1.).mul(255.).round().to(torch.uint8)
    return np.rint(np.clip(-np.asarray(normal)[2], 0., 1.) * 255.).astype(np.uint8)


def relative_poses(pose, poses):
    """float32 [n,3,4]: (T_s T_ref^-1)[:3] for every world -> camera pose T_s of `poses`, with T_ref = pose — the motions reference
    camera -> source camera ops.depth_consistency takes —, formed in float64 on the host and rounded once."""
    inv = np.linalg.inv(_host4(pose, "relative_poses"))
    return np.stack([(_host4(m, "relative_poses") @ inv)[:3] for m in poses]).astype(np.float32)


def _host4(extM, who):
    m = _host_matrix(extM, who)
    return m if m.shape == (4, 4) else np.vstack([m, [0.0, 0.0, 0.0, 1.0]])


def filter_depth(depth, pose, sources, poses, intrinsics, rel=0.01, min_views=1, depth_range=(0., float("inf")), gate=None, gate_thr=None,
                 source_gates=None, votes=None, out=None):
    """A depth map cross-checked against other views' maps, for a caller with a loop of its own (no TSDFVolume, no stream): one launch
    (ops.depth_consistency).  depth [H,W] CUDA fp32 at the host world -> camera pose `pose`; sources: the other views' maps at the
    same size and intrinsics, a CUDA fp32 tensor [S,H,W] (read where it lies) or a sequence of [H,W] maps (stacked here), at most
    NRGBD_CONSISTENCY_MAX_SRC, with their world -> camera `poses`; intrinsics: (fx, fy, cx, cy) at the maps' size or a
    cam_intrinsics dict (intrinsics_at); a source agrees with a pixel where |ds - q_z| <= rel q_z (a parameter, not a measurement);
    gate / gate_thr with source_gates (a stack or a sequence like `sources`): a pixel of either side counts where its gate >=
    gate_thr; depth_range = (d_near, d_far] alike.  Returns (filtered, votes): the map with every pixel that fails its own tests or
    that fewer than min_views sources agree with set to 0 — what to hand to TSDFVolume.integrate or track without a gate —, and
    the agreeing views per pixel (-1: the pixel failed its own tests).  votes / out: tensors to write into (out may be `depth`).
    Synchronises nothing."""
    if depth.dim() == 3 and depth.shape[0] == 1:
        depth = depth[0]
        gate = gate if gate is None else gate.view(depth.shape)
    if (gate is None) != (gate_thr is None) or (len(sources) > 0 and (gate is None) != (source_gates is None)):
        raise ValueError("filter_depth: gate, gate_thr and source_gates come together")
    stack = lambda maps: maps if isinstance(maps, torch.Tensor) else torch.stack([m.view(depth.shape) for m in maps])
    src = dict(src_depth=None, src_T=None)
    if len(sources) > 0:
        if len(poses) != len(sources):
            raise ValueError("filter_depth: %d sources with %d poses" % (len(sources), len(poses)))
        src = dict(src_depth=stack(sources), src_gate=None if source_gates is None else stack(source_gates),
                   src_T=relative_poses(pose, poses))
    if isinstance(intrinsics, dict):
        intrinsics = intrinsics_at(intrinsics, *depth.shape)
    got = ops.depth_consistency(depth, intrinsics, rel_thr=rel, min_views=min_views, depth_range=depth_range, gate=gate,
                                gate_thr=0.0 if gate_thr is None else gate_thr, votes=votes, depth_out=out, **src)
    return got[1], got[0]


def paged_extract(volume, store, what="mesh", w_min=1., colors=False):
    """The whole world of a paged volume — the live window and what `store` holds — as one mesh or point set on the host:
    (vertices [n,3] fp32, faces [m,3] int32[, colors [n,3] fp32]) for what='mesh', (points [n,3] fp32[, colors]) for 'points', numpy
    arrays.  The world's voxel bounds — the window and the store's blocks — are cut into tiles of volume.dims voxels whose origins
    are dims - 1 apart, so that every mesh cell (eight neighbouring voxels) lies in exactly one tile; the tiles are visited in
    ascending (z, y, x) order.  A tile is assembled in one scratch TSDFVolume of the volume's shape (allocated at the first call,
    zeroed per tile): the store's blocks that touch it go host -> staging, the live window's by ops.tsdf_blocks_gather from the live
    buffer, and one ops.tsdf_blocks_scatter writes both — tile origins are not block-aligned, so the blocks are clipped at the tile's
    faces.  The tile is then extracted with TSDFVolume.mesh / points at w_min, and the parts are concatenated with each part's face
    rows offset by the vertices before it, as FusionVideoStream.world_mesh does for chunks.  A tile that no block touches is
    skipped.  The vertices on a face two tiles share exist in both, each part being a mesh of its own; a point set holds such a
    crossing twice.  A vertex is origin + voxel_size (i + q) with the TILE's origin and index: the same surface comes out within a
    few ulp of, not bit for bit as, one large volume's.  Neither the store nor the live volume is modified.  Synchronises (every
    extraction reads its counts back)."""
    if what not in ("mesh", "points"):
        raise ValueError("paged_extract: what is 'mesh' or 'points', got %r" % (what,))
    volume._live("paged_extract")
    volume._paged("paged_extract", store)
    dims, offset = np.asarray(volume.dims, np.int64), np.asarray(volume.offset, np.int64)
    live_lo, live_hi = _window_blocks(offset, dims)
    lo, hi = offset, offset + dims
    if len(store):
        b = store.bounds()
        lo, hi = np.minimum(lo, np.asarray(b[0]) * BLOCK), np.maximum(hi, np.asarray(b[1]) * BLOCK)
    if volume._page_scratch is None:
        volume._page_scratch = (TSDFVolume(volume.dims, volume.voxel_size, volume.origin, trunc=volume.trunc, w_max=volume.w_max,
                                           device=volume.device, color=volume.color is not None),
                                _Staging(volume._buf.shape[0], volume.device))
    tile, staging = volume._page_scratch
    starts = [list(range(int(lo[k]), max(int(hi[k]) - 1, int(lo[k]) + 1), max(int(dims[k]) - 1, 1))) for k in range(3)]
    parts = []
    for tz in starts[2]:
        for ty in starts[1]:
            for tx in starts[0]:
                t = np.array([tx, ty, tz], np.int64)
                keys = _box_keys(t // BLOCK, (t + dims - 1) // BLOCK + 1)
                live = keys[((keys >= live_lo) & (keys < live_hi)).all(axis=1)]
                found, data = store.get(_outside(keys, live_lo, live_hi))
                n = len(live) + len(found)
                if n == 0:
                    continue
                blocks = staging.need(n)[0]
                if len(live):
                    _in_calls(ops.tsdf_blocks_gather, volume._buf, live * BLOCK - offset, blocks[:len(live)], staging.flags[:len(live)])
                if len(found):
                    blocks[len(live):n].copy_(torch.from_numpy(data))
                tile.offset = tuple(int(v) for v in t)
                tile.origin = tuple(o + volume.voxel_size * int(k) for o, k in zip(volume._origin0, t))    # as shift forms it
                tile.reset()
                _in_calls(ops.tsdf_blocks_scatter, tile._buf, np.concatenate([live, found]) * BLOCK - t, blocks[:n])
                got = (tile.mesh if what == "mesh" else tile.points)(w_min=w_min, colors=colors)[:-1]
                parts.append(tuple(a.cpu().numpy() for a in got))
    empty = (np.zeros((0, 3), np.float32),) + ((np.zeros((0, 3), np.int32),) if what == "mesh" else ()) + (
        (np.zeros((0, 3), np.float32),) if colors else ())
    if not parts:
        return empty
    out = (np.concatenate([p[0] for p in parts]),)
    if what == "mesh":
        base = np.cumsum([0] + [len(p[0]) for p in parts[:-1]])
        out += (np.concatenate([p[1] + np.int32(b) for p, b in zip(parts, base)]).astype(np.int32),)
    return out + ((np.concatenate([p[-1] for p in parts]),) if colors else ())


class _Frame(typing.NamedTuple):
    """What FusionVideoStream integrates a frame with: built once per frame, rebuilt from the history's slots for a held one."""
    depth: torch.Tensor
    gate: typing.Optional[torch.Tensor]
    gate_thr: typing.Optional[float]
    weight: typing.Optional[torch.Tensor]
    depth_range: tuple
    color: typing.Optional[torch.Tensor]            # the picture, its intrinsics and affine: None without colour
    color_intrinsics: typing.Optional[tuple]
    color_affine: typing.Optional[tuple]

    def fuse_kw(self):
        """The keywords of TSDFVolume.integrate / deintegrate / reintegrate beside the depth map and the poses."""
        kw = self._asdict()
        del kw["depth"]
        return kw

    def track_kw(self, photo):
        """The keywords of TSDFVolume.track; photo: with the picture, for the photometric term."""
        kw = dict(gate=self.gate, gate_thr=self.gate_thr, depth_range=self.depth_range)
        if photo:
            kw.update(image=self.color, image_affine=self.color_affine)
        return kw


class _Held(typing.NamedTuple):
    """A frame of FusionVideoStream's history; a pose correction overwrites `pose` in place."""
    ref_index: int
    pose: np.ndarray                                # float64 [4,4]: where the frame is integrated now
    slot: int                                       # its row of the slot tensors
    shifts: int                                     # n_shifts when it was integrated


class FusionVideoStream(VideoDepthStream):
    """VideoDepthStream + a TSDFVolume: push(frame, extM) returns what VideoDepthStream.push returns, and every depth frame that comes
    out is integrated into `volume` with the extrinsic pushed with its reference frame — one depth-regression launch and one
    integration launch on the caller's HIP stream after the frame (eager: not part of the captured graph).
    source: 'refined' (the R-Net volume at the network size) or 'dpv' (the K-Net volume at the plane-sweep grid);
    conf_threshold c: only pixels with max_k logp >= float32(log c) count (evaluate.log_thresholds' gate);
    weight: 'uniform' (1 per observation) or 'conf' (exp(max_k logp), from ops.export_depth_u16).
    color=True (a colour volume): the frame's own picture is fused with its depth map — read straight from the slot of the frame ring
    the reference frame still occupies, at the network size with intrinsics_at(cam, H, W) (also when source='dpv' puts the depth map at
    the plane-sweep grid), through the affine a = std, b = mean, which undoes the ingest's normalisation: colours in [0, 1].
    The R-Net's volume is read where it lies (its channels-last view) when the candidates fill the kernels' candidate width (64 or
    128 candidates, 256 with if_upsample_d); another count runs zero-padded to that width, the view is then a slice of the padded
    pixels and ops.depth_regress makes a planar copy of it first.
    track=True: frame-to-model tracking (tracking.FrameTracker; track_kwargs go to TSDFVolume.track).  The first depth frame of a
    trajectory is integrated at its pushed pose.  For every later one, with E the pushed extrinsics and T the poses that were
    integrated, the guess is E_i E_prev^-1 T_prev — the pushed relative motion on top of the last integrated pose —, the frame's
    regressed depth map is tracked against the volume from it with the stream's own gate and depth range, and the map is integrated
    at the tracked pose; where the track is lost it is integrated at the guess and `n_track_lost` counts it.  `last_ext` is the pose
    that was integrated (what render() uses), `tracked_poses` keeps (ref_index, extM, ok).  A tracked push synchronises once per depth
    frame (the tracker reads its result back).  The network's own cost volume keeps using the pushed poses: tracking touches only
    where the map is integrated.  With track=False nothing of this is constructed or launched.
    photo=True (with color=True, track=True and source='refined': the depth map is then the ring picture's size): the track also
    carries the photometric term (FrameTracker(photo=True)) — the picture is the reference frame's ring slot and the affine
    (std, mean), what the colour integration already uses.  With photo=False nothing of this is constructed or launched.
    history=N: the stream keeps what the last N integrated frames were integrated with — the regressed depth map, the gate and the
    weight map where it uses them, with color=True a copy of the picture (the ring's slot is overwritten later), in device slots
    allocated once and filled by memory copies, and on the host (ref_index, integrated pose): `history_poses()`.  `repose(ref_index,
    extM)` moves such a frame to a corrected pose (TSDFVolume.reintegrate, one launch) and `retrack(ref_index)` registers it again
    against the model without it; a frame that falls out of the history stays fused for good; reset() clears it.  With history=0
    (the default) nothing of this is constructed or launched.
    consistency=k >= 1 (needs history >= k): every depth map is cross-checked against the held frames before it is used — one launch
    (ops.depth_consistency) with the held frames' RAW regressed maps and gates as sources, their transforms float32((T_s T_ref^-1)[:3])
    formed in float64 on the host from `history_poses()`' current poses (a repose counts) and the pose the frame is about to be
    integrated or tracked from (track=False: the pushed pose; track=True: the guess), at most the newest NRGBD_CONSISTENCY_MAX_SRC of
    them, min_views = min(k, sources), the stream's depth_range and gate.  The filtered map — 0 where the pixel fails its own tests
    or fewer than min_views sources agree — replaces the regressed one for track, integrate and the history's `depth` slot (the slot
    holds what was integrated: repose and retrack stay exact), and with the gate folded into it they take no gate.  The history holds
    one more slot tensor, `raw`, and its `gate` slots are the sources' gates: a later frame is checked against what the network
    regressed, not against what survived, so a newly seen region that was filtered out once can still gain support.  The first frame
    of a trajectory has no sources and is fused as before; after that a region is fused from the k-th time after its first sighting
    on: surfaces enter the volume k frames late, the price of never fusing what no other view confirms.  consistency_rel: a source
    agrees where |ds - q_z| <= consistency_rel q_z; like the tracker's dist_thr a parameter, not a measurement.  `last_votes` is
    the votes map of the last frame (a buffer the next frame overwrites).  With consistency=0 (the default) nothing of this is
    constructed or launched, and the stream's launches and bits are what they were.
    follow=distance (metres): the volume follows the camera.  Before a depth frame is tracked or fused, follow_shift is evaluated
    from the pose the frame is about to be tracked or integrated from (the pose the consistency filter uses) with `distance`,
    follow_margin and follow_step — parameters, not measurements, like the tracker's dist_thr and consistency_rel —, and a non-zero
    result moves the volume (TSDFVolume.shift: one launch; the volume's second buffer is allocated at the first shift).
    follow_spill says what becomes of the part that leaves: 'mesh' (the default) or 'points' — the stream extracts the spill volume
    with w_min = follow_w_min (with colours on a colour stream) and appends the result as host numpy arrays to `chunks`, which
    synchronises once per shift (shifts are rare, and the extraction reads its counts back anyway) —, a callable that is handed the
    spill volume (valid until the next shift), or None: what leaves is dropped and nothing is spilled.  follow_spill='page': nothing
    is extracted and `chunks` stays empty; what leaves is kept as 8^3 voxel blocks in `store` — a BlockStore the stream builds, or
    the one passed as follow_store=, which lets a saved map continue — and what the store holds of the region that enters comes
    back bit for bit (TSDFVolume.shift(store=...): the camera that returns tracks against, and fuses into, the model it left);
    `n_paged_out` and `n_paged_in` count the blocks; `world_mesh()` / `world_points()` are then paged_extract over the live window
    and the store at follow_w_min; follow_step and the volume's dims must be multiples of 8 (refused at construction otherwise);
    reset() keeps the store, as it keeps the chunks.  `n_shifts` counts the shifts;
    `world_mesh()` / `world_points()` return every chunk followed by the live volume's extraction.  reset() keeps the chunks, as
    the volume keeps accumulating across it.  A held frame (history=N) that was integrated before a shift can no longer be taken out
    exactly — the region that entered never held it —: `repose` and `retrack` of such a frame raise ValueError; it still serves as
    a consistency source, which uses only its maps and pose.  With follow=None (the default) nothing of this is constructed,
    allocated or launched, and the stream's launches and bits are what they were."""

    def __init__(self, model, cam_intrinsics, d_candi, volume, t_win_r=2, source="refined", conf_threshold=0., weight="uniform",
                 depth_range=None, color=False, track=False, track_kwargs=None, photo=False, history=0, consistency=0,
                 consistency_rel=0.01, follow=None, follow_margin=0.25, follow_step=8, follow_spill="mesh", follow_w_min=1.,
                 follow_store=None, **video_kwargs):
        from .nets import require_volume_refiner
        require_volume_refiner(model, "FusionVideoStream")
        if source not in ("refined", "dpv"):
            raise ValueError("FusionVideoStream: source is 'refined' or 'dpv', got %r" % (source,))
        if weight not in ("uniform", "conf"):
            raise ValueError("FusionVideoStream: weight is 'uniform' or 'conf', got %r" % (weight,))
        c = float(conf_threshold)
        if not 0 <= c < 1:
            raise ValueError("FusionVideoStream: conf_threshold %s is not in [0, 1)" % (conf_threshold,))
        if bool(color) != (getattr(volume, "color", None) is not None):
            raise ValueError("FusionVideoStream: color=%s takes a volume %s colour (TSDFVolume(..., color=%s))"
                             % (bool(color), "with" if color else "without", bool(color)))
        self.color = bool(color)
        self.volume = volume
        self.source, self.weight_mode, self.conf_threshold = source, weight, c
        self.gate_thr = None if c == 0 else float(np.log(np.float64(c)).astype(np.float32))      # the log in double, rounded once
        self.depth_range = (0., float("inf")) if depth_range is None else (float(depth_range[0]), float(depth_range[1]))
        self.cam, self.d_candi = cam_intrinsics, d_candi
        self.n_slots = 2 * t_win_r + 2
        self.ext_ring = GtRing(self.n_slots)                    # which push's extrinsic a slot holds: evaluate.GtRing's pairing
        self._ext = [None] * self.n_slots
        self.n_integrated = 0
        self.track = bool(track)
        if track_kwargs is not None and not self.track:
            raise ValueError("FusionVideoStream: track_kwargs come with track=True")
        self.track_kwargs = dict(track_kwargs or {})
        self.photo = bool(photo)
        if self.photo and not (self.color and self.track and source == "refined"):
            raise ValueError("FusionVideoStream: photo=True needs color=True, track=True and source='refined' (the depth map at the "
                             "ring picture's size)")
        self.n_track_lost = 0
        self.tracked_poses = []
        self._prev = None                                       # (pushed extrinsic, integrated pose) of the last frame integrated
        self.history = int(history)
        if self.history < 0 or self.history != history:
            raise ValueError("FusionVideoStream: history is a number of frames >= 0, got %r" % (history,))
        self._held = []                                         # _Held records, oldest first
        self._slots = None                                      # the maps of the held frames, allocated at the first one
        self._n_held = 0
        self.consistency = int(consistency)
        if self.consistency < 0 or self.consistency != consistency:
            raise ValueError("FusionVideoStream: consistency is a number of views >= 0, got %r" % (consistency,))
        if self.consistency > self.history:
            raise ValueError("FusionVideoStream: consistency=%d needs history >= %d (the held frames are the sources), got history=%d"
                             % (self.consistency, self.consistency, self.history))
        self.consistency_rel = float(consistency_rel)
        if not (self.consistency_rel > 0 and math.isfinite(self.consistency_rel)):
            raise ValueError("FusionVideoStream: consistency_rel must be positive and finite, got %r" % (consistency_rel,))
        if self.consistency and self.depth_range[0] < 0:
            raise ValueError("FusionVideoStream: consistency writes 0 for a dropped pixel, which depth_range = %s would fuse"
                             % (self.depth_range,))
        self._votes = self._filtered = None                     # the filter's two outputs, allocated at the first frame
        self.last_votes = None
        self.follow = None if follow is None else float(follow)
        self.follow_margin, self.follow_step, self.follow_spill, self.follow_w_min = follow_margin, follow_step, follow_spill, float(follow_w_min)
        if self.follow is not None:
            follow_shift(np.eye(4), volume, self.follow, follow_margin, follow_step)      # the parameter refusals, at construction
            if not (follow_spill is None or follow_spill in ("mesh", "points", "page") or callable(follow_spill)):
                raise ValueError("FusionVideoStream: follow_spill is 'mesh', 'points', 'page', None or a callable, got %r" % (follow_spill,))
        paged = self.follow is not None and follow_spill == "page"
        if follow_store is not None and not paged:
            raise ValueError("FusionVideoStream: follow_store comes with follow=distance and follow_spill='page'")
        self.store = None                                       # follow_spill='page': what left the volume, as blocks on the host
        self.n_paged_out = self.n_paged_in = 0                  # blocks this stream put into the store / took out of it
        if paged:
            if int(follow_step) % BLOCK:
                raise ValueError("FusionVideoStream: follow_spill='page' moves the volume by whole blocks: follow_step is a multiple "
                                 "of %d, got %r" % (BLOCK, follow_step))
            self.store = BlockStore(volume._buf.shape[0]) if follow_store is None else follow_store
            volume._paged("shift", self.store)                  # the planes, and dims and offset on the block lattice
        self.n_shifts = 0
        self.chunks = []                                        # what left the volume, per shift: host arrays (follow_spill)
        super().__init__(model, cam_intrinsics, d_candi, t_win_r=t_win_r, **video_kwargs)
        if _indexed(volume.device) != _indexed(self.device):
            raise ValueError("FusionVideoStream: the volume is on %s, the stream on %s" % (volume.device, self.device))

    def reset(self):
        """New trajectory: drops the frames, the filter state and the extrinsic ring; the volume stays (volume.reset() empties it)."""
        super().reset()
        self.ext_ring.clear()
        self._ext = [None] * self.n_slots
        self.last_ext = None                                    # the extrinsic of the last frame integrated on this trajectory
        self._prev = None
        self.tracked_poses = []
        self._held = []                                         # the history goes with the trajectory (its slots stay allocated)
        self.last_votes = None

    def render(self, extM=None, size=None, normals=False, color=False, **kw):
        """The fused model as a depth map (and normals, and with color=True its colours): TSDFVolume.raycast from extM — by default the extrinsic of the last frame
        that was integrated — at `size` (default: the network's image size) with the stream's intrinsics and, unless given, its
        depth_range.  An eager launch on the caller's stream; the frame ring and the captured graph are not touched."""
        if extM is None:
            extM = self.last_ext
            if extM is None:
                raise ValueError("FusionVideoStream.render: no frame has been integrated yet; pass extM")
        kw.setdefault("depth_range", self.depth_range)
        if color:
            kw["color"] = True
        return self.volume.raycast(extM, self.cam, (self.H, self.W) if size is None else size, normals=normals, **kw)

    def mesh(self, **kw):
        """The fused model as a triangle mesh: TSDFVolume.mesh(**kw) of the stream's volume (colors=True: with vertex colours)."""
        return self.volume.mesh(**kw)

    def _fuse(self, out):
        if out is None:
            return out
        ref_index, refined, dpv = out
        slot = self.ext_ring.lookup(ref_index)
        if slot is None:                                        # a NaN pose: its windows produce no maps, so this does not happen
            return out
        vol = (refined if self.source == "refined" else dpv)[0]
        D = vol.shape[0]
        d_candi = self.d_candi
        if D == 4 * len(d_candi):
            d_candi = misc.d_candi_up4(d_candi)
        elif D != len(d_candi):
            raise ValueError("FusionVideoStream: a volume of %d planes over %d candidates" % (D, len(d_candi)))
        d_dev = warp_homo._d_candi_dev(d_candi, vol.device)
        cl = ops.is_channels_last_view(vol)
        depth, logconf = ops.depth_regress(vol, d_dev, channels_last=cl)
        wmap = ops.export_depth_u16(vol, d_dev, channels_last=cl)[1] if self.weight_mode == "conf" else None
        gate = None if self.gate_thr is None else logconf
        # frame ref_index is at most t_win_r + 1 pushes behind the newest (pipeline=True; flush() included) and the ring holds the
        # last 2 t_win_r + 1 >= t_win_r + 2: its slot still holds its picture, written by an ingest enqueued on this stream
        image = self.ring[ref_index % self.R] if self.color else None
        pose = self._ext[slot]
        tracked = self.track and self._prev is not None
        if tracked:
            pose = pose @ np.linalg.solve(self._prev[0], self._prev[1])        # the guess E_i E_prev^-1 T_prev, float64 on the host
        if self.follow is not None:                             # before the frame is tracked or fused: the volume around its focus
            self._follow(pose)
        raw = None
        if self.consistency:
            raw, depth = depth, self._consistent(depth, gate, pose)
        fr = self._frame(depth, gate, wmap, image)
        if tracked:
            res = self._track(fr, pose)
            self.n_track_lost += 0 if res.ok else 1
            self.tracked_poses.append((ref_index, res.extM, res.ok))
            pose = res.extM                                     # lost: the guess (as the ray casts used it, float32-rounded)
        if self.volume.integrate(fr.depth, pose, self.cam, **fr.fuse_kw()):
            self.n_integrated += 1
            self.last_ext = pose
            if self.track:
                self._prev = (np.asarray(self._ext[slot], dtype=np.float64), np.asarray(pose, dtype=np.float64))
            if self.history:
                self._hold(ref_index, pose, fr, gate, raw)
        return out

    def _frame(self, depth, gate, wmap, image):
        """The record of a frame of this stream from its maps (`gate`: the stream's own, or None) and its picture.  With consistency
        the gate is already folded into `depth` — the filtered map — and the record takes none: the one place that says so."""
        if self.consistency:
            gate = None
        colour = (image, intrinsics_at(self.cam, self.H, self.W), (self.std, self.mean)) if self.color else (None, None, None)
        return _Frame(depth, gate, None if gate is None else self.gate_thr, wmap, self.depth_range, *colour)

    def _track(self, fr, pose, **track_kwargs):
        """The frame registered against the volume from `pose` (with its picture when photo=True): -> tracking.TrackResult."""
        return self.volume.track(fr.depth, pose, self.cam, **fr.track_kw(self.photo), **dict(self.track_kwargs, **track_kwargs))

    def _follow(self, pose):
        """Moves the volume when the focus of `pose` has left its middle (follow_shift), and hands out what leaves."""
        s = follow_shift(pose, self.volume, self.follow, self.follow_margin, self.follow_step)
        if s == (0, 0, 0):
            return
        if self.store is not None:                              # 'page': what leaves goes to the store, what it holds comes back
            before = (self.store.n_put, self.store.n_taken)
            self.volume.shift(s, store=self.store)
            self.n_shifts += 1
            self.n_paged_out += self.store.n_put - before[0]
            self.n_paged_in += self.store.n_taken - before[1]
            return
        spill = self.volume.shift(s, spill=self.follow_spill is not None)
        self.n_shifts += 1
        if callable(self.follow_spill):
            self.follow_spill(spill)
        elif self.follow_spill == "mesh":                       # (vertices, faces[, colors]); reads its counts back: synchronises
            self.chunks.append(self._on_host(spill.mesh))
        elif self.follow_spill == "points":                     # (points[, colors])
            self.chunks.append(self._on_host(spill.points))

    def _on_host(self, extract):
        """A volume's `mesh` or `points` at follow_w_min (with colours on a colour stream) as host arrays, without the counts."""
        return tuple(t.cpu().numpy() for t in extract(w_min=self.follow_w_min, colors=self.color)[:-1])

    def world_mesh(self):
        """Everything fused so far as one mesh on the host (follow_spill='mesh'): every chunk in the order it left, then the live
        volume's mesh(w_min=follow_w_min), concatenated with each part's face rows offset by the vertices before it: (vertices [n,3]
        fp32, faces [m,3] int32[, colors [n,3] fp32 on a colour stream]) as numpy arrays.  The parts partition the model's cells:
        no triangle is missing and none occurs twice; the seam vertices exist in both neighbours, each part being a mesh of its
        own.  Synchronises (the live extraction reads its counts back)."""
        if self.store is not None:
            return paged_extract(self.volume, self.store, "mesh", w_min=self.follow_w_min, colors=self.color)
        if self.follow is not None and self.follow_spill != "mesh":
            raise ValueError("FusionVideoStream.world_mesh: the chunks are meshes only with follow_spill='mesh', got %r" % (self.follow_spill,))
        parts = list(self.chunks) + [self._on_host(self.volume.mesh)]
        base = np.cumsum([0] + [len(p[0]) for p in parts[:-1]])
        out = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] + np.int32(b) for p, b in zip(parts, base)]).astype(np.int32))
        return out + ((np.concatenate([p[2] for p in parts]),) if self.color else ())

    def world_points(self):
        """The same for points: every chunk's points (a mesh chunk's vertices ARE its points), then the live volume's
        points(w_min=follow_w_min): (points [n,3] fp32[, colors [n,3] fp32]) as numpy arrays.  A crossing between two rim voxels
        occurs in the chunk and in what follows it."""
        if self.store is not None:
            return paged_extract(self.volume, self.store, "points", w_min=self.follow_w_min, colors=self.color)
        if self.follow is not None and self.follow_spill not in ("mesh", "points"):
            raise ValueError("FusionVideoStream.world_points: no chunks are kept with follow_spill=%r" % (self.follow_spill,))
        parts = [(p[0], p[-1]) for p in self.chunks]
        parts.append(self._on_host(self.volume.points))
        out = (np.concatenate([p[0] for p in parts]),)
        return out + ((np.concatenate([p[-1] for p in parts]),) if self.color else ())

    def _consistent(self, depth, gate, pose):
        """The regressed map checked against the held frames' raw maps from `pose` (one launch): -> the filtered map, in a buffer
        the next frame overwrites; `last_votes` beside it."""
        if self._votes is None:
            self._votes, self._filtered = torch.empty_like(depth), torch.empty_like(depth)
        held = self._held[-ops.CONSISTENCY_MAX_SRC:]
        src = dict(src_depth=None, src_T=None)
        if held:
            src = dict(src_depth=self._slots["raw"], src_gate=self._slots["gate"], src_slots=[h.slot for h in held],
                       src_T=relative_poses(pose, [h.pose for h in held]))
        ops.depth_consistency(depth, intrinsics_at(self.cam, *depth.shape), rel_thr=self.consistency_rel,
                              min_views=min(self.consistency, len(held)), depth_range=self.depth_range, gate=gate,
                              gate_thr=0.0 if self.gate_thr is None else self.gate_thr, votes=self._votes, depth_out=self._filtered, **src)
        self.last_votes = self._votes
        return self._filtered

    # ---- the history: what the last `history` frames were integrated with, so that a corrected pose can move them ----------------

    def _hold(self, ref_index, pose, fr, gate, raw):
        """Copies what the frame was integrated with into the oldest slot (contiguous fp32 device-to-device copies: memory copies,
        no kernel) and notes its pose; the frame that held the slot stays fused for good.  gate: the stream's gate of the regressed
        map, and raw (consistency > 0): that map before the filter — what later frames are checked against; fr.depth is then the
        filtered map that was integrated."""
        maps = dict(depth=fr.depth, gate=gate, wmap=fr.weight, image=fr.color, raw=raw)
        if self._slots is None:                                 # once: the maps' size is the source's
            self._slots = {key: None if t is None else torch.empty((self.history,) + tuple(t.shape), dtype=torch.float32, device=self.device)
                           for key, t in maps.items()}
        slot = self._n_held % self.history
        self._n_held += 1
        for key, t in maps.items():
            if t is not None:
                self._slots[key][slot].copy_(t)
        self._held = [h for h in self._held if h.slot != slot] + [_Held(ref_index, np.array(pose, dtype=np.float64), slot, self.n_shifts)]

    def history_poses(self):
        """[(ref_index, extM)] of the frames the history holds, oldest first: the poses they are integrated at now."""
        return [(h.ref_index, h.pose.copy()) for h in self._held]

    def _held_frame(self, ref_index, who):
        """The history entry of a frame and what it was integrated with, its record rebuilt from the slots: (entry, depth, keywords
        of integrate / deintegrate / reintegrate — with the depth map, a _Frame again)."""
        for h in self._held:
            if h.ref_index == ref_index:
                break
        else:
            raise KeyError("FusionVideoStream.%s: frame %r is not in the history (history=%d holds %s)"
                           % (who, ref_index, self.history, [e.ref_index for e in self._held]))
        if h.shifts != self.n_shifts:
            raise ValueError("FusionVideoStream.%s: frame %r was integrated before the volume shifted: it cannot be taken out exactly "
                             "any more (the region that entered never held it); it still serves as a consistency source"
                             % (who, ref_index))
        pick = lambda key: None if self._slots[key] is None else self._slots[key][h.slot]
        fr = self._frame(pick("depth"), pick("gate"), pick("wmap"), pick("image"))
        return h, fr.depth, fr.fuse_kw()

    def _reposed(self, h, pose):
        h.pose[...] = pose
        if self._held[-1] is h:                                 # the last frame integrated: tracking goes on from the corrected pose
            self.last_ext = h.pose.copy()
            if self._prev is not None:
                self._prev = (self._prev[0], h.pose.copy())

    def repose(self, ref_index, extM):
        """A pose correction for a frame of the history: the frame is taken out of the volume at the pose it was integrated with
        and put back at extM (host [4,4] world -> camera) in one launch — TSDFVolume.reintegrate with the frame's own maps, the
        stream's gate, weights, depth range and colour arguments.  The new pose is what the history holds from now on; for the last
        frame integrated it also becomes `last_ext` and the pose tracking continues from.  KeyError: the frame is not (or no
        longer) held.  Allocates nothing and synchronises nothing."""
        h, depth, kw = self._held_frame(ref_index, "repose")
        new = self._extrinsic(extM)
        if not np.all(np.isfinite(new)):
            raise ValueError("FusionVideoStream.repose: the pose is not finite")
        done = self.volume.reintegrate(depth, h.pose, new, self.cam, **kw)
        self._reposed(h, new)
        return done

    def retrack(self, ref_index, **track_kwargs):
        """A held frame registered again, against the model WITHOUT it (track=True): the frame is de-integrated, its depth map is
        tracked against what remains from its stored pose (with its picture from the history when photo=True; track_kwargs go on
        top of the stream's), and it is integrated at the tracked pose — or, when the track is lost, back at the stored pose: the
        volume then differs from before by rounding only.  Returns the tracking.TrackResult; the history's pose is updated as
        `repose` does.  Synchronises once (the tracker reads its result back)."""
        if not self.track:
            raise ValueError("FusionVideoStream.retrack: the stream was built with track=False")
        h, depth, kw = self._held_frame(ref_index, "retrack")
        self.volume.deintegrate(depth, h.pose, self.cam, **kw)
        res = self._track(_Frame(depth, **kw), h.pose, **track_kwargs)
        pose = res.extM if res.ok else h.pose
        self.volume.integrate(depth, pose, self.cam, **kw)
        self._reposed(h, pose)
        return res

    def push(self, frame, extM):
        """As VideoDepthStream.push; the maps that come out (of frame ref_index) are integrated before they are returned."""
        ext = self._extrinsic(extM)
        index = self.n_pushed
        out = super().push(frame, extM)                         # raises before anything is counted
        valid = bool(np.all(np.isfinite(ext)))
        slot = self.ext_ring.store(index, valid)
        self._ext[slot] = ext if valid else None
        return self._fuse(out)

    def flush(self):
        """pipeline=True: the frame that is still owed, integrated like any other; None otherwise."""
        return self._fuse(super().flush())


def fuse_sequence(stream, frames, extMs):
    """One trajectory through a FusionVideoStream: resets the stream's trajectory state (the volume keeps accumulating), pushes every
    frame, flushes, and returns the number of depth frames integrated by this call."""
    stream.reset()
    before = stream.n_integrated
    for frame, extM in zip(frames, extMs):
        stream.push(frame, extM)
    stream.flush()
    stream.check()
    return stream.n_integrated - before


def save_ply(path, points, faces=None, binary=False, colors=None):
    """[n,3] points (a tensor on any device, or an array) as a PLY file, written on the host; returns the vertex count.  faces: [m,3]
    vertex rows (TSDFVolume.mesh's) written as an `element face` block (property list uchar int vertex_indices); binary: the
    binary_little_endian 1.0 form, written by numpy in one piece, else ASCII, in which %.9g round-trips fp32.  colors: [n,3] colours of
    the points, written as `property uchar red / green / blue` after z — fp32 in [0, 1] through to_uint8, or uint8 as given."""
    if isinstance(points, torch.Tensor):
        points = points.detach().cpu().numpy()
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    header = "ply\nformat %s 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % (
        "binary_little_endian" if binary else "ascii", len(p))
    rgb = None
    if colors is not None:
        if isinstance(colors, torch.Tensor):
            colors = colors.detach().cpu().numpy()
        rgb = np.asarray(colors)
        if rgb.dtype != np.uint8:
            if not np.issubdtype(rgb.dtype, np.floating):
                raise ValueError("save_ply: colors are fp32 in [0, 1] or uint8, got %s" % rgb.dtype)
            rgb = to_uint8(rgb)
        rgb = rgb.reshape(-1, 3)
        if len(rgb) != len(p):
            raise ValueError("save_ply: %d colours for %d points" % (len(rgb), len(p)))
        header += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    tri = None
    if faces is not None:
        if isinstance(faces, torch.Tensor):
            faces = faces.detach().cpu().numpy()
        tri = np.asarray(faces).reshape(-1, 3)
        if len(tri) and not (np.issubdtype(tri.dtype, np.integer) and tri.min() >= 0 and tri.max() < len(p)):
            raise ValueError("save_ply: faces hold integer rows of the %d points" % len(p))
        tri = tri.astype("<i4")
        header += "element face %d\nproperty list uchar int vertex_indices\n" % len(tri)
    header += "end_header\n"
    if binary:
        with open(path, "wb") as f:
            f.write(header.encode("ascii"))
            if rgb is None:
                f.write(p.astype("<f4").tobytes())
            else:
                vert = np.empty(len(p), dtype=[("p", "<f4", (3,)), ("c", "u1", (3,))])
                vert["p"], vert["c"] = p, rgb
                f.write(vert.tobytes())
            if tri is not None:
                rec = np.empty(len(tri), dtype=[("n", "u1"), ("v", "<i4", (3,))])
                rec["n"], rec["v"] = 3, tri
                f.write(rec.tobytes())
        return len(p)
    with open(path, "w") as f:
        f.write(header)
        if rgb is None:
            for x, y, z in p:
                f.write("%.9g %.9g %.9g\n" % (x, y, z))
        else:
            for (x, y, z), (r, g, b) in zip(p, rgb):
                f.write("%.9g %.9g %.9g %d %d %d\n" % (x, y, z, r, g, b))
        for a, b, c in (tri if tri is not None else ()):
            f.write("3 %d %d %d\n" % (a, b, c))
    return len(p)
