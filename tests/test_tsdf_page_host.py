"""Host-side checks of the paged TSDF volume (csrc/tsdf_page.hip, fusion.BlockStore, TSDFVolume.shift(store=...), fusion.paged_extract):
BlockStore's round trips and refusals; the gather / scatter restatements of tests/tsdf_page_ref.py against the one-voxel-at-a-time
definition, with every mutant of the rule caught; the out-and-back window scenario in numpy — a window that follows the camera out and
back, with a store, holds together with the store what a static volume over the same views holds, bit for bit —; the tiling of that
world; TSDFVolume.shift(store=...) and paged_extract with the restatements in the launches' place; the C entries (declared, bound,
exported, every refusal without a GPU and in the documented order).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tsdf_mesh_ref as mref
import tsdf_page_ref as pr
import tsdf_shift_ref as sr
from conftest import ROOT
from neuralrgbd_amd import _lib, fusion, ops

E_NULL, E_SHAPE, E_ARG = -1, -2, -4
GATHER, SCATTER = "nrgbd_tsdf_blocks_gather_f32", "nrgbd_tsdf_blocks_scatter_f32"
DIMS = ((16, 16, 16), (24, 16, 8), (13, 10, 9))


def _same_bits(a, b):
    return np.array_equal(sr.bits(a), sr.bits(b))


# ---- 1. BlockStore
def _blocks(n, planes, seed):
    return np.stack([sr.pattern(planes, (8, 8, 8), seed + b) for b in range(n)])


@pytest.mark.parametrize("planes", [2, 5])
def test_block_store_round_trips(planes, tmp_path):
    st = fusion.BlockStore(planes)
    keys = np.array([(0, 0, 0), (-3, 2, 1), (5, -1, -7), (1 << 27, 0, -(1 << 27)), (2, 2, 2)])
    data = _blocks(5, planes, 3)
    assert np.isnan(data).any() and (sr.bits(data) == np.int32(-2 ** 31)).any()
    assert len(st) == 0 and st.bounds() is None and st.nbytes == 0 and st.keys() == []
    assert st.put(keys, data, np.array([1, 1, 0, 7, 1], np.int32)) == 4         # the unflagged block is dropped
    assert (st.n_put, st.n_dropped, st.n_taken) == (4, 1, 0)
    assert len(st) == 4 and st.nbytes == 4 * planes * 512 * 4 and (5, -1, -7) not in st and (-3, 2, 1) in st
    assert st.keys() == sorted(tuple(int(v) for v in k) for k in keys[[0, 1, 3, 4]])
    assert st.bounds() == ((-3, 0, -(1 << 27)), ((1 << 27) + 1, 3, 3))
    data_before = data.copy()
    data[:] = 0                                                     # put copied
    found, got = st.get([(2, 2, 2), (9, 9, 9), (-3, 2, 1)])
    assert found.tolist() == [[2, 2, 2], [-3, 2, 1]] and _same_bits(got, data_before[[4, 1]]) and len(st) == 4
    got[:] = 0                                                      # get copied
    path = str(tmp_path / "map.npz")
    st.save(path)
    back = fusion.BlockStore.load(path)
    assert back.planes == planes and back.keys() == st.keys() and (back.n_put, back.n_dropped, back.n_taken) == (0, 0, 0)
    for k in st.keys():
        assert _same_bits(back.get([k])[1], st.get([k])[1])
    found, got = st.take([(2, 2, 2), (9, 9, 9), (-3, 2, 1)])
    assert found.tolist() == [[2, 2, 2], [-3, 2, 1]] and _same_bits(got, data_before[[4, 1]])
    assert len(st) == 2 and st.n_taken == 2 and st.take([(2, 2, 2)])[0].shape == (0, 3) and st.take([])[1].shape == (0, planes, 8, 8, 8)
    assert st.put([(2, 2, 2)], data_before[4:5]) == 1               # taken: it may come back; without flags every block counts
    st.clear()
    assert len(st) == 0 and st.bounds() is None
    assert len(back) == 4                                           # a store of its own


def test_block_store_refusals():
    st = fusion.BlockStore(2)
    data = _blocks(2, 2, 0)
    st.put([(1, 2, 3)], data[:1])
    for call in (lambda: st.put([(1, 2, 3)], data[:1]),             # already held
                 lambda: st.put([(4, 4, 4), (1, 2, 3)], data, [1, 1]),
                 lambda: st.put([(7, 7, 7), (7, 7, 7)], data),       # twice in one call
                 lambda: st.put([(5, 5, 5)], data),                 # shapes
                 lambda: st.put([(5, 5, 5)], _blocks(1, 5, 0)),
                 lambda: st.put([(5, 5, 5)], np.zeros((1, 2, 8, 8, 8), np.float64)),
                 lambda: st.put([(5, 5, 5)], data[:1], [1, 1]),
                 lambda: fusion.BlockStore(3), lambda: fusion.BlockStore(2, block=4)):
        with pytest.raises(ValueError):
            call()
    assert st.keys() == [(1, 2, 3)] and st.n_put == 1               # a refused put stores nothing
    assert st.put([(1, 2, 3)], data[:1], [0]) == 0                  # an unflagged block is not stored: nothing to refuse


# ---- 2. the restatements against the definition, and the mutants
@pytest.mark.parametrize("planes", [2, 5])
@pytest.mark.parametrize("dims", DIMS, ids=str)
def test_restatements_equal_the_definition_and_every_mutant_differs(dims, planes):
    vol = pr.prepared(planes, dims, seed=planes)
    before = np.full(vol.shape, sr.GARBAGE, np.int32).view(np.float32)
    caught = {m: 0 for m in pr.KERNEL_MUTANTS}
    for name, origins in pr.cases(dims):
        blocks, flags = pr.gather(vol, origins)
        want = pr.gather_by_definition(vol, origins)
        assert _same_bits(blocks, want[0]) and np.array_equal(flags, want[1]), (name, dims)
        after = pr.scatter(before, origins, blocks)
        assert _same_bits(after, pr.scatter_by_definition(before, origins, blocks)), (name, dims)
        again = pr.gather(pr.scatter(np.zeros_like(vol), origins, blocks), origins)
        assert _same_bits(again[0], blocks) and np.array_equal(again[1], flags)
        for m in pr.KERNEL_MUTANTS:
            got = pr.gather(vol, origins, m)
            caught[m] += not (_same_bits(got[0], blocks) and np.array_equal(got[1], flags) and _same_bits(pr.scatter(before, origins, blocks, m), after))
        if name == "prepared":
            assert flags.tolist() == [0, 1]                         # the all-zero block; the one that is zero except a -0.0
        if name == "outside":
            assert not flags.any() and not sr.bits(blocks).any() and _same_bits(after, before)
    print("[page] dims %s planes %d: lists that catch each mutant: %s" % (dims, planes, caught))
    for m, n in caught.items():
        if m == "flag_ignores_colour" and planes == 2:
            assert n == 0                                           # no colour plane to ignore
        else:
            assert n > 0, m


# ---- 3. the out-and-back window scenario
def test_out_and_back_window_with_a_store_equals_the_static_volume():
    r = pr.out_and_back_host()
    print("[page] out and back: %s, %d voxels of the last window with weight >= 2" % (r["counts"], int((r["live"][1] >= 2).sum())))
    assert len(pr.out_and_back()) == 84 and r["boxes_ok"]           # every view's unclipped frustum box inside the window
    assert r["counts"] == pr.SCENARIO_COUNTS
    X = sr.WINDOW_DIMS[0]
    assert r["off"] == 0 and _same_bits(r["live"], r["static"][:, :, :, r["off"]:r["off"] + X])
    whole, lo = pr.world(r["live"], (r["off"], 0, 0), r["store"], bounds=((0, 0, 0), sr.STATIC_DIMS))
    assert lo == (0, 0, 0) and _same_bits(whole, r["static"])
    assert int((r["live"][1] >= 2).sum()) >= 100                    # observations of both passes in one voxel: 696 measured


@pytest.mark.parametrize("mutant", ["take_keeps", "sets_swapped"])
def test_store_mutants_are_caught_by_the_scenario(mutant):
    good, bad = pr.out_and_back_host(), pr.out_and_back_host(mutant)
    whole = pr.world(bad["live"], (bad["off"], 0, 0), bad["store"], bounds=((0, 0, 0), sr.STATIC_DIMS))[0]
    assert bad["counts"] != good["counts"]
    if mutant == "sets_swapped":
        assert not _same_bits(whole, good["static"]) and len(bad["store"]) == 0     # nothing was kept: the first pass is lost
        assert int((bad["live"][1] >= 2).sum()) < int((good["live"][1] >= 2).sum())


# ---- 4. the tiling of that world
W_MIN = 1.0


def test_tiles_of_the_world_mesh_like_the_static_volume():
    r = pr.out_and_back_host()
    parts = pr.tiles(r["live"], (r["off"], 0, 0), r["store"], sr.WINDOW_DIMS)
    assert [t for t, _ in parts] == [(0, 0, 0), (31, 0, 0), (62, 0, 0)]          # stride 31; the store ends at x = 88
    v, f, meshes = pr.tiled_mesh(parts, sr.WINDOW_ORIGIN, sr.VS, W_MIN)
    sv, sf = mref.mesh(r["static"][0], r["static"][1], sr.WINDOW_ORIGIN, sr.VS, W_MIN)
    print("[page] tiles: triangles %s = %d, the static volume's %d" % ([len(m[1]) for m in meshes], len(f), len(sf)))
    assert len(f) == len(sf) > 500 and f.max() < len(v)
    a, b = pr.sorted_triangles(v, f), pr.sorted_triangles(sv, sf)
    ulp = np.spacing(np.float32(max(np.abs(sv).max(), np.abs(v).max())))
    worst = np.abs(a.astype(np.float64) - b.astype(np.float64)).max()
    print("[page] tiles: largest position difference %.3g = %.2f ulp of the largest coordinate" % (worst, worst / ulp))
    assert worst <= 4 * ulp                                         # o + vs (i + q): two roundings an evaluation, two evaluations


class _HostLaunches:
    """The restatements in the launches' place, on host tensors."""

    def __init__(self, monkeypatch):
        self.calls = []
        put = lambda t, a: t.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).view(t.dtype).reshape(t.shape))

        def shift(src, dst, s, spill=False):
            assert not spill
            put(dst, sr.shift(src.numpy(), s, dst_before=dst.numpy())[0])
            self.calls.append(("shift", tuple(s)))

        def gather(buf, origins, out=None, nonempty=None):
            blocks, flags = pr.gather(buf.numpy(), origins)
            put(out[:len(origins)], blocks)
            nonempty[:len(origins)].copy_(torch.from_numpy(flags))
            self.calls.append(("gather", len(origins)))
            return out[:len(origins)], nonempty[:len(origins)]

        def scatter(buf, origins, blocks):
            assert ops.tsdf_blocks_overlap(origins, buf.shape[:0:-1]) is None
            put(buf, pr.scatter(buf.numpy(), origins, blocks[:len(origins)].numpy()))
            self.calls.append(("scatter", len(origins)))

        def mesh(vol, w_min=1., capacity=None, colors=False):
            v, f = mref.mesh(vol._buf[0].numpy(), vol._buf[1].numpy(), vol.origin, vol.voxel_size, w_min)
            return torch.from_numpy(np.asarray(v, np.float32)), torch.from_numpy(np.asarray(f, np.int32)), (len(v), len(f))
        monkeypatch.setattr(ops, "tsdf_shift", shift)
        monkeypatch.setattr(ops, "tsdf_blocks_gather", gather)
        monkeypatch.setattr(ops, "tsdf_blocks_scatter", scatter)
        monkeypatch.setattr(fusion.TSDFVolume, "mesh", mesh)


def test_paged_extract_equals_the_restatement_run_per_tile(monkeypatch):
    _HostLaunches(monkeypatch)
    r = pr.out_and_back_host()
    vol = fusion.TSDFVolume(sr.WINDOW_DIMS, sr.VS, sr.WINDOW_ORIGIN, trunc=sr.WINDOW_TRUNC, device="cpu")
    vol._buf.copy_(torch.from_numpy(r["live"].copy()))
    st = fusion.BlockStore(2)
    st.put(sorted(r["store"]), np.stack([r["store"][k] for k in sorted(r["store"])]))
    keep = vol._buf.clone()
    v, f = fusion.paged_extract(vol, st, "mesh", w_min=W_MIN)
    wv, wf, _ = pr.tiled_mesh(pr.tiles(r["live"], (0, 0, 0), r["store"], sr.WINDOW_DIMS), sr.WINDOW_ORIGIN, sr.VS, W_MIN)
    assert v.dtype == np.float32 and f.dtype == np.int32 and _same_bits(v, wv) and np.array_equal(f, wf) and len(f) > 500
    assert len(st) == 13 and st.n_taken == 0 and torch.equal(vol._buf.view(torch.int32), keep.view(torch.int32))       # nothing modified
    assert vol.offset == (0, 0, 0) and vol.origin == tuple(sr.WINDOW_ORIGIN)
    scratch = vol._page_scratch
    fusion.paged_extract(vol, st, "mesh", w_min=W_MIN)
    assert vol._page_scratch is scratch                             # allocated at the first call
    empty = fusion.paged_extract(fusion.TSDFVolume((8, 8, 8), 1.0, (0, 0, 0), device="cpu"), fusion.BlockStore(2))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)
    with pytest.raises(ValueError):
        fusion.paged_extract(vol, st, "ply")
    with pytest.raises(ValueError):
        fusion.paged_extract(vol, fusion.BlockStore(5))


# ---- 5. TSDFVolume.shift(store=...) with the restatements in the launches' place
def test_paged_shift_follows_the_restatement(monkeypatch):
    host = _HostLaunches(monkeypatch)
    dims = (16, 8, 24)
    start = sr.pattern(5, dims, 4)
    vol = fusion.TSDFVolume(dims, 0.5, (1.0, 2.0, 3.0), device="cpu", color=True)
    vol._buf.copy_(torch.from_numpy(start.view(np.int32)).view(torch.float32))
    st, want_store, want, off = fusion.BlockStore(5), {}, start, (0, 0, 0)
    assert vol.shift((0, 0, 0), store=st) is None and vol._spare is None and vol._page_out is None and host.calls == []
    staging = None
    for s in ((8, 0, 0), (0, 0, -16), (-8, 8, 0), (0, -8, 16), (32, 0, 0), (-32, 0, 0), (8, 0, 8), (-8, 0, -8)):
        assert vol.shift(s, store=st) is None
        want, off, counts = pr.paged_shift(want, off, s, want_store)
        assert vol.offset == off and _same_bits(vol._buf.numpy(), want), s
        assert st.keys() == sorted(want_store) and all(_same_bits(st.get([k])[1][0], want_store[k]) for k in want_store)
        if staging is None:
            staging = vol._page_out
        assert vol._page_out is staging                             # allocated once, grown in place
    assert vol.offset == (0, 0, 0) and _same_bits(vol._buf.numpy(), start) and len(st) == 0          # everything came back
    assert st.n_put == st.n_taken > 0 and st.n_dropped > 0          # dropped: the empty blocks that entered and left again
    kinds = [c[0] for c in host.calls]
    assert kinds[:3] == ["shift", "gather", "shift"] and "scatter" in kinds
    for bad in (dict(voxels=(4, 0, 0)), dict(voxels=(8, 0, 0), spill=True), dict(voxels=(8, 0, 0), store=fusion.BlockStore(2)),
                dict(voxels=(8, 0, 0), store={})):
        with pytest.raises(ValueError):
            vol.shift(**dict(dict(store=st), **bad))
    vol.shift((4, 0, 0))                                            # without a store any whole voxels, as before
    with pytest.raises(ValueError, match="multiples of 8"):
        vol.shift((8, 0, 0), store=st)                              # the offset has left the block lattice
    odd = fusion.TSDFVolume((12, 8, 8), 0.5, (0, 0, 0), device="cpu")
    with pytest.raises(ValueError, match="multiples of 8"):
        odd.shift((8, 0, 0), store=fusion.BlockStore(2))
    assert odd._spare is None                                       # refused before anything was launched or allocated


def test_overlap_check_of_the_scatter_wrapper():
    dims = (16, 16, 16)
    assert ops.tsdf_blocks_overlap(np.zeros((0, 3), np.int64), dims) is None
    assert ops.tsdf_blocks_overlap([(0, 0, 0), (8, 0, 0), (0, 8, 0), (8, 8, 8)], dims) is None
    assert ops.tsdf_blocks_overlap([(0, 0, 0), (8, 0, 0), (7, 7, 7)], dims) == (0, 2)
    assert ops.tsdf_blocks_overlap([(3, 1, 0), (3, 1, 0)], dims) == (0, 1)
    assert ops.tsdf_blocks_overlap([(-4, 0, 0), (0, 0, 0)], dims) == (0, 1)
    assert ops.tsdf_blocks_overlap([(-4, 0, 0), (-8, 0, 0)], dims) is None      # they share voxels outside the grid only
    assert ops.tsdf_blocks_overlap([(20, 0, 0), (20, 0, 0)], dims) is None
    for dims in DIMS:
        for name, origins in pr.cases(dims):
            assert ops.tsdf_blocks_overlap(origins, dims) is None, (dims, name)
            pairs = any(pr.overlap_in_grid(a, b, dims) for i, a in enumerate(origins.tolist()) for b in origins.tolist()[:i])
            assert not pairs


# ---- 6. the C entries
def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nrgbd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in ((GATHER, 10), (SCATTER, 9)):
        decl = re.search(r"\bint %s\((.*?)\);" % name, code, flags=re.S).group(1)
        assert decl.count(",") + 1 == len(_lib.SIGNATURES[name][1]) == n_args
        assert hasattr(lib, name)
        assert re.search(r"%s — no counterpart in the reference" % name, header)
        assert name in header[:header.index("#define NRGBD_INTERFACE_VERSION")]
    assert re.search(r"#define NRGBD_TSDF_BLOCK\s+8\b", header) and re.search(r"#define NRGBD_TSDF_MAX_BLOCKS\s+\(1 << 20\)", header)
    assert ops.TSDF_BLOCK == fusion.BLOCK == pr.B == 8 and ops.TSDF_MAX_BLOCKS == 1 << 20


P, Q, O = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 25)      # non-NULL: every refusal comes before the device


def test_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()

    def gather(vol=P, planes=2, X=8, Y=8, Z=8, origins=O, n=1, blocks=Q, nonempty=None):
        return lib.nrgbd_tsdf_blocks_gather_f32(vol, planes, X, Y, Z, origins, n, blocks, nonempty, None)

    def scatter(vol=P, planes=2, X=8, Y=8, Z=8, origins=O, n=1, blocks=Q, nonempty=None):
        return lib.nrgbd_tsdf_blocks_scatter_f32(vol, planes, X, Y, Z, origins, n, blocks, None)
    at = lambda a: ctypes.c_void_p(a)
    for call in (gather, scatter):
        for kw in (dict(vol=None), dict(origins=None), dict(blocks=None), dict(vol=None, origins=None, blocks=None), dict(vol=None, n=0)):
            assert call(**kw) == E_NULL, kw
        for kw in (dict(planes=0), dict(planes=1), dict(planes=3), dict(planes=4), dict(planes=6), dict(planes=-2), dict(X=0), dict(Y=-1),
                   dict(Z=0), dict(X=1 << 16, Y=1 << 16, Z=1), dict(n=-1), dict(n=(1 << 20) + 1), dict(n=-(1 << 31))):
            assert call(**kw) == E_SHAPE, kw
        for kw in (dict(blocks=at((1 << 30) + 4)), dict(blocks=at((1 << 30) + 8)), dict(blocks=at((1 << 30) + 15)), dict(planes=5, blocks=at(12))):
            assert call(**kw) == E_ARG, kw
        # the order: NULL, shape, argument
        assert call(vol=None, planes=3, blocks=at(4)) == E_NULL and call(origins=None, n=-1) == E_NULL
        assert call(planes=3, blocks=at(4)) == E_SHAPE and call(n=-1, blocks=at(4)) == E_SHAPE
        # n == 0 launches nothing: no device is needed, and the block pointers may be NULL
        assert call(n=0) == 0 and call(n=0, origins=None, blocks=None) == 0 and call(n=0, planes=3) == E_SHAPE


def test_the_wrappers_check_before_they_call():
    """The block wrappers need CUDA tensors: a host tensor is refused by name, with no fallback."""
    buf, blocks = torch.zeros(2, 8, 8, 8), torch.zeros(1, 2, 8, 8, 8)
    with pytest.raises(_lib.NrgbdError, match="buf"):
        ops.tsdf_blocks_gather(buf, [(0, 0, 0)])
    with pytest.raises(_lib.NrgbdError, match="buf"):
        ops.tsdf_blocks_scatter(buf, [(0, 0, 0)], blocks)
    with pytest.raises(TypeError):
        ops.tsdf_blocks_gather(buf.numpy(), [(0, 0, 0)])
    for bad in ([(0, 0)], [(0.5, 0, 0)], [((1 << 30) + 1, 0, 0)], np.zeros((2, 3, 1), np.int32)):
        with pytest.raises(ValueError):
            ops.tsdf_block_origins(bad, "cpu")
    with pytest.raises(TypeError):
        ops.tsdf_block_origins(torch.zeros(1, 3, dtype=torch.int32), "cpu")
    o = ops.tsdf_block_origins([(1, 2, 3), (-4, 5, 1 << 30)], "cpu")
    assert o.host.dtype == np.int32 and o.dev.dtype == torch.int32 and o.dev.tolist() == o.host.tolist() == [[1, 2, 3], [-4, 5, 1 << 30]]
    assert ops.tsdf_block_origins(o, "cpu") is o and ops.tsdf_block_origins([], "cpu").host.shape == (0, 3)
