"""GPU: ops.tsdf_blocks_gather / ops.tsdf_blocks_scatter (csrc/tsdf_page.hip) against the numpy restatement of tests/tsdf_page_ref.py,
as int32 bits: grids that take the 16-byte form ((16,16,16), (24,16,8)) and one that takes the element form ((13,10,9)), 2 and 5
planes, the origin lists of tsdf_page_ref.cases — an aligned interior block, ox = 4 and ox = 3, blocks half outside each of the six
faces, blocks wholly outside, an all-zero block, a block that is zero except one -0.0 in the last plane, n = 1 and n = 0 — on a
recognisable pattern with NaN payloads, infinities, -0.0 and denormals in every plane, guard words around the volume and the staging
tensor, a volume base off the 16-byte grid, the round trip, the wrapper's refusals, and a captured graph replayed twice."""
import numpy as np
import pytest
import torch

import tsdf_page_ref as pr
import tsdf_shift_ref as sr
from neuralrgbd_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, GUARD_WORD = 64, 0x5A5A5A5A
DIMS = ((16, 16, 16), (24, 16, 8), (13, 10, 9))


def _guarded(words, off=0):
    """A device buffer holding `words` (any shape, 4-byte items) `off` floats off the 16-byte grid, between guard words: -> (the whole
    allocation as int32, the buffer as fp32 of that shape)."""
    words = np.ascontiguousarray(words)
    n = words.size
    whole = torch.full((n + 2 * GUARD + 4,), GUARD_WORD, dtype=torch.int32, device=DEV)
    assert whole.data_ptr() % 16 == 0
    body = whole[GUARD + off:GUARD + off + n]
    body.copy_(torch.from_numpy(words.reshape(-1).view(np.int32)).to(DEV))
    return whole, body.view(torch.float32).view(words.shape)


def _guards_intact(whole, n, off=0):
    w = whole.cpu().numpy()
    return (w[:GUARD + off] == GUARD_WORD).all() and (w[GUARD + off + n:] == GUARD_WORD).all()


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _check(vol, dims, origins, off=0):
    """Gather, scatter into garbage, and the round trip through a zero volume, on guarded buffers."""
    P, n = vol.shape[0], len(origins)
    want_blocks, want_flags = pr.gather(vol, origins)
    whole_v, buf = _guarded(vol, off)
    assert buf.data_ptr() % 16 == 4 * off
    whole_b, staged = _guarded(np.full((n, P, 8, 8, 8), sr.GARBAGE, np.int32))
    flags = torch.full((n + 2,), 77, dtype=torch.int32, device=DEV)
    blocks, nonempty = ops.tsdf_blocks_gather(buf, origins, out=staged, nonempty=flags)
    assert tuple(blocks.shape) == (n, P, 8, 8, 8) and tuple(nonempty.shape) == (n,)
    assert n == 0 or (blocks.data_ptr() == staged.data_ptr() and nonempty.data_ptr() == flags.data_ptr())      # written where they lie
    assert np.array_equal(_bits(blocks), sr.bits(want_blocks)), "blocks differ: dims %s origins %s" % (dims, origins.tolist())
    assert np.array_equal(nonempty.cpu().numpy(), want_flags) and flags[n:].tolist() == [77, 77]
    assert np.array_equal(_bits(buf), sr.bits(vol)), "gather wrote the volume"
    assert _guards_intact(whole_v, vol.size, off) and _guards_intact(whole_b, staged.numel())
    # scatter into a buffer full of garbage: every word outside the blocks keeps its bits
    before = np.full(vol.shape, sr.GARBAGE, np.int32).view(np.float32)
    whole_d, dst = _guarded(before, off)
    ops.tsdf_blocks_scatter(dst, origins, blocks)
    assert np.array_equal(_bits(dst), sr.bits(pr.scatter(before, origins, want_blocks))), "scatter differs: dims %s origins %s" % (dims, origins.tolist())
    assert _guards_intact(whole_d, vol.size, off) and np.array_equal(_bits(blocks), sr.bits(want_blocks))
    # gather -> scatter into a zero volume -> gather: identical bits
    zero = torch.zeros(vol.shape, device=DEV)
    ops.tsdf_blocks_scatter(zero, origins, blocks)
    again, again_flags = ops.tsdf_blocks_gather(zero, origins)
    assert torch.equal(again.view(torch.int32), blocks.view(torch.int32)) and torch.equal(again_flags, nonempty)
    return want_flags


@pytest.mark.parametrize("planes", [2, 5])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(str(n) for n in d))
def test_gather_and_scatter_equal_the_restatement_bit_for_bit(dims, planes):
    vol = pr.prepared(planes, dims, seed=planes)
    b = sr.bits(vol)
    for p in range(planes):                                         # the payloads are there, in every plane
        assert np.isnan(vol[p]).any() and np.isinf(vol[p]).any() and (b[p] == np.int32(-2 ** 31)).any() and (b[p] == 1).any()
    names = []
    for name, origins in pr.cases(dims):
        flags = _check(vol, dims, origins)
        names.append(name)
        if name == "prepared":
            assert flags.tolist() == [0, 1]                         # all zero; zero except one -0.0 in the last plane
        if name == "outside":
            assert not flags.any()
    assert {"prepared", "ox4", "ox3", "face0", "face5", "outside", "mixed", "one", "none"} <= set(names)


@pytest.mark.parametrize("dims", [(16, 16, 16), (13, 10, 9)], ids=lambda d: "x".join(str(n) for n in d))
def test_a_base_off_the_16_byte_grid_takes_the_element_form(dims):
    vol = pr.prepared(5, dims, seed=7)
    for off in (1, 2, 3):
        for name, origins in pr.cases(dims):
            if name in ("prepared", "ox4", "ox3", "mixed", "face1"):
                _check(vol, dims, origins, off)


def test_default_outputs_and_uploaded_origins():
    dims = (16, 16, 16)
    vol = pr.prepared(2, dims, seed=1)
    buf = torch.from_numpy(vol.view(np.int32)).to(DEV).view(torch.float32)
    origins = dict(pr.cases(dims))["mixed"]
    want = pr.gather(vol, origins)
    blocks, flags = ops.tsdf_blocks_gather(buf, origins.tolist())   # a list of tuples is a host int array too
    assert blocks.dtype == torch.float32 and flags.dtype == torch.int32 and blocks.data_ptr() % 16 == 0
    assert np.array_equal(_bits(blocks), sr.bits(want[0])) and np.array_equal(flags.cpu().numpy(), want[1])
    up = ops.tsdf_block_origins(origins, DEV)
    again, _ = ops.tsdf_blocks_gather(buf, up)
    assert torch.equal(again.view(torch.int32), blocks.view(torch.int32)) and up.dev.device == buf.device
    empty, none = ops.tsdf_blocks_gather(buf, [])
    assert tuple(empty.shape) == (0, 2, 8, 8, 8) and tuple(none.shape) == (0,)
    ops.tsdf_blocks_scatter(buf, [], empty)
    assert np.array_equal(_bits(buf), sr.bits(vol))


def test_argument_errors():
    buf = torch.zeros(2, 16, 16, 16, device=DEV)
    blocks = torch.zeros(2, 2, 8, 8, 8, device=DEV)
    for origins in ([(0, 0, 0), (7, 7, 7)], [(3, 1, 0), (3, 1, 0)], [(-4, 0, 0), (0, 0, 0)], [(12, 12, 12), (15, 15, 15)]):
        with pytest.raises(ValueError, match="overlap"):
            ops.tsdf_blocks_scatter(buf, origins, blocks)
    ops.tsdf_blocks_scatter(buf, [(-4, 0, 0), (-8, 0, 0)], blocks)  # they share voxels outside the grid only
    ops.tsdf_blocks_scatter(buf, [(0, 0, 0), (8, 0, 0)], blocks)
    two = [(0, 0, 0), (8, 8, 8)]
    for bad in (torch.zeros(1, 2, 8, 8, 8, device=DEV), torch.zeros(2, 5, 8, 8, 8, device=DEV), torch.zeros(2, 2, 8, 8, 4, device=DEV),
                torch.zeros(4, 2, 8, 8, 8, device=DEV)[::2], torch.zeros(2 * 2 * 512 + 1, device=DEV)[1:].view(2, 2, 8, 8, 8)):
        with pytest.raises(ValueError):
            ops.tsdf_blocks_scatter(buf, two, bad)
        with pytest.raises(ValueError):
            ops.tsdf_blocks_gather(buf, two, out=bad)
    for bad_buf in (buf[0], torch.zeros(3, 16, 16, 16, device=DEV), buf[:, :, :, ::2]):
        with pytest.raises(ValueError):
            ops.tsdf_blocks_gather(bad_buf, two)
    for bad_flags in (torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV),
                      torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(ValueError):
            ops.tsdf_blocks_gather(buf, two, nonempty=bad_flags)
    with pytest.raises(TypeError):
        ops.tsdf_blocks_gather(buf.double(), two)
    with pytest.raises(TypeError):
        ops.tsdf_blocks_scatter(buf, two, None)
    with pytest.raises(ValueError):
        ops.tsdf_blocks_gather(buf, [(0, 0)])
    assert not buf.any() and not blocks.any()


def test_two_runs_and_a_captured_graph_give_the_same_bits():
    from neuralrgbd_amd.distributed import graph_capture_mode
    dims = (24, 16, 8)
    vol = pr.prepared(5, dims, seed=11)
    origins = dict(pr.cases(dims))["mixed"]
    want_blocks, want_flags = pr.gather(vol, origins)
    before = np.full(vol.shape, sr.GARBAGE, np.int32).view(np.float32)
    want_dst = sr.bits(pr.scatter(before, origins, want_blocks))
    buf = torch.from_numpy(vol.view(np.int32)).to(DEV).view(torch.float32)
    dst = torch.from_numpy(before.view(np.int32)).to(DEV).view(torch.float32)
    up = ops.tsdf_block_origins(origins, DEV)                       # uploaded before the capture: an upload is not a graph node
    staged = torch.full((len(origins), 5, 8, 8, 8), float("nan"), device=DEV)
    flags = torch.full((len(origins),), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=graph_capture_mode()):
        ops.tsdf_blocks_gather(buf, up, out=staged, nonempty=flags)
        ops.tsdf_blocks_scatter(dst, up, staged)
    assert torch.isnan(staged).all() and (flags == -1).all() and np.array_equal(_bits(dst), sr.bits(before))     # a capture executes nothing
    for _ in range(2):
        staged.fill_(float("nan"))
        flags.fill_(-1)
        dst.copy_(torch.from_numpy(before.view(np.int32)).to(DEV).view(torch.float32))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(staged), sr.bits(want_blocks)) and np.array_equal(flags.cpu().numpy(), want_flags)
        assert np.array_equal(_bits(dst), want_dst)
