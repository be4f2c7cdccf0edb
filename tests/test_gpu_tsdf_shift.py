"""GPU: ops.tsdf_shift (csrc/tsdf_shift.hip) against the numpy restatement of tests/tsdf_shift_ref.py, as int32 bits on BOTH buffers:
every grid of tsdf_ref.GRIDS, 2 and 5 planes, spill off and on, shifts that take every path (zero, one voxel either way on every axis,
whole groups and odd counts along x — the 16-byte and the element source forms —, mixed signs on two and three axes, n - 1, n and
n + 3 voxels), a recognisable pattern with NaN payloads, infinities, -0.0 and denormals in every plane, guard words around both
buffers, bases off the 16-byte grid, src untouched without spill, the same bits in two runs and through a captured graph."""
import numpy as np
import pytest
import torch

import tsdf_ref as ref
import tsdf_shift_ref as sr
from neuralrgbd_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, GUARD_WORD = 64, 0x5A5A5A5A


def shifts_for(dims):
    X, Y, Z = dims
    out = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (4, 0, 0), (-4, 0, 0), (8, 0, 0), (-8, 0, 0),
           (2, 0, 0), (3, 0, 0), (5, 0, 0), (-3, 0, 0), (4, -1, 0), (-1, 2, 0), (0, 1, -1), (4, 1, -1), (-8, 2, 1), (3, -2, 1), (-1, -1, -1),
           (12, -6, 3)]
    for k, n in enumerate(dims):
        for v in (n - 1, n, n + 3, -(n - 1), -n):
            s = [0, 0, 0]
            s[k] = v
            out.append(tuple(s))
    out.append((2 ** 31 - 1, 0, 0))
    out.append((0, -(2 ** 31), 0))
    return list(dict.fromkeys(out))


def _guarded(words, n, off):
    """A device buffer of n fp32 words `off` floats off the 16-byte grid, between guard words: -> (the whole allocation as int32, the
    buffer as fp32)."""
    whole = torch.full((n + 2 * GUARD + 4,), GUARD_WORD, dtype=torch.int32, device=DEV)
    assert whole.data_ptr() % 16 == 0
    body = whole[GUARD + off:GUARD + off + n]
    body.copy_(torch.from_numpy(np.ascontiguousarray(words).reshape(-1).view(np.int32)).to(DEV))
    return whole, body.view(torch.float32)


def _run(start, dims, s, spill, off=(0, 0)):
    """One launch on guarded buffers: -> (dst bits, src bits afterwards) as numpy int32, the guards checked."""
    X, Y, Z = dims
    P = start.shape[0]
    n = start.size
    whole_s, src = _guarded(start, n, off[0])
    whole_d, dst = _guarded(np.full(n, sr.GARBAGE, np.int32).view(np.float32), n, off[1])
    assert src.data_ptr() % 16 == 4 * off[0] and dst.data_ptr() % 16 == 4 * off[1]
    ops.tsdf_shift(src.view(P, Z, Y, X), dst.view(P, Z, Y, X), s, spill=spill)
    torch.cuda.synchronize()
    for whole, o in ((whole_s, off[0]), (whole_d, off[1])):
        w = whole.cpu().numpy()
        assert (w[:GUARD + o] == GUARD_WORD).all() and (w[GUARD + o + n:] == GUARD_WORD).all(), "a guard word was overwritten"
    return dst.view(torch.int32).cpu().numpy().reshape(start.shape), src.view(torch.int32).cpu().numpy().reshape(start.shape)


def _check(start, dims, s, spill, off=(0, 0)):
    got_dst, got_src = _run(start, dims, s, spill, off)
    want_dst, want_src = sr.shift(start, s, spill=spill)
    assert np.array_equal(got_dst, sr.bits(want_dst)), "dst differs: dims %s shift %s spill %s off %s" % (dims, s, spill, off)
    assert np.array_equal(got_src, sr.bits(want_src)), "src differs: dims %s shift %s spill %s off %s" % (dims, s, spill, off)
    if not spill:
        assert np.array_equal(got_src, sr.bits(start)), "src was written without spill"
    return got_dst, got_src


@pytest.mark.parametrize("planes", [2, 5])
@pytest.mark.parametrize("dims", ref.GRIDS, ids=lambda d: "x".join(str(n) for n in d))
def test_shift_equals_the_restatement_bit_for_bit(dims, planes):
    start = sr.pattern(planes, dims, seed=planes)
    b = sr.bits(start)
    if b.size >= 5 * 64:                                            # the payloads are there, in every plane
        for p in range(planes):
            assert np.isnan(start[p]).any() and np.isinf(start[p]).any() and (b[p] == np.int32(-2 ** 31)).any() and (b[p] == 1).any()
    for s in shifts_for(dims):
        for spill in (False, True):
            _check(start, dims, s, spill)


@pytest.mark.parametrize("dims", [(64, 3, 2), (48, 40, 36), (67, 5, 3), (4, 3, 3)], ids=lambda d: "x".join(str(n) for n in d))
def test_bases_off_the_16_byte_grid_take_the_element_form(dims):
    start = sr.pattern(5, dims, seed=7)
    for off in ((1, 0), (0, 2), (3, 3), (2, 1)):
        for s in ((4, 0, 0), (-8, 1, 0), (3, 0, -1), (0, 0, 0), (dims[0], 0, 0)):
            _check(start, dims, s, True, off)
            _check(start[:2], dims, s, False, off)


def test_two_runs_and_a_captured_graph_give_the_same_bits():
    from neuralrgbd_amd.distributed import graph_capture_mode
    dims, s = ref.PLANE_GRID, (8, -3, 2)
    X, Y, Z = dims
    start = sr.pattern(5, dims, seed=11)
    first = _check(start, dims, s, True)
    again = _check(start, dims, s, True)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    src = torch.from_numpy(start.view(np.int32)).to(DEV).view(torch.float32)
    dst = torch.full(start.shape, float("nan"), device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=graph_capture_mode()):
        ops.tsdf_shift(src, dst, s, spill=True)
    assert torch.isnan(dst).all() and np.array_equal(src.view(torch.int32).cpu().numpy(), sr.bits(start))       # a capture executes nothing
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(dst.view(torch.int32).cpu().numpy(), first[0]) and np.array_equal(src.view(torch.int32).cpu().numpy(), first[1])
    # a replay on the spilled source: the retained voxels are already empty, the rim and what left keep their bits — dst changes, src not
    want_dst, want_src = sr.shift(first[1].view(np.float32), s, spill=True)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(dst.view(torch.int32).cpu().numpy(), sr.bits(want_dst)) and np.array_equal(src.view(torch.int32).cpu().numpy(), sr.bits(want_src))
    assert np.array_equal(sr.bits(want_src), first[1])


def test_argument_errors():
    a = torch.zeros(2, 3, 4, 8, device=DEV)
    b = torch.zeros(2, 3, 4, 8, device=DEV)
    for src, dst in ((a, a), (a, a.view(2, 3, 4, 8)), (a, torch.zeros(5, 3, 4, 8, device=DEV)), (a, torch.zeros(2, 3, 4, 9, device=DEV)),
                     (a[:, :, :, ::2], b[:, :, :, ::2]), (torch.zeros(3, 3, 4, 8, device=DEV), torch.zeros(3, 3, 4, 8, device=DEV)),
                     (a[0], b[0])):
        with pytest.raises(ValueError):
            ops.tsdf_shift(src, dst, (1, 0, 0))
    whole = torch.zeros(3 * a.numel() // 2, device=DEV)
    with pytest.raises(ValueError):                                 # two views of one storage whose bytes overlap
        ops.tsdf_shift(whole[:a.numel()].view(2, 3, 4, 8), whole[a.numel() // 2:].view(2, 3, 4, 8), (1, 0, 0))
    for bad in ((1, 0), (1.5, 0, 0)):
        with pytest.raises(ValueError):
            ops.tsdf_shift(a, b, bad)
    with pytest.raises(TypeError):
        ops.tsdf_shift(a.double(), b.double(), (1, 0, 0))
    assert not a.any() and not b.any()
