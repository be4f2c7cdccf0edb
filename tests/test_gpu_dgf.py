"""nrgbd_dgf_refine_f32 on the GPU (csrc/dgf.hip) against the float64 comparator of tests/dgf_ref.py and its per-pixel bound, at
shapes placed around the kernel's tile (ops.DGF_TILE): every window clipped, s = 2 / 3 / 4, odd extents, one tile minus s, one tile,
one tile plus s, two tiles plus s per axis, and 256 x 384; noise guides and noise with a constant patch; n = 1 and 2.  Bit-for-bit
checks: n = 2 against two n = 1 calls, two runs, hipGraph replay, unaligned outputs; guard words and inputs untouched.  On the golden
fixtures the kernel's error against the reference's float64 output does not exceed the reference's own fp32 error."""
import functools

import numpy as np
import pytest
import torch

import dgf_ref
import gen_dgf_golden as gg
from neuralrgbd_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                  # floats on either side of the output
SENTINEL = -12345.5
SHAPES = dgf_ref.gpu_shapes(ops.DGF_TILE)


@functools.lru_cache(maxsize=None)
def _reference(h, w, s, patch):
    inp = dgf_ref.shape_inputs(h, w, s, patch)
    return inp, dgf_ref.dgf(*inp, bound=True)


def _run(dev_inputs, targets, offset=0):
    """dgf_refine of depth[targets] into a buffer between guard words, `offset` floats past a 16-byte boundary -> (out, guards ok)."""
    depth, img, w1, b1, w2, b2 = dev_inputs
    d = depth[targets].contiguous()
    n, (H, W) = d.shape[0], img.shape[1:]
    buf = torch.full((GUARD + offset + n * H * W + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[GUARD + offset:GUARD + offset + n * H * W]
    res = ops.dgf_refine(d, img, w1, b1, w2, b2, 1e-8, out=out)
    assert res.data_ptr() == out.data_ptr() and tuple(res.shape) == (n, 1, H, W)
    ok = bool((buf[:GUARD + offset] == SENTINEL).all()) and bool((buf[GUARD + offset + n * H * W:] == SENTINEL).all())
    return res[:, 0].clone(), ok


@pytest.mark.parametrize("patch", [False, True], ids=["noise", "patch"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_against_the_comparator(shape, patch):
    inp, (want, bound) = _reference(*shape, patch)
    dev = [torch.from_numpy(a).to(DEV) for a in inp]
    before = [t.clone() for t in dev]
    both, ok2 = _run(dev, [0, 1])
    first, ok0 = _run(dev, [0])
    second, ok1 = _run(dev, [1])
    again, _ = _run(dev, [0, 1])
    torch.cuda.synchronize()
    assert ok0 and ok1 and ok2, "guard words around the output were overwritten"
    assert all(torch.equal(a, b) for a, b in zip(dev, before)), "an input was written"
    assert ops.dgf_refine(*dev).data_ptr() % 16 == 0            # the default output is a fresh [n,1,H,W] tensor
    # |out - comparator| <= bound at every pixel, n = 1 and n = 2
    for name, got, w_, b_ in (("n=2", both, want, bound), ("n=1 [0]", first, want[:1], bound[:1]), ("n=1 [1]", second, want[1:], bound[1:])):
        err = np.abs(got.cpu().numpy().astype(np.float64) - w_)
        print("[dgf] %s %s %s: max |d| %.3e mean %.3e, worst |d| / bound %.4f" % (shape, "patch" if patch else "noise", name, err.max(),
                                                                               err.mean(), (err / b_).max()))
        assert np.isfinite(err).all() and (err <= b_).all()
    # a target's bits do not depend on n; two runs are identical
    assert torch.equal(both[0], first[0]) and torch.equal(both[1], second[0])
    assert torch.equal(again, both)
    # an output that starts 4, 8 or 12 bytes past a 16-byte boundary (and every odd W) takes the element stores: the same bits
    for offset in (1, 2, 3):
        moved, ok = _run(dev, [0, 1], offset)
        assert ok and torch.equal(moved, both), "offset %d" % offset
    H, W = both.shape[1:]
    inner = np.zeros((H, W), bool)
    inner[H // 3 + 2:H - H // 3 - 2, W // 3 + 2:W - W // 3 - 2] = True          # every window of every contributing A inside the patch
    if patch and inner.any():
        # where the guide is constant var = 0: the output is the double box mean of y, within the bound
        y, _ = dgf_ref.upsample(inp[0].astype(np.float64), H, W)
        err = np.abs(both.cpu().numpy().astype(np.float64) - dgf_ref.box_mean_twice(y))
        assert (err[:, inner] <= bound[:, inner]).all()


@pytest.mark.parametrize("case", sorted(gg.CASES))
def test_kernel_is_no_worse_than_the_reference_in_fp32(case):
    """max and mean of |out - reference float64| against the reference fp32's own (recorded in the fixture), margin 1 x: a kernel that
    sums nine values directly has no reason to be worse than differences of cumsums."""
    g = np.load(gg.path(case))
    dev = [torch.from_numpy(g[k]).to(DEV) for k in ("w1", "b1", "w2", "b2")]
    out = ops.dgf_refine(torch.from_numpy(g["depth"])[None].to(DEV), torch.from_numpy(g["img"]).to(DEV), *dev)[0, 0]
    err = np.abs(out.cpu().numpy().astype(np.float64) - g["ref64"])
    ref_max, ref_mean = g["ref32_err"]
    print("[dgf] golden %s: kernel max %.3e mean %.3e; reference fp32 max %.3e mean %.3e (ratios %.1f / %.1f)"
          % (case, err.max(), err.mean(), ref_max, ref_mean, ref_max / err.max(), ref_mean / err.mean()))
    assert err.max() <= ref_max and err.mean() <= ref_mean
    _, bound = dgf_ref.dgf(g["depth"][None], g["img"], g["w1"], g["b1"], g["w2"], g["b2"], bound=True)
    assert (err <= bound[0] + 1e-10).all()              # ref64 is within 1e-10 of the comparator (tests/test_dgf_host.py)


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[-2], SHAPES[-1]], ids=str)
def test_graph_replay_equals_eager(shape):
    from neuralrgbd_amd.distributed import graph_capture_mode
    inp, _ = _reference(*shape, False)
    dev = [torch.from_numpy(a).to(DEV) for a in inp]
    eager = ops.dgf_refine(*dev).clone()
    static = [t.clone() for t in dev]
    static[0].zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=graph_capture_mode()):
        out = ops.dgf_refine(*static)
    static[0].copy_(dev[0])                             # capture does not execute: the replays read the inputs as they are now
    g.replay()
    first = out.clone()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, eager) and torch.equal(out, eager)


def test_wrapper_refusals_on_the_device():
    from neuralrgbd_amd._lib import NrgbdError
    inp, _ = _reference(*SHAPES[2], False)
    depth, img, w1, b1, w2, b2 = [torch.from_numpy(a).to(DEV) for a in inp]
    with pytest.raises(NrgbdError, match="code -4"):
        ops.dgf_refine(depth, img, w1, b1, w2, b2, eps=-1.0)
    with pytest.raises(NrgbdError, match="code -4"):
        ops.dgf_refine(torch.cat([depth, depth[:1]]), img, w1, b1, w2, b2)
    with pytest.raises(NrgbdError, match="code -2"):
        ops.dgf_refine(depth[:, :2], img, w1, b1, w2, b2)
    with pytest.raises(ValueError):
        ops.dgf_refine(depth, img, w1[:32], b1, w2, b2)
    with pytest.raises(ValueError):
        ops.dgf_refine(depth, img, w1, b1, w2, b2, out=torch.empty(5, device=DEV))
    with pytest.raises(TypeError):
        ops.dgf_refine(depth.double(), img, w1, b1, w2, b2)
