"""GPU: nrgbd_icp_terms_photo_f32 against the restatement of tests/icp_photo_ref.py at icp_ref.TERMS_SIZES, with seeded pictures that
carry holes, NaN / inf colours and depth steps.  Each shape is a place the kernel can go wrong: (1,1,1) no pixel has four neighbours;
(5,7,1), (33,65,1) a partial wave and a partial workgroup; (48,64,2), (48,64,4) sub-sampling; (260,256,1) the grid-stride second
pass past 256 workgroups.

Gates.  `resid` equals nrgbd_icp_terms_f32's output on the same inputs bit for bit; `resid_photo` equals the fp32 restatement bit for
bit, the quiet NaNs included; both counts are exact.  Every term of the 28 sums has the same bits on both sides, so a sum of n = pairs
+ photometric pairs terms differs from the comparator's fsum by the order of its additions alone: |S_gpu - S_ref| <= gamma_{n-1} S|t|
(icp_ref.sum_bound; derived, not measured).  Two runs give the same bits.  Every buffer lies between guard words that must be intact
afterwards; the picture and the model colour are cut from larger NaN-filled allocations, and no NaN reaches a sum."""
import functools

import numpy as np
import pytest
import torch

import icp_photo_ref as pr
import icp_ref as ir
from neuralrgbd_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENT = -12345.5


class Guarded:
    """Named device buffers, each cut from a larger allocation with GUARD words of `fill` on either side."""

    def __init__(self):
        self._outer, self._inner, self._fill = {}, {}, {}

    def add(self, name, array=None, shape=None, dtype=torch.float32, fill=SENT):
        if array is not None:
            src = torch.from_numpy(np.ascontiguousarray(array))
            shape, dtype = tuple(src.shape), src.dtype
        n = int(np.prod(shape))
        outer = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        inner = outer[GUARD:GUARD + n].view(shape)
        if array is not None:
            inner.copy_(src)
        self._outer[name], self._inner[name], self._fill[name] = outer, inner, fill
        return inner

    def __getitem__(self, name):
        return self._inner[name]

    def intact(self):
        ok = True
        for name, outer in self._outer.items():
            n = self._inner[name].numel()
            guard = torch.cat([outer[:GUARD], outer[GUARD + n:]])
            ok = ok and bool((torch.isnan(guard) if self._fill[name] != self._fill[name] else guard == self._fill[name]).all())
        return ok


@functools.lru_cache(maxsize=None)
def _case(H, W, sub):
    """Inputs and the fp32 restatement of one size, computed once and shared (never modified)."""
    case = pr.make_photo_case(H, W, sub)
    return case, pr.terms_photo_of(np.float32, case)


def _buffers(case):
    H, W = case["depth"].shape
    g = Guarded()
    for name in ("depth", "gate", "mdepth", "mnormal"):
        g.add(name, case[name])
    for name in ("image", "mrgb"):
        g.add(name, case[name], fill=float("nan"))
    nwg = ops.icp_workgroups(H // case["sub"], W // case["sub"])
    g.add("state", shape=(ops.ICP_STATE_WORDS,), dtype=torch.float64)
    for name in ("partial", "partial_old"):
        g.add(name, shape=(nwg, ops.ICP_RECORD_WORDS), dtype=torch.float64)
    for name in ("resid", "resid_photo", "resid_old"):
        g.add(name, shape=(H, W))
    ops.icp_update(g["state"], 0, init=case["T"])
    return g, nwg


def _run(case, g, partial, resid, resid_photo):
    return ops.icp_terms_photo(g["depth"], case["K"], case["sub"], g["mdepth"], g["mnormal"], case["Km"], g["state"], partial,
                               case["dist_thr"], case["huber"], g["image"], g["mrgb"], case["photo_weight"], case["photo_huber"],
                               image_affine=case["affine"], depth_range=case["depth_range"], gate=g["gate"], gate_thr=case["gate_thr"],
                               resid=resid, resid_photo=resid_photo)


@pytest.mark.parametrize("H,W,sub", pr.TERMS_SIZES)
def test_photo_terms_against_the_restatement(H, W, sub):
    case, want = _case(H, W, sub)
    g, nwg = _buffers(case)
    old = ops.icp_terms(g["depth"], case["K"], sub, g["mdepth"], g["mnormal"], case["Km"], g["state"], g["partial_old"], case["dist_thr"],
                        case["huber"], depth_range=case["depth_range"], gate=g["gate"], gate_thr=case["gate_thr"], resid=g["resid_old"])
    got = _run(case, g, g["partial"], g["resid"], g["resid_photo"])
    torch.cuda.synchronize()
    assert got == old == nwg == ir.workgroups(H // sub, W // sub)
    assert g.intact(), "a guard word was overwritten"
    # the geometric half is the old entry's
    assert torch.equal(g["resid"].view(torch.int32), g["resid_old"].view(torch.int32)), "resid differs from nrgbd_icp_terms_f32's"
    resid = g["resid"].cpu().numpy()
    assert np.array_equal(resid.view(np.int32), want["resid"].view(np.int32))
    rp = g["resid_photo"].cpu().numpy()
    assert np.array_equal(np.isnan(rp), np.isnan(want["resid_photo"])), "the set of photometric pairs differs"
    assert np.array_equal(rp.view(np.int32), want["resid_photo"].view(np.int32)), "photometric residual bits differ"
    rec, rec_old = g["partial"].cpu().numpy(), g["partial_old"].cpu().numpy()
    count, pcount = int(rec[:, 28].view(np.int64).sum()), int(rec[:, 29].view(np.int64).sum())
    assert count == want["count"] == int(rec_old[:, 28].view(np.int64).sum()) and pcount == want["photo_count"]
    assert not rec_old[:, 29].any()                                 # the old entry still writes the padding word as 0
    assert np.isfinite(rec[:, :28]).all(), "a NaN reached a sum"
    S = ir.add_records(rec[:, :28])
    bound = ir.sum_bound(want["abs_sums"], count + pcount)
    diff = np.abs(S - want["sums"])
    with np.errstate(all="ignore"):
        print("[icp photo] %dx%d sub %d: %d pairs, %d photometric, in %d records; worst |S_gpu - fsum| / bound %.3g (worst diff %.3g)"
              % (H, W, sub, count, pcount, len(rec), np.nanmax(np.where(bound > 0, diff / bound, 0.0)) if count else 0.0, diff.max()))
    assert (diff <= bound).all(), (diff, bound)
    if pcount:                                                      # the photometric terms are in the sums
        assert (np.abs(S - ir.add_records(rec_old[:, :28])) > 0).any()
    # the same inputs give the same bits; without the residual maps the records are the same and the maps are not touched
    g.add("partial2", shape=(nwg, ops.ICP_RECORD_WORDS), dtype=torch.float64)
    g.add("untouched", shape=(H, W))
    _run(case, g, g["partial2"], None, None)
    torch.cuda.synchronize()
    assert torch.equal(g["partial2"].view(torch.int64), g["partial"].view(torch.int64))
    assert bool((g["untouched"] == SENT).all()) and g.intact()


def test_wrapper_refusals_on_the_device():
    from neuralrgbd_amd._lib import NrgbdError
    case, _ = _case(16, 16, 1)
    g, nwg = _buffers(case)
    args = (g["depth"], case["K"], 1, g["mdepth"], g["mnormal"], case["Km"], g["state"], g["partial"], 0.3, 0.05)
    with pytest.raises(NrgbdError, match="code -4"):
        ops.icp_terms_photo(*args, g["image"], g["mrgb"], 0.0, 0.1)
    with pytest.raises(NrgbdError, match="code -4"):
        ops.icp_terms_photo(*args, g["image"], g["mrgb"], 0.1, 0.1, image_affine=((1, 1, float("nan")), (0, 0, 0)))
    with pytest.raises(ValueError, match="image"):
        ops.icp_terms_photo(*args, g["image"][:, :8], g["mrgb"], 0.1, 0.1)
    with pytest.raises(ValueError, match="mrgb"):
        ops.icp_terms_photo(*args, g["image"], g["mrgb"][:2], 0.1, 0.1)
    with pytest.raises(ValueError, match="image_affine"):
        ops.icp_terms_photo(*args, g["image"], g["mrgb"], 0.1, 0.1, image_affine=((1, 1), (0, 0)))
    torch.cuda.synchronize()
    assert g.intact()
