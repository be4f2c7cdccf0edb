"""What the GPU tests of the cost-volume backward share (tests/test_gpu_costvol_bwd.py: the atomic kernels, tests/test_gpu_costvol_bwd_det.py:
the bit-reproducible path): upload of a tests/costvol_bwd_exact.py case, one call of ops.costvol_bwd on it, and the element-by-element
comparison with the exact-position float64 comparator at 1 x its bound.  A plain module, imported by name."""
import numpy as np
import torch

import costvol_bwd_exact as cx
from neuralrgbd_amd import ops

DEV = "cuda:0"

# shapes whose 16-byte channel word of one source view fits in LDS (the atomic side runs its LDS kernel on them)
LDS_SHAPES = [
    (64, 96, 64, 4, 67, "driver"),     # the training shape: slices = CUs / (V Cp / 4), long same-cell runs on the far planes
    (64, 96, 16, 2, 67, "small"),
    (33, 47, 1, 3, 5, "small"),        # fewer candidates than slices
    (33, 47, 2, 3, 5, "small"),
    (9, 11, 6, 2, 3, "small"), (33, 47, 6, 2, 3, "small"),      # every ncomp of the last channel word, hw no multiple of the block
    (33, 47, 6, 2, 4, "small"), (33, 47, 6, 2, 5, "large"), (33, 47, 6, 2, 64, "small"), (33, 47, 6, 2, 67, "large"),
]


def _upload(case):
    V, C, h, w = case["src"].shape
    Cp = ops.padded_channels(C)
    tex = torch.zeros(V + 1, h, w, Cp)
    tex[:V, ..., :C] = torch.from_numpy(case["src"]).permute(0, 2, 3, 1)
    tex[V, ..., :C] = torch.from_numpy(case["ref"]).permute(1, 2, 0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return tex.to(DEV), dev(case["KR"]), dev(case["Kt"]), dev(case["rays"]), dev(case["d_candi"]), dev(case["g_cost"])


def _nchw(g_ref, g_src):
    return g_ref.permute(2, 0, 1).cpu().numpy(), g_src.permute(0, 3, 1, 2).cpu().numpy()


def _run(case, dist, align, deterministic=False, stream=None):
    """ops.costvol_bwd on the case -> (g_ref [Cp,h,w], g_src [V,Cp,h,w]) as numpy."""
    V, C = case["src"].shape[:2]
    tex, KR, Kt, rays, d, g = _upload(case)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):                    # None: the current stream
        out = ops.costvol_bwd(tex[V], tex[:V], KR, Kt, rays, d, case["cx"], case["cy"], case["sigma"], C, g, dist=dist,
                              align_corners=align, deterministic=deterministic)
    torch.cuda.synchronize()
    return _nchw(*out)


def _where(name, at, ex):
    if name == "g_ref":
        c, y, x = at
        return "g_ref channel %d pixel (%d, %d), %d terms" % (c, y, x, ex["n_ref"][y, x])
    v, c, y, x = at
    return "g_src view %d channel %d texel (%d, %d), %d terms (%d whatever g)" % (v, c, y, x, ex["n_src"][v, y, x], ex["reach_src"][v, y, x])


def _compare(label, case, dist, align, got_ref, got_src, tag):
    """Assert both gradients within 1 x bound of the comparator; returns the comparator's result.  tag names the path in the
    printed line (costvol_bwd or costvol_bwd_det)."""
    V, C, h, w = case["src"].shape
    ex = cx.exact_case(case, dist, align)
    share = ex["ties"] / max(1, ex["elements"]) if dist == "L1" else 0.0
    r_ref, at_ref, bad_ref = cx.worst_ratio(got_ref[:C], ex["g_ref"], ex["bound_ref"])
    r_src, at_src, bad_src = cx.worst_ratio(got_src[:, :C], ex["g_src"], ex["bound_src"])
    print("[parity] %-56s %s align=%d: worst error / bound g_ref %.3f g_src %.3f, tie share %.1e, max |g_ref| %.1f |g_src| %.1f"
          % (tag + " " + label, dist, align, r_ref, r_src, share, np.abs(ex["g_ref"]).max(), np.abs(ex["g_src"]).max()))
    assert share <= cx.TIE_CAP
    assert np.abs(ex["g_src"]).max() > 0 and np.abs(ex["g_ref"]).max() > 0
    assert bad_ref == 0, "%d elements beyond the bound, worst %.2f x at %s" % (bad_ref, r_ref, _where("g_ref", at_ref, ex))
    assert bad_src == 0, "%d elements beyond the bound, worst %.2f x at %s" % (bad_src, r_src, _where("g_src", at_src, ex))
    # the padding lanes C ... Cp-1 carry no gradient
    assert (got_ref[C:] == 0).all() and (got_src[:, C:] == 0).all()
    return ex
