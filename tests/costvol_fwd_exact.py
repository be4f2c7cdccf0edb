"""Inputs, comparator and bounds of the cost-volume FORWARD (csrc/costvol.hip `gather`, csrc/costvol_lds.hip `lds`, csrc/costvol_quad.hip
`quad`, selected by the generation argument of nrgbd_costvol_fwd_gen).

`make_case(h, w, D, V, C, family, seed)` takes the geometry and the features of warp_exact.make_case (Cs plays C; families small,
large, behind, zoom_far, on_plane, border: see there) or, for "scatter", of costvol_bwd_exact.make_case (candidates in a strided,
non-monotonic order, which the C ABI allows), and sigma = 3.  `exact(case, dist, align)` is costvol_bwd_exact.exact_cost, unchanged
and computed once: positions from cpu_oracle.sweep_positions (the kernels' own fp32 chain, bit for bit), everything after them in
float64, and per element

    bound_k = 2 / sigma  sum_v [ sum_c eterm  +  (C + 2 + V) u sum_c term ],      e = 8 u (sum |w tap| + |ref|),  u = 2^-24,
    term = df^2, eterm = 2 |df| e + e^2  (L2);    term = |df|, eterm = e  (L1).

The bound was derived for the oracle's sequence (one rounding per operation).  What follows walks the sequences of the kernels
that differ from it and counts their roundings against the same three budgets: 8 per tap term on df, C + 1 on the channel sum and
the division, V on the view sum.  (First order in u throughout; the factor 2 in front carries the higher orders.)

  weights (all generations: tap_weights / bilinear_zeros)  1 - fx, 1 - fy, their product: 3 roundings on a weight, as in the oracle
      (fx = ix - floor(ix) is exact wherever the tap is valid, except in (-1, 0) where its rounding takes the place of 1 - fx).
  oracle  s = ((A nw + B ne) + C sw) + D se, df = s - ref: the nw term meets its product, three additions and the subtraction (5),
      with its weight 8; ne 8, sw 7, se 6, ref 1.  Each rounding is relative to a partial sum that is at most sum |w tap| + |ref|:
      |df_fp32 - df| <= 8 u (sum |w tap| + |ref|) = e.
  gather, lds, gather_point (lerp4, then - ref)  A nw, three fma, one subtraction: 5 roundings of partial sums + 3 of the weight
      = 8 for nw, fewer for the others.  Covered by e.
  quad word_acc  lo = fma(A, nw, -ref), then three fma: the chain STARTS from -ref, so ref meets 4 roundings instead of 1 and the
      nw term 4 + 3 = 7.  Every partial sum is still bounded by sum |w tap| + |ref|, the worst count is 7 <= 8.  Covered by e.
  quad rgb_word  fma(D, se, fma(C, sw, fma(B, ne, A nw))) - ref: lerp4's count (8).  Its distance is s * s (one rounding) added to
      an accumulator that starts at 0; the channels beyond `tail` add an exact 0.
  channel sum  C non-negative terms.  Oracle: C products (1 each) and C - 1 additions in sequence: a term meets at most C roundings;
      division by sigma 1: C + 1 <= C + 2.  Any other order of the same additions gives a term no more than C - 1 of them, and an
      fma folds the product's rounding into the addition's:
        gather      one fma chain over the words in order: C roundings at most;
        lds         two 2-wide chains pa / pb per channel block (at most 9 words = 9 fma each), pa + pb, .x + .y, acc += part per
                    block.  Cp = 68 has TWO blocks: block 0 computes words 0 .. 8, block 1 stages words 8 .. 16 (it overlaps its
                    predecessor by one word so that both stage 9) and computes words 9 .. 16 only (L0 = 1): every channel is
                    counted once, a term meets at most 9 + 2 + 2 roundings;
        quad        per lane 4 words into pa / pb (4 fma each), pa + pb, .x + .y, two DPP additions over the quad, + the RGB
                    word's partial sum (product 1 + at most 3 additions): at most 10 roundings;
        zero_sample_dist (lds with nothing in view, gather_point with four zero weights)  s = 0 - ref is exact and equals the
                    comparator's df there (every weight is exactly 0); then the same fma chain as above over the words.
      All are <= C for every C tested except C = 7 (lds: 2 fma + 2 + 1 = 5 <= 7).  The division is IEEE (`/`, contraction off) in
      gather and lds and div_by_const in quad (the correctly rounded quotient; were it one ulp off, C + 2 has that one to spare).
  view sum  total = total + acc / sigma in view order, starting from an exact 0 (quad: in its LDS accumulators, `prev + ...` with
      prev = 0 for the first view): V - 1 roundings <= V.
  L1  |df| is exact given df; the sums are the same.

No sequence needed an extension of the derivation.  The bound is derived from the arithmetic, never from what a kernel gives.

Log-probabilities (log_softmax of -cost over the candidates) are held two ways:
  `logp_bound`       against float64 log_softmax(-exact): logp_k = z_k - lse(z) and |d lse| <= max_j |d z_j|, so the cost bound
                     propagates as b_k + max_j b_j; plus the project's contract of 1e-4 for log-probability volumes
                     (tests/test_gpu_ops.py) for the soft-max's own arithmetic;
  `logp_self_bound`  against float64 log_softmax of the cost the kernel itself returned: 4 u (|z_k - m| + |logp_k|) for the two
                     fp32 subtractions (z_k - m) - log(sum), doubled, + 5e-6 for exp / log / the sum at D <= 128 (what
                     test_logsoftmax_and_nll_training_kernels_vs_torch_fp64 grants the same arithmetic).  |logp| reaches ~115 in
                     the border family: a flat absolute figure would be wrong.

`fp32_cost(case, dist, align, variant)` is a numpy fp32 evaluation from the same positions, for the host test only: "plain" follows
the rule; "reject_behind" (samples with a negative denominator contribute nothing), "border_lt" (x1 valid iff x1 < w - 1), "trunc"
(trunc for floor) and "shift" (ix moved by 2^-10 texel) are deliberately wrong and must be caught by the bound at the families
that aim at them: a condition on the inputs, checked without a GPU by tests/test_costvol_fwd_host.py.

`quad_branches` and `lds_branches` restate the two staged generations' footprint rules on the host (corner boxes, `bad` planes, the
launchers' chunks and single-candidate workgroups, the run selection) and count which branches a case reaches: patches inside the
image and on its apron, groups from global memory, "nothing in view", the per-candidate split and the direct-gather fallback.
They say what the matrix exercises; no kernel result is judged by them.
"""
import numpy as np

import costvol_bwd_exact as cx
import warp_exact as wx
from oracle import cpu_oracle as co

U = 2.0 ** -24
SIGMA = 3.0
FAMILIES = wx.FAMILIES + ("scatter",)
L1_FAMILIES = ("large", "behind", "border")
VARIANTS = ("plain", "reject_behind", "border_lt", "trunc", "shift")
LOGP_CONTRACT = 1e-4
LOGP_SELF_ABS = 5e-6

# (h, w, D, V, C) -> the generations that run it: the smallest shapes that reach each branch of the three kernels.  On grids this
# small the lds launcher gives each of the first 8 candidates a workgroup of its own; groups of up to 8 follow.
SHAPES = [
    ((17, 23, 9, 2, 64), ("quad", "lds", "gather")),    # ragged 8x8 and 16x16 tiles; 9 quad tiles in plain order; Cp = 64: no RGB word; fused soft-max; lds 8 singles + a group of 1
    ((16, 32, 5, 4, 67), ("quad", "lds", "gather")),    # the grid where `border` is exact; 8 tiles: the XCD band map; tail 3; Cp4 = 17: two channel blocks; lds 5 singles
    ((24, 40, 12, 3, 67), ("quad", "lds", "gather")),   # 15 tiles; quad nchunk 1 with 3 groups of 4; lds 8 singles + a group of 4 on 2 x 3 ragged tiles
    ((24, 40, 40, 3, 67), ("quad", "lds")),             # quad nchunk 4 (chunks of 10, separate soft-max launch, plain map); lds 8 singles + 4 groups of 8
    ((24, 40, 12, 3, 65), ("quad",)),                   # run-time tail: one valid channel in the RGB word
    ((20, 36, 8, 2, 7), ("lds", "gather")),             # the Cp4 = 2 instantiation
    ((20, 36, 8, 2, 21), ("gather",)),                  # Cp4 = 6: the generic gather kernel; lds and quad must refuse it
]
UNSUPPORTED = [((20, 36, 8, 2, 21), ("lds", "quad"))]


def matrix():
    """[(shape, family, dist, align)]: every shape x 7 families x both align_corners at L2, and L1 at large, behind and border."""
    out = []
    for shape, _ in SHAPES:
        for align in (False, True):
            out += [(shape, f, "L2", align) for f in FAMILIES]
            out += [(shape, f, "L1", align) for f in L1_FAMILIES]
    return out


_cases = {}
_exact = {}


def make_case(h, w, D, V, C, family="small", seed=0):
    key = ("fwd", h, w, D, V, C, family, seed)
    if key not in _cases:
        base = cx.make_case(h, w, D, V, C, "scatter", seed=seed) if family == "scatter" else wx.make_case(h, w, D, V, C, family, seed)
        case = dict(base)
        case["sigma"] = SIGMA
        case["key"] = key
        _cases[key] = case
    return _cases[key]


def exact(case, dist="L2", align=False):
    """(cost [D,h,w] float64, bound [D,h,w]) of costvol_bwd_exact.exact_cost, once per (case, dist, align)."""
    key = (case["key"], dist, bool(align))
    if key not in _exact:
        _exact[key] = cx.exact_cost(case, dist, bool(align))
    return _exact[key]


def oracle_cost(case, dist="L2", align=False):
    return co.costvol(case["ref"], case["src"], case["KR"], case["Kt"], case["rays"], case["d_candi"], case["cx"], case["cy"],
                      case["sigma"], dist=dist, align_corners=bool(align))


def positions(case, align=False):
    V, C, h, w = case["src"].shape
    return co.sweep_positions(case["KR"], case["Kt"], case["rays"], case["d_candi"], case["cx"], case["cy"], h, w, bool(align))


def log_softmax64(z):
    """float64 log_softmax over axis 0."""
    z = np.asarray(z, np.float64)
    e = z - z.max(axis=0, keepdims=True)
    return e - np.log(np.exp(e).sum(axis=0, keepdims=True))


def logp_bound(bound):
    """Tolerance per element of logp against log_softmax64(-exact cost), from the cost's bound [D,h,w]."""
    return bound + bound.max(axis=0, keepdims=True) + LOGP_CONTRACT


def logp_self_bound(cost_got):
    """(float64 log_softmax of minus the cost a kernel returned, tolerance per element of the logp it returned with it)."""
    z = -np.asarray(cost_got, np.float64)
    want = log_softmax64(z)
    return want, 4.0 * U * (np.abs(z - z.max(axis=0, keepdims=True)) + np.abs(want)) + LOGP_SELF_ABS


def fp32_cost(case, dist="L2", align=False, variant="plain"):
    """The cost [D,h,w] evaluated in numpy fp32 (one rounding per operation) from the oracle's positions; see the module docstring
    for the deliberately wrong variants."""
    if variant not in VARIANTS:
        raise ValueError(variant)
    f32 = np.float32
    V, C, h, w = case["src"].shape
    D, hw = len(case["d_candi"]), h * w
    ix_all, iy_all = positions(case, align)
    den = wx.denominators(case) if variant == "reject_behind" else None           # [V,D,hw]
    ref = np.ascontiguousarray(case["ref"].reshape(C, hw).T)                      # [hw,C]
    total = np.zeros((D, hw), f32)
    for v in range(V):
        src = np.ascontiguousarray(case["src"][v].reshape(C, hw).T)
        ix, iy = ix_all[v].reshape(-1), iy_all[v].reshape(-1)
        if variant == "shift":
            ix = ix + f32(2.0 ** -10)
        rnd = np.trunc if variant == "trunc" else np.floor
        x0, y0 = rnd(ix), rnd(iy)
        fx, fy = ix - x0, iy - y0
        ex, ey = f32(1) - fx, f32(1) - fy
        x1, y1 = x0 + f32(1), y0 + f32(1)
        vx0, vy0 = (x0 >= 0) & (x0 <= w - 1), (y0 >= 0) & (y0 <= h - 1)
        vx1, vy1 = (x1 >= 0) & ((x1 < w - 1) if variant == "border_lt" else (x1 <= w - 1)), (y1 >= 0) & (y1 <= h - 1)
        s = np.zeros((D * hw, C), f32)
        for k, (vx, vy, xf, yf, wgt) in enumerate(((vx0, vy0, x0, y0, ey * ex), (vx1, vy0, x1, y0, ey * fx),
                                                   (vx0, vy1, x0, y1, fy * ex), (vx1, vy1, x1, y1, fy * fx))):
            ok = vx & vy
            if den is not None:
                ok = ok & ~(den[v].reshape(-1) < 0)
            idx = np.where(ok, yf, 0).astype(np.int64) * w + np.where(ok, xf, 0).astype(np.int64)
            tap = np.where(ok[:, None], src[idx], f32(0)) * wgt[:, None]
            s = tap if k == 0 else s + tap
        df = (s.reshape(D, hw, C) - ref[None]).astype(f32)
        term = df * df if dist == "L2" else np.abs(df)
        acc = term.sum(axis=2, dtype=f32)
        total = total + acc / f32(case["sigma"])
    assert total.dtype == f32
    return total.reshape(D, h, w)


def population(case, align=False):
    """Over the V * D * h * w samples of a case: partly / wholly outside the source image, behind the source camera (fp32
    denominator < 0; behind_in_image: those mirrored onto a valid tap), planes (view, candidate) whose denominator is 1e-10 on
    every pixel, and how often a position equals a given value (at_x, at_y)."""
    V, C, h, w = case["src"].shape
    ix, iy = positions(case, align)
    _, _, valid = cx._taps(ix.reshape(-1), iy.reshape(-1), h, w)
    nv = sum(x.astype(np.int64) for x in valid)
    den = wx.denominators(case)
    behind = (den < 0).reshape(-1)
    return {"samples": int(nv.size), "partly_outside": int(((nv > 0) & (nv < 4)).sum()), "wholly_outside": int((nv == 0).sum()),
            "behind": int(behind.sum()), "behind_in_image": int((behind & (nv > 0)).sum()),
            "planes_at_min_den": int((den == np.float32(1e-10)).all(axis=2).sum()),
            "at_x": lambda val: int((ix == np.float32(val)).sum()), "at_y": lambda val: int((iy == np.float32(val)).sum())}


def _corner_boxes(case, align, tile):
    """Per (view, candidate, tile row, tile column): the extremes of the four corner pixels' positions (xmin, xmax, ymin, ymax) and
    `bad` (a corner with a denominator <= 0 or a position of 1e8 or beyond): what quad_boxes and region_box start from."""
    V, C, h, w = case["src"].shape
    D = len(case["d_candi"])
    ix, iy = positions(case, align)
    den = wx.denominators(case).reshape(V, D, h, w)
    y0, x0 = np.arange(0, h, tile), np.arange(0, w, tile)
    y1, x1 = np.minimum(y0 + tile - 1, h - 1), np.minimum(x0 + tile - 1, w - 1)
    corners = [(ya[:, None], xa[None, :]) for ya in (y0, y1) for xa in (x0, x1)]
    cxs = np.stack([ix[:, :, ya, xa] for ya, xa in corners])                      # [4,V,D,ty,tx]
    cys = np.stack([iy[:, :, ya, xa] for ya, xa in corners])
    cden = np.stack([den[:, :, ya, xa] for ya, xa in corners])
    with np.errstate(invalid="ignore"):
        bad = ~((cden > 0) & (np.abs(cxs) < 1e8) & (np.abs(cys) < 1e8)).all(axis=0)
    return cxs.min(0), cxs.max(0), cys.min(0), cys.max(0), bad


def quad_branches(case, align=False):
    """Which branches of costvol_quad.hip a case reaches, from a host restatement of its footprint rule (quad_boxes, the launcher's
    candidate chunks, quad_pick_run): counts over (view, tile, chunk, pass) of staged runs (interior / touching the one-texel apron),
    of groups taken straight from global memory, of unbounded (`bad`) planes, and the launcher's nchunk."""
    V, C, h, w = case["src"].shape
    D = len(case["d_candi"])
    f32 = np.float32
    xmin, xmax, ymin, ymax, bad = _corner_boxes(case, align, 8)
    g = f32(0.015625)
    bx0 = np.clip(np.floor(np.maximum(xmin, f32(-4)) - g).astype(np.int64), -1, w - 1)
    bx1 = np.minimum(np.maximum(np.floor(np.minimum(xmax, f32(w + 4)) + g).astype(np.int64) + 1, bx0 + 1), w)
    by0 = np.clip(np.floor(np.maximum(ymin, f32(-4)) - g).astype(np.int64), -1, h - 1)
    by1 = np.minimum(np.maximum(np.floor(np.minimum(ymax, f32(h + 4)) + g).astype(np.int64) + 1, by0 + 1), h)
    big = 1 << 20
    bx0, bx1, by0, by1 = np.where(bad, -big, bx0), np.where(bad, big, bx1), np.where(bad, -big, by0), np.where(bad, big, by1)
    tiles = bad.shape[2] * bad.shape[3]
    nchunk = 1
    while tiles * nchunk < 768 and -(-D // (2 * nchunk)) >= 8:
        nchunk *= 2
    kchunk = -(-D // nchunk)
    out = {"nchunk": nchunk, "tiles": tiles, "bad_planes": int(bad.sum()), "staged_interior": 0, "staged_apron": 0, "staged_candidates": 0,
           "global_groups": 0, "longest_run": 0}
    for v in range(V):
        for ty in range(bad.shape[2]):
            for tx in range(bad.shape[3]):
                for kb_all in range(0, D, kchunk):
                    ke_all = min(D, kb_all + kchunk)
                    for kb in range(kb_all, ke_all, 32):
                        ke, lo = min(ke_all, kb + 32), kb
                        while lo < ke:
                            nmax, n = min(32, ke - lo), 0
                            u = [1 << 30, -(1 << 30), 1 << 30, -(1 << 30)]
                            box = None
                            for c in range(lo, lo + nmax):
                                u = [min(u[0], bx0[v, c, ty, tx]), max(u[1], bx1[v, c, ty, tx]), min(u[2], by0[v, c, ty, tx]), max(u[3], by1[v, c, ty, tx])]
                                bw, bh = u[1] - u[0] + 1, u[3] - u[2] + 1
                                if not (bw <= 156 and bh <= 156 and bw * bh <= 156):
                                    break
                                n, box = n + 1, list(u)
                            if n >= 2:
                                inside = box[0] >= 0 and box[2] >= 0 and box[1] <= w - 1 and box[3] <= h - 1
                                out["staged_interior" if inside else "staged_apron"] += 1
                                out["staged_candidates"] += n
                                out["longest_run"] = max(out["longest_run"], n)
                            else:
                                n = min(4, nmax)
                                out["global_groups"] += 1
                            lo += n
    return out


def lds_branches(case, align=False):
    """Which branches of costvol_lds.hip a case reaches, from a host restatement of region_box, the launcher's single-candidate
    workgroups and the run selection: counts over (view, tile, workgroup) of runs staged (by length), runs with nothing in view,
    candidates gathered directly (footprint unbounded or larger than the patch), and unbounded planes."""
    V, C, h, w = case["src"].shape
    D = len(case["d_candi"])
    f32 = np.float32
    cp4 = (C + 3) // 4
    pmax = 4032 // (min(cp4, 9) | 1)
    xmin, xmax, ymin, ymax, bad = _corner_boxes(case, align, 16)
    bx0 = np.maximum(np.floor(np.maximum(xmin, f32(-4))).astype(np.int64) - 1, 0)
    bx1 = np.minimum(np.floor(np.minimum(xmax, f32(w + 4))).astype(np.int64) + 2, w - 1)
    by0 = np.maximum(np.floor(np.maximum(ymin, f32(-4))).astype(np.int64) - 1, 0)
    by1 = np.minimum(np.floor(np.minimum(ymax, f32(h + 4))).astype(np.int64) + 2, h - 1)
    empty = ~bad & ((bx0 > bx1) | (by0 > by1))
    tiles = bad.shape[2] * bad.shape[3]
    nsingle = min(D, 8) if tiles * -(-D // 8) < 4 * 256 else 0
    groups = [(k, 1) for k in range(nsingle)] + [(k, min(8, D - k)) for k in range(nsingle, D, 8)]
    out = {"nsingle": nsingle, "groups": len(groups), "bad_planes": int(bad.sum()), "empty_planes": int(empty.sum()), "staged_runs": {},
           "nothing_in_view": 0, "gathered": 0}
    for v in range(V):
        for ty in range(bad.shape[2]):
            for tx in range(bad.shape[3]):
                for k0, nk in groups:
                    j0 = 0
                    while j0 < nk:
                        n, state = 8, None
                        while n >= 1:
                            if (j0 & (n - 1)) or j0 + n > nk:
                                n >>= 1
                                continue
                            ks = [k for k in range(k0 + j0, k0 + j0 + n) if not empty[v, k, ty, tx]]
                            if not ks:
                                state = "nothing_in_view"
                                break
                            if not any(bad[v, k, ty, tx] for k in ks):
                                area = (max(bx1[v, k, ty, tx] for k in ks) - min(bx0[v, k, ty, tx] for k in ks) + 1) * \
                                       (max(by1[v, k, ty, tx] for k in ks) - min(by0[v, k, ty, tx] for k in ks) + 1)
                                if area <= pmax:
                                    state = "staged"
                                    break
                            n >>= 1
                        if state == "staged":
                            out["staged_runs"][n] = out["staged_runs"].get(n, 0) + 1
                            j0 += n
                        elif state == "nothing_in_view":
                            out["nothing_in_view"] += 1
                            j0 += n
                        else:
                            out["gathered"] += 1
                            j0 += 1
    return out


worst_ratio = cx.worst_ratio
