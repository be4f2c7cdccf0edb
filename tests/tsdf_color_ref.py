"""Comparator and inputs of the colour carried through the TSDF volume (csrc/tsdf.hip, tsdf_extract.hpp, tsdf_raycast.hip;
include/nrgbd.h spells out the operation sequences: nrgbd_tsdf_integrate_color_f32, nrgbd_tsdf_extract_points_color /
nrgbd_tsdf_extract_mesh_color, nrgbd_tsdf_raycast_color_f32).

One numpy operation per operation of the header, in a given dtype: float32 is the kernels' arithmetic bit for bit, float64 the
yardstick; both read the same inputs (tsdf_ref's convention: every scalar rounded to float32 first, then promoted).  The cases, poses,
depth maps and the chain up to (t, w) are tsdf_ref's; the hit of a ray is tsdf_raycast_ref's.

Bounds of fp32 against float64 (u = 2^-24, first order; from the operation count, never from an output), with m = max |c| over the
colours that enter:
    c = image * a + b        the product rounds once, the sum once, on values of at most m (the image value is the same fp32 number on
                             both sides: the same pixel):                      e(c) = 2 u m
    C' = (C Wt + c w)/(Wt+w) a convex combination of C and c, so an inherited error is not amplified; its own roundings and the
                             relative error of the accumulated weight cost 8 u on a quantity of at most 1 in tsdf_ref's header (the
                             same argument, the same operations), here on one of at most m:
                                                                                e(C') <= max(e(C), e(c)) + 8 u m
    col = Ca + q (Cb - Ca)   the difference rounds once (u |Cb - Ca|), the product once (u |q (Cb - Ca)| <= u |Cb - Ca|), the sum once
                             (u |col| <= u m); inherited: e(Ca), e(Cb) combine convexly (q in [0, 1]) to at most e(C), twice where
                             the rounded difference is scaled, and q's own error scales the difference:
                                                    e(col) <= e(C) + (e(q) + 3 u) |Cb - Ca| + u m       (|Cb - Ca| bounded by what is
                             stored plus 2 e(C); the host test adds that term)
It holds on voxels where both evaluations took the same decisions and read the same depth pixel and the same colour pixel in every
view; the others count as flips, capped per case by the host test."""
import functools

import numpy as np

import tsdf_raycast_ref as rref
import tsdf_ref as ref
from neuralrgbd_amd import camera, fusion

U = ref.U
DEPTH_SIZES = ((7, 9), (48, 64))
VARIANTS = ("same", "x4", "odd", "one")
AFFINE = ((0.229, 0.224, 0.225), (0.485, 0.456, 0.406))            # a non-trivial affine: a = std, b = mean of the ingest


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def image_size(variant, size):
    H, W = size
    return {"same": (H, W), "x4": (4 * H, 4 * W), "odd": (13, 17), "one": (1, 1)}[variant]


def color_K(case, variant):
    """The colour intrinsics of a variant: the depth map's own at the depth size (uc is then u, bit for bit), the same fields of view
    at 4 x the size, and for the unrelated size a longer focal length with an off-centre principal point, which pushes part of the
    projections beyond the image: onto the clamp."""
    H, W = case["size"]
    Hc, Wc = image_size(variant, case["size"])
    if variant == "same":
        return tuple(case["K"])
    if variant == "odd":
        return (1.9 * Wc, 2.3 * Hc, 0.35 * Wc, 0.7 * Hc)
    if case["family"] == "edge":                                    # the edge family's intrinsics are hand-made: scale them
        fx, fy, cx, cy = case["K"]
        return (fx * Wc / W, fy * Hc / H, cx * Wc / W, cy * Hc / H)
    return fusion.intrinsics_at(camera.scannet_intrinsics(Wc, Hc), Hc, Wc)


@functools.lru_cache(maxsize=None)
def make_image(family, dims, size, variant, view, specials=True):
    """The colour image of a view, fp32 [3,Hc,Wc] in [0, 1); specials: a NaN pixel and an inf pixel (in one channel each) where the
    image has room for them."""
    Hc, Wc = image_size(variant, size)
    rng = np.random.RandomState(7000 + 100 * ref.FAMILIES.index(family) + 10 * ref.GRIDS.index(dims) + VARIANTS.index(variant) + 1000 * view
                                + ref.SIZES.index(size))
    img = rng.rand(3, Hc, Wc).astype(np.float32)
    if specials and Hc * Wc >= 4:
        at = rng.choice(Hc * Wc, 2, replace=False)
        img[0].reshape(-1)[at[0]] = np.nan
        img[2].reshape(-1)[at[1]] = np.inf
    return img


# ---- integration --------------------------------------------------------------------------------------------------------------------

def observe(dtype, case, view, image, Kc, affine=None, box=None, bound=False):
    """tsdf_ref.observe (ok, t, w, pix) and, for the voxels it marks, the colour: 'c' [3,Z,Y,X], 'fin' (ok and the three values
    finite), 'cpix' (icv Wc + icu where ok, else -1)."""
    out = ref.observe(dtype, case, view, box=box, bound=bound)
    ok = out["ok"]
    X, Y, Z = case["dims"]
    c = lambda v: dtype(np.float32(v))
    r = _f32(np.float32(case["views"][view]["extM"][:3, :4])).reshape(3, 4).astype(dtype)
    ox, oy, oz = (c(o) for o in case["origin"])
    vs = c(case["vs"])
    fi = [np.arange(n, dtype=np.float32).astype(dtype) for n in (X, Y, Z)]
    xw, yw, zw = ox + vs * fi[0], oy + vs * fi[1], oz + vs * fi[2]

    def row(k):
        a, b, cc = r[k, 0] * xw, r[k, 1] * yw, r[k, 2] * zw
        return ((a[None, None, :] + b[None, :, None]) + cc[:, None, None]) + r[k, 3]
    xc, yc, zc = row(0), row(1), row(2)
    Hc, Wc = image.shape[1:]
    fxc, fyc, cxc, cyc = (c(k) for k in Kc)
    a3, b3 = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)) if affine is None else affine
    with np.errstate(all="ignore"):
        uc = fxc * (xc / zc) + cxc
        vc = fyc * (yc / zc) + cyc
        uc = np.minimum(np.maximum(uc, dtype(0)), c(Wc - 1))
        vc = np.minimum(np.maximum(vc, dtype(0)), c(Hc - 1))
        icu = np.where(ok, np.floor(uc), 0).astype(np.int64)
        icv = np.where(ok, np.floor(vc), 0).astype(np.int64)
        col = [_f32(image)[j][icv, icu].astype(dtype) * c(a3[j]) + c(b3[j]) for j in range(3)]
        fin = ok & np.isfinite(col[0]) & np.isfinite(col[1]) & np.isfinite(col[2])
    out["c"] = np.stack([np.where(fin, v, 0) for v in col]).astype(dtype)
    out["fin"] = fin
    out["cpix"] = np.where(ok, icv * Wc + icu, -1)
    out["uc"] = np.where(ok, uc, 0)
    return out


def integrate(dtype, C, Wt, obs):
    """C_j' = (C_j Wt + c_j w) / (Wt + w) with the OLD Wt on the voxels obs['fin'] marks: [3,Z,Y,X] of `dtype`."""
    C, Wt, w = C.astype(dtype), Wt.astype(dtype), obs["w"].astype(dtype)
    with np.errstate(all="ignore"):
        den = Wt + w
        new = [(C[j] * Wt + obs["c"][j].astype(dtype) * w) / den for j in range(3)]
    return np.stack([np.where(obs["fin"], new[j], C[j]) for j in range(3)]).astype(dtype)


@functools.lru_cache(maxsize=None)
def fused(family, dims, size, variant, dtype_name="float32", affine=True, specials=True):
    """The colour volume of tsdf_ref.make_case(family, dims, size) after every view: [(T, W, C) after view 0, ...]."""
    dtype = getattr(np, dtype_name)
    case = ref.make_case(family, dims, size)
    X, Y, Z = dims
    T, Wt, C = np.zeros((Z, Y, X), dtype), np.zeros((Z, Y, X), dtype), np.zeros((3, Z, Y, X), dtype)
    out = []
    Kc = color_K(case, variant)
    for i in range(len(case["views"])):
        obs = observe(dtype, case, i, make_image(family, dims, size, variant, i, specials), Kc, AFFINE if affine else None)
        C = integrate(dtype, C, Wt, obs)
        T, Wt = ref.integrate(dtype, T, Wt, obs, case["w_max"])
        out.append((T, Wt, C))
    return out


# ---- extraction ---------------------------------------------------------------------------------------------------------------------

def extract(dtype, tsdf, weight, color, w_min, with_q=False):
    """The colours of nrgbd_tsdf_extract_points_color's points, [N,3] of `dtype` in tsdf_ref.extract's order (+ q, |Cb - Ca| [N,3])."""
    Z, Y, X = tsdf.shape
    T, Wt, C = _f32(tsdf).astype(dtype), _f32(weight).astype(dtype), np.asarray(color).astype(dtype)
    with np.errstate(all="ignore"):
        side = (Wt >= dtype(np.float32(w_min))) & (np.abs(T) < 1)
    neg = T < 0
    iz, iy, ix = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    lin = (iz * Y + iy) * X + ix
    keys, cols, qs, ds = [], [], [], []
    for k in range(3):
        ax = 2 - k
        sl_a, sl_b = [slice(None)] * 3, [slice(None)] * 3
        sl_a[ax], sl_b[ax] = slice(0, -1), slice(1, None)
        sl_a, sl_b = tuple(sl_a), tuple(sl_b)
        cross = side[sl_a] & side[sl_b] & (neg[sl_a] != neg[sl_b])
        Ta, Tb = T[sl_a][cross], T[sl_b][cross]
        with np.errstate(all="ignore"):
            q = Ta / (Ta - Tb)
            Ca = [C[j][sl_a][cross] for j in range(3)]
            Cb = [C[j][sl_b][cross] for j in range(3)]
            cols.append(np.stack([Ca[j] + q * (Cb[j] - Ca[j]) for j in range(3)], axis=1).reshape(-1, 3))
            ds.append(np.stack([np.abs(Cb[j] - Ca[j]) for j in range(3)], axis=1).reshape(-1, 3))
        qs.append(q)
        keys.append(lin[sl_a][cross] * 3 + k)
    order = np.argsort(np.concatenate(keys), kind="stable")
    cols = np.concatenate(cols)[order].astype(dtype)
    if with_q:
        return cols, np.concatenate(qs)[order], np.concatenate(ds)[order]
    return cols


# ---- the ray cast -------------------------------------------------------------------------------------------------------------------

def raycast(dtype, cast, Wt, color, origin, vs, extM, K, size, w_min):
    """rgb [3,H,W] of nrgbd_tsdf_raycast_color_f32 from tsdf_raycast_ref.raycast's result `cast` (its 'depth' and 'hit') of the same
    dtype and arguments."""
    H, W = size
    Z, Y, X = Wt.shape
    dims = (X, Y, Z)
    Wt, C = np.asarray(Wt).astype(dtype), np.asarray(color).astype(dtype)
    c = lambda v: dtype(np.float32(v))
    pose32 = np.ascontiguousarray(np.asarray(extM)[:3, :4], dtype=np.float32)
    r = pose32.astype(dtype)
    centre = rref.camera_centre(pose32).astype(dtype)
    o = [c(v) for v in origin]
    vs, w_min = c(vs), c(w_min)
    fx, fy, cx, cy = (c(k) for k in K)
    P = H * W
    depth, hit = cast["depth"].reshape(P).astype(dtype), cast["hit"].reshape(P)
    rgb = np.zeros((3, P), dtype)
    rows = np.flatnonzero(hit)
    with np.errstate(all="ignore"):
        xn = np.broadcast_to((((np.arange(W, dtype=np.float32).astype(dtype) + dtype(0.5)) - cx) / fx)[None, :], (H, W)).reshape(P)
        yn = np.broadcast_to((((np.arange(H, dtype=np.float32).astype(dtype) + dtype(0.5)) - cy) / fy)[:, None], (H, W)).reshape(P)
        d = [(r[0, k] * xn + r[1, k] * yn) + r[2, k] for k in range(3)]
        go = [(centre[k] - o[k]) / vs for k in range(3)]
        gd = [d[k] / vs for k in range(3)]
        p = [go[a] + depth[rows] * gd[a][rows] for a in range(3)]
        ok = rref._inside(dtype, p, dims)
        p = [np.where(ok, p[a], 0) for a in range(3)]
        i, f = rref._cell(dtype, p, dims)
        w = rref._corners(Wt, i)
        for j in range(8):
            ok &= w[j] >= w_min
        for j in range(3):
            rgb[j, rows] = np.where(ok, rref._trilinear(rref._corners(C[j], i), f), 0)
    return rgb.reshape(3, H, W), p, ok, rows


def affine_field(dims, coef, dtype=np.float32):
    """A colour volume that is an affine function of the lattice index with small-integer coefficients: plane j holds
    coef[j][0] + coef[j][1] ix + coef[j][2] iy + coef[j][3] iz, exact in fp32."""
    X, Y, Z = dims
    iz, iy, ix = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return np.stack([k[0] + k[1] * ix + k[2] * iy + k[3] * iz for k in coef]).astype(dtype)
