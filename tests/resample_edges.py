"""Edge inputs of PREDICT (csrc/resample.hpp, resample.hip: dpv_resample / dpv_resample_to), and what each of them holds.

The reference of the GPU test is cpu_oracle.dpv_resample: resample_vol_cuda restated in the same operation order in fp32.

GATE.  Per output element the kernel and the oracle may differ by at most

    gate = 24 * 2^-24 * max(max |dpv|, |pad|)

if they take their taps in the same cell.  One output is sum_i tap_i w_i over up to eight corners.  Roundings between the (shared)
clipped coordinates and the output: the three weight differences (x0 + 1) - fx, ... (3; fx - x0 is exact), two products per corner
weight (2), the product with the tap (1), up to seven additions (7; the first adds to 0): at most 12 on the path of any one term, each
relative to a partial sum bounded by sum_i |tap_i| w_i <= max |tap| (the trilinear weights sum to at most 1).  Doubled: 24.  The clamp
is monotone and does not expand differences.  If the build's arithmetic is operation for operation the oracle's, the difference is 0.
A difference beyond the gate means another cell or another weight: a finding, not something a wider gate may absorb.

`population(...)` restates the oracle's coordinate chain in numpy fp32 (one rounding per operation; the fma of the pose chain through
float64, where the product of two fp32 numbers is exact: a double rounding in about one input in 2^29, immaterial for counts) and
counts, over the D_out * h * w output voxels: coordinates clipped at 0 and at size - 1 per axis (the latter are the dropped x1 / y1 /
z1 taps), footprints that touch each of the six pad faces with a non-zero weight, points behind the camera (q_z + 1e-10 < 0), points
with q_z = 0 exactly, non-finite coordinates, and whether every tap index lies inside the volume.
"""
import math

import numpy as np

from neuralrgbd_amd import camera, synth
from oracle import cpu_oracle as co

U = 2.0 ** -24
GATE_C = 24.0
GRIDS = [(7, 9), (20, 36)]
DEPTHS = [1, 2, 8]
POSES = ("identity", "right_up", "left_down", "forward", "backward", "on_plane", "rot")

_cases = {}


def candidates(D):
    return np.linspace(0.3, 5.0, D).astype(np.float32) if D > 1 else np.array([1.5], np.float32)


def pose(name, d, seed=0):
    T = np.eye(4, dtype=np.float32)
    if name == "right_up":
        T[:3, 3] = (0.4, -0.3, 0.0)
    elif name == "left_down":
        T[:3, 3] = (-0.4, 0.3, 0.0)
    elif name == "forward":
        T[2, 3] = 1.5
    elif name == "backward":
        T[2, 3] = -1.2
    elif name == "on_plane":                     # q_z = fma(-d_k, 1, 1 * (d_k * 1)) = 0 exactly on plane k
        T[2, 3] = -d[len(d) // 2]
    elif name == "rot":
        T = np.linalg.inv(synth.random_pose(np.random.RandomState(12 + seed), 0.2, 0.5)).astype(np.float32)
    elif name == "nonfinite":                    # see test_non_finite_pose_entry
        T[0, 3], T[1, 3] = np.nan, np.inf
    elif name != "identity":
        raise ValueError(name)
    return T


def make_case(h, w, D, values="logp", seed=0):
    key = (h, w, D, values, seed)
    if key in _cases:
        return _cases[key]
    cam = camera.scannet_intrinsics(w, h)
    rng = np.random.RandomState(100 * seed + 7 * h + 3 * w + D)
    if values == "logp":                         # realistic log-probabilities
        dpv = rng.uniform(-20.0, 0.0, (D, h, w)).astype(np.float32)
    elif values == "wide":                       # [-2000, 5] in 2 x 3 x 3 blocks of either sign: both ends of the clamp (-1000, 0) act
        z, y, x = np.meshgrid(np.arange(D), np.arange(h), np.arange(w), indexing="ij")
        positive = (z // 2 + y // 3 + x // 3) % 2 == 0
        dpv = np.where(positive, rng.uniform(0.5, 5.0, (D, h, w)), rng.uniform(-2000.0, -1000.0, (D, h, w))).astype(np.float32)
    else:
        raise ValueError(values)
    d = candidates(D)
    case = {"dpv": dpv, "rays": cam["unit_ray_array_2D"].numpy().astype(np.float32), "d_candi": d,
            "tan_hh": math.tan(math.radians(cam["hfov"]) * .5), "tan_hv": math.tan(math.radians(cam["vfov"]) * .5), "key": key}
    _cases[key] = case
    return case


def gate(case, pad):
    return GATE_C * U * max(float(np.abs(case["dpv"]).max()), abs(float(pad)))


def z_range(d_candi, new_candi):
    """(z_half, z_radius) as the two forms of resample_vol_cuda compute them: fp32 arithmetic, or float64 of the SOURCE candidates
    rounded to fp32 when the output planes are new candidates."""
    if not new_candi:
        zh, zr = co.z_range(d_candi)
        return float(zh), float(zr)
    d64 = np.asarray(d_candi, np.float64)
    return float(np.float32((d64.max() + d64.min()) * .5)), float(np.float32((d64.max() - d64.min()) * .5))


def coordinates(case, T, d_out=None):
    """fp32 restatement of the oracle's chain -> dict of [D_out, hw] arrays: ux, uy, uz (before the clip), fx, fy, fz (after), qz."""
    f32, f64 = np.float32, np.float64
    D, h, w = case["dpv"].shape
    d = case["d_candi"] if d_out is None else np.asarray(d_out, f32)
    zh, zr = z_range(case["d_candi"], d_out is not None)
    T = np.asarray(T, f32)
    fma = lambda a, b, c: (f64(a) * b.astype(f64) + c.astype(f64)).astype(f32)
    with np.errstate(all="ignore"):
        X, Y, Z = [(d[:, None] * case["rays"][i][None]).astype(f32) for i in range(3)]
        q = []
        for r in range(4):
            a = (T[r, 0] * X).astype(f32)
            a = fma(T[r, 1], Y, a)
            a = fma(T[r, 2], Z, a)
            a = fma(T[r, 3], np.ones_like(a), a)
            q.append(a)
        den = (q[2] + f32(1e-10)).astype(f32)
        wq = (q[3] + f32(1e-10)).astype(f32)
        g = [((q[0] / den) / f32(case["tan_hh"])) / wq, ((q[1] / den) / f32(case["tan_hv"])) / wq, ((q[2] - f32(zh)) / f32(zr)) / wq]
        out = {"qz": q[2], "den": den}
        for name, gi, size in zip("xyz", g, (w, h, D)):
            u = (((gi.astype(f32) + f32(1)) * f32(size) - f32(1)) / f32(2)).astype(f32)
            c = np.where(u < 0, f32(0), u)
            c = np.where(c < f32(size - 1), c, f32(size - 1)).astype(f32)
            out["u" + name], out["f" + name] = u, c
    return out


def population(case, T, d_out=None):
    D, h, w = case["dpv"].shape
    c = coordinates(case, T, d_out)
    pop = {"voxels": int(c["ux"].size), "behind": int((c["den"] < 0).sum()), "qz_zero": int((c["qz"] == 0).sum()),
           "qz_zero_planes": int((c["qz"] == 0).all(axis=1).sum()),
           "nonfinite": int((~np.isfinite(c["ux"]) | ~np.isfinite(c["uy"]) | ~np.isfinite(c["uz"])).sum())}
    inside = True
    touch = {}
    for name, size in zip("xyz", (w, h, D)):
        u, f = c["u" + name], c["f" + name]
        with np.errstate(invalid="ignore"):
            pop[name + "_clip_lo"] = int((u < 0).sum())
            pop[name + "_clip_hi"] = int((~(u < size - 1)).sum())               # NaN lands on size - 1 too
        i0 = np.floor(f).astype(np.int64)
        frac = f - np.floor(f)
        pop[name + "_dropped_tap"] = int((i0 + 1 >= size).sum())
        inside = inside and bool((i0 >= 0).all() and (i0 <= size - 1).all())
        # the footprint on this axis: i0 always (weight 1 - frac > 0), i0 + 1 when it exists and frac > 0
        touch[name] = ((i0 == 0), (i0 == size - 1) | ((i0 + 1 == size - 1) & (frac > 0)))
        pop[name + "_face_lo"], pop[name + "_face_hi"] = int(touch[name][0].sum()), int(touch[name][1].sum())
    pop["interior"] = int((~(touch["x"][0] | touch["x"][1] | touch["y"][0] | touch["y"][1] | touch["z"][0] | touch["z"][1])).sum())
    pop["indices_inside"] = inside
    return pop


def oracle(case, T, pad, clamp=(-1000.0, 0.0), d_out=None):
    return co.dpv_resample(case["dpv"], T, case["rays"], np.asarray(case["d_candi"], np.float64) if d_out is not None else
                           case["d_candi"], case["tan_hh"], case["tan_hv"], pad, clamp=clamp, d_candi_new=d_out)


def plane_aligned_candidates(case):
    """Output candidates whose z coordinate falls on the source planes under the identity: fz = j  <=>  g_z = (2 j + 1) / D - 1."""
    D = case["dpv"].shape[0]
    zh, zr = z_range(case["d_candi"], True)
    return (zh + zr * ((2.0 * np.arange(D) + 1.0) / D - 1.0)).astype(np.float32)


def bordered(case, pad):
    v = case["dpv"].astype(np.float64).copy()
    for ax in range(3):
        idx = [slice(None)] * 3
        for face in (0, -1):
            idx[ax] = face
            v[tuple(idx)] = pad
    return v


def float64_from_coordinates(case, T, pad, clamp=(-1000.0, 0.0), d_out=None):
    """Trilinear interpolation of the bordered volume in float64 at the clipped fp32 coordinates of `coordinates` (taps beyond
    size - 1 carry a zero weight there, so dropping them changes nothing) -> [D_out, h, w].  The witness that `coordinates` is the
    oracle's chain: it agrees with the oracle within the gate only if both take every tap in the same cell."""
    D, h, w = case["dpv"].shape
    c = coordinates(case, T, d_out)
    vol = bordered(case, pad)
    f = [c["fz"].astype(np.float64), c["fy"].astype(np.float64), c["fx"].astype(np.float64)]
    i0 = [np.floor(a).astype(np.int64) for a in f]
    fr = [a - np.floor(a) for a in f]
    i1 = [np.minimum(i + 1, s - 1) for i, s in zip(i0, (D, h, w))]
    out = np.zeros(f[0].shape)
    for bz in (0, 1):
        for by in (0, 1):
            for bx in (0, 1):
                wgt = (fr[0] if bz else 1 - fr[0]) * (fr[1] if by else 1 - fr[1]) * (fr[2] if bx else 1 - fr[2])
                out += wgt * vol[(i1[0] if bz else i0[0]), (i1[1] if by else i0[1]), (i1[2] if bx else i0[2])]
    if clamp is not None:
        out = np.clip(out, clamp[0], clamp[1])
    return out.reshape(-1, h, w)


def new_candidates(case, form):
    """Output candidates of the d_candi_new form: fewer, more, or differently spaced (uniform in inverse depth, beyond the source
    range at both ends) than the source's."""
    D = case["dpv"].shape[0]
    if form == "fewer":
        return np.linspace(0.5, 4.0, max(1, D // 2))
    if form == "more":
        return np.linspace(0.2, 6.0, 2 * D + 1)
    if form == "inverse":
        return 1.0 / np.linspace(1 / 7.0, 1 / 0.2, D)
    raise ValueError(form)
