"""Comparator of the multi-view depth consistency kernel (csrc/consistency.hip; include/nrgbd.h spells out every operation).

`votes` restates nrgbd_depth_consistency_f32 in numpy, one numpy operation per operation of the header, vectorised over the pixels:
with dtype float32 it is the kernel's arithmetic bit for bit (votes and the filtered map are equal or the kernel is wrong), with float64
the yardstick, which also says where it cannot decide: a pixel is UNDECIDED when one of its comparisons lies so close to its threshold
that fp32 rounding may legitimately fall on the other side — a projected coordinate within 1e-4 px of a pixel border, an agreement
test within 1e-5 q_z of its threshold, a validity test within the same relative margin.  fp32 evaluates u from about six rounded
operations on values of the map's width (64 px here: 6 x 2^-24 x 64 = 2.3e-5 px < 1e-4) and the tests from three or four (4 x 2^-24 =
2.4e-7 < 1e-5 relative).  MUTANTS are the slips the GPU tests' bit-for-bit gate has to catch.  The fixtures: the corner scene of
tests/icp_ref.py seen from a reference and four source views with seeded flying pixels, seeded maps that reach every branch, and
three small cases for the mutants the corner scene cannot show."""
import functools

import numpy as np

import icp_ref as ir
import tsdf_raycast_ref as rc

MAX_SRC = 16
MUTANTS = ("lt", "far_lt", "round_u", "no_qz", "no_src_gate", "rel_ds", "no_slots")
PX_MARGIN, REL_MARGIN = 1e-4, 1e-5


def _valid(f, d, g, d_near, d_far, gate_thr, mutant=None):
    """The four tests on a depth (and its gate, or None) -> (valid, within REL_MARGIN of a threshold)."""
    with np.errstate(invalid="ignore"):
        far = d < d_far if mutant == "far_lt" else d <= d_far
        ok = (d > d_near) & far & np.isfinite(d)
        scale = np.maximum(np.abs(d), np.abs(d_near))
        near = np.abs(d - d_near) <= REL_MARGIN * scale
        if np.isfinite(d_far):
            near |= np.abs(d - d_far) <= REL_MARGIN * np.maximum(np.abs(d), np.abs(d_far))
        if g is not None:
            ok &= g >= gate_thr
            near |= np.abs(g - gate_thr) <= REL_MARGIN * np.maximum(np.abs(g), np.abs(gate_thr))
    return ok, near & np.isfinite(d)


def votes(dtype, depth, K, src_depth=None, src_slots=None, src_T=None, rel_thr=0.01, depth_range=(0.0, float("inf")), gate=None,
          gate_thr=0.0, src_gate=None, mutant=None):
    """-> {'votes' [H,W] float32 (the agreeing sources, -1: the pixel is invalid), 'undecided' [H,W] bool (float64: see the module
    docstring; float32: all False)}.  src_depth (and src_gate) [S,H,W]; source s is map src_slots[s] (default s) seen through src_T[s]
    = (R | t), reference camera -> source camera; every scalar and every transform is rounded to float32 first."""
    assert mutant is None or mutant in MUTANTS
    f = dtype
    c = lambda v: f(np.float32(v))
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    n_src = 0 if src_depth is None else (len(src_depth) if src_slots is None else len(src_slots))
    assert n_src <= MAX_SRC
    slots = list(range(n_src)) if (src_slots is None or mutant == "no_slots") else [int(s) for s in src_slots]
    fx, fy, cx, cy = (c(k) for k in K)
    d_near, d_far, thr, rel = c(depth_range[0]), c(depth_range[1]), c(gate_thr), c(rel_thr)
    Y, X = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        d = depth.astype(f)
        g = None if gate is None else np.asarray(gate, np.float32).astype(f)
        ok, undecided = _valid(f, d, g, d_near, d_far, thr, mutant)
        xn = ((X.astype(np.float32).astype(f) + f(0.5)) - cx) / fx
        yn = ((Y.astype(np.float32).astype(f) + f(0.5)) - cy) / fy
        p = [xn * d, yn * d, d]
        agree = np.zeros((H, W), np.int64)
        for s in range(n_src):
            T = np.asarray(src_T[s], np.float64)[:3, :4].astype(np.float32).astype(f)
            sd = np.asarray(src_depth[slots[s]], np.float32).astype(f)
            sg = None if (src_gate is None or mutant == "no_src_gate") else np.asarray(src_gate[slots[s]], np.float32).astype(f)
            q = [((T[j, 0] * p[0] + T[j, 1] * p[1]) + T[j, 2] * p[2]) + T[j, 3] for j in range(3)]
            front = np.ones((H, W), bool) if mutant == "no_qz" else q[2] > 0
            u = fx * (q[0] / q[2]) + cx
            v = fy * (q[1] / q[2]) + cy
            inside = front & (u >= 0) & (u < c(W)) & (v >= 0) & (v < c(H))
            pick = np.rint if mutant == "round_u" else np.floor
            iu = np.clip(np.where(inside, pick(u), 0), 0, W - 1).astype(np.int64)
            iv = np.where(inside, np.floor(v), 0).astype(np.int64)
            ds = sd[iv, iu]
            sok, snear = _valid(f, ds, None if sg is None else sg[iv, iu], d_near, d_far, thr, mutant)
            width = rel * (ds if mutant == "rel_ds" else q[2])
            gap = np.abs(ds - q[2])
            hit = inside & sok & ((gap < width) if mutant == "lt" else (gap <= width))
            agree += ok & hit
            if f is np.float64:
                border = (np.abs(u - np.rint(u)) <= PX_MARGIN) | (np.abs(v - np.rint(v)) <= PX_MARGIN)
                close = np.abs(gap - width) <= REL_MARGIN * np.abs(q[2])
                behind = np.abs(q[2]) <= REL_MARGIN * np.abs(d)
                reach = ok & np.isfinite(u) & np.isfinite(v) & (u > -1) & (u < W + 1) & (v > -1) & (v < H + 1)
                undecided |= behind & ok
                undecided |= reach & (border | (inside & (snear | (sok & close))))
    out = np.where(ok, agree, -1).astype(np.float32)
    return {"votes": out, "undecided": undecided if f is np.float64 else np.zeros((H, W), bool)}


def filtered(depth, v, min_views):
    """depth_out of the entry from its votes: agreeing >= min_views ? d : 0 (an invalid pixel has -1 votes)."""
    depth = np.asarray(depth, np.float32)
    return np.where(v >= np.float32(min_views), depth, np.float32(0)).astype(np.float32)


def relative(pose, poses):
    """float32 [n,3,4]: (T_s T_ref^-1)[:3], float64 on the host, rounded once (fusion.relative_poses)."""
    inv = np.linalg.inv(np.asarray(pose, np.float64))
    return np.stack([(np.asarray(m, np.float64) @ inv)[:3] for m in poses]).astype(np.float32)


# ---- the corner fixture: a reference view with seeded flying pixels and four source views ------------------------------------------
CORNER_REL, CORNER_SHARE = 0.02, 0.05
CORNER_MOVES = (((0.021, -0.027, 0.013), (0.052, -0.031, 0.018)), ((-0.031, 0.022, -0.019), (-0.061, 0.042, -0.027)),
                ((0.026, 0.033, 0.011), (0.035, 0.071, 0.024)), ((-0.018, -0.029, 0.031), (-0.044, -0.058, -0.049)))
# (rotation vector rad, translation m) on top of the reference pose: 0.03 - 0.05 rad and 5 - 10 cm, no axis singled out


@functools.lru_cache(maxsize=None)
def corner_fixture():
    """{'depth' [H,W] (5 % of the hit pixels replaced by d U(0.6, 0.9) or d U(1.1, 1.4)), 'clean' (before), 'outlier' [H,W] bool,
    'sources' [4,H,W], 'pose', 'poses', 'T' [4,3,4] float32, 'K'}: icp_ref's room corner ray cast (tsdf_raycast_ref, float32) from
    corner_poses()[0] and from four views CORNER_MOVES away."""
    from neuralrgbd_amd import synth
    C = ir.CORNER
    vol = ir.corner_field(C["dims"], C["origin"], C["vs"], C["trunc"], C["planes"])
    pose = ir.corner_poses()[0]
    poses = []
    for rv, t in CORNER_MOVES:
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = synth.rotvec_to_R(rv), t
        poses.append(m @ pose)
    cast = lambda m: rc.raycast(np.float32, vol[0], vol[1], C["origin"], C["vs"], m, C["K"], C["size"], 0.0, float("inf"), 1.0, None)["depth"]
    clean = cast(pose).astype(np.float32)
    sources = np.stack([cast(m) for m in poses]).astype(np.float32)
    rng = np.random.RandomState(2024)
    outlier = (rng.rand(*clean.shape) < CORNER_SHARE) & (clean > 0)
    scale = np.where(rng.rand(*clean.shape) < 0.5, rng.uniform(0.6, 0.9, clean.shape), rng.uniform(1.1, 1.4, clean.shape))
    depth = np.where(outlier, clean * scale, clean).astype(np.float32)
    for a in (depth, clean, outlier, sources):
        a.setflags(write=False)
    return {"depth": depth, "clean": clean, "outlier": outlier, "sources": sources, "pose": pose, "poses": poses,
            "T": relative(pose, poses), "K": C["K"]}


def corner_votes(dtype, mutant=None, depth=None):
    fx = corner_fixture()
    return votes(dtype, fx["depth"] if depth is None else depth, fx["K"], fx["sources"], None, fx["T"], CORNER_REL, mutant=mutant)


# ---- seeded maps that reach every branch, shared by the host and the GPU tests ----------------------------------------------------
SIZES = ((1, 1), (7, 9), (48, 64), (67, 130))
N_SRC = (0, 1, 3, 16)
STACK = 5
PARAMS = {"rel_thr": 0.01, "depth_range": (0.1, 1.75), "gate_thr": 0.15}


def slot_list(n_src):
    """The stack's maps from the last one back, each twice: reversed, with repeats."""
    return [STACK - 1 - (s // 2) % STACK for s in range(n_src)]


def _seed_bad(rng, a, share=0.02):
    """NaN, +inf, -inf, 0 and negative values seeded into a map."""
    kind = rng.rand(*a.shape)
    for k, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -1.3)):
        a[(kind >= k * share) & (kind < (k + 1) * share)] = v
    return a


@functools.lru_cache(maxsize=None)
def make_case(H, W, n_src, gated, seed=None):
    """Inputs of one nrgbd_depth_consistency_f32 call: a smooth surface seen from nearby cameras, every map with its own per-pixel
    error of 0, 1/2, 3/2 or 4 thresholds (so the agreement test falls on both sides and depends on the very pixel read), values
    beyond d_far, NaN, +-inf, 0 and negative depths in the reference and in the sources, gates with NaN; source 1 looks away (behind
    the camera) and source 2 stands 100 m to the side (every projection falls outside) when there are that many."""
    from neuralrgbd_amd import synth
    rng = np.random.RandomState(100000 * gated + 1000 * H + 10 * W + n_src if seed is None else seed)
    K = (0.9 * W, 0.9 * W, W / 2.0, H / 2.0)
    Y, X = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = 1.5 + 0.2 * np.sin(X / 5.0) + 0.1 * np.cos(Y / 4.0)
    noisy = lambda: _seed_bad(rng, base * (1.0 + PARAMS["rel_thr"] * rng.choice([0.0, 0.5, -0.5, 1.5, -1.5, 4.0], (H, W)))).astype(np.float32)
    depth = noisy()
    stack = np.stack([noisy() for _ in range(STACK)])
    new_gate = lambda: np.where(rng.rand(H, W) < 0.01, np.nan, rng.rand(H, W)).astype(np.float32)
    gate = new_gate() if gated else None
    src_gate = np.stack([new_gate() for _ in range(STACK)]) if gated else None
    T = []
    for s in range(n_src):
        m = np.eye(4)
        m[:3, :3] = synth.rotvec_to_R(rng.normal(0, 0.01, 3))
        m[:3, 3] = rng.normal(0, 0.02, 3)
        if s == 1:
            m[:3, :3] = synth.rotvec_to_R([0.0, np.pi, 0.0]) @ m[:3, :3]
        if s == 2:
            m[0, 3] = 100.0
        T.append(m[:3])
    for a in (depth, stack, gate, src_gate):
        if a is not None:
            a.setflags(write=False)
    return dict(PARAMS, depth=depth, K=K, src_depth=stack if n_src else None, src_slots=slot_list(n_src) if n_src else None,
                src_T=np.stack(T).astype(np.float32) if n_src else None, gate=gate, src_gate=src_gate if n_src else None,
                gate_thr=PARAMS["gate_thr"] if gated else 0.0)


def votes_of(dtype, case, mutant=None):
    return votes(dtype, case["depth"], case["K"], case["src_depth"], case["src_slots"], case["src_T"], case["rel_thr"], case["depth_range"],
                 case["gate"], case["gate_thr"], case["src_gate"], mutant)


# ---- the small cases for the mutants the scenes above cannot show -----------------------------------------------------------------
def edge_case():
    """The identity onto a map exactly one threshold away: d = 1, ds = 1.25, rel = 0.25 (all exact in fp32: |ds - q_z| == rel q_z)."""
    H, W = 4, 6
    depth = np.ones((H, W), np.float32)
    return dict(depth=depth, K=(5.0, 5.0, 3.0, 2.0), src_depth=np.full((1, H, W), 1.25, np.float32), src_slots=[0],
                src_T=np.eye(4, dtype=np.float32)[None, :3], rel_thr=0.25, depth_range=(0.0, float("inf")), gate=None, gate_thr=0.0,
                src_gate=None)


def far_case():
    """A frame against itself with every depth exactly at d_far: depth_range = (0, 1], d = ds = 1."""
    case = edge_case()
    case.update(src_depth=np.ones_like(case["src_depth"]), depth_range=(0.0, 1.0))
    return case


def look_away_case():
    """A source turned by pi about y, so that q_z = -d < 0 for every pixel; the remaining tests would pass without `q_z > 0`: the
    range reaches below zero, the source holds exactly q_z, and rel q_z underflows to -0, which |ds - q_z| = 0 does not exceed."""
    H, W = 4, 6
    d = np.float32(1e-30)
    T = np.zeros((1, 3, 4), np.float32)
    T[0, 0, 0], T[0, 1, 1], T[0, 2, 2] = -1.0, 1.0, -1.0
    return dict(depth=np.full((H, W), d, np.float32), K=(5.0, 5.0, 3.0, 2.0), src_depth=np.full((1, H, W), -d, np.float32), src_slots=[0],
                src_T=T, rel_thr=1e-20, depth_range=(-1.0, 1.0), gate=None, gate_thr=0.0, src_gate=None)


def gate_plane_case():
    """A frame against itself with a gate that passes everywhere and a source gate that fails on the right half."""
    H, W = 6, 8
    depth = np.full((H, W), 2.0, np.float32)
    sg = np.ones((1, H, W), np.float32)
    sg[0, :, W // 2:] = 0.0
    return dict(depth=depth, K=(7.0, 7.0, 4.0, 3.0), src_depth=depth[None].copy(), src_slots=[0], src_T=np.eye(4, dtype=np.float32)[None, :3],
                rel_thr=0.01, depth_range=(0.0, float("inf")), gate=np.ones((H, W), np.float32), gate_thr=0.5, src_gate=sg)


def permuted_slots_case():
    """A frame against a stack of three planes, of which only the last is its own; the slot list names that one."""
    H, W = 6, 8
    depth = np.full((H, W), 2.0, np.float32)
    stack = np.stack([np.full((H, W), v, np.float32) for v in (1.0, 3.0, 2.0)])
    return dict(depth=depth, K=(7.0, 7.0, 4.0, 3.0), src_depth=stack, src_slots=[2], src_T=np.eye(4, dtype=np.float32)[None, :3],
                rel_thr=0.01, depth_range=(0.0, float("inf")), gate=None, gate_thr=0.0, src_gate=None)


SMALL_CASES = {"edge": edge_case, "far": far_case, "look_away": look_away_case, "gate_plane": gate_plane_case,
               "permuted_slots": permuted_slots_case}
