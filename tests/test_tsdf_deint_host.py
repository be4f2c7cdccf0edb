"""Host-side checks of the TSDF de-integration: the two C entries (declared, bound, exported, every refusal without a GPU and in the
documented order), and the properties of the fp32 restatement tests/tsdf_deint_ref.py on tsdf_ref's cases — removing a view equals
fusing the others inside the bound derived in tsdf_deint_ref's header, a voxel the others leave empty comes out exactly (0, 0),
removing every view empties the volume bit for bit, and a view fused at a wrong pose is repaired by taking it out and putting it back.
No GPU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import tsdf_deint_ref as dref
import tsdf_ref as ref
from conftest import ROOT
from neuralrgbd_amd import _lib

U = ref.U
ENTRIES = {"nrgbd_tsdf_reintegrate_f32": ("nrgbd_tsdf_integrate_f32", 28), "nrgbd_tsdf_reintegrate_color_f32": ("nrgbd_tsdf_integrate_color_f32", 37)}


# ---- 1. the C entries
def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nrgbd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, (plain, nargs) in ENTRIES.items():
        decl = re.search(r"\bint %s\((.*?)\);" % name, code, flags=re.S).group(1)
        assert decl.count(",") + 1 == len(_lib.SIGNATURES[name][1]) == nargs, name
        assert nargs == len(_lib.SIGNATURES[plain][1]) + 2          # the integration's arguments, a second pose and w_floor
        assert hasattr(lib, name)
        assert re.search(r"%s\b[^.]*— no counterpart in the reference" % name, header), name
        assert name in header[:header.index("#define NRGBD_INTERFACE_VERSION")]       # named in the list at the top
    assert header.count('#define NRGBD_INTERFACE_VERSION "0.10"') == 1                 # no entry changed or disappeared


E_NULL, E_SHAPE, E_ARG = -1, -2, -4
P = ctypes.c_void_p(64)                     # never dereferenced: every call below is refused before anything touches the device
NAN, INF = float("nan"), float("inf")
POSE = (ctypes.c_float * 12)(*np.eye(4, dtype=np.float32)[:3].reshape(-1))
GRID_SHAPES = (dict(X=0), dict(Y=-1), dict(Z=0), dict(H=0), dict(W=-3), dict(X=2 ** 16, Y=2 ** 15, Z=2), dict(X=2 ** 31 - 1, Y=2, Z=1),
               dict(X=2 ** 16, Y=2 ** 16, Z=2 ** 16), dict(box=(-1, 0, 0, 8, 6, 4)), dict(box=(0, 0, 0, 9, 6, 4)), dict(box=(0, 0, 0, 8, 7, 4)),
               dict(box=(0, 0, 0, 8, 6, 5)), dict(box=(3, 0, 0, 3, 6, 4)), dict(box=(0, 4, 0, 8, 2, 4)), dict(box=(0, 0, 4, 8, 6, 4)))
INTEGRATE_ARGS = (dict(vs=0.), dict(vs=-1.), dict(vs=NAN), dict(vs=INF), dict(trunc=0.), dict(trunc=NAN), dict(trunc=INF), dict(w_max=0.),
                  dict(w_max=-2.), dict(w_max=NAN), dict(w_max=INF), dict(d_near=1., d_far=1.), dict(d_near=2., d_far=1.), dict(d_near=NAN),
                  dict(d_far=NAN))
FLOORS = (dict(w_floor=-1e-30), dict(w_floor=-1.), dict(w_floor=NAN), dict(w_floor=INF), dict(w_floor=-INF))


@pytest.mark.parametrize("add", [False, True], ids=["remove", "remove-and-add"])
def test_reintegrate_refuses_bad_arguments_without_a_gpu(add):
    fn = _lib.load().nrgbd_tsdf_reintegrate_f32

    def call(null=None, X=8, Y=6, Z=4, H=5, W=7, vs=.05, trunc=.15, d_near=0., d_far=INF, w_max=64., w_floor=1e-3, box=None):
        ptr = [None if i == null else (ctypes.cast(POSE, ctypes.c_void_p) if i == 3 else P) for i in range(4)]       # tsdf, weight, depth, pose_remove
        cbox = None if box is None else (ctypes.c_int * 6)(*box)
        return fn(ptr[0], ptr[1], X, Y, Z, 0., 0., 0., vs, ptr[2], None, None, ptr[3], ctypes.cast(POSE, ctypes.c_void_p) if add else None,
                  H, W, 30., 30., 3.5, 2.5, trunc, d_near, d_far, w_max, w_floor, 0., cbox, None)
    for i in range(4):
        assert call(null=i) == E_NULL, i                            # pose_remove NULL: that call is nrgbd_tsdf_integrate_f32
    for kw in GRID_SHAPES:
        assert call(**kw) == E_SHAPE, kw
    for kw in INTEGRATE_ARGS + FLOORS:
        assert call(**kw) == E_ARG, kw
    # the order: NULL, shape, the integration's arguments — and w_floor is an argument
    assert call(null=3, X=0, w_floor=-1.) == E_NULL and call(X=0, w_floor=-1.) == E_SHAPE and call(box=(0, 0, 0, 9, 6, 4), w_floor=NAN) == E_SHAPE
    assert call(X=2 ** 16, Y=2 ** 15, Z=1, w_floor=-1.) == E_ARG    # exactly 2^31 voxels is a grid


@pytest.mark.parametrize("add", [False, True], ids=["remove", "remove-and-add"])
def test_reintegrate_color_refuses_bad_arguments_without_a_gpu(add):
    fn = _lib.load().nrgbd_tsdf_reintegrate_color_f32

    def call(null=None, X=8, Y=6, Z=4, H=5, W=7, vs=.05, trunc=.15, d_near=0., d_far=INF, w_max=64., w_floor=1e-3, box=None, Hc=9, Wc=11,
             Kc=(40., 40., 5.5, 4.5), affine=(1., 1., 1., 0., 0., 0.)):
        ca = (ctypes.c_float * 6)(*affine)
        host = {3: ctypes.cast(POSE, ctypes.c_void_p), 6: ctypes.cast(ca, ctypes.c_void_p)}
        ptr = [None if i == null else host.get(i, P) for i in range(7)]       # tsdf, weight, depth, pose_remove, color, image, affine
        cbox = None if box is None else (ctypes.c_int * 6)(*box)
        return fn(ptr[0], ptr[1], ptr[4], X, Y, Z, 0., 0., 0., vs, ptr[2], None, None, ptr[3], ctypes.cast(POSE, ctypes.c_void_p) if add else None,
                  H, W, 30., 30., 3.5, 2.5, trunc, d_near, d_far, w_max, w_floor, 0., cbox, ptr[5], Hc, Wc, Kc[0], Kc[1], Kc[2], Kc[3], ptr[6],
                  None)
    for i in range(7):
        assert call(null=i) == E_NULL, i
    for kw in GRID_SHAPES + (dict(Hc=0), dict(Wc=0), dict(Hc=-2), dict(Wc=-1)):
        assert call(**kw) == E_SHAPE, kw
    bad = lambda seq, i, v: tuple(v if j == i else x for j, x in enumerate(seq))
    args = list(INTEGRATE_ARGS + FLOORS)
    args += [dict(Kc=bad((40., 40., 5.5, 4.5), i, v)) for i in range(4) for v in (NAN, INF, -INF)]
    args += [dict(affine=bad((1., 1., 1., 0., 0., 0.), i, v)) for i in range(6) for v in (NAN, INF)]
    for kw in args:
        assert call(**kw) == E_ARG, kw
    # the order of nrgbd_tsdf_integrate_color_f32, w_floor behind it
    assert call(null=4, X=0, vs=0.) == E_NULL and call(null=6, Hc=0) == E_NULL and call(X=0, vs=0.) == E_SHAPE
    assert call(Hc=0, w_floor=-1.) == E_SHAPE and call(box=(0, 0, 0, 9, 6, 4), affine=(NAN,) * 6) == E_SHAPE
    assert call(Wc=0, Kc=(NAN,) * 4) == E_SHAPE and call(w_floor=NAN, Kc=(NAN,) * 4) == E_ARG


# ---- 2. the restatement: removing a view against fusing the others
CASES = [("front", ref.PLANE_GRID, (48, 64)), ("front", (67, 5, 3), (7, 9)), ("inside", ref.PLANE_GRID, (48, 64)),
         ("edge", ref.PLANE_GRID, (48, 64)), ("side", (64, 3, 2), (48, 64))]


def _fuse(case, views):
    """fp32 (T, W), the voxels whose weight ever reached w_max, and the observations per voxel, of the given views in order."""
    X, Y, Z = case["dims"]
    T, Wt = np.zeros((Z, Y, X), np.float32), np.zeros((Z, Y, X), np.float32)
    sat, m = np.zeros((Z, Y, X), bool), np.zeros((Z, Y, X), np.int64)
    for i in views:
        obs = ref.observe(np.float32, case, i)
        with np.errstate(all="ignore"):
            sat |= obs["ok"] & ~(Wt + obs["w"] < np.float32(case["w_max"]))
        T, Wt = ref.integrate(np.float32, T, Wt, obs, case["w_max"])
        m += obs["ok"]
    return T, Wt, sat, m


@pytest.mark.parametrize("clean", [True, False], ids=["clean", "seeded"])
@pytest.mark.parametrize("family,dims,size", CASES, ids=lambda v: str(v))
def test_removing_a_view_equals_fusing_the_others(family, dims, size, clean):
    """Every view k of the case, after all views were fused (fp32, w_floor = 1e-3): on the voxels view k updated whose weight never
    reached w_max, T and W lie inside removal_bound of the volume of the other views (the bound is derived in tsdf_deint_ref's header
    from the operation count; the restatement measured at most 6 u on T and 4 u on W with an amplification of at most 4.6), and every
    voxel the other views leave empty is exactly (0, 0).  The amplification itself is bounded by the inputs: unit weights give
    (m + 1) / (m - 1) <= 3, the seeded maps hold weights in [0.5, 1.5) below w_max = 3: (3 + 1.5) / 0.5 = 9."""
    case = ref.make_case(family, dims, size, clean)
    n = len(case["views"])
    T, Wt, sat, m = _fuse(case, range(n))
    checked = emptied = 0
    for k in range(n):
        obs = ref.observe(np.float32, case, k)
        To, Wo, _, _ = _fuse(case, [i for i in range(n) if i != k])
        Td, Wd = dref.remove(np.float32, T, Wt, obs)
        skipped = ~obs["ok"]
        assert np.array_equal(Td[skipped].view(np.int32), T[skipped].view(np.int32)) and np.array_equal(Wd[skipped].view(np.int32), Wt[skipped].view(np.int32))
        upd = obs["ok"] & ~sat
        alone = upd & (Wo == 0)
        assert not Td[alone].view(np.int32).any() and not Wd[alone].view(np.int32).any(), "a voxel the others leave empty is not (0, 0)"
        rest = upd & ~alone
        eT, eW, amp = dref.removal_bound(Wt, obs["w"], Wd, Wo, m)
        assert (Wd[rest] > 0).all()
        assert (np.abs(Td.astype(np.float64) - To)[rest] <= eT[rest]).all(), (k, (np.abs(Td.astype(np.float64) - To) / U)[rest].max())
        assert (np.abs(Wd.astype(np.float64) - Wo)[rest] <= eW[rest]).all(), (k, (np.abs(Wd.astype(np.float64) - Wo) / U)[rest].max())
        assert rest.sum() == 0 or amp[rest].max() <= (3.0 if clean else 9.0)
        assert (np.abs(Td[obs["ok"]]) <= 1).all()                   # the clamp, saturated voxels included
        checked += int(rest.sum())
        emptied += int(alone.sum())
    assert checked + emptied > 0, "the case removes nothing"
    if dims == ref.PLANE_GRID and family == "front":
        assert checked > 10000 and emptied > 100


def test_the_seeded_cases_saturate_and_the_floor_matters():
    """Not vacuous: the seeded plane case holds voxels at w_max (where the removal is no inverse, and the test above leaves them out),
    and with weight maps the removals leave a rounding residue: w_floor = 0 keeps it as a weight, 1e-3 empties the voxel."""
    case = ref.make_case("front", ref.PLANE_GRID, (48, 64))
    _, _, sat, m = _fuse(case, range(len(case["views"])))
    assert sat.sum() > 1000 and (m > 1).sum() > 10000
    residue = 0
    for order in ((1, 2), (2, 1)):                                  # views 1 and 2 carry weight maps; 1.5 + 1.5 stays below w_max
        T, Wt, two_sat, _ = _fuse(case, (1, 2))
        assert not two_sat.any()
        T0, W0 = T, Wt
        for k in order:
            obs = ref.observe(np.float32, case, k)
            T, Wt = dref.remove(np.float32, T, Wt, obs)
            T0, W0 = dref.remove(np.float32, T0, W0, obs, 0.0)
        assert not Wt.view(np.int32).any() and not T.view(np.int32).any()
        residue += int((W0 > 0).sum())
        assert (W0 < 1e-6).all()
    assert residue > 0


@pytest.mark.parametrize("family,dims,size", CASES[:2] + CASES[3:4], ids=lambda v: str(v))
def test_removing_every_view_of_a_clean_case_in_any_order_leaves_zeros(family, dims, size):
    case = ref.make_case(family, dims, size, True)
    n = len(case["views"])
    T0, W0, _, _ = _fuse(case, range(n))
    assert W0.any()
    orders = list(itertools.permutations(range(n))) if n <= 3 else [tuple(range(n)), tuple(range(n))[::-1], (3, 0, 5, 1, 4, 2), (2, 4, 1, 5, 0, 3)]
    for order in orders:
        T, Wt = T0, W0
        for k in order:
            T, Wt = dref.remove(np.float32, T, Wt, ref.observe(np.float32, case, k))
        assert not T.view(np.int32).any() and not Wt.view(np.int32).any(), order


# ---- 3. the repair
def test_a_view_fused_at_a_wrong_pose_is_repaired():
    """The clean plane scene, view 3 fused 6 cm along the optical axis and 2 cm sideways off: the extracted surface is measurably worse;
    taking the view out at the wrong pose and putting it back at the right one gives the clean volume's weights bit for bit, its point
    count, and a surface whose largest distance to the plane differs from the clean one's by no more than the T bound moves a crossing:
    q = Ta / (Ta - Tb) moves by at most 2 e / |Ta - Tb| voxels, and |Ta - Tb| across a crossing of this scene is a voxel's share of
    the band, vs / trunc = 1/3, the plane tilted by at most 1 / max(n) — bounded below by 0.25 here and asserted."""
    case = ref.make_case("front", ref.PLANE_GRID, (48, 64), True)
    X, Y, Z = case["dims"]
    n = len(case["views"])
    wrong = case["views"][3]["extM"].copy()
    wrong[2, 3] += 0.06
    wrong[0, 3] += 0.02

    def obs(i, extM=None):
        v = case["views"][i]
        return ref.chain(np.float32, case["dims"], case["origin"], case["vs"], np.float32((v["extM"] if extM is None else extM)[:3, :4]),
                         case["K"], v["depth"], case["trunc"], case["depth_range"][0], case["depth_range"][1])

    def surface(T, Wt):
        return ref.plane_distance(ref.extract(np.float32, T, Wt, case["origin"], case["vs"], 1.0), case["vs"])
    Tc, Wc = ref.fused("front", ref.PLANE_GRID, (48, 64), "float32", True)[-1]
    T, Wt = np.zeros((Z, Y, X), np.float32), np.zeros((Z, Y, X), np.float32)
    for i in range(n):
        T, Wt = ref.integrate(np.float32, T, Wt, obs(i, wrong if i == 3 else None), case["w_max"])
    clean, corrupt = surface(Tc, Wc), surface(T, Wt)
    assert clean.max() < 0.1 and corrupt.max() > 10 * clean.max()
    Tr, Wr = dref.reintegrate(np.float32, T, Wt, obs(3, wrong), obs(3), case["w_max"])
    repaired = surface(Tr, Wr)
    assert np.array_equal(Wr.view(np.int32), Wc.view(np.int32))     # unit weights: the sums are exact
    assert len(repaired) == len(clean) and np.array_equal(Tr < 0, Tc < 0)
    # T' against the mean of the other five (removal_bound without the other side's own error is smaller still), one more update
    # (8 u) to the mean of all six, and the clean volume's own 8 u m; a voxel the wrong pose never touched: two orders of the same sum
    m = np.rint(Wt).astype(np.int64)                                # the observations while the wrong one was in (unit weights)
    eT = dref.removal_bound(Wt, np.ones_like(Wt), np.maximum(Wt - 1, 0), np.maximum(Wt - 1, 0), m)[0] + 8 * U + 8 * U * (np.rint(Wc) + m)
    touched = Wc > 0
    assert (np.abs(Tr.astype(np.float64) - Tc)[touched] <= eT[touched]).all()
    # a crossing between a and a + e_k lies at q = Ta / (Ta - Tb); an error e on both moves it by at most 2 e / |Ta - Tb| voxels along
    # axis k (|q| <= 1, first order), and the distance to the plane by |n_k| times that
    side = (Wc >= 1) & (np.abs(Tc) < 1)
    effect = 0.0
    for k, (a, b) in enumerate((((slice(None), slice(None), slice(0, -1)), (slice(None), slice(None), slice(1, None))),
                                ((slice(None), slice(0, -1)), (slice(None), slice(1, None))), ((slice(0, -1),), (slice(1, None),)))):
        cross = side[a] & side[b] & ((Tc[a] < 0) != (Tc[b] < 0))
        e = np.maximum(eT[a], eT[b])[cross]
        effect = max(effect, (2 * e * abs(ref.PLANE_N[k]) / np.abs(Tc[a].astype(np.float64) - Tc[b])[cross]).max())
    assert effect < 1e-3                                            # the repair is far inside what the corruption did
    assert np.abs(repaired - clean).max() <= 1.01 * effect + 8 * U  # the same crossings in the same order; 8 u: the point's own roundings
