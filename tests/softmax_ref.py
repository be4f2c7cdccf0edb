"""Comparator of the depth-probability head (csrc/softmax.hip): float64 restatements, error bounds and the case tables that the
host test (test_softmax_ref_host.py) and the GPU test (test_gpu_softmax_edges.py) share.  numpy only.

Restatements.  `logsoftmax` forms z = fl32(fl32(scale a) + b) in float32 — the library is built with -ffp-contract=off, so these
are the kernel's own two roundings and z has the kernel's bits — and does everything after that in float64 with the maximum
subtracted.  `logsoftmax_bwd`, `regress`, `to_u16` and `nll` are the definitions in float64 on the kernels' fp32 inputs.
Non-finite values follow IEEE (and torch): a -inf entry stays -inf; a column of nothing but -inf, a +inf entry or a NaN entry makes
the whole column NaN; the confidence is the NaN-propagating maximum.

Error bounds, u = 2^-24 (the unit roundoff of fp32: fl(x) = x (1 + d), |d| <= u).  K_e u and K_l u are the relative errors of the
device's expf and logf (one to two ulps; K below stands for them and is the only constant that is measured).

  Forward, out_k = fl32((z_k - m) - logf(S)), the two subtractions in double (z_k - m is exact there, the second rounds at 2^-53) and
  ONE rounding to fp32; S the fp32 sum of the D values expf(fl(z_k - m)):
    t_k  = fl(z_k - m)  = (z_k - m)(1 + d1)                  the argument of expf only: |t_k - (z_k - m)| <= u |z_k - m|        (1)
    e_k  = expf(t_k)    = exp(z_k - m) (1 + h_k),            |h_k| <= K_e u + |z_k - m| u     (the argument moved by (1))
    S    = sum of the e_k in some order = s (1 + H),  s = sum_k exp(z_k - m) >= 1 (the maximum contributes exp(0)):
           the additions cost at most (D - 1) u relative; the K_e u of every term stays K_e u of the sum; the moved arguments
           weigh |t| e^t <= 1/e each, at most D u / e in all, relative to s >= 1.   |H| <= (D - 1 + K_e + D / e) u              (2)
    L    = logf(S)      = log(S)(1 + l), |l| <= K_l u:       |L - log s| <= |H| + K_l u |log s|                                  (3)
    out  = fl32((z_k - m) - L):                              the one rounding costs u |out_k| <= u (|z_k - m| + |log s|)          (4)
  (3) + (4):  |out_k - ref_k| <= u (|z_k - m| + (1 + K_l) |log s| + (1 + 1/e) D + K_e)   to first order: the gate's form
  K u (|z_k - m| + |log s| + D)  — the subtractions, logf, the sum of D exponentials — with |z_k - m| counted once, as the gate
  counts it.  A column of D = 1 has s = 1, log s = 0 and out = 0 exactly.
  (Until this comparator existed the kernels took both subtractions in fp32, fl(fl(z_k - m) - L): two roundings at the magnitude
  |z_k - m|, which the gate's form does not hold at small D, where the D term cannot absorb the second one — four table entries at
  D = 3 and 5 came out at 1.38 to 1.50 times the bound.  The kernels now round once; profiles/softmax_edges.txt has both.)

  Backward, gz_k = fl(scale fl(g_k - fl(expf(logp_k) S))), S the fp32 sum of the D values g_k:
    S        within (D - 1) u sum|g| of sum g;   p_k = expf(logp_k) within K_e u p_k;   the product within u p_k |S|;
    the subtraction within u (|g_k| + p_k |S|);  the scaling within u of the result (exact for the powers of two the nets use).
    |gz_k - ref_k| <= |scale| u (2 |g_k| + (K_e + 3) p_k |sum g| + D p_k sum|g|)    to first order; the gate is the issue's
    K u |scale| (|g_k| + p_k (|sum g| + D sum|g|)),  again sufficient from K = 2 on.  Where logp_k = -inf, p_k = 0 and gz_k = scale g_k
    exactly.

  Depth, acc = fl(acc + fl(expf(v_k) d_k)) over k in order from 0.f:  every term carries K_e u (expf) + u (product), every one of
    the D - 1 additions u of a partial sum whose magnitude is at most sum_k p_k |d_k|:
    |depth - ref| <= u (K + D + 1) sum_k p_k |d_k| + D 2^-126 max|d|    (the second term: exponentials below the normal range may be
    flushed to zero).  The export kernel's exponential is correctly rounded (K_e = 1/2) and obeys the same gate.

  NLL, loss = sum of the counted -logp[target] / count.  The terms are fp32 values (the negation is exact).  Pass 1 adds the 256
    terms of a workgroup in a binary tree of 8 fp32 levels: relative to the sum of their magnitudes at most gamma_8 (fp32).  Pass 2
    adds the partial sums and divides in double (gamma_G 2^-53: nothing on this scale) and rounds the quotient to fp32 once (u).
    The counts are integers below 2^24 and exact throughout.  |loss - ref| <= gamma_10(fp32) sum|t| / count, gamma_k = k u / (1 - k u)
    (10 = 8 levels + the final rounding + one for the second-order terms), which is far inside the gamma_n sum|t| / count of a plain
    sum of n fp32 terms in any order (`nll_bound` returns both; the loss is an fp32 word, so u = 2^-24 is the only unit that can
    hold — icp_ref.sum_bound is the same rule for sums formed in double).

K: fixed from one GPU run as the issue of this comparator lays down — the worst |error| / bound at K = 1 over the benign family
(unit-normal x 5, D in {64, 128, 200}; `benign_volume`), doubled because a sample does not hit every argument.  Measured 0.6673,
so K = 1.3346 (profiles/softmax_edges.txt, header of test_gpu_softmax_edges.py).  The run was made on the kernels as they were then
(two fp32 subtractions); K stands for the device's expf and logf, which the later change of the subtraction does not touch, so it
holds as fixed and was not measured again (the same family now comes out lower; the profile records it)."""
import math

import numpy as np

U = 2.0 ** -24
K_MEASURED = 0.6673          # worst |error| / bound at K = 1 over the benign family on an MI355X (D = 64; 0.4074 at 128, 0.3133 at 200)
K = 2.0 * K_MEASURED         # 1.3346: gates every family

PLANAR_D = (1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 256)
PLANAR_N = (1, 63, 64, 65, 257)
SCALES = (-1.0, 1.0, 0.5)
BWD_D = (3, 5, 63, 65, 127, 129, 200, 256)
BWD_N = (1, 65)
ROWS_D = (4, 60, 68, 132, 1024)
ROWS_N = (1, 127, 128, 129)
BENIGN_D = (64, 128, 200)
BENIGN_N = 257
U16_IN = (-1.0, -0.0, 0.4, 0.99999994, 1.0, 65534.996, 65535.0, 65536.0, 1e9, float("inf"), float("nan"))
U16_OUT = (0, 0, 0, 0, 1, 65534, 65535, 65535, 65535, 65535, 0)
NLL_IGNORE = (0, -100, 3)
NLL_CASES = ((65792, 2, False), (65792, 64, True), (960, 256, True))          # (n, D, channels_last)

BENIGN, ONEHOT, WIDE, OFFSET, CONST, NEGINF, ALLNEGINF, POSINF, NAN = range(9)
FAMILIES = ("benign", "onehot", "wide", "offset", "const", "neginf", "allneginf", "posinf", "nan")
FINITE_FAMILIES = (BENIGN, ONEHOT, WIDE, OFFSET, CONST)                      # every output finite
LANE_ORDER = (BENIGN, ALLNEGINF, ONEHOT, POSINF, WIDE, NAN, OFFSET, CONST, NEGINF)
MUTANTS = ("drop_candidate", "d_minus_1", "clamp_tail")                    # of logsoftmax; regress has "drop_chunk"


def planar_cases():
    """(D, n) of the planar tables: every D at n = 65, every n at D in {5, 65, 129}."""
    cases = [(D, 65) for D in PLANAR_D]
    cases += [(D, n) for D in (5, 65, 129) for n in PLANAR_N if n != 65]
    return cases


def planar_variants():
    """(scale, with_b) of the planar tables."""
    return [(s, wb) for s in SCALES for wb in (False, True)]


def gamma32(k):
    """gamma_k = k u / (1 - k u) with fp32's u."""
    return k * U / (1 - k * U) if k > 0 else 0.0


# ---- restatements ----------------------------------------------------------------------------------------------------------------------
def form_z(a, b, scale):
    """z = fl32(fl32(scale a) + b): the kernel's bits."""
    with np.errstate(all="ignore"):
        z = np.float32(scale) * np.asarray(a, np.float32)
        if b is not None:
            z = z + np.asarray(b, np.float32)
    assert z.dtype == np.float32
    return z


def logsoftmax(a, b, scale, mutant=None):
    """a, b [D, n] float32 (b may be None) -> (out [D, n] float64, bound [D, n] float64 at K = 1).  Where out is not finite the
    bound is not used: the class (NaN, +inf, -inf) is compared exactly (`compare`)."""
    assert mutant is None or mutant in MUTANTS
    z = form_z(a, b, scale).astype(np.float64)
    D, n = z.shape
    if mutant == "clamp_tail" and n > 1:                            # the last pixel read from its neighbour
        z = z.copy()
        z[:, n - 1] = z[:, n - 2]
    used = np.ones(D, bool)
    if mutant == "drop_candidate" and D > 1:
        used[D // 2] = False
    if mutant == "d_minus_1" and D > 1:
        used[D - 1] = False
    with np.errstate(all="ignore"):
        m = np.max(z[used], axis=0)                                 # np.max propagates NaN, as the column does
        t = z - m[None]
        s = np.sum(np.exp(t[used]), axis=0)
        ls = np.log(s)
        out = t - ls[None]
        bound = U * (np.abs(t) + np.abs(ls)[None] + D)
    return out, bound


def logsoftmax_bwd(logp32, g32, scale):
    """scale (g - exp(logp) sum_k g) in float64 from the fp32 inputs -> (gz [D, n] float64, bound [D, n] at K = 1)."""
    return bwd64(np.asarray(logp32, np.float32).astype(np.float64), np.asarray(g32, np.float32).astype(np.float64),
                 float(np.float32(scale)))


def bwd64(lp, g, sc):
    """The backward on float64 arrays (what test_softmax_ref_host.py holds against autograd)."""
    D = lp.shape[0]
    with np.errstate(all="ignore"):
        p = np.exp(lp)
        S = np.sum(g, axis=0)
        A = np.sum(np.abs(g), axis=0)
        gz = sc * (g - p * S[None])
        bound = U * abs(sc) * (np.abs(g) + p * (np.abs(S) + D * A)[None])
    return gz, bound


def nanmax(v, axis=0):
    """The maximum that propagates NaN (torch.max)."""
    with np.errstate(all="ignore"):
        return np.max(v, axis=axis)


def regress(logp32, d32, mutant=None):
    """logp [D, n], d [D] float32 -> (depth [n] float64, conf [n] float64 = the NaN-propagating max, bound [n] without its K:
    `depth_bound(bound_terms, K)`)."""
    assert mutant in (None, "drop_chunk")
    lp = np.asarray(logp32, np.float32).astype(np.float64)
    d = np.asarray(d32, np.float32).astype(np.float64)
    D = lp.shape[0]
    used = np.ones(D, bool)
    if mutant == "drop_chunk" and D > 64:
        used[64:128] = False
    with np.errstate(all="ignore"):
        p = np.exp(lp[used])
        depth = np.sum(p * d[used, None], axis=0)
        mag = np.sum(p * np.abs(d[used, None]), axis=0)
    return depth, nanmax(lp), {"mag": mag, "D": D, "dmax": float(np.max(np.abs(d[np.isfinite(d)]))) if np.isfinite(d).any() else 0.0}


def depth_bound(terms, k):
    """u (K + D + 1) sum p |d| + D 2^-126 max|d| (module docstring)."""
    return U * (k + terms["D"] + 1) * terms["mag"] + terms["D"] * 2.0 ** -126 * terms["dmax"]


def to_u16(v):
    """The definition: NaN or v <= 0 -> 0; v >= 65535 -> 65535; otherwise truncated."""
    v = np.asarray(v, np.float32)
    out = np.zeros(v.shape, np.uint16)
    for i, x in np.ndenumerate(v):
        x = float(x)
        if math.isnan(x) or x <= 0.0:
            out[i] = 0
        elif x >= 65535.0:
            out[i] = 65535
        else:
            out[i] = int(math.floor(x))
    return out


def nll(logp32, target, ignore, D):
    """logp [D, n] float32 (planar view), target [n] int64 -> {'loss' float64 (fsum / count; NaN when nothing is counted), 'count',
    'abs_sum' (fsum of |term|), 'counted' [n] bool}.  A target outside [0, D) counts as ignored."""
    lp = np.asarray(logp32, np.float32)
    t = np.asarray(target, np.int64)
    assert lp.shape[0] == D and lp.shape[1] == t.shape[0]
    counted = (t != ignore) & (t >= 0) & (t < D)
    idx = np.nonzero(counted)[0]
    terms = -lp[t[idx], idx].astype(np.float64)
    count = int(counted.sum())
    total = math.fsum(terms.tolist())
    return {"loss": total / count if count else float("nan"), "count": count, "abs_sum": math.fsum(np.abs(terms).tolist()),
            "counted": counted}


def nll_grad(target, counted, D, g_out, count):
    """[D, n] float32: fl32(-g_out / count) at (target[p], p) of the counted pixels, 0 elsewhere."""
    t = np.asarray(target, np.int64)
    g = np.zeros((D, t.shape[0]), np.float32)
    idx = np.nonzero(counted)[0]
    with np.errstate(all="ignore"):
        g[t[idx], idx] = -np.float32(g_out) / np.float32(count)
    return g


def nll_bound(abs_sum, count, n):
    """(the derived gate gamma_10 sum|t| / count, the plain-sum gate gamma_n sum|t| / count) in fp32's u."""
    c = max(count, 1)
    return gamma32(10) * abs_sum / c, gamma32(n) * abs_sum / c


# ---- comparison --------------------------------------------------------------------------------------------------------------------------
def compare(got, ref, bound, k):
    """Every element: where ref is not finite the class must be the same (NaN, +inf, -inf); everywhere else |got - ref| <= k bound.
    -> (ok, worst |got - ref| / bound over the finite elements (at K = 1), number of elements that fail)."""
    got = np.asarray(got).astype(np.float64)
    ref, bound = np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape == bound.shape
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        cls = np.where(np.isnan(ref), np.isnan(got), got == ref)    # +-inf == +-inf compares the sign too
        diff = np.abs(got - ref)
        good = np.where(fin, diff <= k * bound, cls)                # a NaN or an infinity where a number is due fails the <=
        ratio = np.where(fin & (bound > 0), diff / np.where(bound > 0, bound, 1.0), np.where(fin & (diff > 0), np.inf, 0.0))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    return bool(good.all()), float(ratio.max()) if ratio.size else 0.0, int((~good).sum())


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------------
def family_of(D, n):
    """The family of every pixel: neighbouring lanes of a wave hold different families, and no two NaN families are neighbours (a
    pixel that reads its neighbour's column is then always visible)."""
    return np.array(LANE_ORDER)[(np.arange(n) + D) % len(FAMILIES)]


def make_volume(D, n, scale, with_b, seed=0):
    """-> (a [D, n] float32, b [D, n] float32 or None, fam [n]).  The families are properties of z = fl32(fl32(scale a) + b):
    benign (unit-normal x 5), one-hot (one z = 0, the others <= -200), wide (uniform in [-150, 0], one entry near 0 and one below
    -110 when D >= 2), offset (1e4 + unit-normal), const, neginf (about a third of the entries -inf, through b when there is one),
    allneginf, posinf (one +inf), nan (one NaN).  With D = 1 the neginf family keeps its entry finite."""
    rng = np.random.RandomState(100003 * D + 101 * n + 7 * int(with_b) + int(round(4 * scale)) + 1000 * seed + 17)
    fam = family_of(D, n)
    sc = np.float32(scale)
    z = np.zeros((D, n), np.float64)                               # the target of z
    peak = rng.randint(0, D, n)
    cols = np.arange(n)
    z[:] = 5.0 * rng.randn(D, n)
    f = fam == ONEHOT
    z[:, f] = -(250.0 + 50.0 * rng.rand(D, int(f.sum())))
    f = fam == WIDE
    z[:, f] = -150.0 * rng.rand(D, int(f.sum()))
    f = fam == OFFSET
    z[:, f] = 1e4 + rng.randn(D, int(f.sum()))
    f = fam == CONST
    z[:, f] = rng.randn(1, int(f.sum()))
    if with_b:
        a = (2.0 * rng.randn(D, n)).astype(np.float32)
        a[:, fam == CONST] = a[0:1, fam == CONST]
        sa = sc * a                                                 # fl32(scale a)
        b = (z - sa.astype(np.float64)).astype(np.float32)
    else:
        a = (z / float(sc)).astype(np.float32)
        b = None
        sa = sc * a

    def put(k, p, value):
        """z[k, p] becomes `value` exactly (0, +-inf or NaN)."""
        if b is not None and (value == 0.0 or value == -float("inf")):
            b[k, p] = -sa[k, p] if value == 0.0 else value          # fl32(scale a) + (-fl32(scale a)) = 0; finite + -inf = -inf
        elif value == 0.0:
            a[k, p] = 0.0
        elif math.isnan(value):
            a[k, p] = np.nan
        else:
            a[k, p] = np.float32(value) * np.sign(sc)               # scale a = value for an infinity

    for p in cols[fam == ONEHOT]:
        put(peak[p], p, 0.0)
    if D >= 2:
        for p in cols[fam == WIDE]:
            k0, k1 = peak[p], (peak[p] + 1 + rng.randint(0, D - 1)) % D
            if b is not None:
                b[k0, p] = np.float32(-0.25 * rng.rand()) - sa[k0, p]
                b[k1, p] = np.float32(-(110.0 + 40.0 * rng.rand())) - sa[k1, p]
            else:
                a[k0, p] = np.float32(-0.25 * rng.rand() / float(sc))
                a[k1, p] = np.float32(-(110.0 + 40.0 * rng.rand()) / float(sc))
        for p in cols[fam == NEGINF]:
            drop = rng.rand(D) < 0.35
            drop[peak[p]] = False
            drop[(peak[p] + 1) % D] = True
            for k in np.nonzero(drop)[0]:
                put(k, p, -float("inf"))
    for p in cols[fam == ALLNEGINF]:
        for k in range(D):
            put(k, p, -float("inf"))
    for p in cols[fam == POSINF]:
        put(peak[p], p, float("inf"))
    for p in cols[fam == NAN]:
        put(peak[p], p, float("nan"))
    return a, b, fam


def benign_volume(D, seed=0):
    """The calibration family of K: a and b unit-normal x 5, scale 1, [D, BENIGN_N]."""
    rng = np.random.RandomState(5000 + D + seed)
    return (5.0 * rng.randn(D, BENIGN_N)).astype(np.float32), (5.0 * rng.randn(D, BENIGN_N)).astype(np.float32)


def make_logp(D, n, seed=0):
    """A log-probability volume [D, n] float32 for the backward, regression and NLL tests: the float64 log-softmax of a
    `make_volume` (every family: -inf entries and NaN columns included) rounded to fp32, and the families.  A column of the nan
    family is a copy of the first benign column with ONE NaN entry (first, middle or last candidate in turn) when there is a
    benign column; the allneginf and posinf columns are NaN throughout."""
    a, b, fam = make_volume(D, n, 1.0, True, seed=seed + 1)
    with np.errstate(all="ignore"):
        lp = logsoftmax(a, b, 1.0)[0].astype(np.float32)
    benign = np.nonzero(fam == BENIGN)[0]
    if benign.size:
        for i, p in enumerate(np.nonzero(fam == NAN)[0]):
            lp[:, p] = lp[:, benign[0]]
            lp[(0, D // 2, D - 1)[i % 3], p] = np.nan
    return lp, fam


def make_d_candi(D, seed=0):
    """Depth candidates: increasing, metres, not round numbers."""
    rng = np.random.RandomState(77 + D + seed)
    return np.cumsum(0.01 + 0.05 * rng.rand(D)).astype(np.float32) + np.float32(0.4)


def make_targets(n, D, ignore, seed=0):
    """[n] int64: uniform over the classes of [0, D) that are not the ignore value, then about 10 % the ignore value and about 2 %
    each of -1, -100, D and D + 5."""
    rng = np.random.RandomState(31 * n + D + 3 * (ignore % 7) + seed)
    classes = np.array([k for k in range(D) if k != ignore], np.int64)
    t = classes[rng.randint(0, len(classes), n)]
    kind = rng.rand(n)
    t[kind < 0.10] = ignore
    for i, v in enumerate((-1, -100, D, D + 5)):
        t[(kind >= 0.10 + 0.02 * i) & (kind < 0.12 + 0.02 * i)] = v
    if n >= 8:                                                      # every kind is present whatever the draw
        t[:5] = (ignore, -1, -100, D, D + 5)
    return t


def make_nll_logp(n, D, seed=0):
    """[D, n] float32 log-probabilities of unit-normal x 3 logits (finite)."""
    rng = np.random.RandomState(900 + D + seed)
    z = (3.0 * rng.randn(D, n)).astype(np.float32).astype(np.float64)
    m = z.max(0)
    return ((z - m) - np.log(np.exp(z - m).sum(0))).astype(np.float32)
