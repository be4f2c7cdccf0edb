"""float64 comparator of the depth evaluation (neuralrgbd_amd/csrc/depth_eval.hip) and the seeded inputs its tests share.

The comparator forms every term in the operation sequence of the kernel from the promoted fp32 values, so each term has the kernel's
bits (IEEE double +, -, *, /; only `log` is a library function on both sides), and adds the terms of a set with math.fsum: its own
summation error is nil.  What is left between the two is the order of the kernel's N additions and the two logs."""
import math

import numpy as np

RATIOS = (1.0, 1.25, 1.5625, 1.953125)        # d / g of the exact classes: equal, and the three delta boundaries (on the "not <" side)
CONF_8 = (0., .1, .2, .3, .4, .5, .6, .7)     # the J = 8 confidence thresholds of the tests
GT_RANGE = (0.75, 7.0)                        # inside the drawn [0.5, 8]: some ground truth falls outside on either side


def log_thresholds(conf):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(conf, dtype=np.float64)).astype(np.float32)


def terms(d, g):
    """The six terms and the ratio r of pixels (d, g) fp32 -> float64 arrays, in the kernel's operation sequence."""
    dd, gd = np.asarray(d, np.float32).astype(np.float64), np.asarray(g, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        e = dd - gd
        a = np.abs(e)
        t1 = a / gd
        ee = e * e
        t2 = ee / gd
        q = dd / gd
        l = np.log(q)
        t4 = l * l
        r = np.maximum(q, gd / dd)
    return [a, t1, t2, ee, t4, l], r


def evaluate(depth, logconf, gt, log_thr, gt_range):
    """-> dict: sums [J,6] float64 (fsum), abs_sums [J,6] (fsum of |t|: the scale of the summation bound), counts [J,4] int64,
    header [4] int64 = (1, gt-valid, bad, 0), err_map fp32 (np.abs(g - d) * (g > 0))."""
    d = np.asarray(depth, np.float32).reshape(-1)
    m = np.asarray(logconf, np.float32).reshape(-1)
    g = np.asarray(gt, np.float32).reshape(-1)
    thr = np.asarray(log_thr, np.float32)
    lo, hi = np.float32(gt_range[0]), np.float32(gt_range[1])
    J = thr.size
    with np.errstate(all="ignore"):
        valid = (g > 0) & (g >= lo) & (g <= hi)
        ok = valid & (d > 0) & np.isfinite(d) & ~np.isnan(m)
        err_map = np.abs(g - d) * (g > 0).astype(np.float32)
    t, r = terms(d[ok], g[ok])
    mo = m[ok]
    sums, abs_sums, counts = np.zeros((J, 6)), np.zeros((J, 6)), np.zeros((J, 4), np.int64)
    for j in range(J):
        s = mo >= thr[j]
        for k in range(6):
            v = t[k][s].tolist()
            sums[j, k] = math.fsum(v)
            abs_sums[j, k] = math.fsum(abs(x) for x in v)
        counts[j] = (int(s.sum()), int((r[s] < 1.25).sum()), int((r[s] < 1.5625).sum()), int((r[s] < 1.953125).sum()))
    header = np.array([1, int(valid.sum()), int((valid & ~ok).sum()), 0], np.int64)
    return {"sums": sums, "abs_sums": abs_sums, "counts": counts, "header": header, "err_map": err_map.astype(np.float32)}


def add_records(recs):
    """The comparator's total of several frames: fsum of the frames' sums per entry, integer sums of counts and headers."""
    out = {"sums": np.zeros_like(recs[0]["sums"]), "abs_sums": np.zeros_like(recs[0]["sums"])}
    for key in ("sums", "abs_sums"):
        for idx in np.ndindex(out[key].shape):
            out[key][idx] = math.fsum(r[key][idx] for r in recs)
    out["counts"] = sum(r["counts"] for r in recs)
    out["header"] = sum(r["header"] for r in recs)
    return out


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u), u = 2^-53: the relative bound on a sum of k + 1 terms added in any order."""
    u = 2.0 ** -53
    return k * u / (1 - k * u) if k > 0 else 0.0


def sum_bounds(abs_sums, n, U):
    """[J,6] absolute gates on the sums of sets whose pixel counts are n [J]: gamma_{n-1} S|t| for t0 .. t3 (every term has the same
    bits on both sides, only the order of the additions differs), and 2 U 2^-53 S|t| more for t4, t5 (a log of U ulps on either side)."""
    b = np.array([gamma(int(c) - 1) for c in n])[:, None] * abs_sums
    b[:, 4:] += 2 * U * 2.0 ** -53 * abs_sums[:, 4:]
    return b


def make_inputs(n, seed, conf):
    """(depth, logconf, gt) fp32 [n] for confidence thresholds `conf`:
    g on a 2^-10 grid in [0.5, 8] (14 significant bits), 20 % holes; d = g x {1, 1.25, 1.5625, 1.953125} — exact in fp32, the
    multipliers have 7 bits — or g x a ratio drawn in [0.3, 3]; 4 % of the pixels with ground truth have d in {0, -1, inf, NaN} and
    2 % of all have m = NaN; m = float32(log u), u uniform, 10 % of them moved exactly onto a threshold (-inf included)."""
    rng = np.random.RandomState(seed)
    thr = log_thresholds(conf)
    g = (rng.randint(512, 8193, n) / 1024.0).astype(np.float32)
    cls = rng.randint(0, 5, n)
    ratio = rng.uniform(0.3, 3.0, n).astype(np.float32)
    for c, f in enumerate(RATIOS):
        ratio[cls == c] = f
    d = g * ratio                                                   # fp32 product: exact for the four fixed classes
    g[rng.rand(n) < 0.2] = 0.0
    special = (rng.rand(n) < 0.04) & (g > 0)
    d[special] = np.array([0.0, -1.0, np.inf, np.nan], np.float32)[rng.randint(0, 4, int(special.sum()))]
    with np.errstate(divide="ignore"):
        m = np.log(rng.rand(n)).astype(np.float32)
    on = rng.rand(n) < 0.1
    m[on] = thr[rng.randint(0, thr.size, int(on.sum()))]
    m[rng.rand(n) < 0.02] = np.nan
    return d, m, g
