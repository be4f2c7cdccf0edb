"""Comparator of the TSDF de-integration (csrc/tsdf_reint.hip; include/nrgbd.h spells out the operation sequence:
nrgbd_tsdf_reintegrate_f32, nrgbd_tsdf_reintegrate_color_f32).

`remove` / `remove_color` restate the removal of one observation in numpy, one numpy operation per operation of the header, in a given
dtype: in float32 they are the kernel's arithmetic bit for bit.  The observation (ok, t, w, c, fin) is tsdf_ref.chain's /
tsdf_color_ref.observe's — the chain is the integration's, unchanged.  `reintegrate` is the removal followed by tsdf_ref.integrate /
tsdf_color_ref.integrate on its result: what the fused launch computes by definition.

Bound of removing view k from the fp32 volume of all views against the fp32 volume of the other views (`removal_bound`; u = 2^-24,
first order, from the operation count, never from an output).  Both sides run the same fp32 chain, so every (t_i, w_i) is the same
number on both; what differs is the order of the sums.  For a voxel with m observations let M_A = sum_A t_i w_i / sum_A w_i in real
arithmetic (|M_A| <= 1: every t lies in [-1, 1]) and W_A = sum_A w_i.  tsdf_ref's header gives, per update, 8 u on the running average
and one u of relative error on the accumulated weight (the first sum, 0 + w, is exact):
    all views:     |T - M_all| <= e_all = 8 u m,          W = W_all (1 + d), |d| <= d_all = (m - 1) u
    other views:   |T_o - M_oth| <= 8 u (m - 1),          W_o = W_oth (1 + d'), |d'| <= (m - 2) u
The removal forms Wn = W - w, N = T W - t w, T' = N / Wn, and M_oth = (M_all W_all - t w) / W_oth exactly:
    T W            inherits W_all (e_all + d_all) and rounds once:                      W_all (e_all + d_all + u)
    t w            rounds once:                                                         u w
    N              rounds once, |N| <= W_oth to first order:                            u W_oth
    Wn             inherits d_all W_all and rounds once (u W_oth); it scales T' (|M_oth| <= 1) by that over W_oth
    T'             the division rounds once: u; the clamp to [-1, 1] moves T' towards M_oth, never away
    |T' - M_oth| <= (W_all / W_oth) (e_all + 2 d_all + u) + u w / W_oth + 3 u  <=  amp (e_all + 2 d_all + 2 u) + 3 u
with amp = (W + w) / Wn, the amplification the stored values themselves show (>= W_all / W_oth and >= w / W_oth to first order).  So
    |T' - T_o|  <=  1.01 [amp (8 m + 2 (m - 1) + 2) u + 3 u + 8 (m - 1) u]
    |Wn - W_o|  <=  1.01 [(m - 1) u W + u Wn + (m - 2) u W_o]          (the two summation errors and the subtraction's rounding)
A voxel with m = 1 holds W = w exactly (0 + w), Wn is exactly 0 and the voxel is fresh again: (0, 0) bit for bit, weight maps or not.
The bound holds on voxels whose weight never reached w_max (the clamp forgets what it cut)."""
import numpy as np

import tsdf_color_ref as cref
import tsdf_ref as ref

U = ref.U
W_FLOOR = 1e-3


def remove(dtype, T, Wt, obs, w_floor=W_FLOOR):
    """One observation taken out of (T, Wt) on the voxels obs['ok'] marks: (T', W') as new arrays of `dtype`."""
    ok, t, w = obs["ok"], obs["t"].astype(dtype), obs["w"].astype(dtype)
    T, Wt = T.astype(dtype), Wt.astype(dtype)
    with np.errstate(all="ignore"):
        Wn = Wt - w
        stays = Wn > dtype(np.float32(w_floor))                    # a NaN fails
        Tn = np.fmin(dtype(1), np.fmax(dtype(-1), (T * Wt - t * w) / Wn))          # fminf / fmaxf: a NaN quotient gives -1
    Tn, Wn = np.where(stays, Tn, dtype(0)), np.where(stays, Wn, dtype(0))
    return np.where(ok, Tn, T).astype(dtype), np.where(ok, Wn, Wt).astype(dtype)


def remove_color(dtype, C, Wt, obs, w_floor=W_FLOOR):
    """The colour of that observation taken out of C [3,Z,Y,X] with the STORED Wt (before `remove` replaces it): an emptied voxel's
    colour is 0, a voxel whose pixel was not finite keeps its bits."""
    ok, fin, w = obs["ok"], obs["fin"], obs["w"].astype(dtype)
    C, Wt = C.astype(dtype), Wt.astype(dtype)
    with np.errstate(all="ignore"):
        Wn = Wt - w
        gone = ok & ~(Wn > dtype(np.float32(w_floor)))
        new = [(C[j] * Wt - obs["c"][j].astype(dtype) * w) / Wn for j in range(3)]
    return np.stack([np.where(gone, dtype(0), np.where(fin, new[j], C[j])) for j in range(3)]).astype(dtype)


def reintegrate(dtype, T, Wt, obs_old, obs_new, w_max, w_floor=W_FLOOR, C=None):
    """obs_old out, then obs_new in (None: the removal alone): (T', W') or, with the colour planes C, (T', W', C')."""
    Cn = None if C is None else remove_color(dtype, C, Wt, obs_old, w_floor)
    Tn, Wn = remove(dtype, T, Wt, obs_old, w_floor)
    if obs_new is not None:
        if C is not None:
            Cn = cref.integrate(dtype, Cn, Wn, obs_new)
        Tn, Wn = ref.integrate(dtype, Tn, Wn, obs_new, w_max)
    return (Tn, Wn) if C is None else (Tn, Wn, Cn)


def removal_bound(W, w, Wn, Wo, m):
    """(bound on |T' - T_o|, bound on |Wn - W_o|, amp) of the header, float64 arrays; m: the observations of each voxel."""
    W, w, Wn, Wo, m = (np.asarray(a, np.float64) for a in (W, w, Wn, Wo, m))
    with np.errstate(all="ignore"):
        amp = np.where(Wn > 0, (W + w) / Wn, 0.0)
    eT = 1.01 * U * (amp * (8 * m + 2 * (m - 1) + 2) + 3 + 8 * (m - 1))
    eW = 1.01 * U * ((m - 1) * W + Wn + np.maximum(m - 2, 0) * Wo)
    return eT, eW, amp
