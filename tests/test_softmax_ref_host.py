"""CPU: the comparator of the depth-probability head (tests/softmax_ref.py) against torch in float64, the teeth of its input
families, and mutants of the restatement that its bounds have to catch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import softmax_ref as sr

_VOLUMES = {}


def _volume(D, n, scale, with_b):
    """(a, b, fam, out, bound) of one table entry, computed once and never modified."""
    key = (D, n, scale, with_b)
    if key not in _VOLUMES:
        a, b, fam = sr.make_volume(D, n, scale, with_b)
        _VOLUMES[key] = (a, b, fam) + sr.logsoftmax(a, b, scale)
    return _VOLUMES[key]


def _entries():
    return [(D, n, s, wb) for D, n in sr.planar_cases() for s, wb in sr.planar_variants()]


def _rel(got, want):
    with np.errstate(all="ignore"):
        return np.abs(got - want) / np.maximum(1.0, np.abs(want))


def test_tables_are_what_the_issue_lists():
    cases = sr.planar_cases()
    assert len(cases) == len(set(cases)) == len(sr.PLANAR_D) + 3 * (len(sr.PLANAR_N) - 1)
    assert {D for D, n in cases if n == 65} == set(sr.PLANAR_D)
    for D in (5, 65, 129):
        assert {n for d, n in cases if d == D} == set(sr.PLANAR_N)
    assert set(sr.planar_variants()) == {(s, wb) for s in (-1.0, 1.0, 0.5) for wb in (False, True)}
    for D, n in cases:                                              # neighbouring lanes hold different families
        fam = sr.family_of(D, n)
        assert (np.diff(fam) != 0).all() and (n < 9 or set(fam) == set(range(9)))


@pytest.mark.parametrize("D,n,scale,with_b", _entries())
def test_logsoftmax_and_its_gradient_against_torch_float64(D, n, scale, with_b):
    a, b, fam, out, bound = _volume(D, n, scale, with_b)
    z = torch.from_numpy(sr.form_z(a, b, scale).astype(np.float64)).requires_grad_(True)
    with np.errstate(all="ignore"):
        want = torch.log_softmax(z, dim=0)
        w = want.detach().numpy()
        # every family: the class torch gives (NaN columns whole, -inf entries -inf), and the finite values to 1e-12
        assert np.array_equal(np.isnan(out), np.isnan(w))
        assert np.array_equal(np.isinf(out), np.isinf(w)) and (out[np.isinf(out)] < 0).all()
        fin = np.isfinite(w)
        assert (_rel(out[fin], w[fin]) <= 1e-12).all()
        for f in (sr.ALLNEGINF, sr.POSINF, sr.NAN):
            assert np.isnan(out[:, fam == f]).all()
        if D >= 2:
            col = out[:, fam == sr.NEGINF]
            assert np.isinf(col).any(0).all() and np.isfinite(col).any(0).all()
        cols = np.isin(fam, sr.FINITE_FAMILIES)
        assert np.isfinite(out[:, cols]).all() and np.isfinite(bound[:, cols]).all()
        # the gradient, on the finite families (autograd through a NaN column is NaN on both sides)
        g = np.random.RandomState(D + n).randn(D, n)
        g[:, ~cols] = 0.0
        want.backward(torch.from_numpy(g))
        sc = float(np.float32(scale))
        gz, _ = sr.bwd64(out, g, sc)
        assert (_rel(gz[:, cols], sc * z.grad.numpy()[:, cols]) <= 1e-12).all()


@pytest.mark.parametrize("D,n,scale,with_b", _entries())
def test_each_family_keeps_its_teeth(D, n, scale, with_b):
    a, b, fam, out, bound = _volume(D, n, scale, with_b)
    z = sr.form_z(a, b, scale)
    zo = z[:, fam == sr.ONEHOT]
    if zo.size:                                                     # exact expected output: 0.0 at the peak, z_k elsewhere
        assert ((zo == 0).sum(0) == 1).all() and (zo[zo != 0] <= -200).all()
        assert np.array_equal(out[:, fam == sr.ONEHOT], np.where(zo == 0, 0.0, zo.astype(np.float64)))
    zw = z[:, fam == sr.WIDE].astype(np.float64)
    if zw.size and D >= 2:
        assert ((zw - zw.max(0)).min(0) < -104).all() and (zw <= 0).all() and (zw >= -150).all()
    zf = z[:, fam == sr.OFFSET]
    assert (zf > 9.9e3).all()
    zc = z[:, fam == sr.CONST]
    assert (zc == zc[0:1]).all()
    if D >= 2:
        zn = z[:, fam == sr.NEGINF]
        assert ((zn == -np.inf).sum(0) >= 1).all() and np.isfinite(zn).any(0).all()
        if with_b and zn.size:                                      # through b
            assert (b[:, fam == sr.NEGINF] == -np.inf).sum() == (zn == -np.inf).sum() and np.isfinite(a[:, fam == sr.NEGINF]).all()
    assert (z[:, fam == sr.ALLNEGINF] == -np.inf).all()
    zp = z[:, fam == sr.POSINF]
    assert ((zp == np.inf).sum(0) == 1).all() and not np.isnan(zp).any()
    zq = z[:, fam == sr.NAN]
    assert (np.isnan(zq).sum(0) == 1).all()
    assert np.isfinite(z[:, np.isin(fam, sr.FINITE_FAMILIES)]).all()


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_the_forward_bound_catches_each_mutant(mutant):
    """A candidate left out of the sum, D - 1 instead of D terms, the tail pixel read from its neighbour: beyond K x bound on every
    table entry that the slip can touch (D >= 2, resp. n >= 2, and a column family whose other candidates carry weight)."""
    caught = 0
    for D, n, scale, with_b in _entries():
        a, b, fam, out, bound = _volume(D, n, scale, with_b)
        got, _ = sr.logsoftmax(a, b, scale, mutant=mutant)
        ok, worst, bad = sr.compare(got.astype(np.float32), out, bound, sr.K)
        touched = D >= 2 and n >= (2 if mutant == "clamp_tail" else 9)     # D = 1: every finite column is 0.0
        if touched:
            assert not ok, (mutant, D, n, scale, with_b, worst)
            caught += 1
        # and the restatement itself, rounded to fp32, passes its own gate
        assert sr.compare(out.astype(np.float32), out, bound, sr.K)[0]
    assert caught >= len(sr.PLANAR_D) - 1


def test_the_backward_bound_catches_a_dropped_candidate():
    for D in sr.BWD_D:
        for n in sr.BWD_N:
            logp, fam = sr.make_logp(D, n)
            g = np.random.RandomState(D).randn(D, n).astype(np.float32)
            want, bound = sr.logsoftmax_bwd(logp, g, 0.5)
            g2 = g.copy()
            g2[D // 2] = 0                                          # left out of the sum (and of its own output)
            got, _ = sr.logsoftmax_bwd(logp, g2, 0.5)
            assert sr.compare(want.astype(np.float32), want, bound, sr.K)[0]
            assert n < 9 or not sr.compare(got.astype(np.float32), want, bound, sr.K)[0]      # n = 1 may be a NaN column
            inf = np.isneginf(logp)
            assert np.array_equal(want[inf], 0.5 * g[inf].astype(np.float64))


@pytest.mark.parametrize("D", sr.ROWS_D)
def test_regress_against_torch_and_the_dropped_chunk(D):
    for n in sr.ROWS_N:
        logp, fam = sr.make_logp(D, n)
        d = sr.make_d_candi(D)
        depth, conf, terms = sr.regress(logp, d)
        lp = torch.from_numpy(logp.astype(np.float64))
        want = (torch.exp(lp) * torch.from_numpy(d.astype(np.float64))[:, None]).sum(0).numpy()
        wc = lp.max(0).values.numpy()                               # torch.max propagates NaN
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(depth), nan) and np.array_equal(np.isnan(conf), np.isnan(wc))
        assert np.array_equal(nan, np.isin(fam, (sr.ALLNEGINF, sr.POSINF, sr.NAN)))
        assert (_rel(depth[~nan], want[~nan]) <= 1e-12).all() and np.array_equal(conf[~nan], wc[~nan])
        one = fam == sr.ONEHOT
        assert np.array_equal(depth[one], d[np.argmax(logp[:, one], 0)].astype(np.float64)) and (conf[one] == 0).all()
        bound = sr.depth_bound(terms, sr.K)
        assert sr.compare(depth.astype(np.float32), depth, bound, 1.0)[0]
        if D > 64 and n >= 9:
            assert not sr.compare(sr.regress(logp, d, mutant="drop_chunk")[0].astype(np.float32), depth, bound, 1.0)[0]


def test_to_u16_table():
    assert len(sr.U16_IN) == len(sr.U16_OUT) == 11
    assert sr.to_u16(np.array(sr.U16_IN, np.float32)).tolist() == list(sr.U16_OUT)
    # the table's decimal inputs are the fp32 neighbours they are meant to be
    assert np.float32(0.99999994) == np.float32(1.0) - np.float32(2.0 ** -24) and np.float32(65534.996) == np.float32(65535 - 2.0 ** -8)


@pytest.mark.parametrize("n,D,channels_last", sr.NLL_CASES)
@pytest.mark.parametrize("ignore", sr.NLL_IGNORE)
def test_nll_against_torch_float64(n, D, channels_last, ignore):
    logp = sr.make_nll_logp(n, D)
    t = sr.make_targets(n, D, ignore)
    ref = sr.nll(logp, t, ignore, D)
    # teeth: negative targets, targets >= D, ignored ones, and at least half of the pixels counted
    assert (t == -1).any() and (t == -100).any() and (t == D).any() and (t == D + 5).any() and (t == ignore).any()
    assert ref["count"] >= n // 2 and ref["count"] == int(((t >= 0) & (t < D) & (t != ignore)).sum()) < n
    # torch on the pixels it accepts: a class in [0, D) or the ignore value itself
    ok = ((t >= 0) & (t < D)) | (t == ignore)
    lp = torch.from_numpy(logp[:, ok].T.astype(np.float64).copy()).requires_grad_(True)
    want = F.nll_loss(lp, torch.from_numpy(t[ok]), ignore_index=ignore)
    assert abs(ref["loss"] - want.item()) <= 1e-12 * abs(want.item())
    (3.0 * want).backward()
    g = sr.nll_grad(t, ref["counted"], D, 3.0, ref["count"])
    assert (g[:, ~ok] == 0).all() and (g[:, ~ref["counted"]] == 0).all()
    wg = lp.grad.numpy().T
    assert (np.abs(g[:, ok] - wg) <= 2.0 ** -23 * np.abs(wg)).all()
    assert int((g != 0).sum()) == ref["count"]
    tight, plain = sr.nll_bound(ref["abs_sum"], ref["count"], n)
    assert 0 < tight <= plain
    # a pixel left out of the sum is beyond the derived gate
    first = int(np.nonzero(ref["counted"])[0][0])
    t2 = t.copy()
    t2[first] = -1
    assert abs(sr.nll(logp, t2, ignore, D)["loss"] * (ref["count"] - 1) / ref["count"] - ref["loss"]) > tight
    assert np.isnan(sr.nll(logp, np.full(n, ignore, np.int64), ignore, D)["loss"])
