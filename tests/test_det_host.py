"""Host side of the bit-reproducible training mode (no GPU): the switch of neuralrgbd_amd.autograd, the keywords that carry it, and
a numpy model of the fixed-point accumulation of csrc/costvol_bwd_det.hip (maximum of the |term| bit patterns -> exact power-of-two
scale -> one rounding to an integer per term -> integer sum -> double -> one rounding to fp32)."""
import inspect
import math

import numpy as np
import pytest

from neuralrgbd_amd import autograd as ag

U = 2.0 ** -24


# ---- the switch ----------------------------------------------------------------------------------------------------------------

def test_switch_defaults_off_nests_and_restores():
    assert ag.is_deterministic() is False
    with ag.deterministic():
        assert ag.is_deterministic() is True
        with ag.deterministic(False):
            assert ag.is_deterministic() is False
            with ag.deterministic(None):               # None: follow whatever is set
                assert ag.is_deterministic() is False
            with ag.deterministic(True):
                assert ag.is_deterministic() is True
            assert ag.is_deterministic() is False
        assert ag.is_deterministic() is True
    assert ag.is_deterministic() is False


def test_switch_is_restored_after_an_exception():
    with pytest.raises(ValueError):
        with ag.deterministic():
            raise ValueError("x")
    assert ag.is_deterministic() is False
    prev = ag.set_deterministic(True)
    try:
        assert prev is False and ag.is_deterministic() is True
        with pytest.raises(ValueError):
            with ag.deterministic(False):
                raise ValueError("x")
        assert ag.is_deterministic() is True
        with ag.deterministic(None):
            assert ag.is_deterministic() is True
    finally:
        ag.set_deterministic(False)
    assert ag.is_deterministic() is False


def test_switch_ignores_torch_and_the_environment(monkeypatch):
    import torch
    monkeypatch.setenv("NRGBD_DETERMINISTIC", "1")
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        assert ag.is_deterministic() is False
    finally:
        torch.use_deterministic_algorithms(before)


def test_keywords():
    from neuralrgbd_amd import ops, train_step
    assert inspect.signature(ops.costvol_bwd).parameters["deterministic"].default is False
    assert inspect.signature(train_step.train).parameters["deterministic"].default is None
    assert inspect.signature(train_step.TrainGraph.__init__).parameters["deterministic"].default is None
    # PlaneSweepCost.apply keeps its positional signature
    assert list(inspect.signature(ag.PlaneSweepCost.forward).parameters) == [
        "ctx", "texels", "KR", "Kt", "rays", "d_candi", "cx", "cy", "sigma", "C", "dist", "align_corners"]
    tg = train_step.TrainGraph(None, None, 2, None, None, deterministic=True)
    assert tg.deterministic is True and train_step.TrainGraph(None, None, 2, None, None).deterministic is None


def test_abi_has_the_entries():
    from neuralrgbd_amd import _lib
    assert _lib.SIGNATURES["nrgbd_costvol_bwd_det"] == _lib.SIGNATURES["nrgbd_costvol_bwd"]
    assert _lib.SIGNATURES["nrgbd_costvol_bwd_det_workspace"] == _lib.SIGNATURES["nrgbd_costvol_bwd_workspace"]


# ---- the fixed-point accumulation ----------------------------------------------------------------------------------------------

def scale_exponent(h, w, D):
    """S of costvol_bwd_det.hip (det_scale_exponent), None where the shape is refused."""
    n = h * w * D
    lg = 0
    while (1 << lg) < n:
        lg += 1
    S = min(40, 61 - lg)
    return None if S < 32 else S


def fixed_point_sum(terms, S=40):
    """The kernel's three passes on one element: fp32 terms -> (integer sum, fp32 result)."""
    t = np.asarray(terms, np.float32)
    bits = t.view(np.uint32) & np.uint32(0x7fffffff)
    m = int(bits.max()) if t.size else 0                      # pass 1: integer max of the |term| bit patterns
    if m == 0:
        return 0, np.float32(0.0)
    if m >= 0x7f800000:
        return None, np.float32(np.nan)
    ef = max(m >> 23, 1)                                      # exponent field; subnormal maxima count as 2^-126
    q = np.rint(t.astype(np.float64) * 2.0 ** (S + 127 - ef)).astype(np.int64)        # pass 2: exact scaling, one rounding (even)
    s = int(q.sum())                                          # integer sum: any order
    return s, np.float32(float(s) * 2.0 ** (ef - 127 - S))    # pass 3: int64 -> double -> exact scaling -> one rounding


def _terms(rng, n, binades):
    return (rng.standard_normal(n) * 2.0 ** rng.uniform(-binades / 2.0, binades / 2.0, n)).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 3, 17, 256, 1000, 4096])
@pytest.mark.parametrize("binades", [0, 8, 30])
def test_fixed_point_sum_is_order_independent_and_within_its_error(n, binades):
    rng = np.random.RandomState(100 * n + binades)
    for trial in range(4):
        t = _terms(rng, n, binades)
        s0, r0 = fixed_point_sum(t)
        for _ in range(6):
            p = rng.permutation(n)
            s1, r1 = fixed_point_sum(t[p])
            assert s1 == s0 and r1.tobytes() == r0.tobytes()
        # also in chunks (what separate lanes and workgroups do: partial sums in any grouping)
        cut = sorted(rng.randint(0, n + 1, 3))
        ef = max((int((t.view(np.uint32) & np.uint32(0x7fffffff)).max()) >> 23), 1)
        q = np.rint(t.astype(np.float64) * 2.0 ** (40 + 127 - ef)).astype(np.int64)
        assert sum(int(c.sum()) for c in np.split(q, cut)) == s0
        exact = math.fsum(float(x) for x in t)
        M = float(np.abs(t).max())
        assert abs(s0) < 2 ** 62 and float(np.abs(q).max()) < 2.0 ** 41
        assert abs(float(r0) - exact) <= n * M * 2.0 ** -40 + U * abs(exact)
        # and therefore inside the comparator's allowance for the summation alone: gamma(n) A with A = sum |t| >= M
        A = math.fsum(abs(float(x)) for x in t)
        assert n * M * 2.0 ** -40 + U * abs(exact) <= (n * U / (1 - n * U)) * A + U * abs(exact)


def test_fixed_point_sum_cancellation_keeps_small_terms():
    """+M, -M and a term 2^-30 M: the small one survives (it is a multiple of 2^(E-40))."""
    t = np.array([3.0, -3.0, 3.0 * 2.0 ** -30], np.float32)
    for p in ([0, 1, 2], [2, 0, 1], [0, 2, 1]):
        _, r = fixed_point_sum(t[p])
        assert r == np.float32(3.0 * 2.0 ** -30)


def test_fixed_point_sum_special_values():
    assert fixed_point_sum([]) == (0, np.float32(0.0))
    s, r = fixed_point_sum([0.0, -0.0, 0.0])
    assert s == 0 and r.tobytes() == np.float32(0.0).tobytes()              # +0, never -0
    for bad in (np.inf, -np.inf, np.nan):
        for order in ([1.0, bad, -2.0], [bad, 1.0, -2.0], [1.0, -2.0, bad]):
            assert np.isnan(fixed_point_sum(order)[1])
    assert np.isnan(fixed_point_sum([np.inf, -np.inf])[1]) and np.isnan(fixed_point_sum([np.inf, np.inf])[1])
    # subnormal terms: scaled as 2^-126, summed exactly
    tiny = np.array([1e-40, 2e-40, -5e-41], np.float32)
    _, r = fixed_point_sum(tiny)
    assert r == np.float32(math.fsum(float(x) for x in tiny))
    # the largest finite terms: no overflow of the scaled value, the sum rounds to inf only if the exact sum does
    big = np.array([3e38, -3e38, 1e38], np.float32)
    assert fixed_point_sum(big)[1] == np.float32(1e38)


def test_scale_exponent_leaves_headroom():
    assert scale_exponent(64, 96, 64) == 40 and scale_exponent(24, 40, 64) == 40
    assert scale_exponent(192, 256, 64) == 39
    assert scale_exponent(2048, 2048, 128) == 32 and scale_exponent(2048, 2048, 256) is None
    for h, w, D in ((64, 96, 64), (192, 256, 64), (480, 640, 128), (2048, 2048, 128)):
        S = scale_exponent(h, w, D)
        assert h * w * D * 2 ** (S + 1) <= 2 ** 62            # every term below 2^(S+1), at most h w D of them per element
