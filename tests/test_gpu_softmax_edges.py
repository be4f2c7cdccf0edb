"""GPU: the depth-probability head (csrc/softmax.hip) at its dispatch edges against the float64 comparator of tests/softmax_ref.py.

Gates (derived in softmax_ref's docstring; u = 2^-24).  Planar forward |out - ref| <= K u (|z - m| + |log s| + D), backward
|gz - ref| <= K u |scale| (|g| + p (|sum g| + D sum|g|)), depth |depth - ref| <= u (K + D + 1) sum p |d|; wherever the expected value
is not finite its class (NaN, +inf, -inf) is compared exactly, so no element is left out.  One-hot columns, constant columns, the
-inf entries of the backward, the rows forms against the planar ones, the uint16 maps and the NLL gradient are compared bit for
bit; the NLL count is exact and the loss within gamma_10 sum|t| / count (fp32's u), itself inside gamma_n sum|t| / count.

K: the worst |error| / bound at K = 1 over the benign family (a, b unit-normal x 5, D in {64, 128, 200}, 257 pixels) measured on an
MI355X was 0.6673 (D = 64; 0.4074 at 128, 0.3133 at 200; softmax_ref.K_MEASURED, profiles/softmax_edges.txt holds the run); K is
twice that, 1.3346, and gates every edge family.  (That run was made while the kernels took (z - m) - log s in two fp32
subtractions; K stands for expf and logf and holds as fixed.  With the one rounding the kernels take now the family measures 0.3474.)

Every buffer a kernel is handed lies between sentinel words that must be intact afterwards."""
import ctypes

import numpy as np
import pytest
import torch

import softmax_ref as sr
from neuralrgbd_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                    # guard words on either side of every buffer
SENT = {torch.float32: -12345.5, torch.int64: -12345, torch.int16: -12345}


class Guarded:
    """Named device buffers, each between GUARD sentinel words: `add(name, array)` uploads a copy, `add(name, shape=, dtype=)` makes a
    sentinel-filled one (uint16 maps are kept as int16 words)."""

    def __init__(self):
        self._outer, self._inner = {}, {}

    def add(self, name, array=None, shape=None, dtype=torch.float32):
        if array is not None:
            src = torch.from_numpy(np.ascontiguousarray(array))
            shape, dtype = tuple(src.shape), src.dtype
        n = int(np.prod(shape))
        outer = torch.full((n + 2 * GUARD,), SENT[dtype], dtype=dtype, device=DEV)
        inner = outer[GUARD:GUARD + n].view(shape)
        if array is not None:
            inner.copy_(src)
        self._outer[name], self._inner[name] = outer, inner
        return inner

    def __getitem__(self, name):
        return self._inner[name]

    def np(self, name):
        return self._inner[name].cpu().numpy()

    def intact(self):
        ok = True
        for name, outer in self._outer.items():
            n = self._inner[name].numel()
            ok = ok and bool((outer[:GUARD] == SENT[outer.dtype]).all()) and bool((outer[GUARD + n:] == SENT[outer.dtype]).all())
        return ok


def _call(entry, *args):
    with torch.cuda.device(DEV):
        rc = getattr(_lib.load(), entry)(*args, ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    _lib.check(rc, entry)


def _done(g):
    torch.cuda.synchronize()
    assert g.intact(), "a guard word was overwritten"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(a, b):
    """Bit for bit, a NaN matching a NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _forward(a, b, scale):
    g = Guarded()
    g.add("a", a)
    if b is not None:
        g.add("b", b)
    D, n = a.shape
    g.add("out", shape=(D, n))
    _call("nrgbd_logsoftmax_d", ops._p(g["a"]), ops._p(g["b"] if b is not None else None), float(scale), ops._p(g["out"]), D, n)
    _done(g)
    return g.np("out")


def _backward(logp, gr, scale):
    g = Guarded()
    g.add("logp", logp)
    g.add("g", gr)
    D, n = logp.shape
    g.add("gz", shape=(D, n))
    _call("nrgbd_logsoftmax_d_bwd", ops._p(g["logp"]), ops._p(g["g"]), float(scale), ops._p(g["gz"]), D, n)
    _done(g)
    return g.np("gz")


def _regress(logp, d, rows, export, scales=(1000.0, 60000.0)):
    """logp [D, n] -> depth, conf (and the two uint16 maps of the export) of the planar or the channels-last (`rows`) entry."""
    D, n = logp.shape
    g = Guarded()
    g.add("logp", logp.T if rows else logp)
    g.add("d", d)
    g.add("depth", shape=(n,))
    g.add("conf", shape=(n,))
    if export:
        g.add("du", shape=(n,), dtype=torch.int16)
        g.add("cu", shape=(n,), dtype=torch.int16)
        _call("nrgbd_export_depth_u16_rows" if rows else "nrgbd_export_depth_u16", ops._p(g["logp"]), ops._p(g["d"]), float(scales[0]),
              float(scales[1]), ops._p(g["depth"]), ops._p(g["conf"]), ops._p(g["du"]), ops._p(g["cu"]), D, n)
    else:
        _call("nrgbd_depth_regress_rows" if rows else "nrgbd_depth_regress", ops._p(g["logp"]), ops._p(g["d"]), ops._p(g["depth"]),
              ops._p(g["conf"]), D, n)
    _done(g)
    out = (g.np("depth"), g.np("conf"))
    return out + ((g.np("du").view(np.uint16), g.np("cu").view(np.uint16)) if export else ())


def test_the_constant_K_is_what_was_measured():
    """The benign family at K = 1: the figure K was fixed from (twice the worst ratio), and K gates it as it gates every edge family."""
    worst = 0.0
    for D in sr.BENIGN_D:
        a, b = sr.benign_volume(D)
        want, bound = sr.logsoftmax(a, b, 1.0)
        ok, ratio, bad = sr.compare(_forward(a, b, 1.0), want, bound, sr.K)
        print("[softmax] benign D %d: worst |error| / bound at K = 1: %.4f" % (D, ratio))
        assert ok, (D, ratio, bad)
        worst = max(worst, ratio)
    print("[softmax] benign family: worst ratio %.4f (recorded %s, K %.4f)" % (worst, sr.K_MEASURED, sr.K))
    assert sr.K == 2.0 * sr.K_MEASURED and sr.K <= 4.0
    assert worst <= 1.25 * sr.K_MEASURED                           # the recorded figure still describes the device's functions


@pytest.mark.parametrize("D,n", sr.planar_cases())
def test_planar_forward_over_the_tables(D, n):
    """Every family and every (scale, b) variant of one table entry: the bound, the classes, one-hot and constant columns bit for
    bit, two runs the same bits.

    Measured on an MI355X (worst |error| / bound at K = 1; the gate is K = 1.3346): D 1: 0, D 2: 0.784, D 3: 0.893, D 5: 0.928,
    D 63: 0.652, D 64: 0.655, D 65: 0.647, D 127: 0.498, D 128: 0.500, D 129: 0.500, D 256: 0.321.  With both subtractions of
    (z - m) - log s in fp32, as the kernels took them before, D 3 n 65 stood at 1.384, D 5 at 1.496 (n 65), 1.431 (n 63) and 1.459
    (n 257): two roundings at the magnitude |z - m| where the bound's form counts one."""
    worst, failed = 0.0, []
    for scale, with_b in sr.planar_variants():
        a, b, fam = sr.make_volume(D, n, scale, with_b)
        want, bound = sr.logsoftmax(a, b, scale)
        got = _forward(a, b, scale)
        ok, ratio, bad = sr.compare(got, want, bound, sr.K)
        worst = max(worst, ratio)
        if not ok:
            by_fam = {sr.FAMILIES[f]: round(sr.compare(got[:, fam == f], want[:, fam == f], bound[:, fam == f], sr.K)[1], 3)
                      for f in set(fam.tolist()) if not sr.compare(got[:, fam == f], want[:, fam == f], bound[:, fam == f], sr.K)[0]}
            failed.append((scale, with_b, bad, by_fam))
        z = sr.form_z(a, b, scale)
        one = fam == sr.ONEHOT                                      # exact: +0.0 at the peak, z_k elsewhere
        assert np.array_equal(_bits(got[:, one]), _bits(np.where(z[:, one] == 0, np.float32(0.0), z[:, one]))), (scale, with_b)
        const = got[:, fam == sr.CONST]
        assert (_bits(const) == _bits(const)[0:1]).all() and np.isfinite(const).all(), (scale, with_b)
        assert np.array_equal(_bits(_forward(a, b, scale)), _bits(got)), "two runs differ"
    print("[softmax] forward D %d n %d: worst |error| / bound at K = 1: %.4f (K %.4f)" % (D, n, worst, sr.K))
    assert not failed, failed


@pytest.mark.parametrize("D", sr.BWD_D)
def test_planar_backward(D):
    worst = 0.0
    for n in sr.BWD_N:
        logp, fam = sr.make_logp(D, n)
        gr = np.random.RandomState(40 + D + n).randn(D, n).astype(np.float32)
        for scale in sr.SCALES:
            want, bound = sr.logsoftmax_bwd(logp, gr, scale)
            got = _backward(logp, gr, scale)
            ok, ratio, bad = sr.compare(got, want, bound, sr.K)
            worst = max(worst, ratio)
            assert ok, (D, n, scale, ratio, bad)
            inf = np.isneginf(logp)
            assert n < 9 or inf.any()
            assert np.array_equal(_bits(got[inf]), _bits(np.float32(scale) * gr[inf])), "gz != scale g at a -inf entry"
    print("[softmax] backward D %d: worst |error| / bound at K = 1: %.4f (K %.4f)" % (D, worst, sr.K))


def test_backward_through_LogSoftmaxD_with_scale_and_b():
    """scale = 0.5 with a second operand: the two input gradients come from two launches (scale and 1)."""
    from neuralrgbd_amd.autograd import LogSoftmaxD
    D, h, w = 129, 5, 13
    a, b, fam = sr.make_volume(D, h * w, 0.5, True)
    ta = torch.from_numpy(a).to(DEV).view(1, D, h, w).requires_grad_(True)
    tb = torch.from_numpy(b).to(DEV).view(1, D, h, w).requires_grad_(True)
    gr = np.random.RandomState(3).randn(D, h * w).astype(np.float32)
    out = LogSoftmaxD.apply(ta, tb, 0.5)
    out.backward(torch.from_numpy(gr).to(DEV).view(1, D, h, w))
    want, bound = sr.logsoftmax(a, b, 0.5)
    logp = out.detach().cpu().numpy().reshape(D, -1)
    assert sr.compare(logp, want, bound, sr.K)[0]
    for grad, scale in ((ta.grad, 0.5), (tb.grad, 1.0)):
        wg, bg = sr.logsoftmax_bwd(logp, gr, scale)
        ok, ratio, bad = sr.compare(grad.cpu().numpy().reshape(D, -1), wg, bg, sr.K)
        assert ok, (scale, ratio, bad)


@pytest.mark.parametrize("D", sr.ROWS_D)
def test_rows_forms_have_the_planar_bits_and_the_depth_its_bound(D):
    d = sr.make_d_candi(D)
    for n in sr.ROWS_N:
        logp, fam = sr.make_logp(D, n)
        depth, conf, terms = sr.regress(logp, d)
        bound = sr.depth_bound(terms, sr.K)
        nan = np.isnan(conf)
        assert np.array_equal(nan, np.isin(fam, (sr.ALLNEGINF, sr.POSINF, sr.NAN))) and np.array_equal(nan, np.isnan(depth))
        one = fam == sr.ONEHOT
        planar = _regress(logp, d, False, False)
        rows = _regress(logp, d, True, False)
        eplanar = _regress(logp, d, False, True)
        erows = _regress(logp, d, True, True)
        for x, y in zip(planar + eplanar[:2], rows + erows[:2]):
            assert _same_bits(x, y), "rows and planar bits differ (D %d n %d)" % (D, n)
        assert np.array_equal(eplanar[2], erows[2]) and np.array_equal(eplanar[3], erows[3])
        for name, got in (("regress", planar), ("export", eplanar)):
            ok, ratio, bad = sr.compare(got[0], depth, bound, 1.0)
            assert ok, (name, D, n, ratio, bad)
            assert np.array_equal(_bits(got[0][one]), _bits(d[np.argmax(logp[:, one], 0)])), "one-hot depth is not d_k"
            # a column holding a NaN: depth NaN and confidence NaN (torch.max), nowhere else
            assert np.array_equal(np.isnan(got[0]), nan) and np.array_equal(np.isnan(got[1]), nan), (name, D, n)
        assert np.array_equal(_bits(planar[1][~nan]), _bits(conf[~nan].astype(np.float32))) and (planar[1][one] == 0).all()
        with np.errstate(all="ignore"):
            ec = np.exp(conf)
        assert sr.compare(eplanar[1], ec, sr.U * (1 + 1e-6) * ec, 1.0)[0] and (eplanar[1][one] == 1).all()
        with np.errstate(all="ignore"):                             # the uint16 maps by the definition, from the kernel's own fp32 maps
            assert np.array_equal(eplanar[2], sr.to_u16(eplanar[0] * np.float32(1000.0)))
            assert np.array_equal(eplanar[3], sr.to_u16(eplanar[1] * np.float32(60000.0)))
        assert (eplanar[2][nan] == 0).all() and (eplanar[3][nan] == 0).all()
        assert (eplanar[3][one] == 60000).all()


def test_to_u16_table_through_the_kernels():
    """depth = exp(0) v and conf = exp(0), scaled by 1 resp. v: the export's two conversions see the table's values themselves."""
    for v, want in zip(sr.U16_IN, sr.U16_OUT):
        for rows in (False, True):
            D = 4 if rows else 1                                    # the rows entry takes multiples of 4: three candidates of weight 0
            logp = np.full((D, 3), -np.inf, np.float32)
            logp[0] = 0.0
            d = np.ones(D, np.float32)
            d[0] = v
            depth, conf, du, cu = _regress(logp, d, rows, True, scales=(1.0, v))
            assert du.tolist() == [want] * 3 and cu.tolist() == [want] * 3, (v, rows, du, cu, depth)
            assert _same_bits(depth, np.full(3, np.float32(0.0) + np.float32(v), np.float32)) and (conf == 1).all()


@pytest.mark.parametrize("n,D,channels_last", sr.NLL_CASES)
@pytest.mark.parametrize("ignore", sr.NLL_IGNORE)
def test_nll_loss_count_and_gradient(n, D, channels_last, ignore):
    logp = sr.make_nll_logp(n, D)
    t = sr.make_targets(n, D, ignore)
    ref = sr.nll(logp, t, ignore, D)
    G = _lib.load().nrgbd_nll_workgroups(n)
    assert G == (n + 255) // 256 and (n != 65792 or G == 257)
    g = Guarded()
    g.add("logp", logp.T if channels_last else logp)
    g.add("target", t)
    g.add("partial", shape=(G, 2))
    g.add("stat", shape=(2,))
    g.add("gout", np.array([3.0], np.float32))
    g.add("grad", shape=(n, D) if channels_last else (D, n))
    _call("nrgbd_nll_fwd", ops._p(g["logp"]), ctypes.c_void_p(g["target"].data_ptr()), int(ignore), D, n, int(channels_last),
          ops._p(g["partial"]), ops._p(g["stat"]))
    _call("nrgbd_nll_bwd", ctypes.c_void_p(g["target"].data_ptr()), int(ignore), ops._p(g["gout"]), ops._p(g["stat"]), ops._p(g["grad"]),
          D, n, int(channels_last))
    _done(g)
    loss, count = (float(x) for x in g.np("stat"))
    tight, plain = sr.nll_bound(ref["abs_sum"], ref["count"], n)
    print("[softmax] nll n %d D %d cl %d ignore %d: |loss - fsum| %.3g, derived gate %.3g, gamma_n gate %.3g, count %d"
          % (n, D, channels_last, ignore, abs(loss - ref["loss"]), tight, plain, ref["count"]))
    assert count == ref["count"]
    assert abs(loss - ref["loss"]) <= tight <= plain
    want = sr.nll_grad(t, ref["counted"], D, 3.0, ref["count"])
    grad = g.np("grad")
    assert np.array_equal(_bits(grad.T if channels_last else grad), _bits(want)), "gradient bits differ"
    assert int((grad != 0).sum()) == ref["count"]


def test_nll_with_every_pixel_ignored_is_nan():
    n, D = 300, 8
    logp = sr.make_nll_logp(n, D)
    for t in (np.full(n, 3, np.int64), np.full(n, -1, np.int64), np.full(n, D, np.int64)):
        g = Guarded()
        g.add("logp", logp)
        g.add("target", t)
        g.add("partial", shape=(2, 2))
        g.add("stat", shape=(2,))
        _call("nrgbd_nll_fwd", ops._p(g["logp"]), ctypes.c_void_p(g["target"].data_ptr()), 3, D, n, 0, ops._p(g["partial"]), ops._p(g["stat"]))
        _done(g)
        stat = g.np("stat")
        assert np.isnan(stat[0]) and stat[1] == 0
