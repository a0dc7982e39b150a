"""Kernel-level tests of the BatchNorm and channel-sum kernels of csrc/train_glue.hip (-m gpu): the C entry points called directly,
every reference float64 on the CPU and computed from exactly the fp32 / bf16 values handed to the kernel.  Outputs and scratch are
carved out of NaN-filled allocations whose guard bands must come back untouched.  Gates and measured figures:
tests/golden/README_train_glue.md."""
import math

import pytest
import torch

from cobevt_amd import autograd as ag
from cobevt_amd import ops
from carved import BF16, DTYPES, ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED, F32, U, UB, Carved, _dev, _int_map, _lib, _ok
from util import assert_close

pytestmark = pytest.mark.gpu


def _scratch(scratch_blocks, rows, c, dev):
    """exactly scratch_blocks * 2 * C doubles; the band behind it holds what a launch of one workgroup per row of a thread would write
    (the library wants one per 8 rows of a thread before the cap)"""
    rstep = max(1, 256 // max(1, c // 8))
    return Carved(scratch_blocks * 2 * c, torch.float64, dev, behind=(rows + rstep - 1) // rstep * 2 * c)


def _group_path(c):
    return c >= 8 and c % 8 == 0 and c // 8 <= 256


def _rows_list(c):
    """1; rstep - 1; a thread gets three rows (the paired loop and the tail both run); three workgroups with a partial last one;
    4001 (<= 4096: integer sums stay exact in fp32), where scratch_blocks = 3 caps the workgroup count"""
    if not _group_path(c):
        return [1, 255, 1000, 4001]
    rstep = 256 // (c // 8)
    return sorted({1, max(1, rstep - 1), 2 * rstep + 1, min(24 * rstep - 5, 4001), 4001})


def _channel_sums(dev, x, shift, want_sq, want_f, scratch_blocks):
    """-> (rc, sum/sumsq Carved, out_f Carved | None, scratch Carved | None)"""
    rows, c = x.shape
    n = 2 * c if want_sq else c
    acc = Carved(n, torch.float64, dev)
    out_f = Carved(n, F32, dev) if want_f else None
    scr = _scratch(scratch_blocks, rows, c, dev) if _group_path(c) else None
    rc = _lib().cobevt_channel_sums(ag._p(x), ag._p(shift), ag._p(acc.t), ag._p(acc.t[c:]) if want_sq else None,
                                    ag._p(out_f.t) if want_f else None, ag._p(scr.t) if scr else None, scratch_blocks,
                                    ops.dcode(x.dtype), rows, c, ag._stream())
    return rc, acc, out_f, scr


# ----------------------------------------------------------------------------------------------
# 1. cobevt_channel_sums, cobevt_f64_to_f32
# ----------------------------------------------------------------------------------------------
GROUP_C = [8, 24, 40, 64, 96, 2048]                  # G = 3, 5, 12 do not divide 256
GENERIC_C = [2, 3, 13, 260, 2056]                    # 260: two blockIdx.x blocks, C % 8 != 0; 2056: G > 256


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", GROUP_C + GENERIC_C)
def test_channel_sums_exact(cuda, dtype, c):
    """integer-valued input: every fp32 partial sum is an exact integer below 2^24 (|x - shift| <= 11, <= 4001 rows), so the fp64 sums
    must EQUAL the int64 reference - for every combination of sumsq / out_f / shift and for scratch_blocks 1, 3 and 512"""
    group = _group_path(c)
    for rows in _rows_list(c):
        x = _int_map(rows, c, dtype, 100 + rows)
        xd = x.to(cuda)
        sh = ((torch.arange(c) * 5) % 7 - 3).float()
        for shift in ((None, sh) if group else (None,)):
            a = x.to(torch.int64) - (0 if shift is None else shift.to(torch.int64))
            ref = torch.cat([a.sum(0), (a * a).sum(0)])
            shd = None if shift is None else shift.to(cuda)
            for want_sq in (True, False):
                for want_f in ((True, False) if group else (False,)):
                    for sb in ((1, 3, 512) if group else (0,)):
                        what = "channel_sums C=%d rows=%d %s shift=%s sumsq=%s out_f=%s scratch_blocks=%d" % (
                            c, rows, dtype, shift is not None, want_sq, want_f, sb)
                        rc, acc, out_f, scr = _channel_sums(cuda, xd, shd, want_sq, want_f, sb)
                        _ok(rc, what)
                        n = 2 * c if want_sq else c
                        got = acc.check(what).cpu()
                        assert torch.equal(got, ref[:n].double()), what
                        if scr is not None:
                            scr.check(what + " scratch", written=None)
                        if out_f is not None:
                            assert torch.equal(out_f.check(what + " out_f").cpu(), ref[:n].float()), what + " out_f"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", GROUP_C + GENERIC_C)
def test_channel_sums_rounding(cuda, dtype, c):
    """N(0, 1) input, the shapes of the exact cases: |err| <= k 2^-24 sum|a_i| per channel, the bound of any fp32 summation order of k
    terms per partial, k = ceil(rows / scratch_blocks) from the arguments; the fp64 combination of the partials adds nothing at this scale.
    Holds for every map: a launch that gives a thread more than k rows keeps that thread's sums in fp64 and rounds them once."""
    worst, missed = 0.0, []
    for rows in _rows_list(c):
        g = torch.Generator().manual_seed(7 * rows + c)
        x = torch.randn(rows, c, generator=g).to(dtype)
        xd = x.to(cuda)
        a = x.double()
        ref = torch.cat([a.sum(0), (a * a).sum(0)])
        mag = torch.cat([a.abs().sum(0), (a * a).sum(0)])
        for sb in ((1, 3, 512) if _group_path(c) else (512,)):
            what = "channel_sums C=%d rows=%d %s scratch_blocks=%d" % (c, rows, dtype, sb)
            rc, acc, out_f, scr = _channel_sums(cuda, xd, None, True, _group_path(c), sb)
            _ok(rc, what)
            got = acc.check(what).cpu()
            if scr is not None:
                scr.check(what + " scratch", written=None)
            k = (rows + sb - 1) // sb
            ratio = float(((got - ref).abs() / (k * U * mag)).max())
            worst = max(worst, ratio)
            print("%s: max |err| / (k u sum|a|) = %.3f (k = %d)" % (what, ratio, k))
            if ratio > 1.0:
                missed.append("%s: %.3f" % (what, ratio))
            if out_f is not None:
                assert torch.equal(out_f.check(what + " out_f").cpu(), got.float()), what + " out_f"
    print("channel_sums rounding C=%d %s: worst ratio %.3f" % (c, dtype, worst))
    assert not missed, "max |err| / (k u sum|a_i|) > 1: " + "; ".join(missed)


def test_channel_sums_error_codes(cuda):
    """shift / out_f are not available off the 8-channel piece (COBEVT_ERR_UNSUPPORTED); sumsq must be sum + C (COBEVT_ERR_ARG);
    a refused call writes nothing"""
    x = torch.ones(5, 13, device=cuda)
    for want_shift, want_f in ((True, False), (False, True)):
        acc, out_f = Carved(26, torch.float64, cuda), Carved(26, F32, cuda)
        shift = torch.zeros(13, device=cuda) if want_shift else None
        rc = _lib().cobevt_channel_sums(ag._p(x), ag._p(shift), ag._p(acc.t), ag._p(acc.t[13:]), ag._p(out_f.t) if want_f else None,
                                        None, 0, 1, 5, 13, ag._stream())
        assert rc == ERR_UNSUPPORTED
        acc.check("refused call", written=False)
        out_f.check("refused call", written=False)
    x = torch.ones(5, 16, device=cuda)
    acc, scr = Carved(48, torch.float64, cuda), _scratch(4, 5, 16, cuda)
    rc = _lib().cobevt_channel_sums(ag._p(x), None, ag._p(acc.t), ag._p(acc.t[32:]), None, ag._p(scr.t), 4, 1, 5, 16, ag._stream())
    assert rc == ERR_ARG
    acc.check("refused call", written=False)
    scr.check("refused call", written=False)


@pytest.mark.parametrize("n", [1, 257, 1000])
def test_f64_to_f32(cuda, n):
    """round-to-nearest-even of every element, nothing past n"""
    g = torch.Generator().manual_seed(n)
    v = torch.randn(n, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-30, 30, (n,), generator=g).double()
    v[0] = 1.0 + 2.0 ** -24                            # a tie: rounds to even (1.0)
    out, vd = Carved(n, F32, cuda), v.to(cuda)
    _ok(_lib().cobevt_f64_to_f32(ag._p(vd), ag._p(out.t), n, ag._stream()), "cobevt_f64_to_f32")
    assert torch.equal(out.check("f64_to_f32").cpu(), v.float())


# ----------------------------------------------------------------------------------------------
# 2. cobevt_bn_batch_stats, cobevt_bn_finalize
# ----------------------------------------------------------------------------------------------
class Stats(object):
    """the four per-channel outputs + running statistics + num_batches_tracked, all guard-banded"""

    def __init__(self, c, dev, tracked, seed=0, running_mean=None):
        g = torch.Generator().manual_seed(1000 + seed)
        self.c, self.dev, self.tracked = c, dev, tracked
        self.out = {k: Carved(c, F32, dev) for k in ("scale", "shift", "mean", "rstd")}
        self.rm0 = (torch.randn(c, generator=g) * 0.2) if running_mean is None else running_mean.clone()
        self.rv0 = torch.rand(c, generator=g) + 0.5
        self.rm, self.rv, self.nbt = Carved(c, F32, dev), Carved(c, F32, dev), Carved(1, torch.int64, dev)
        self.rm.t.copy_(self.rm0)
        self.rv.t.copy_(self.rv0)
        self.nbt.t.fill_(41)

    def ptrs(self):
        return [ag._p(self.out[k].t) for k in ("scale", "shift", "mean", "rstd")]

    def check(self, what, ref, training=True, tol=1e-5):
        """ref: dict of float64 mean / var (biased) / unbiased / gamma / beta / eps / momentum"""
        rstd = 1.0 / torch.sqrt(ref["var"] + ref["eps"])
        gamma = torch.ones(self.c, dtype=torch.float64) if ref["gamma"] is None else ref["gamma"].double()
        beta = torch.zeros(self.c, dtype=torch.float64) if ref["beta"] is None else ref["beta"].double()
        want = {"mean": ref["mean"], "rstd": rstd, "scale": gamma * rstd, "shift": beta - ref["mean"] * gamma * rstd}
        for k in ("mean", "rstd", "scale", "shift"):
            assert_close(self.out[k].check(what + " " + k), want[k], tol, what + " " + k)
        rm, rv, nbt = self.rm.check(what + " running_mean"), self.rv.check(what + " running_var"), self.nbt.check(what + " nbt")
        if self.tracked and training:
            m = ref["momentum"]
            assert_close(rm, (1.0 - m) * self.rm0.double() + m * ref["mean"], tol, what + " running_mean")
            assert_close(rv, (1.0 - m) * self.rv0.double() + m * ref["unbiased"], tol, what + " running_var")
            assert int(nbt) == 42, what + ": num_batches_tracked must rise by exactly 1"
        else:
            assert torch.equal(rm.cpu(), self.rm0) and torch.equal(rv.cpu(), self.rv0) and int(nbt) == 41, what + ": running statistics touched"


def _ref_stats(x, gamma, beta, eps, momentum):
    a = x.double()
    rows = a.shape[0]
    mean = a.mean(0)
    var = ((a - mean) ** 2).mean(0)
    eps64 = float(torch.tensor(eps, dtype=torch.float32))
    return {"mean": mean, "var": var, "unbiased": var * rows / (rows - 1) if rows > 1 else var * 0.0, "gamma": gamma, "beta": beta,
            "eps": eps64, "momentum": float(torch.tensor(momentum, dtype=torch.float32))}


def _batch_stats(dev, x, st, gamma, beta, eps, momentum, scratch_blocks=512):
    rows, c = x.shape
    scr = _scratch(scratch_blocks, rows, c, dev)
    tr = st.tracked
    xd, gd, bd = _dev(dev, x, gamma, beta)
    rc = _lib().cobevt_bn_batch_stats(ag._p(xd), ag._p(gd), ag._p(bd), ag._p(st.rm.t) if tr else None,
                                      ag._p(st.rv.t) if tr else None, *st.ptrs(), ag._p(scr.t), scratch_blocks, ops.dcode(x.dtype), rows, c,
                                      eps, momentum, ag._p(st.nbt.t) if tr else None, ag._stream())
    _ok(rc, "cobevt_bn_batch_stats")
    scr.check("bn_batch_stats scratch", written=None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,rows", [(8, 300), (24, 343), (64, 2049), (2048, 19), (64, 1), (24, 1)])
@pytest.mark.parametrize("tracked", [True, False])
@pytest.mark.parametrize("affine", [True, False])
def test_bn_batch_stats(cuda, dtype, c, rows, tracked, affine):
    """well-centred input (|mean| / std = 0.35): mean, rstd, scale, shift and the running-stat update (momentum 0.07, unbiased variance)
    against float64 at 1e-5; one channel constant (variance exactly 0 in the reference); rows == 1; scratch_blocks 512 and 2"""
    g = torch.Generator().manual_seed(c + rows)
    x = (torch.randn(rows, c, generator=g) * 2.0 + 0.7).to(dtype)
    x[:, 3] = x[0, 3]                                               # a constant channel
    gamma = (torch.rand(c, generator=g) + 0.5) if affine else None
    beta = (torch.randn(c, generator=g) * 0.3) if affine else None
    eps, momentum = 1e-3, 0.07
    ref = _ref_stats(x, gamma, beta, eps, momentum)
    for sb in (512, 2):
        st = Stats(c, cuda, tracked, seed=c)
        _batch_stats(cuda, x, st, gamma, beta, eps, momentum, sb)
        what = "bn_batch_stats C=%d rows=%d %s tracked=%s scratch_blocks=%d" % (c, rows, dtype, tracked, sb)
        st.check(what, ref)
        # the constant channel (every channel when rows == 1): rstd = 1 / sqrt(eps) to fp32 rounding, the mean to 1 ulp
        const = slice(None) if rows == 1 else slice(3, 4)
        rstd, mean = st.out["rstd"].t.cpu()[const].double(), st.out["mean"].t.cpu()[const].double()
        want = 1.0 / math.sqrt(ref["eps"])
        assert bool(((rstd - want).abs() <= 2.0 ** -23 * want).all()), what + ": rstd of a constant channel"
        assert bool(((mean - ref["mean"][const]).abs() <= 2.0 ** -23 * ref["mean"][const].abs()).all()), what + ": mean of a constant channel"


def test_bn_batch_stats_error_codes(cuda):
    """exactly one of running_mean / running_var null: COBEVT_ERR_ARG; C = 12 or 2056: COBEVT_ERR_SHAPE; nothing written"""
    for c, only_mean, only_var, want in ((16, True, False, ERR_ARG), (16, False, True, ERR_ARG), (12, True, True, ERR_SHAPE),
                                         (2056, True, True, ERR_SHAPE), (2056, False, False, ERR_SHAPE)):
        x = torch.ones(4, c, device=cuda)
        st = Stats(c, cuda, True)
        scr = _scratch(2, 4, c, cuda)
        rc = _lib().cobevt_bn_batch_stats(ag._p(x), None, None, ag._p(st.rm.t) if only_mean else None, ag._p(st.rv.t) if only_var else None,
                                          *st.ptrs(), ag._p(scr.t), 2, 1, 4, c, 1e-5, 0.1, None, ag._stream())
        assert rc == want, (c, only_mean, only_var, rc)
        for k in st.out:
            st.out[k].check("refused call", written=False)
        scr.check("refused call", written=False)
        assert torch.equal(st.rm.t.cpu(), st.rm0) and torch.equal(st.rv.t.cpu(), st.rv0)


@pytest.mark.parametrize("c", [8, 24, 64, 2048])
def test_bn_finalize_eval(cuda, c):
    """frozen statistics: scale / shift / mean / rstd from the running statistics, which stay bit-identical"""
    g = torch.Generator().manual_seed(c)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    for affine in (True, False):
        st = Stats(c, cuda, True, seed=c)
        gd, bd = _dev(cuda, gamma, beta)
        rc = _lib().cobevt_bn_finalize(None, None, ag._p(gd) if affine else None, ag._p(bd) if affine else None,
                                       ag._p(st.rm.t), ag._p(st.rv.t), *st.ptrs(), c, 77, 1e-3, 0.07, 0, 0, None, ag._stream())
        _ok(rc, "cobevt_bn_finalize")
        ref = {"mean": st.rm0.double(), "var": st.rv0.double(), "gamma": gamma if affine else None, "beta": beta if affine else None,
               "eps": float(torch.tensor(1e-3, dtype=torch.float32))}
        st.check("bn_finalize eval C=%d" % c, ref, training=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,rows", [(8, 300), (24, 343), (64, 2049), (2048, 19)])
@pytest.mark.parametrize("shifted", [True, False])
def test_bn_finalize_training_from_channel_sums(cuda, dtype, c, rows, shifted):
    """the three-launch form: cobevt_channel_sums (about the running mean when `shifted`) -> cobevt_bn_finalize(training = 1)"""
    g = torch.Generator().manual_seed(c + rows + 1)
    x = (torch.randn(rows, c, generator=g) * 2.0 + 0.7).to(dtype)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    st = Stats(c, cuda, True, seed=c + 1)
    rc, acc, _, scr = _channel_sums(cuda, x.to(cuda), st.rm.t if shifted else None, True, False, 512)
    _ok(rc, "cobevt_channel_sums")
    gd, bd = _dev(cuda, gamma, beta)
    rc = _lib().cobevt_bn_finalize(ag._p(acc.t), ag._p(acc.t[c:]), ag._p(gd), ag._p(bd), ag._p(st.rm.t), ag._p(st.rv.t),
                                   *st.ptrs(), c, rows, 1e-3, 0.07, 1, int(shifted), ag._p(st.nbt.t), ag._stream())
    _ok(rc, "cobevt_bn_finalize")
    st.check("bn_finalize training C=%d rows=%d %s shifted=%s" % (c, rows, dtype, shifted), _ref_stats(x, gamma, beta, 1e-3, 0.07))


# mean-dominated input: R = |batch mean - pivot| / std with std = 1; (name, batch mean, running mean | None)
MEAN_DOMINATED = [("untracked R=0", 0.0, None), ("untracked R=10", 10.0, None), ("untracked R=100", 100.0, None),
                  ("tracked, running mean = batch mean, R=100", 100.0, "batch"), ("tracked, running mean 100 std away", 0.0, 100.0)]


# (rows, scratch_blocks): at C = 64 a launch gives a thread 8 rows.  2880 rows over 512 slots: k = ceil(rows / scratch_blocks) = 6 < 8, the
# per-thread sums are fp64; over 256 slots (k = 12) and 5760 rows over 512 (k = 12) they are fp32 - the path of every training-size map
MEAN_DOMINATED_LAUNCHES = [(2880, 512), (2880, 256), (5760, 512)]


@pytest.mark.parametrize("rows,scratch_blocks", MEAN_DOMINATED_LAUNCHES, ids=["2880x512-f64sums", "2880x256-f32sums", "5760x512-f32sums"])
@pytest.mark.parametrize("name,offset,running", MEAN_DOMINATED, ids=[m[0].replace(" ", "_").replace(",", "") for m in MEAN_DOMINATED])
def test_bn_mean_dominated(cuda, name, offset, running, rows, scratch_blocks):
    """fp32 N(offset, 1), C = 64, gamma 1, beta 0, no residual, no activation: the statistics pushed through cobevt_bn_apply, on the
    fp64 and on the fp32 per-thread sums.  max |y - y_ref| (float64) may be at most max(4 x the same error of torch's fp32 F.batch_norm,
    1e-5 max|y_ref|): the factor 4 covers another summation order, the floor is the project's forward gate.  The sums are taken about
    row 0 of x: the pivot lies inside the data whatever the mean and the running mean (figures: tests/golden/README_train_glue.md)."""
    c, eps = 64, 1e-5
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, c, generator=g) + offset
    a = x.double()
    mean = a.mean(0)
    var = ((a - mean) ** 2).mean(0)
    y_ref = (a - mean) / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    rm = None if running is None else (mean.float() if running == "batch" else torch.full((c,), running))
    st = Stats(c, cuda, rm is not None, running_mean=rm)
    xd = x.to(cuda)
    _batch_stats(cuda, x, st, None, None, eps, 0.1, scratch_blocks)
    y = Carved(rows * c, F32, cuda)
    _ok(_lib().cobevt_bn_apply(ag._p(xd), None, ag._p(st.out["scale"].t), ag._p(st.out["shift"].t), ag._p(y.t), 1, rows, c, 0, ag._stream()),
        "cobevt_bn_apply")
    err = float((y.check(name).cpu().double().view(rows, c) - y_ref).abs().max())
    yt = torch.nn.functional.batch_norm(xd, None if rm is None else rm.to(cuda), None if rm is None else st.rv0.to(cuda), None, None, True, 0.1, eps)
    err_torch = float((yt.cpu().double() - y_ref).abs().max())
    gate = max(4.0 * err_torch, 1e-5 * float(y_ref.abs().max()))
    print("bn mean-dominated [%s, %d rows, scratch_blocks %d]: kernel %.3e, torch fp32 %.3e, gate %.3e" % (name, rows, scratch_blocks, err, err_torch, gate))
    assert err <= gate, "%s: max |y - y_ref| %.3e > %.3e (torch's fp32 batch_norm: %.3e)" % (name, err, gate, err_torch)


# ----------------------------------------------------------------------------------------------
# 3. cobevt_bn_apply          4. cobevt_bn_backward
# ----------------------------------------------------------------------------------------------
# (C, rows): items = rows C / 8 at 1023 | 1024 | 1025 | 2049 around the walk threshold 4 * 256 with a partial last span; a walk with
# G > 1; C = 24 (256 % G != 0): the piece-per-thread form on a large map; C = 2048, 4 rows: G = 256, items = 1024
APPLY_SHAPES = [(8, 1023), (8, 1024), (8, 1025), (8, 2049), (64, 257), (24, 500), (2048, 4)]


def _signed_zeros(t, rows, c):
    """rows 0 / 1 (when there are two) of channels 0 and 1: +0 and -0"""
    t[0, 0], t[0, 1] = 0.0, -0.0
    if rows > 1:
        t[1, 0], t[1, 1] = -0.0, 0.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,rows", APPLY_SHAPES)
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("res", [False, True])
def test_bn_apply(cuda, dtype, c, rows, act, res):
    """y = act(x scale + shift (+ res)) with scale / shift supplied by the test.  fp32: |err| <= 4 u (|x scale| + |shift| + |res|)
    elementwise (one fma, one add, slack 2); bf16: + 2^-8 |ref| for the output rounding.  Pre-activations of exactly +0 / -0 give 0."""
    g = torch.Generator().manual_seed(c * 13 + rows)
    x = torch.randn(rows, c, generator=g).to(dtype)
    r = torch.randn(rows, c, generator=g).to(dtype) if res else None
    scale, shift = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    shift[0], shift[1] = 0.0, -0.0
    _signed_zeros(x, rows, c)
    x[:, 1] = -x[:, 1].abs()                          # channel 1: x scale <= -0, shift = -0 (fma(-0, s, -0) = -0)
    x[:2, 1] = -0.0
    if res:
        r[:2, :2] = -0.0
    y = Carved(rows * c, dtype, cuda)
    xd, rd, scd, shd = _dev(cuda, x, r, scale, shift)
    rc = _lib().cobevt_bn_apply(ag._p(xd), ag._p(rd), ag._p(scd), ag._p(shd), ag._p(y.t), ops.dcode(dtype), rows, c, act, ag._stream())
    _ok(rc, "cobevt_bn_apply")
    got = y.check("bn_apply").cpu().double().view(rows, c)
    xs = x.double() * scale.double()
    ref = xs + shift.double() + (r.double() if res else 0.0)
    if act:
        ref = ref.clamp_min(0.0)
    bound = 4.0 * U * (xs.abs() + shift.double().abs() + (r.double().abs() if res else 0.0)) + (UB * ref.abs() if dtype == BF16 else 0.0)
    err = (got - ref).abs()
    print("bn_apply C=%d rows=%d %s act=%d res=%s: max |err| / bound = %.3f" % (c, rows, dtype, act, res, float((err / bound.clamp_min(1e-300)).max())))
    bad = err > bound
    assert not bool(bad.any()), "bn_apply: %d elements off, first at %s" % (int(bad.sum()), bad.nonzero()[0].tolist())
    assert bool((got[:2, :2] == 0.0).all()), "a pre-activation of +0 / -0 must give 0"


def _bwd_inputs(c, rows, dtype, exact, seed):
    g = torch.Generator().manual_seed(seed)
    if exact:                                          # integer x, dy, mean; rstd a power of two: every term is an exact integer multiple
        x = _int_map(rows, c, dtype, seed)
        dy = torch.randint(-8, 9, (rows, c), generator=g).to(dtype)
        mean, rstd = torch.zeros(c), torch.ones(c)
    else:
        x = torch.randn(rows, c, generator=g).to(dtype)
        dy = torch.randn(rows, c, generator=g).to(dtype)
        mean, rstd = torch.randn(c, generator=g) * 0.2, torch.rand(c, generator=g) + 0.5
    y = torch.randn(rows, c, generator=g).to(dtype)     # only its sign pattern matters; exact zeros of both signs included
    _signed_zeros(y, rows, c)
    gamma = torch.rand(c, generator=g) + 0.5
    return x, y, dy, mean, rstd, gamma


def _bn_backward(dev, x, y, dy, mean, rstd, gamma, want_f, want_dres, sb, act, training):
    rows, c = x.shape
    acc = Carved(2 * c, torch.float64, dev)
    gf = Carved(2 * c, F32, dev) if want_f else None
    dx = Carved(rows * c, x.dtype, dev)
    dres = Carved(rows * c, x.dtype, dev) if want_dres else None
    scr = _scratch(sb, rows, c, dev)
    xd, yd, dyd, md, rsd, gd = _dev(dev, x, y, dy, mean, rstd, gamma)
    rc = _lib().cobevt_bn_backward(ag._p(xd), ag._p(yd) if act else None, ag._p(dyd), ag._p(md), ag._p(rsd), ag._p(gd), ag._p(acc.t), ag._p(gf.t) if gf else None, ag._p(scr.t), sb,
                                   ag._p(dx.t), ag._p(dres.t) if dres else None, ops.dcode(x.dtype), rows, c, act, training, ag._stream())
    _ok(rc, "cobevt_bn_backward")
    scr.check("bn_backward scratch", written=None)
    return acc, gf, dx, dres


BWD_VARIANTS = ((True, True, True, 512), (False, False, False, 1), (True, True, False, 1))     # gamma, grads_f, dres, scratch_blocks


def _bwd_reference(x, y, dy, mean, rstd, act):
    g = dy.double() * ((y.double() > 0).double() if act else 1.0)
    xhat = (x.double() - mean.double()) * rstd.double()
    return g, xhat


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,rows", APPLY_SHAPES)
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("training", [0, 1])
def test_bn_backward(cuda, dtype, c, rows, act, training):
    """mean, rstd and y supplied by the test; dx and dres elementwise against float64 of the formula, fed the dgamma / dbeta the call
    returned (fp64, gated on their own below: the apply kernel is handed exactly these):
    |err| <= 4 u |gamma rstd| (|g| + (|dbeta| + |xhat dgamma|) / rows) (+ 2^-8 |ref| in bf16) - the magnitudes of the terms, since the
    expression cancels.  dres = g exactly; grads_f = the fp64 sums rounded to fp32.  Where y is +0 or -0 under the ReLU mask the gradient
    is 0 in dres and, with frozen statistics, in dx.  Variants: gamma null, dres null, grads_f null, scratch_blocks 512 and 1."""
    x, y, dy, mean, rstd, gamma = _bwd_inputs(c, rows, dtype, False, c * 17 + rows)
    g, xhat = _bwd_reference(x, y, dy, mean, rstd, act)
    for variant, (use_gamma, want_f, want_dres, sb) in enumerate(BWD_VARIANTS):
        what = "bn_backward C=%d rows=%d %s act=%d training=%d variant %d" % (c, rows, dtype, act, training, variant)
        acc, gf, dx, dres = _bn_backward(cuda, x, y, dy, mean, rstd, gamma if use_gamma else None, want_f, want_dres, sb, act, training)
        got = acc.check(what).cpu()
        dgamma, dbeta = got[:c], got[c:]
        if gf is not None:
            assert torch.equal(gf.check(what + " grads_f").cpu(), got.float()), what + " grads_f"
        kk = (gamma.double() if use_gamma else 1.0) * rstd.double()
        if training:
            ref = kk * (g - (dbeta + xhat * dgamma) / rows)
            mag = g.abs() + (dbeta.abs() + (xhat * dgamma).abs()) / rows
        else:
            ref, mag = kk * g, g.abs()
        bound = 4.0 * U * kk.abs() * mag + (UB * ref.abs() if dtype == BF16 else 0.0)
        gdx = dx.check(what + " dx").cpu().double().view(rows, c)
        err = (gdx - ref).abs()
        print("%s: dx max |err| / bound = %.3f" % (what, float((err / bound.clamp_min(1e-300)).max())))
        bad = err > bound
        assert not bool(bad.any()), "%s dx: %d elements off, first at %s" % (what, int(bad.sum()), bad.nonzero()[0].tolist())
        if dres is not None:
            assert torch.equal(dres.check(what + " dres").cpu().double().view(rows, c), g + 0.0), what + " dres"
        if act:
            assert bool((g[:2, :2] == 0).all())
            if not training:
                assert bool((gdx[:2, :2] == 0).all()), what + ": y = +-0 must give a zero gradient"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,rows", APPLY_SHAPES)
@pytest.mark.parametrize("act", [0, 1])
def test_bn_backward_reductions_rounding(cuda, dtype, c, rows, act):
    """N(0, 1) x and dy, general mean / rstd: dgamma / dbeta (fp64) against float64, |err| <= k u sum|terms| with
    k = ceil(rows / scratch_blocks), scratch_blocks 512 and 1.  A thread's sums are fp64, rounded once: one rounding per partial."""
    x, y, dy, mean, rstd, gamma = _bwd_inputs(c, rows, dtype, False, c * 17 + rows)
    g, xhat = _bwd_reference(x, y, dy, mean, rstd, act)
    ref = torch.cat([(g * xhat).sum(0), g.sum(0)])
    mag = torch.cat([(g * xhat).abs().sum(0), g.abs().sum(0)])
    missed = []
    for sb in (512, 1):
        what = "bn_backward C=%d rows=%d %s act=%d scratch_blocks=%d" % (c, rows, dtype, act, sb)
        acc, _, _, _ = _bn_backward(cuda, x, y, dy, mean, rstd, gamma, False, False, sb, act, 1)
        k = (rows + sb - 1) // sb
        ratio = float(((acc.check(what).cpu() - ref).abs() / (k * U * mag).clamp_min(1e-300)).max())
        print("%s: dgamma / dbeta max |err| / (k u sum|terms|) = %.3f (k = %d)" % (what, ratio, k))
        if ratio > 1.0:
            missed.append("%s: %.3f" % (what, ratio))
    assert not missed, "max |err| / (k u sum|terms|) > 1: " + "; ".join(missed)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,rows", APPLY_SHAPES + [(24, 4001), (2048, 1000)])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("centred", [True, False])
def test_bn_backward_reductions_exact(cuda, dtype, c, rows, act, centred):
    """integer x and dy with mean 0, rstd 1 (centred) or an integer mean and rstd a power of two: every term g (x - mean) rstd and every
    fp32 partial of dgamma / dbeta is an exact multiple of 1/2 below 2^23, so the fp64 results EQUAL the reference for scratch_blocks 1
    and 512, with and without the ReLU mask"""
    x, y, dy, mean, rstd, _ = _bwd_inputs(c, rows, dtype, True, c + rows)
    if not centred:
        mean = ((torch.arange(c) * 5) % 7 - 3).float()
        rstd = 2.0 ** ((torch.arange(c) % 3) - 1).float()
    g, xhat = _bwd_reference(x, y, dy, mean, rstd, act)          # exact in float64 too
    ref = torch.cat([(g * xhat).sum(0), g.sum(0)])
    for sb in (1, 512):
        acc, gf, _, _ = _bn_backward(cuda, x, y, dy, mean, rstd, None, True, False, sb, act, 1)
        what = "bn_backward exact C=%d rows=%d %s act=%d scratch_blocks=%d" % (c, rows, dtype, act, sb)
        assert torch.equal(acc.check(what).cpu(), ref), what
        assert torch.equal(gf.check(what).cpu(), ref.float()), what + " grads_f"


def test_bn_backward_refuses_misaligned_scratch(cuda):
    """the dx pass reads its coefficients from the scratch 16 bytes at a time: a scratch that is only 8-byte aligned is COBEVT_ERR_ARG,
    and nothing is written"""
    c, rows = 16, 5
    x, y, dy, mean, rstd, gamma = _bwd_inputs(c, rows, F32, False, 1)
    xd, yd, dyd, md, rsd, gd = _dev(cuda, x, y, dy, mean, rstd, gamma)
    acc, dx = Carved(2 * c, torch.float64, cuda), Carved(rows * c, F32, cuda)
    scr = Carved(2 * 2 * c + 1, torch.float64, cuda)
    rc = _lib().cobevt_bn_backward(ag._p(xd), ag._p(yd), ag._p(dyd), ag._p(md), ag._p(rsd), ag._p(gd), ag._p(acc.t), None, ag._p(scr.t[1:]), 2,
                                   ag._p(dx.t), None, 1, rows, c, 1, 1, ag._stream())
    assert rc == ERR_ARG
    for buf in (acc, dx, scr):
        buf.check("refused call", written=False)


# ----------------------------------------------------------------------------------------------
# 5. through autograd: the wrappers pass the right pointers and flags
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,dtype,track,relu,res", [(24, BF16, True, True, True), (96, BF16, True, False, False), (24, F32, False, True, True),
                                                    (96, F32, False, False, False)])
def test_batch_norm_act_vs_float64(cuda, c, dtype, track, relu, res):
    """ag.batch_norm_act against a float64 CPU autograd reference fed the same fp32 / bf16 values: EfficientNet widths in bf16,
    track_running_stats=False in fp32.  fp32: forward 1e-5, gradients 1e-4, running statistics 1e-5 (test_batch_norm_act_vs_torch);
    bf16: 4e-3 for the single output rounding (test_group_mean_vs_torch)"""
    g = torch.Generator().manual_seed(c)
    n, h, w = 3, 7, 9
    x0 = (torch.randn(n, c, h, w, generator=g) * 2.0 + 0.7).to(dtype)
    r0 = torch.randn(n, c, h, w, generator=g).to(dtype) if res else None
    wgt = torch.randn(n, c, h, w, generator=g).to(dtype)             # d loss / dy, exact in the maps' type
    bns = [torch.nn.BatchNorm2d(c, eps=1e-3, momentum=0.07, track_running_stats=track) for _ in range(2)]
    with torch.no_grad():
        bns[0].weight.copy_(torch.rand(c, generator=g) + 0.5)
        bns[0].bias.copy_(torch.randn(c, generator=g) * 0.3)
        if track:
            bns[0].running_mean.copy_(torch.randn(c, generator=g) * 0.2)
            bns[0].running_var.copy_(torch.rand(c, generator=g) + 0.5)
    bns[1].load_state_dict(bns[0].state_dict())
    bn, bn64 = bns[0].to(cuda).train(), bns[1].double().train()
    tol_f, tol_g = (1e-5, 1e-4) if dtype == F32 else (4e-3, 4e-3)
    with torch.enable_grad():
        x = x0.to(cuda).requires_grad_(True)
        r = None if r0 is None else r0.to(cuda).requires_grad_(True)
        y = ag.batch_norm_act(x, bn, residual=r, relu=relu)
        (y.float() * wgt.to(cuda).float()).sum().backward()
        xr = x0.double().requires_grad_(True)
        rr = None if r0 is None else r0.double().requires_grad_(True)
        yr = bn64(xr)
        yr = yr if rr is None else yr + rr
        yr = torch.relu(yr) if relu else yr
        (yr * wgt.double()).sum().backward()
    assert y.dtype == dtype and x.grad.dtype == dtype
    assert_close(y.float(), yr, tol_f, "bn forward")
    assert_close(x.grad.float(), xr.grad, tol_g, "bn dx")
    if res:
        assert_close(r.grad.float(), rr.grad, tol_g, "bn dres")
    assert_close(bn.weight.grad, bn64.weight.grad, tol_g, "bn dgamma")
    assert_close(bn.bias.grad, bn64.bias.grad, tol_g, "bn dbeta")
    if track:
        assert_close(bn.running_mean, bn64.running_mean, 1e-5, "running_mean")
        assert_close(bn.running_var, bn64.running_var, 1e-5, "running_var")
        assert int(bn.num_batches_tracked) == 1
    else:
        assert bn.running_mean is None and bn.running_var is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [2, 3])
def test_column_sum_head_widths(cuda, dtype, c):
    """ag.column_sum at the 2- and 3-class heads' widths (the generic kernel + cobevt_f64_to_f32): fp32 out, 1e-5 of the float64 sums"""
    g = torch.Generator().manual_seed(c)
    x = torch.randn(1531, c, generator=g).to(dtype)
    out = ag.column_sum(x.to(cuda))
    assert out.dtype == F32 and out.shape == (c,)
    assert_close(out, x.double().sum(0), 1e-5, "column_sum")
