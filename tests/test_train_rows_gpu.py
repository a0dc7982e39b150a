"""Kernel-level tests of the LayerNorm, activation and loss kernels of the training glue (-m gpu): csrc/train_rows.hip (LayerNorm both
directions, GELU), csrc/train_nusc.hip (swish, depthwise weight gradient, bilinear resize adjoint, focal-loss gradient) and the loss
forwards of csrc/postprocess.hip.  The C entry points are called directly; every reference is float64 on the CPU and computed from
exactly the fp32 / bf16 values handed to the kernel; outputs and scratch are carved out of NaN-filled allocations whose guard bands
must come back untouched, the scratch at exactly the size the header promises.  Two kinds of case: EXACT ones (every intermediate
representable, so the result must equal the reference in any summation order) and ROUNDING ones, gated by carved.rounding_gate
against torch's own fp32 error on the same inputs.  Gates and measured figures: tests/golden/README_train_rows.md."""
import itertools
import math

import numpy as np
import pytest
import torch

from cobevt_amd import autograd as ag
from cobevt_amd import ops
from carved import BF16, ERR_ARG, ERR_SHAPE, F32, Carved, _dev, _int_map, _lib, _ok, carved_from, rounding_gate
from util import focal_reference

pytestmark = pytest.mark.gpu

Fn = torch.nn.functional
I64 = torch.int64


def _code(dtype):
    return ops.dcode(dtype)


def _f32(v):
    """the float32 value of a Python number, as a float (what the entry point receives)"""
    return float(torch.tensor(v, dtype=F32))


# ----------------------------------------------------------------------------------------------
# 1. LayerNorm: cobevt_layernorm_fwd_t, cobevt_layernorm_bwd, cobevt_layernorm_bwd_t, cobevt_layernorm
# ----------------------------------------------------------------------------------------------
NARROW_POW2, NARROW_ODD = [4, 8, 64, 128], [12, 100, 124]          # C <= 128: a row per half-wave; 1 / C exact at the powers of two
WIDE_POW2, WIDE_ODD = [256, 512, 1024], [132, 260, 1020]           # a row per wave, 1 - 4 float4 groups per lane
LN_COMBOS = list(itertools.product((1, 0), repeat=3))              # [x, dy, dx] storage codes of cobevt_layernorm_bwd_t, 1 = fp32, 0 = bf16
_STORE = {1: F32, 0: BF16}


def _ln_launch(rows, c):
    """the launch arithmetic of cobevt_layernorm_bwd / _bwd_t (csrc/train_rows.hip ln_bwd_rows_per_block) -> (form, rows in flight per
    workgroup and round, rows per workgroup, workgroups)"""
    rpb = ((rows + 1023) // 1024 + 3) // 4 * 4
    if c <= 128:
        if rows >= 16384:
            rpb = ((rows + 255) // 256 + 63) // 64 * 64
            return "narrow16", 64, rpb, (rows + rpb - 1) // rpb
        rpb = (rpb + 15) // 16 * 16
        return "narrow4", 16, rpb, (rows + rpb - 1) // rpb
    return "wide", 4, rpb, (rows + rpb - 1) // rpb


_HW4, _SWITCH = 8, 16384            # half-waves of a four-wave workgroup; the first row count on sixteen waves
# narrow4 (rows < 16384: 16 rows per workgroup = ONE round of 8 half-waves x 2 rows in flight, the second is row + 8):
#   1: one half-wave, okb false | 7: seven half-waves, the eighth idle | 8: all eight, okb false everywhere | 9: okb true for half-wave 0
#   only, so true and false inside wave 0 | 17, 33: a second / third workgroup with one row | 1000: 63 workgroups, the last with 8 rows |
#   4001: 251, the last with 1 row | 16383: 1024 workgroups, the last with 15 rows (okb false for half-wave 7 only)
# narrow16 (32 half-waves): 16384: 64 rows per workgroup, one full round, 256 workgroups | 16385: 128 rows per workgroup = two rounds,
#   129 workgroups, the last with one row | 20001: 157 workgroups, the last with 33 rows (okb true for half-wave 0 only)
NARROW_ROWS = [1, _HW4 - 1, _HW4, _HW4 + 1, 2 * _HW4 + 1, 4 * _HW4 + 1, 1000, 4001, _SWITCH - 1, _SWITCH, _SWITCH + 1, 20001]
# wide (4 waves, 4 rows per workgroup up to 4096 rows): 1, 3: waves without a row | 4: full | 5: a second workgroup with one row | 1000: 250 full
#   workgroups | 4001: 1001, the last with one row | 4101: 8 rows per workgroup = two rounds, the last workgroup with 5 rows (added to the issue's list)
WIDE_ROWS = [1, 3, 4, 5, 1000, 4001, 4101]


def test_layernorm_row_lists_reach_every_launch_form():
    """the row lists above against the entry points' arithmetic: every form, one and two rounds, full and partial last workgroups; and
    cobevt_layernorm_bwd_scratch = one {dgamma, dbeta} record per workgroup"""
    seen = {}
    for c, rows_list in ((128, NARROW_ROWS), (256, WIDE_ROWS)):
        for rows in rows_list:
            form, flight, rpb, blocks = _ln_launch(rows, c)
            seen.setdefault(form, []).append((rows, rpb // flight, blocks, rows - (blocks - 1) * rpb))      # rows, rounds, workgroups, rows of the last
            assert _lib().cobevt_layernorm_bwd_scratch(rows, c) == blocks * 2 * c
    assert [s[0] for s in seen["narrow4"]] == NARROW_ROWS[:9] and [s[0] for s in seen["narrow16"]] == NARROW_ROWS[9:]
    assert [s[1:] for s in seen["narrow4"]] == [(1, 1, 1), (1, 1, 7), (1, 1, 8), (1, 1, 9), (1, 2, 1), (1, 3, 1), (1, 63, 8), (1, 251, 1), (1, 1024, 15)]
    assert [s[1:] for s in seen["narrow16"]] == [(1, 256, 64), (2, 129, 1), (2, 157, 33)]
    assert [s[1:] for s in seen["wide"]] == [(1, 1, 1), (1, 1, 3), (1, 1, 4), (1, 2, 1), (1, 250, 4), (1, 1001, 1), (2, 513, 5)]
    assert [_lib().cobevt_layernorm_bwd_scratch(r, c) for r, c in ((0, 64), (5, 2), (5, 6), (5, 1028))] == [0, 0, 0, 0]


def _ln_rows(c, limit=None):
    rows = NARROW_ROWS if c <= 128 else WIDE_ROWS
    return [r for r in rows if limit is None or r <= limit]


def _ln_exact_inputs(rows, c, seed):
    """x = m_r + s_r (+-1), C / 2 entries of each sign in a per-row permutation, m_r an integer in [-8, 8], s_r in {1, 2, 4}; dy integers
    in [-8, 8] with a distinct offset per channel; gamma integers in [-3, 3], beta integers in [-5, 5]"""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(-8, 9, (rows, 1), generator=g).float()
    s = 2.0 ** torch.randint(0, 3, (rows, 1), generator=g).float()
    sign = torch.cat([torch.ones(c // 2), -torch.ones(c // 2)]).expand(rows, c)
    sign = torch.gather(sign, 1, torch.rand(rows, c, generator=g).argsort(1))
    x = m + s * sign
    dy = _int_map(rows, c, F32, seed + 1)
    gamma = ((torch.arange(c) * 5) % 7 - 3).float()
    beta = ((torch.arange(c) * 3) % 11 - 5).float()
    # the construction is exact in the kernels' own fp32 order of operations: sum, / C, subtract, square, sum, * (1 / C), 1 / sqrt
    mean = x.sum(1, keepdim=True) / torch.tensor(float(c))
    a = x - mean
    rstd = 1.0 / torch.sqrt((a * a).sum(1, keepdim=True) * (torch.tensor(1.0) / float(c)))
    assert mean.dtype == F32 and torch.equal(mean, m) and torch.equal(rstd, 1.0 / s) and torch.equal(a * rstd, sign)
    return x, dy, gamma, beta


def _ln_ref(x, dy, gamma, beta, eps):
    """float64 LayerNorm: y, dx, dgamma, dbeta (gamma / beta None: 1 / 0)"""
    x, dy = x.double(), dy.double()
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + eps)
    xh = (x - mean) * rstd
    g = dy if gamma is None else dy * gamma.double()
    y = xh if gamma is None else xh * gamma.double() + beta.double()
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return y, dx, (dy * xh).sum(0), dy.sum(0)


def _ln_bwd(dev, xd, dyd, gd, rows, c, eps, combo, prefill, what):
    """combo None: cobevt_layernorm_bwd (fp32), else the storage codes [x, dy, dx] of cobevt_layernorm_bwd_t; xd / dyd: device tensors in
    that storage; prefill: (dgamma, dbeta) start values, or None = both pointers null.  -> (dx (rows, C) on the CPU in its storage type,
    dgamma, dbeta) after the guard-band checks; a dgamma / dbeta that is not passed must still hold the sentinel, and so must the scratch"""
    out_dtype = F32 if combo is None else _STORE[combo[2]]
    dx = Carved(rows * c, out_dtype, dev)
    dg = Carved(c, F32, dev) if prefill is None else carved_from(prefill[0], dev)
    db = Carved(c, F32, dev) if prefill is None else carved_from(prefill[1], dev)
    pg, pb = (None, None) if prefill is None else (ag._p(dg.t), ag._p(db.t))
    scr = Carved(_lib().cobevt_layernorm_bwd_scratch(rows, c), F32, dev)          # exactly the promised size; handed over even where it must stay untouched
    if combo is None:
        rc = _lib().cobevt_layernorm_bwd(ag._p(xd), ag._p(dyd), ag._p(gd), ag._p(dx.t), pg, pb, rows, c, eps, ag._p(scr.t), ag._stream())
    else:
        rc = _lib().cobevt_layernorm_bwd_t(ag._p(xd), ag._p(dyd), ag._p(gd), ag._p(dx.t), pg, pb, rows, c, eps, ag._ints(combo), ag._p(scr.t), ag._stream())
    _ok(rc, what)
    scr.check(what + " scratch", written=prefill is not None)                       # every record written, or none
    got = dx.check(what + " dx").cpu().view(rows, c)
    return got, dg.check(what + " dgamma", written=prefill is not None).cpu(), db.check(what + " dbeta", written=prefill is not None).cpu()


def _stored(ref, dtype):
    """the float64 reference rounded ONCE to the storage type, to nearest even (float64 -> bf16 goes through fp32; every exact case is
    exactly representable in fp32)"""
    return ref.float() if dtype == F32 else ref.float().to(BF16)


@pytest.mark.parametrize("c", NARROW_POW2 + WIDE_POW2)
def test_layernorm_backward_exact(cuda, c):
    """power-of-two C, eps = 0, the construction of _ln_exact_inputs: mean, rstd and xhat = +-1 are exact, so dx, dgamma and dbeta are
    dyadic rationals below 24 bits and must EQUAL float64 (dx rounded once where it is stored as bf16) - cobevt_layernorm_bwd and all eight
    storage combinations of cobevt_layernorm_bwd_t at every row count; up to 1000 rows also with dgamma / dbeta pre-filled with integers
    (the header says ADDS), with gamma null, and with dgamma / dbeta null (dx unchanged, the carved dgamma still the sentinel)"""
    zero = (torch.zeros(c), torch.zeros(c))
    pre = (((torch.arange(c) * 3) % 13 - 6).float(), ((torch.arange(c) * 5) % 11 - 5).float())
    for rows in _ln_rows(c):
        x, dy, gamma, beta = _ln_exact_inputs(rows, c, 31 * rows + c)
        _, dx_ref, dg_ref, db_ref = _ln_ref(x, dy, gamma, beta, 0.0)
        _, dx_nog, _, _ = _ln_ref(x, dy, None, None, 0.0)
        xs, dys = {1: x.to(cuda), 0: x.to(BF16).to(cuda)}, {1: dy.to(cuda), 0: dy.to(BF16).to(cuda)}
        assert torch.equal(xs[0].float().cpu(), x) and torch.equal(dys[0].float().cpu(), dy)       # the bf16 copies hold the same values
        gd = gamma.to(cuda)
        for combo in [None] + LN_COMBOS:
            cx, cdy, cdx = (1, 1, 1) if combo is None else combo
            what = "layernorm_bwd exact C=%d rows=%d %s" % (c, rows, "fp32 entry" if combo is None else "dtypes %s" % (combo,))
            dx, dg, db = _ln_bwd(cuda, xs[cx], dys[cdy], gd, rows, c, 0.0, combo, zero, what)
            assert torch.equal(dx, _stored(dx_ref, _STORE[cdx])), what + " dx"
            assert torch.equal(dg.double(), dg_ref) and torch.equal(db.double(), db_ref), what + " dgamma / dbeta"
            if rows > 1000:
                continue
            _, dg2, db2 = _ln_bwd(cuda, xs[cx], dys[cdy], gd, rows, c, 0.0, combo, pre, what + " pre-filled")
            assert torch.equal(dg2.double(), pre[0].double() + dg_ref) and torch.equal(db2.double(), pre[1].double() + db_ref), what + " ADDS"
            dx3, dg3, _ = _ln_bwd(cuda, xs[cx], dys[cdy], None, rows, c, 0.0, combo, zero, what + " gamma null")
            assert torch.equal(dx3, _stored(dx_nog, _STORE[cdx])) and torch.equal(dg3.double(), dg_ref), what + " gamma null"
            dx4, _, _ = _ln_bwd(cuda, xs[cx], dys[cdy], gd, rows, c, 0.0, combo, None, what + " dgamma / dbeta null")
            assert torch.equal(dx4.view(torch.int32 if cdx else torch.int16), dx.view(torch.int32 if cdx else torch.int16)), what + ": dx changed"


def _ln_fwd(dev, xd, gd, bd, rows, c, eps, combo, what):
    """combo [x, y] storage codes: cobevt_layernorm_fwd_t; combo "ln" + the tensor's type: cobevt_layernorm (same storage in and out)"""
    if combo[0] == "ln":
        y = Carved(rows * c, xd.dtype, dev)
        rc = _lib().cobevt_layernorm(ag._p(xd), ag._p(gd), ag._p(bd), ag._p(y.t), _code(xd.dtype), rows, c, eps, 1, 0, 0, 0, ag._stream())
    else:
        y = Carved(rows * c, _STORE[combo[1]], dev)
        rc = _lib().cobevt_layernorm_fwd_t(ag._p(xd), ag._p(gd), ag._p(bd), ag._p(y.t), rows, c, eps, ag._ints(combo), ag._stream())
    _ok(rc, what)
    return y.check(what).cpu().view(rows, c)


def _ln_plain_ok(c):
    """the widths cobevt_layernorm takes: C / 8 a power of two up to 64"""
    g = c // 8
    return c % 8 == 0 and 1 <= g <= 64 and g & (g - 1) == 0


@pytest.mark.parametrize("c", NARROW_POW2 + WIDE_POW2)
def test_layernorm_forward_exact(cuda, c):
    """the same construction through the four storage combinations of cobevt_layernorm_fwd_t and through cobevt_layernorm (fp32 and
    bf16, the widths it takes): y = (+-1) gamma + beta exactly, rounded once where it is stored as bf16; gamma / beta null: y = +-1"""
    for rows in _ln_rows(c, 4101):
        x, _, gamma, beta = _ln_exact_inputs(rows, c, 31 * rows + c)
        y_ref, _, _, _ = _ln_ref(x, x, gamma, beta, 0.0)
        y_nog, _, _, _ = _ln_ref(x, x, None, None, 0.0)
        xs = {1: x.to(cuda), 0: x.to(BF16).to(cuda)}
        gd, bd = _dev(cuda, gamma, beta)
        combos = list(itertools.product((1, 0), repeat=2)) + ([("ln", 1), ("ln", 0)] if _ln_plain_ok(c) else [])
        for combo in combos:
            cx = combo[1] if combo[0] == "ln" else combo[0]
            what = "layernorm forward exact C=%d rows=%d %s" % (c, rows, combo)
            assert torch.equal(_ln_fwd(cuda, xs[cx], gd, bd, rows, c, 0.0, combo, what), _stored(y_ref, _STORE[combo[1]])), what
            assert torch.equal(_ln_fwd(cuda, xs[cx], None, None, rows, c, 0.0, combo, what), _stored(y_nog, _STORE[combo[1]])), what + " no affine"


LN_LOG = []
_CONST = 3.25                       # the constant row: C * 3.25 and every partial sum of it are exact in fp32 up to C = 1024


@pytest.mark.parametrize("kind", ["n01", "n100", "const"])
@pytest.mark.parametrize("c", NARROW_POW2 + NARROW_ODD + WIDE_POW2 + WIDE_ODD)
def test_layernorm_rounding(cuda, c, kind):
    """random rows at every width, eps = 1e-5: N(0, 1); mean-dominated N(100, 1); N(0, 1) with one exactly constant row.  y and dx per
    element, dgamma and dbeta per channel against float64 under carved.rounding_gate, the torch side F.layer_norm and its autograd in
    fp32 on the device; fp32 storage (cobevt_layernorm_bwd, fwd_t [1, 1], cobevt_layernorm) and bf16 storage ([0, 0, 0], [0, 0]).
    On the constant row y must EQUAL beta (mean exact, xhat = 0) and dx must be finite."""
    eps = 1e-5                      # rows: one workgroup | 63 / 250 records | both sides of the sixteen-wave switch (1024 / 256 records) | 157 | 513
    for rows in ([9, 1000, 16383, 16384, 20001] if c <= 128 else [5, 1000, 4101]):
        g = torch.Generator().manual_seed(rows + 7 * c)
        x = torch.randn(rows, c, generator=g) + (100.0 if kind == "n100" else 0.0)
        r_const = min(rows - 1, 5)
        if kind == "const":
            x[r_const] = _CONST
        dy = torch.randn(rows, c, generator=g)
        gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
        gd, bd = _dev(cuda, gamma, beta)
        for dtype in (F32, BF16):
            xq, dyq = x.to(dtype), dy.to(dtype)
            y_ref, dx_ref, dg_ref, db_ref = _ln_ref(xq, dyq, gamma, beta, _f32(eps))
            with torch.enable_grad():
                xt = xq.float().to(cuda).requires_grad_(True)
                gt, bt = gd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
                yt = Fn.layer_norm(xt, (c,), gt, bt, eps)
                yt.backward(dyq.float().to(cuda))
            bf = dtype == BF16
            tag = "layernorm %s C=%d rows=%d %s" % (kind, c, rows, "bf16" if bf else "fp32")
            xd, dyd = xq.to(cuda), dyq.to(cuda)
            zero = (torch.zeros(c), torch.zeros(c))
            dx, dg, db = _ln_bwd(cuda, xd, dyd, gd, rows, c, eps, (0, 0, 0) if bf else None, zero, tag)
            rounding_gate(tag + " dx", dx, dx_ref, xt.grad, bf, LN_LOG)
            rounding_gate(tag + " dgamma", dg, dg_ref, gt.grad, False, LN_LOG)
            rounding_gate(tag + " dbeta", db, db_ref, bt.grad, False, LN_LOG)
            for combo in [(0, 0) if bf else (1, 1)] + ([("ln", 0 if bf else 1)] if _ln_plain_ok(c) else []):
                y = _ln_fwd(cuda, xd, gd, bd, rows, c, eps, combo, tag + " y %s" % (combo,))
                rounding_gate(tag + " y %s" % (combo,), y, y_ref, yt.detach(), bf, LN_LOG)
                if kind == "const":
                    assert torch.equal(y[r_const], _stored(beta.double(), dtype)), tag + " %s: y of a constant row must equal beta" % (combo,)


def test_layernorm_error_codes(cuda):
    """C = 2 (< 4), C = 6 (not a multiple of 4), C = 1028 (> 1024), rows = 0: COBEVT_ERR_SHAPE; exactly one of dgamma / dbeta null, dgamma
    and dbeta without a scratch, a dtype code of 2: COBEVT_ERR_ARG - from all three entry points that take them, before any launch:
    nothing is written"""
    cases = [(2, 5, "both", (1, 1, 1), ERR_SHAPE), (6, 5, "both", (1, 1, 1), ERR_SHAPE), (1028, 5, "both", (1, 1, 1), ERR_SHAPE),
             (64, 0, "both", (1, 1, 1), ERR_SHAPE), (64, 5, "dgamma", (1, 1, 1), ERR_ARG), (64, 5, "dbeta", (1, 1, 1), ERR_ARG),
             (64, 5, "no scratch", (1, 1, 1), ERR_ARG), (64, 5, "both", (1, 2, 1), ERR_ARG), (64, 5, "both", (1, 1, 2), ERR_ARG)]
    for c, rows, grads, combo, want in cases:
        n = max(rows, 1) * c
        x, dy, gamma, beta = torch.ones(n, device=cuda), torch.ones(n, device=cuda), torch.ones(c, device=cuda), torch.ones(c, device=cuda)
        bufs = {k: Carved(n if k in ("dx", "y") else (2 * c if k == "scratch" else c), F32, cuda) for k in ("dx", "y", "dgamma", "dbeta", "scratch")}
        pg = ag._p(bufs["dgamma"].t) if grads in ("both", "dgamma", "no scratch") else None
        pb = ag._p(bufs["dbeta"].t) if grads in ("both", "dbeta", "no scratch") else None
        ps = None if grads == "no scratch" else ag._p(bufs["scratch"].t)
        rcs = [_lib().cobevt_layernorm_bwd_t(ag._p(x), ag._p(dy), ag._p(gamma), ag._p(bufs["dx"].t), pg, pb, rows, c, 1e-5, ag._ints(combo), ps, ag._stream())]
        if combo == (1, 1, 1):
            rcs.append(_lib().cobevt_layernorm_bwd(ag._p(x), ag._p(dy), ag._p(gamma), ag._p(bufs["dx"].t), pg, pb, rows, c, 1e-5, ps, ag._stream()))
        if grads == "both" and (combo == (1, 1, 1) or 2 in combo[:2]):
            rcs.append(_lib().cobevt_layernorm_fwd_t(ag._p(x), ag._p(gamma), ag._p(beta), ag._p(bufs["y"].t), rows, c, 1e-5, ag._ints(combo[:2]), ag._stream()))
        assert rcs == [want] * len(rcs), (c, rows, grads, combo, rcs)
        for k, b in bufs.items():
            b.check("refused layernorm call: " + k, written=False)


# ----------------------------------------------------------------------------------------------
# 2. cobevt_gelu, cobevt_gelu_bf16, cobevt_swish
# ----------------------------------------------------------------------------------------------
# n: one float4 / one 8-group; the last thread of a workgroup short of / at / one past 256 threads; many workgroups with a partial last one
ACT_N = {4: [4, 8, 1020, 1024, 1028, 262148], 8: [8, 16, 2040, 2048, 2056, 262152]}
ACT_CASES = [("gelu", F32), ("gelu", BF16), ("swish", F32), ("swish", BF16)]
ACT_LOG = []
_EDGES = [0.0, -0.0, 0.5, -0.5, 30.0, -30.0, 88.0, -88.0, 100.0, -100.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0]       # all exact in bf16


def _act_width(kind, dtype):
    return 4 if (kind, dtype) == ("gelu", F32) else 8


def _act_call(kind, dtype, xd, dyd, out, n):
    if kind == "swish":
        return _lib().cobevt_swish(ag._p(xd), ag._p(dyd), ag._p(out.t), _code(dtype), n, ag._stream())
    fn = _lib().cobevt_gelu if dtype == F32 else _lib().cobevt_gelu_bf16
    return fn(ag._p(xd), ag._p(dyd), ag._p(out.t), n, ag._stream())


def _act_ref(kind, x, dy):
    """float64: (f(x), dy f'(x))"""
    x, dy = x.double(), dy.double()
    if kind == "gelu":
        cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
        return x * cdf, dy * (cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))
    s = torch.sigmoid(x)
    return x * s, dy * (s + x * s * (1.0 - s))


def _act_torch(kind, xd, dyd):
    """torch's op and its autograd in the storage type, on the device"""
    with torch.enable_grad():
        xt = xd.clone().requires_grad_(True)
        y = Fn.gelu(xt) if kind == "gelu" else xt * torch.sigmoid(xt)
        y.backward(dyd)
    return y.detach(), xt.grad


def _act_run(dev, kind, dtype, x, dy, what):
    """both directions on (x, dy) in `dtype` -> (forward, backward) on the CPU, gated against float64 and torch"""
    n = x.numel()
    xd, dyd = _dev(dev, x, dy)
    f_ref, b_ref = _act_ref(kind, x, dy)
    f_t, b_t = _act_torch(kind, xd, dyd)
    outs = []
    for name, dptr, ref, tor in (("forward", None, f_ref, f_t), ("backward", dyd, b_ref, b_t)):
        out = Carved(n, dtype, dev)
        _ok(_act_call(kind, dtype, xd, dptr, out, n), what)
        got = out.check("%s %s" % (what, name)).cpu()
        rounding_gate("%s %s" % (what, name), got, ref, tor, dtype == BF16, ACT_LOG)
        outs.append(got)
    return outs


@pytest.mark.parametrize("kind,dtype", ACT_CASES, ids=["%s-%s" % (k, "bf16" if d == BF16 else "fp32") for k, d in ACT_CASES])
def test_activation_sweep(cuda, kind, dtype):
    """a dense sweep of x over [-12, 12] with random dy, both directions, elementwise under the rounding gate against F.gelu /
    x sigmoid(x) and their autograd in the same storage type"""
    for n in ACT_N[_act_width(kind, dtype)]:
        g = torch.Generator().manual_seed(n)
        x = torch.linspace(-12.0, 12.0, n).to(dtype)
        dy = torch.randn(n, generator=g).to(dtype)
        _act_run(cuda, kind, dtype, x, dy, "%s %s n=%d" % (kind, "bf16" if dtype == BF16 else "fp32", n))


@pytest.mark.parametrize("kind,dtype", ACT_CASES, ids=["%s-%s" % (k, "bf16" if d == BF16 else "fp32") for k, d in ACT_CASES])
def test_activation_edges(cuda, kind, dtype):
    """+-0, +-0.5, +-30, +-88, +-100 with dy = 1: f(+-0) is a zero; nothing is NaN or infinite (Carved.check), x = -88 and -100 give a
    zero (not 0 x inf) and x = 30, 88, 100 give x and a derivative of 1; swish'(0) = 0.5 exactly; and the gate as in the sweep"""
    x = torch.tensor(_EDGES).to(dtype)
    fwd, bwd = _act_run(cuda, kind, dtype, x, torch.ones_like(x), "%s %s edges" % (kind, "bf16" if dtype == BF16 else "fp32"))
    assert bool((fwd[:2] == 0).all()), "f(+-0) must be a zero"
    assert bool((fwd[[7, 9]].float().abs() <= 1e-30).all()) and bool((bwd[[7, 9]].float().abs() <= 1e-30).all()), "x = -88, -100"
    assert torch.equal(fwd[[4, 6, 8]].float(), torch.tensor([30.0, 88.0, 100.0])) and torch.equal(bwd[[4, 6, 8]].float(), torch.ones(3)), "x = 30, 88, 100"
    if kind == "swish":
        assert bool((bwd[:2].float() == 0.5).all()), "swish'(+-0) must be 0.5 exactly"


def test_activation_error_codes(cuda):
    """n not a multiple of 4 (cobevt_gelu) / 8 (cobevt_gelu_bf16, cobevt_swish), or below it: COBEVT_ERR_SHAPE, nothing written"""
    for kind, dtype in ACT_CASES:
        w = _act_width(kind, dtype)
        for n in (w + w // 2, w - 1, 1022 if w == 4 else 1028):
            x = torch.ones(1032, device=cuda, dtype=dtype)
            out = Carved(1032, dtype, cuda)
            for dyd in (None, x):
                assert _act_call(kind, dtype, x, dyd, out, n) == ERR_SHAPE, (kind, dtype, n)
            out.check("refused activation call", written=False)


# ----------------------------------------------------------------------------------------------
# 3. cobevt_depthwise_wgrad
# ----------------------------------------------------------------------------------------------
# C -> G = C / 8 thread groups: 1 (256 pixel walkers) | 3, 5 (do not divide 256) | 18 (an EfficientNet width) | 144 (one walker, idle threads) | 256
DW_C = [8, 24, 40, 144, 1152, 2048]
# (stride, (pad_top, pad_left), N, Ho, Wo): one pixel | three images of one pixel | 7 x 9 | 5 x 5 x 41 = 1025 pixels: two workgroups of 513 / 512
DW_GEOM = [(1, (0, 0), 1, 1, 1), (2, (2, 2), 3, 1, 1), (1, (1, 1), 2, 7, 9), (2, (0, 1), 2, 7, 9), (1, (2, 2), 2, 7, 9), (2, (0, 0), 2, 7, 9),
           (1, (0, 1), 5, 5, 41), (2, (1, 1), 5, 5, 41)]
_DW_FAR = {(0, 0): (0, 0), (1, 1): (1, 1), (0, 1): (1, 0), (2, 2): (2, 2)}          # nominal bottom / right pad: (0, 1) pads bottom and left only
DW_LOG = []


def _dw_input_size(k, stride, pad, ho, wo):
    """H, W of the input: the padded map is exactly (Ho - 1) stride + k rows; where that leaves no row the map has one and the bottom
    / right pad shrinks (taps outside the map read zero - the implicit TensorFlow-"same" row and column)"""
    (pt, pl), (pb, pr) = pad, _DW_FAR[pad]
    span_h, span_w = (ho - 1) * stride + k, (wo - 1) * stride + k
    h, w = max(1, span_h - pt - pb), max(1, span_w - pl - pr)
    assert pt + h <= span_h and pl + w <= span_w
    return h, w, span_h, span_w


def _dw_ref(x, dy, k, stride, pad, span_h, span_w):
    """dw[a k + b][c] = sum over (n, oy, ox) of dy[n][oy][ox][c] x[n][oy s - pt + a][ox s - pl + b][c] in the type of x (float64 | int64)"""
    n, h, w, c = x.shape
    ho, wo = dy.shape[1], dy.shape[2]
    xp = torch.zeros(n, span_h, span_w, c, dtype=x.dtype)
    xp[:, pad[0]:pad[0] + h, pad[1]:pad[1] + w] = x
    out = torch.zeros(k * k, c, dtype=x.dtype)
    for a in range(k):
        for b in range(k):
            out[a * k + b] = (dy * xp[:, a:a + (ho - 1) * stride + 1:stride, b:b + (wo - 1) * stride + 1:stride]).sum((0, 1, 2))
    return out


def _dw_torch(xd, dyd, k, stride, pad, span_h, span_w):
    """torch's fp32 weight gradient of the same depthwise convolution on the device, as [k k][C]"""
    n, h, w, c = xd.shape
    xn = Fn.pad(xd.float().permute(0, 3, 1, 2), (pad[1], span_w - w - pad[1], pad[0], span_h - h - pad[0]))
    with torch.enable_grad():
        wt = torch.zeros(c, 1, k, k, device=xd.device, requires_grad=True)
        y = Fn.conv2d(xn, wt, None, stride=stride, groups=c)
        y.backward(dyd.float().permute(0, 3, 1, 2))
    return wt.grad[:, 0].permute(1, 2, 0).reshape(k * k, c)


def _dw_call(dev, xd, dyd, dw0, k, stride, pad, what):
    n, h, w, c = xd.shape
    dw = carved_from(dw0, dev)
    dims = ag._ints([_code(xd.dtype), n, h, w, c, k, stride, pad[0], pad[1], dyd.shape[1], dyd.shape[2]])
    _ok(_lib().cobevt_depthwise_wgrad(ag._p(xd), ag._p(dyd), ag._p(dw.t), dims, ag._stream()), what)
    return dw.check(what).cpu().view(k * k, c)


def _dw_case(dev, c, dtype, k, stride, pad, n, ho, wo, seed):
    """exact: integers in [-4, 4], dw pre-filled with integers: == pre-fill + the int64 gradient (every partial an integer below 2^24);
    rounding: N(0, 1), dw zero-filled, per entry against torch's fp32 conv weight gradient"""
    h, w, span_h, span_w = _dw_input_size(k, stride, pad, ho, wo)
    what = "depthwise_wgrad C=%d %s k=%d stride=%d pad=%s N=%d %dx%d -> %dx%d" % (c, "bf16" if dtype == BF16 else "fp32", k, stride, pad, n, h, w, ho, wo)
    g = torch.Generator().manual_seed(seed)
    xi, dyi = torch.randint(-4, 5, (n, h, w, c), generator=g), torch.randint(-4, 5, (n, ho, wo, c), generator=g)
    pre = ((torch.arange(k * k * c) * 7) % 19 - 9).float()
    xd, dyd = _dev(dev, xi.to(dtype), dyi.to(dtype))
    got = _dw_call(dev, xd, dyd, pre, k, stride, pad, what + " exact")
    assert torch.equal(got.to(I64), pre.view(k * k, c).to(I64) + _dw_ref(xi, dyi, k, stride, pad, span_h, span_w)), what + " exact"
    x, dy = torch.randn(n, h, w, c, generator=g).to(dtype), torch.randn(n, ho, wo, c, generator=g).to(dtype)
    xd, dyd = _dev(dev, x, dy)
    got = _dw_call(dev, xd, dyd, torch.zeros(k * k * c), k, stride, pad, what)
    rounding_gate(what, got, _dw_ref(x.double(), dy.double(), k, stride, pad, span_h, span_w), _dw_torch(xd, dyd, k, stride, pad, span_h, span_w),
                  False, DW_LOG)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", DW_C)
def test_depthwise_wgrad(cuda, c, dtype):
    """k = 3 and 5, strides 1 and 2, pads (0, 0), (1, 1), (0, 1), (2, 2), 1 / 3 / 126 / 1025 output pixels (DW_GEOM)"""
    for k in (3, 5):
        for i, (stride, pad, n, ho, wo) in enumerate(DW_GEOM):
            _dw_case(cuda, c, dtype, k, stride, pad, n, ho, wo, 1000 * c + 10 * i + k)


def test_depthwise_wgrad_capped_workgroups(cuda):
    """C = 8, 513 x 512 = 262,656 output pixels: the cap of 256 workgroups gives each 1026 pixels (per_block > 1024)"""
    _dw_case(cuda, 8, F32, 3, 1, (1, 1), 1, 513, 512, 5)


def test_depthwise_wgrad_error_codes(cuda):
    """C = 12 (not a multiple of 8), C = 2056 (G > 256): COBEVT_ERR_SHAPE; k = 4: COBEVT_ERR_UNSUPPORTED (4); a dtype code of 2:
    COBEVT_ERR_ARG; nothing written"""
    for c, k, code, want in ((12, 3, 1, ERR_SHAPE), (2056, 3, 1, ERR_SHAPE), (16, 4, 1, 4), (16, 3, 2, ERR_ARG)):
        x = torch.ones(1, 5, 5, c, device=cuda)
        dw = Carved(25 * c, F32, cuda)
        rc = _lib().cobevt_depthwise_wgrad(ag._p(x), ag._p(x), ag._p(dw.t), ag._ints([code, 1, 5, 5, c, k, 1, 1, 1, 5, 5]), ag._stream())
        assert rc == want, (c, k, code, rc)
        dw.check("refused depthwise_wgrad call", written=False)


# ----------------------------------------------------------------------------------------------
# 4. cobevt_resize_bilinear_bwd (and the forward cobevt_resize_nhwc mode 1 it is the adjoint of)
# ----------------------------------------------------------------------------------------------
# ((H, W), (Ho, Wo), widths): weights exactly 0, 1/2, 1 | the decoder's 2x | a downsample | Ho = Wo = 1 | H = W = 1 | W = 1 |
# inexact scales on one, three (not a power of two) and 64 channel groups
RESIZE_SHAPES = [((5, 7), (9, 13), [8]), ((5, 7), (10, 14), [8, 16]), ((10, 14), (5, 7), [8]), ((4, 4), (1, 1), [8]), ((1, 1), (3, 5), [8]),
                 ((3, 1), (3, 4), [8]), ((25, 25), (50, 50), [8, 24, 512])]
RESIZE_LOG = []


def _axis_matrix(n_in, n_out):
    """(n_out, n_in) float64 matrix of the forward's documented rule src = dst (n_in - 1) / (n_out - 1), floor, clamp, with the source
    coordinate evaluated in float32 exactly as the kernels do - the index from the rounded product, the fraction from the fused
    multiply-subtract (a disagreement is then a wrong index, not another rounding)"""
    s = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    m = np.zeros((n_out, n_in))
    for o in range(n_out):
        i0 = int(np.float32(o) * s)                                 # the index: floor of the product rounded to fp32
        lam = np.float32(float(o) * float(s) - i0)                  # the fraction: fma(dst, scale, -floor), the product unrounded
        m[o, i0] += float(np.float32(1) - lam)
        m[o, min(i0 + 1, n_in - 1)] += float(lam)
    assert m.dtype == np.float64 and np.allclose(m.sum(1), 1.0, rtol=0, atol=1e-6)
    return torch.from_numpy(m)


def _resize_torch(xd, dyd, ho, wo):
    """F.interpolate(align_corners=True) and its autograd in fp32 on the device, channels-last in and out"""
    with torch.enable_grad():
        xt = xd.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        y = Fn.interpolate(xt, size=(ho, wo), mode="bilinear", align_corners=True)
        y.backward(dyd.float().permute(0, 3, 1, 2).contiguous())
    return y.detach().permute(0, 2, 3, 1), xt.grad.permute(0, 2, 3, 1)


def _resize_bwd(dev, dyd, n, h, w, c, ho, wo, what):
    dx = carved_from(torch.zeros(n * h * w * c), dev)
    _ok(_lib().cobevt_resize_bilinear_bwd(ag._p(dyd), ag._p(dx.t), _code(dyd.dtype), n, h, w, c, ho, wo, ag._stream()), what)
    return dx.check(what).cpu().view(n, h, w, c)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", RESIZE_SHAPES, ids=["%dx%d-%dx%d" % (s[0] + s[1]) for s in RESIZE_SHAPES])
def test_resize_bilinear_bwd(cuda, shape, dtype):
    """dx (fp32, guard-banded, zero-initialised) against the float64 adjoint of the forward's rule, per element under the rounding gate
    (torch side: F.interpolate's autograd); (5, 7) -> (9, 13) with integer dy: every weight is 0, 1/2 or 1, dx must EQUAL; and the
    adjoint identity <resize(x), dy> == <x, resize_bwd(dy)> in float64 with the forward kernel, on positive data (a well-conditioned
    inner product), within max(4 x torch's own mismatch, 8 u |ref|) (+ 2^-8 |ref| for the forward's bf16 output)"""
    (h, w), (ho, wo), widths = shape
    n = 2
    ry, rx = _axis_matrix(h, ho), _axis_matrix(w, wo)
    for c in widths:
        what = "resize_bilinear_bwd %s (%d, %d) -> (%d, %d) C=%d" % ("bf16" if dtype == BF16 else "fp32", h, w, ho, wo, c)
        g = torch.Generator().manual_seed(c + ho)
        if (ho, wo) == (9, 13):
            dyi = torch.randint(-8, 9, (n, ho, wo, c), generator=g).to(dtype)
            got = _resize_bwd(cuda, dyi.to(cuda), n, h, w, c, ho, wo, what + " exact")
            assert torch.equal(got.double(), torch.einsum("oh,nopc,pw->nhwc", ry, dyi.double(), rx)), what + " exact"
        dy = torch.randn(n, ho, wo, c, generator=g).to(dtype)
        x = torch.randn(n, h, w, c, generator=g).to(dtype)
        xd, dyd = _dev(cuda, x, dy)
        _, dx_t = _resize_torch(xd, dyd, ho, wo)
        got = _resize_bwd(cuda, dyd, n, h, w, c, ho, wo, what)
        rounding_gate(what, got, torch.einsum("oh,nopc,pw->nhwc", ry, dy.double(), rx), dx_t, False, RESIZE_LOG)
        if c // 8 & (c // 8 - 1):
            continue                                   # the forward takes power-of-two channel groups only
        xp, dyp = (torch.rand(n, h, w, c, generator=g) + 0.5).to(dtype), (torch.rand(n, ho, wo, c, generator=g) + 0.5).to(dtype)
        xd, dyd = _dev(cuda, xp, dyp)
        y = Carved(n * ho * wo * c, dtype, cuda)
        _ok(_lib().cobevt_resize_nhwc(ag._p(xd), ag._p(y.t), _code(dtype), n, h, w, c, ho, wo, 1, ag._stream()), what + " forward")
        yk = y.check(what + " forward").cpu().view(n, ho, wo, c).double()
        dxk = _resize_bwd(cuda, dyd, n, h, w, c, ho, wo, what + " identity").double()
        y_t, dx_t = _resize_torch(xd, dyd, ho, wo)
        y_ref = torch.einsum("oh,nhwc,pw->nopc", ry, xp.double(), rx)
        rounding_gate(what + " forward", yk, y_ref, y_t, dtype == BF16, RESIZE_LOG)       # the forward takes the same weights
        ref = float((y_ref * dyp.double()).sum())
        mis = abs(float((yk * dyp.double()).sum()) - float((xp.double() * dxk).sum()))
        mis_t = abs(float((y_t.cpu().double() * dyp.double()).sum()) - float((xp.double() * dx_t.cpu().double()).sum()))
        gate = max(4.0 * mis_t, 8.0 * 2.0 ** -24 * abs(ref)) + (2.0 ** -8 * abs(ref) if dtype == BF16 else 0.0)
        print("%s adjoint identity: mismatch %.3e torch %.3e gate %.3e (inner product %.3e)" % (what, mis, mis_t, gate, ref))
        RESIZE_LOG.append((what + " identity", mis, mis_t, mis / gate))
        assert mis <= gate, "%s: <resize(x), dy> - <x, resize_bwd(dy)> = %.3e > %.3e" % (what, mis, gate)


def test_resize_bilinear_bwd_error_codes(cuda):
    """C = 12: COBEVT_ERR_SHAPE; a dtype code of 2: COBEVT_ERR_ARG; nothing written"""
    dy = torch.ones(2 * 4 * 4 * 16, device=cuda)
    for c, code, want in ((12, 1, ERR_SHAPE), (16, 2, ERR_ARG)):
        dx = Carved(2 * 2 * 2 * 16, F32, cuda)
        assert _lib().cobevt_resize_bilinear_bwd(ag._p(dy), ag._p(dx.t), code, 2, 2, 2, c, 4, 4, ag._stream()) == want
        dx.check("refused resize_bilinear_bwd call", written=False)


# ----------------------------------------------------------------------------------------------
# 5. cobevt_weighted_cross_entropy, cobevt_weighted_cross_entropy_bwd
# ----------------------------------------------------------------------------------------------
# hw around the 256 pixels of a pass of a workgroup and the 16 x 256 = 4096 pixels of one partial record; 9000: three records per image
WCE_HW = [1, 255, 256, 257, 4095, 4096, 4097, 9000]
WCE_WEIGHTS = {2: [1.0, 75.0], 3: [1.0, 15.0, 50.0], 8: [1.0, 3.0, 0.5, 20.0, 7.0, 1.5, 40.0, 2.0]}
WCE_LOG = []


def _wce_forward(dev, logits, target, weight, what):
    """-> (out[4] on the CPU, the carved out) with scratch carved at exactly 3 N ceil(hw / 4096) floats"""
    n, c, hw = logits.shape
    scr, out = Carved(3 * n * ((hw + 4095) // 4096), F32, dev), Carved(4, F32, dev)
    ld, td, wd = _dev(dev, logits, target, weight)
    _ok(_lib().cobevt_weighted_cross_entropy(ag._p(ld), ag._p(td), ag._p(wd), ag._p(scr.t), ag._p(out.t), _code(logits.dtype), n, c, hw, ag._stream()), what)
    scr.check(what + " scratch", written=True)            # every record of the exact size is written
    return out.check(what + " out", written=None).cpu(), out


def _wce_backward(dev, logits, target, weight, stats, upstream, what):
    n, c, hw = logits.shape
    dl = Carved(n * c * hw, F32, dev)
    ld, td, wd, ud = _dev(dev, logits, target, weight, torch.tensor([upstream]))
    _ok(_lib().cobevt_weighted_cross_entropy_bwd(ag._p(ld), ag._p(td), ag._p(wd), ag._p(stats.t), ag._p(ud), ag._p(dl.t), n, c, hw, ag._stream()), what)
    return dl.check(what, written=None).cpu().view(n, c, hw)


@pytest.mark.parametrize("c", [2, 3, 8])
def test_weighted_cross_entropy_exact(cuda, c):
    """all C logits of a pixel equal (an integer per pixel) and weights that are powers of two: logsumexp - x_y = log C on every counted
    pixel, so out[2] (sum of weights, multiples of 1/2) must be EXACT and out[1] = log C out[2] to 1e-5 (the project's forward gate; a
    pixel's m + log C - m carries half an ulp of m); known numbers of the labels C, -1 and -101 are counted in out[3] exactly; pixels
    labelled -100 carry unequal logits and contribute to nothing.  fp32 and bf16 logits, N = 1 and 3."""
    weight = 2.0 ** ((torch.arange(c) % 3) - 1).float()
    for n, hw, dtype in itertools.product((1, 3), WCE_HW, (F32, BF16)):
        g = torch.Generator().manual_seed(hw + n)
        logits = torch.randint(-8, 9, (n, 1, hw), generator=g).float().expand(n, c, hw).clone()
        target = torch.randint(0, c, (n, hw), generator=g)
        flat = target.view(-1)
        special = torch.randperm(n * hw, generator=g)
        n_bad = [min(k, (n * hw) // 8) for k in (3, 2, 4)]                       # labels C, -1, -101
        n_ign = (n * hw) // 5
        pos = 0
        for label, count in zip((c, -1, -101, -100), n_bad + [n_ign]):
            flat[special[pos:pos + count]] = label
            pos += count
        ign = (target == -100)[:, None].expand(n, c, hw)
        logits[ign] = (torch.arange(c).float() * 50.0)[None, :, None].expand(n, c, hw)[ign]
        valid = (target >= 0) & (target < c)
        den = float(weight[target[valid]].double().sum())
        what = "weighted_cross_entropy exact C=%d N=%d hw=%d %s" % (c, n, hw, "bf16" if dtype == BF16 else "fp32")
        out, _ = _wce_forward(cuda, logits.to(dtype), target, weight, what)
        assert float(out[2]) == den, "%s: sum of weights %r != %r" % (what, float(out[2]), den)
        assert float(out[3]) == float(sum(n_bad)), "%s: %r labels outside [0, C), %d planted" % (what, float(out[3]), sum(n_bad))
        if den > 0:
            assert abs(float(out[1]) - math.log(c) * den) <= 1e-5 * math.log(c) * den, what + " numerator"
            assert abs(float(out[0]) - math.log(c)) <= 1e-5 * math.log(c), what + " loss"


def _wce_inputs(n, c, hw, seed):
    """logits N(0, 3) with one logit at +-80 on a few pixels, 10 % ignore labels"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, c, hw, generator=g) * 3.0
    for j in range(min(6, hw)):
        logits[j % n, j % c, (j * 37) % hw] = 80.0 if j % 2 else -80.0
    target = torch.randint(0, c, (n, hw), generator=g)
    target[torch.rand(n, hw, generator=g) < 0.1] = -100
    return logits, target


def _wce_ref(logits, target, weight):
    """float64: (loss, numerator, denominator, dlogits / upstream)"""
    x = logits.double()
    valid = target != -100
    y = target.clamp_min(0)
    wy = weight.double()[y] * valid
    lse = torch.logsumexp(x, 1)
    num, den = (wy * (lse - x.gather(1, y[:, None])[:, 0])).sum(), wy.sum()
    onehot = torch.zeros_like(x).scatter_(1, y[:, None], 1.0)
    return num / den, num, den, (wy / den)[:, None] * (torch.softmax(x, 1) - onehot)


@pytest.mark.parametrize("c", [2, 3, 8])
def test_weighted_cross_entropy_rounding(cuda, c):
    """out[0..2] (each under the rounding gate, torch side: F.cross_entropy with mean and sum reduction and the fp32 sum of w[y]) for
    fp32 and bf16 logits; the backward for fp32 logits per element with upstream 1 and 0.37 (torch side: autograd of the mean), pixels
    with the ignore label exactly 0 in every class"""
    weight = torch.tensor(WCE_WEIGHTS[c])
    for n, hw in itertools.product((1, 3), WCE_HW):
        logits, target = _wce_inputs(n, c, hw, 11 * hw + n + c)
        if not bool((target != -100).any()):
            target[0, 0] = 0
        for dtype in (F32, BF16):
            lq = logits.to(dtype)
            what = "weighted_cross_entropy C=%d N=%d hw=%d %s" % (c, n, hw, "bf16" if dtype == BF16 else "fp32")
            loss, num, den, dl_ref = _wce_ref(lq, target, weight)
            out, stats = _wce_forward(cuda, lq, target, weight, what)
            assert float(out[3]) == 0.0, what + ": no label is outside [0, C)"
            with torch.enable_grad():
                lt = lq.float().to(cuda).requires_grad_(True)
                td, wd = _dev(cuda, target, weight)
                mean_t = Fn.cross_entropy(lt, td, wd)
                sum_t = Fn.cross_entropy(lt, td, wd, reduction="sum")
                den_t = (wd[td.clamp_min(0)] * (td != -100)).sum()
                mean_t.backward()
            for i, (ref, tor) in enumerate(((loss, mean_t), (num, sum_t), (den, den_t))):
                rounding_gate("%s out[%d]" % (what, i), out[i:i + 1], ref.view(1), tor.detach().view(1), False, WCE_LOG)
            if dtype == BF16:
                continue
            for upstream in (1.0, 0.37):
                got = _wce_backward(cuda, lq, target, weight, stats, upstream, what + " backward")
                assert bool(torch.isfinite(got).all()), what + " backward: non-finite"
                rounding_gate("%s backward upstream=%g" % (what, upstream), got, _f32(upstream) * dl_ref, _f32(upstream) * lt.grad, False, WCE_LOG)
                ign = (target == -100)[:, None].expand(n, c, hw)
                assert bool((got[ign] == 0).all()), what + ": a pixel with the ignore label must get exactly 0 in every class"


def test_weighted_cross_entropy_all_ignored(cuda):
    """every label -100: numerator, denominator and the bad-label count are 0 and the loss is 0 / 0 = NaN, as torch's; the backward
    divides by the zero denominator and writes NaN to every element - inside its buffer (include/cobevt_hip.h states both)"""
    n, c, hw = 3, 3, 4097
    logits, _ = _wce_inputs(n, c, hw, 1)
    target = torch.full((n, hw), -100, dtype=I64)
    out, stats = _wce_forward(cuda, logits, target, torch.tensor(WCE_WEIGHTS[c]), "weighted_cross_entropy all ignored")
    print("weighted_cross_entropy, all labels ignored: out = %s" % out.tolist())
    assert math.isnan(float(out[0])) and out[1:].tolist() == [0.0, 0.0, 0.0]
    got = _wce_backward(cuda, logits, target, torch.tensor(WCE_WEIGHTS[c]), stats, 1.0, "weighted_cross_entropy_bwd all ignored")
    print("weighted_cross_entropy_bwd, all labels ignored: %d of %d elements NaN" % (int(torch.isnan(got).sum()), got.numel()))
    assert bool(torch.isnan(got).all())


def test_weighted_cross_entropy_error_codes(cuda):
    """C = 1 and C = 9: COBEVT_ERR_SHAPE; a dtype code of 2: COBEVT_ERR_ARG; nothing written"""
    x, t, w = torch.zeros(9 * 16, device=cuda), torch.zeros(16, dtype=I64, device=cuda), torch.ones(9, device=cuda)
    for c, code, want in ((1, 1, ERR_SHAPE), (9, 1, ERR_SHAPE), (3, 2, ERR_ARG)):
        scr, out, dl = Carved(3, F32, cuda), Carved(4, F32, cuda), Carved(9 * 16, F32, cuda)
        assert _lib().cobevt_weighted_cross_entropy(ag._p(x), ag._p(t), ag._p(w), ag._p(scr.t), ag._p(out.t), code, 1, c, 16, ag._stream()) == want
        if code == 1:
            assert _lib().cobevt_weighted_cross_entropy_bwd(ag._p(x), ag._p(t), ag._p(w), ag._p(w), ag._p(w), ag._p(dl.t), 1, c, 16, ag._stream()) == want
        for b in (scr, out, dl):
            b.check("refused weighted_cross_entropy call", written=False)


# ----------------------------------------------------------------------------------------------
# 6. cobevt_sigmoid_focal_loss, cobevt_sigmoid_focal_loss_bwd, cobevt_iou_counts
# ----------------------------------------------------------------------------------------------
# hw around the 8 x 256 = 2048 pixels of one partial record; 5000: three records per image
FOCAL_HW = [1, 2047, 2048, 2049, 5000]
# (N, C, NL, soft labels, min_visibility, alpha, gamma): NL = 32 uses bit 31 of label_mask; soft labels need NL == C
FOCAL_CONFIGS = [(1, 1, 1, False, -1, -1.0, 0.0), (2, 3, 12, False, 2, 0.25, 2.0), (2, 1, 32, False, 2, 0.25, 1.5), (1, 3, 3, True, 2, -1.0, 2.0),
                 (2, 1, 1, True, -1, 0.25, 1.0), (1, 3, 32, False, -1, -1.0, 1.5), (2, 3, 3, True, 2, 0.25, 1.5), (1, 1, 12, False, 2, -1.0, 0.0),
                 (2, 1, 1, True, -1, -1.0, 0.0), (1, 3, 12, False, -1, 0.25, 1.0)]
_PLANTED = [20.0, -20.0, 90.0, -90.0, 0.0]
FOCAL_LOG = []


def _label_groups(c, nl):
    """label channels of output channel ch: every c-th from ch, and the last channel (bit NL - 1) for channel 0"""
    groups = [sorted(set(range(ch, nl, c)) | ({nl - 1} if ch == 0 else set())) for ch in range(c)]
    return groups, torch.tensor([sum(1 << l for l in grp) for grp in groups], dtype=I64).to(torch.int32)   # bit 31: the int32 wraps


def _focal_inputs(n, c, nl, hw, soft, seed):
    """logits N(0, 2) with +-20, +-90 and 0 planted where every label channel is exactly 0 or exactly 1 (both occur); binary labels
    (30 % ones), or soft labels uniform in [0, 1) with one value of 1 - 2^-24 under a logit of 20; visibility 0 .. 4"""
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(n, c, hw, generator=g) * 2.0
    label = torch.rand(n, nl, hw, generator=g) if soft else (torch.rand(n, nl, hw, generator=g) < 0.3).float()
    vis = torch.randint(0, 5, (n, hw), generator=g).to(torch.uint8)
    for j in range(min(2 * len(_PLANTED), hw)):
        pix = (j * 131) % hw
        pred[j % n, :, pix] = _PLANTED[j % len(_PLANTED)]
        label[j % n, :, pix] = float((j // len(_PLANTED)) % 2)
        vis[j % n, pix] = 4
    if soft and hw > 2000:
        pred[0, 0, 1999], label[0, 0, 1999], vis[0, 1999] = 20.0, 1.0 - 2.0 ** -24, 4
    return pred, label, vis


def _focal_forward(dev, pred, label, vis, masks, mv, alpha, gamma, soft, what):
    n, c, hw = pred.shape
    scr, out = Carved(2 * n * ((hw + 2047) // 2048), F32, dev), Carved(3, F32, dev)
    pd, ld, vd, md = _dev(dev, pred, label, vis, masks)
    rc = _lib().cobevt_sigmoid_focal_loss(ag._p(pd), ag._p(ld), ag._p(vd), ag._p(md), ag._p(scr.t), ag._p(out.t), n, c, label.shape[1], hw, mv, alpha, gamma,
                                          int(soft), ag._stream())
    _ok(rc, what)
    scr.check(what + " scratch", written=True)
    return out.check(what + " out", written=None).cpu(), out


def _focal_backward(dev, pred, label, vis, masks, stats, gscale, mv, alpha, gamma, soft, what):
    n, c, hw = pred.shape
    dp = Carved(n * c * hw, F32, dev)
    pd, ld, vd, md, gd = _dev(dev, pred, label, vis, masks, torch.tensor([gscale]))
    rc = _lib().cobevt_sigmoid_focal_loss_bwd(ag._p(pd), ag._p(ld), ag._p(vd), ag._p(md), ag._p(stats.t), ag._p(gd), ag._p(dp.t), n, c, label.shape[1], hw,
                                              mv, alpha, gamma, int(soft), ag._stream())
    _ok(rc, what)
    return dp.check(what).cpu().view(n, c, hw)             # finite everywhere: no NaN at the planted values for any gamma


@pytest.mark.parametrize("hw", FOCAL_HW)
def test_sigmoid_focal_loss(cuda, hw):
    """forward: out[2] (the count) exact, out[0] (mean) and out[1] (sum) under the rounding gate, torch side util.focal_reference in fp32
    on the device, reference the same formula in float64; backward with gscale 1 and 0.1: per element under the gate, masked pixels
    exactly 0, every element finite (Carved.check) - grouped binary and soft labels, min_visibility -1 and 2, alpha -1 and 0.25, gamma
    0, 1, 2 and 1.5 (FOCAL_CONFIGS)"""
    for i, (n, c, nl, soft, mv, alpha, gamma) in enumerate(FOCAL_CONFIGS):
        what = "sigmoid_focal_loss hw=%d N=%d C=%d NL=%d soft=%s min_visibility=%d alpha=%g gamma=%g" % (hw, n, c, nl, soft, mv, alpha, gamma)
        pred, label, vis = _focal_inputs(n, c, nl, hw, soft, 100 * hw + i)
        groups, masks = (None, None) if soft else _label_groups(c, nl)
        mvis = None if mv < 0 else mv
        kept = torch.ones(n, hw, dtype=torch.bool) if mv < 0 else vis >= mv
        if not bool(kept.any()):
            vis[0, 0], kept[0, 0] = 4, True
        with torch.enable_grad():
            p64 = pred.double().requires_grad_(True)
            ref_sum = focal_reference(p64, label.double(), vis, groups, mvis, alpha, gamma, "sum")
            ref_sum.backward()
            pt, lt, vt = pred.to(cuda).requires_grad_(True), label.to(cuda), vis.to(cuda)
            tor_mean = focal_reference(pt, lt, vt, groups, mvis, _f32(alpha), _f32(gamma))
            tor_mean.backward()
            tor_sum = focal_reference(pt.detach(), lt, vt, groups, mvis, _f32(alpha), _f32(gamma), "sum")
        count = int(kept.sum()) * c
        out, stats = _focal_forward(cuda, pred, label, vis if mv >= 0 else None, masks, mv, alpha, gamma, soft, what)
        assert float(out[2]) == float(count), "%s: count %r != %d" % (what, float(out[2]), count)
        rounding_gate(what + " mean", out[0:1], (ref_sum.detach() / count).view(1), tor_mean.detach().view(1), False, FOCAL_LOG)
        rounding_gate(what + " sum", out[1:2], ref_sum.detach().view(1), tor_sum.view(1), False, FOCAL_LOG)
        for gscale in (1.0, 0.1):
            got = _focal_backward(cuda, pred, label, vis if mv >= 0 else None, masks, stats, gscale, mv, alpha, gamma, soft, what + " backward")
            rounding_gate("%s backward gscale=%g" % (what, gscale), got, _f32(gscale) * p64.grad / count, _f32(gscale) * pt.grad, False, FOCAL_LOG)
            masked = (~kept)[:, None].expand(n, c, hw)
            assert bool((got[masked] == 0).all()), what + ": a masked pixel must get exactly 0"


def test_sigmoid_focal_loss_all_masked(cuda):
    """no pixel reaches min_visibility: sum and count are 0 and the mean is 0 / 0 = NaN; the backward's `count > 0` guard writes zeros
    (include/cobevt_hip.h states both)"""
    n, c, nl, hw = 2, 3, 12, 2049
    pred, label, vis = _focal_inputs(n, c, nl, hw, False, 3)
    vis.fill_(1)
    _, masks = _label_groups(c, nl)
    out, stats = _focal_forward(cuda, pred, label, vis, masks, 2, 0.25, 2.0, False, "sigmoid_focal_loss all masked")
    print("sigmoid_focal_loss, all pixels masked: out = %s" % out.tolist())
    assert math.isnan(float(out[0])) and out[1:].tolist() == [0.0, 0.0]
    got = _focal_backward(cuda, pred, label, vis, masks, stats, 1.0, 2, 0.25, 2.0, False, "sigmoid_focal_loss_bwd all masked")
    assert bool((got == 0).all())


def test_sigmoid_focal_loss_error_codes(cuda):
    """NL = 33, soft labels with NL != C: COBEVT_ERR_SHAPE; min_visibility >= 0 without a visibility map, grouped labels without masks:
    COBEVT_ERR_ARG; from both directions, nothing written"""
    p, lab, vis, masks = torch.zeros(64, device=cuda), torch.zeros(33 * 16, device=cuda), torch.zeros(16, dtype=torch.uint8, device=cuda), torch.ones(4, dtype=torch.int32, device=cuda)
    for c, nl, soft, mv, with_vis, with_masks, want in ((2, 33, 0, -1, True, True, ERR_SHAPE), (2, 3, 1, -1, True, True, ERR_SHAPE),
                                                        (2, 3, 0, 2, False, True, ERR_ARG), (2, 3, 0, -1, True, False, ERR_ARG)):
        scr, out, dp = Carved(2, F32, cuda), Carved(3, F32, cuda), Carved(64, F32, cuda)
        pv, pm = ag._p(vis) if with_vis else None, ag._p(masks) if with_masks else None
        rc = _lib().cobevt_sigmoid_focal_loss(ag._p(p), ag._p(lab), pv, pm, ag._p(scr.t), ag._p(out.t), 1, c, nl, 16, mv, 0.25, 2.0, soft, ag._stream())
        rcb = _lib().cobevt_sigmoid_focal_loss_bwd(ag._p(p), ag._p(lab), pv, pm, ag._p(p), ag._p(p), ag._p(dp.t), 1, c, nl, 16, mv, 0.25, 2.0, soft, ag._stream())
        assert (rc, rcb) == (want, want), (c, nl, soft, mv, rc, rcb)
        for b in (scr, out, dp):
            b.check("refused sigmoid_focal_loss call", written=False)


IOU_THRESHOLDS = {1: [0.5], 8: [0.4, 0.5, 0.1, 0.9, 0.3, 0.6, 0.7, 0.45]}


@pytest.mark.parametrize("hw", FOCAL_HW)
def test_iou_counts(cuda, hw):
    """(tp, fp, fn) per threshold, integer-exact against numpy, added to pre-filled counts (the metric accumulates); thresholds 0.4, 0.5
    and six more (T = 1 and 8); logits of exactly 0 planted so that sigmoid = 0.5 sits ON a threshold and counts as predicted; random
    logits whose float64 sigmoid lies within 1e-5 of a threshold are moved away (neither side could resolve them)"""
    for (n, c, nl), mv, t in itertools.product(((1, 1, 1), (2, 3, 12), (2, 1, 32), (1, 3, 32)), (-1, 2), (1, 8)):
        what = "iou_counts hw=%d N=%d C=%d NL=%d min_visibility=%d T=%d" % (hw, n, c, nl, mv, t)
        pred, label, vis = _focal_inputs(n, c, nl, hw, False, 7 * hw + nl + t)
        label = label * torch.where(torch.arange(hw) % 2 == 0, 1.0, 0.5)              # non-zero means present, whatever the value
        thr = torch.tensor(IOU_THRESHOLDS[t])
        s = torch.sigmoid(pred.double())
        near = ((s[..., None] - thr.double()).abs() < 1e-5).any(-1) & (pred != 0)
        pred[near] = 3.0
        s = torch.sigmoid(pred.double()).numpy()
        groups, masks = _label_groups(c, nl)
        lab = np.stack([(label[:, grp] != 0).any(1).numpy() for grp in groups], 1)      # (N, C, hw)
        kept = np.broadcast_to((np.ones((n, hw), bool) if mv < 0 else (vis >= mv).numpy())[:, None], lab.shape)
        pre = (torch.arange(3 * t, dtype=I64) * 1000003) % 977
        want = pre.clone().view(t, 3)
        for i, th in enumerate(thr.double().tolist()):
            pr = s >= th
            want[i] += torch.tensor([int((pr & lab & kept).sum()), int((pr & ~lab & kept).sum()), int((~pr & lab & kept).sum())])
        counts = carved_from(pre, cuda)
        pd, ld, vd, md, td = _dev(cuda, pred, label, vis if mv >= 0 else None, masks, thr)
        rc = _lib().cobevt_iou_counts(ag._p(pd), ag._p(ld), ag._p(vd), ag._p(md), ag._p(td), ag._p(counts.t), n, c, nl, hw, t, mv, ag._stream())
        _ok(rc, what)
        assert torch.equal(counts.check(what).cpu().view(t, 3), want), what
        if hw >= len(_PLANTED):
            assert bool((pred == 0).any()), "a logit of exactly 0 is planted"


def teardown_module(module):
    """the figures of tests/golden/README_train_rows.md: per section and output, the worst error / gate with its kernel and torch errors"""
    for name, log in (("layernorm", LN_LOG), ("activations", ACT_LOG), ("depthwise_wgrad", DW_LOG), ("resize_bilinear_bwd", RESIZE_LOG),
                      ("weighted_cross_entropy", WCE_LOG), ("sigmoid_focal_loss", FOCAL_LOG)):
        if log:
            worst = max(log, key=lambda r: r[3])
            print("\n[train_rows] %s: %d gated comparisons, worst err/gate %.3f at %s (kernel %.3e, torch %.3e)" % (name, len(log), worst[3], worst[0], worst[1], worst[2]))
