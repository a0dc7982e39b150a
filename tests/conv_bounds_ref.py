"""Float64 interval reference of the convolution kernels (tests/test_conv_bounds.py on the CPU, tests/test_conv_bounds_gpu.py on the device).

A stage is  out = round(act(sum_k x_k w_k + shift (+ residual)))  with the operands the kernel gets: the input already in the storage
dtype and the folded weights / shift read back from the plan (no folding is re-derived here).  For every output element it gives
    ref   the float64 result
    S     sum_k |x_k| |w_k| + |shift| (+ |residual|)
    e     the bound of the fp32 accumulation before the store:  K 2^-23 S + 2^-23 |pre|  (K = contraction length: Cin k k, plus the
          shortcut's Cin where a projection shortcut is accumulated into the same registers), plus the mode term derived from
          csrc/f32_matrix.hpp (the same terms as tests/test_bev_backbone_gpu.py):
              bf16        nothing: bf16 x bf16 products are exact in the fp32 accumulator
              fp32_split  2^-17 S: operands as hi + lo bf16 halves, |x - hi - lo| <= 2^-17 |x|
                          + 2^-16 S where the kernel takes the THREE-term form (kXPack3: "the dropped w_lo . x_lo term is 2^-16 of a product")
              fp32_fast   2^-11 S: the weights as ONE fp16 term (11 significand bits); + 2^-25 sum_k |x_k| for weights below fp16's normal
                          range (absolute spacing 2^-24 there)
                          + (2^-11 + 2^-22) S where the kernel takes the PACKED form (kXPack: the activations as one fp16 value, too)
    lo, hi   a kernel that rounds ONCE stores a value in [round(act(pre - e)), round(act(pre + e))]: round = round to nearest even to the
          storage dtype (through fp32, as the accumulator is fp32: both roundings are monotone, so is their composition), act = none | ReLU.
          There is no slack for a second rounding, and the statement is the same for fp32 storage.

Fused kernels propagate the interval: an intermediate the kernel keeps in the storage dtype lies in [lo1, hi1] (equal for most
elements, one ulp apart for those that straddle a rounding boundary); the next stage is evaluated at the midpoint and conv(|w2|, d1)
with d1 = (hi1 - lo1) / 2 is added to its e.  Max-pool passes intervals through (max of the lo's, max of the hi's); the uint8 stem
applies its table exactly.

Every network below is written ONCE against a backend: Ref (the intervals, float64) and Emul (a CPU model of a correct kernel: fp32
F.conv2d on the same operands - rounded as f32_matrix.hpp documents in the split / fast modes - and one round-to-nearest-even per
stored stage), which also injects the faults the CPU file must see leave the interval.  GELU / swish epilogues are out of scope
(their approximation error cannot be derived; the activation kernels have float64 tests of their own)."""
import math
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from cobevt_amd import ops
from cobevt_amd.synth import procedural_input

U = 2.0 ** -23
MODES = ("bf16", "fp32", "fp32_split", "fp32_fast")
LIB = {"bf16": "", "fp32": "", "fp32_split": "f32s", "fp32_fast": "f32h"}
F64 = torch.float64
Interval = namedtuple("Interval", "ref S e lo hi")


def store_dtype(mode):
    return torch.bfloat16 if mode == "bf16" else torch.float32


def rne(t, dtype):
    """float64 -> fp32 -> dtype -> float64, each step round to nearest even"""
    return t.to(torch.float32).to(dtype).to(F64)


def _act(t, act):
    return torch.relu(t) if act else t


def _mode_term(mode, packed, mag, absx):
    if mode == "fp32_split":
        return (2.0 ** -17 + (2.0 ** -16 if packed else 0.0)) * mag
    if mode == "fp32_fast":
        return (2.0 ** -11 + ((2.0 ** -11 + 2.0 ** -22) if packed else 0.0)) * mag + 2.0 ** -25 * absx
    return 0.0


class V(object):
    """a map between two stages: Ref keeps (mid, d = half-width, iv), Emul keeps the fp32 tensor in `mid`"""
    __slots__ = ("mid", "d", "iv")

    def __init__(self, mid, d=None, iv=None):
        self.mid, self.d, self.iv = mid, d, iv


class Ref(object):
    def __init__(self, mode):
        self.mode, self.dt, self.inter, self.final = mode, store_dtype(mode), [], None

    def input(self, x):
        x = x.to(F64)
        return V(x, torch.zeros_like(x))

    def _close(self, pre, mag, e, act, dt, inter):
        iv = Interval(_act(pre, act), mag, e, rne(_act(pre - e, act), dt), rne(_act(pre + e, act), dt))
        if inter:
            self.inter.append(iv)
        return V((iv.lo + iv.hi) / 2, (iv.hi - iv.lo) / 2, iv)

    def affine(self, v, scale, shift, relu):
        """the pre-activation BatchNorm (+ ReLU) applied while the tile is gathered: one fma per element (K = 1), rounded to the storage dtype"""
        sc, sh = scale.to(F64)[None, :, None, None], shift.to(F64)[None, :, None, None]
        pre, mag = v.mid * sc + sh, v.mid.abs() * sc.abs() + sh.abs()
        return self._close(pre, mag, U * mag + U * pre.abs(), relu, self.dt, True)

    def up(self, v):
        return V(F.interpolate(v.mid, scale_factor=2, mode="nearest"), F.interpolate(v.d, scale_factor=2, mode="nearest"))

    def conv(self, v, w, shift, k, stride=1, pad=0, act=0, res=None, extra=None, inter=False, packed=False, dt=None, final=False):
        w, shift = w.to(F64), shift.to(F64)[None, :, None, None]
        ax = v.mid.abs() + v.d
        pre = F.conv2d(v.mid, w, None, stride, pad) + shift
        mag = F.conv2d(ax, w.abs(), None, stride, pad)
        absx = F.conv2d(ax, torch.ones_like(w), None, stride, pad)
        unc = F.conv2d(v.d, w.abs(), None, stride, pad)
        if extra is not None:                                 # a projection shortcut accumulated into the same registers
            v2, w2, s2 = extra
            w2 = w2.to(F64)
            ax2 = v2.mid.abs() + v2.d
            pre = pre + F.conv2d(v2.mid, w2, None, s2)
            mag = mag + F.conv2d(ax2, w2.abs(), None, s2)
            absx = absx + F.conv2d(ax2, torch.ones_like(w2), None, s2)
            unc = unc + F.conv2d(v2.d, w2.abs(), None, s2)
        mterm = _mode_term(self.mode, packed, mag, absx)      # (shift and residual are added in fp32 in every mode)
        mag = mag + shift.abs()
        if res is not None:
            r = res if isinstance(res, V) else V(res.to(F64), torch.zeros_like(res, dtype=F64))
            pre, mag, unc = pre + r.mid, mag + r.mid.abs() + r.d, unc + r.d
        e = k * U * mag + U * (pre.abs() + unc) + mterm + unc
        out = self._close(pre, mag, e, act, dt or self.dt, inter)
        if final:
            self.final = out.iv
        return out

    def pool(self, v):
        iv = v.iv
        p = lambda t: F.max_pool2d(t, 3, 2, 1)          # noqa: E731
        iv = Interval(p(iv.ref), None, None, p(iv.lo), p(iv.hi))
        return V((iv.lo + iv.hi) / 2, (iv.hi - iv.lo) / 2, iv)

    def unshuffle(self, v):
        iv = Interval(*[None if t is None else F.pixel_unshuffle(t, 2) for t in v.iv])
        return V(None, None, iv)


def _split_bf16(t):
    hi = t.to(torch.bfloat16).float()
    return hi, (t - hi).to(torch.bfloat16).float()


def truncate_bf16(t):
    """fp32 -> bf16 by dropping the low 16 bits (the fault a pack without rounding makes)"""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


class Emul(object):
    """a correct kernel on the CPU, or one with `fault`: "drop" = the last (non-zero) input channel's centre-tap product missing at the four
    corner pixels of the final convolution, "late" = its residual (else its shift) added after the rounding, "unrounded" = the intermediates kept
    in fp32, "trunc" = the final bf16 store truncates"""

    def __init__(self, mode, fault=None):
        self.mode, self.dt, self.fault = mode, store_dtype(mode), fault

    def _rnd(self, t, dt):
        return t.to(dt).float()

    def input(self, x):
        return V(x.float())

    def affine(self, v, scale, shift, relu):
        y = _act(v.mid * scale.float()[None, :, None, None] + shift.float()[None, :, None, None], relu)
        return V(y if self.fault == "unrounded" else self._rnd(y, self.dt))

    def up(self, v):
        return V(F.interpolate(v.mid, scale_factor=2, mode="nearest"))

    def _terms(self, x, w, packed):
        if self.mode == "fp32_split":
            (xh, xl), (wh, wl) = _split_bf16(x), _split_bf16(w)
            return [(xh + xl, wh + wl, 1.0)] + ([(xl, wl, -1.0)] if packed else [])
        if self.mode == "fp32_fast":
            xh = x.half().float()
            return [(xh if packed else xh + ((x - xh) * 64.0).half().float() / 64.0, w.half().float(), 1.0)]
        return [(x, w, 1.0)]

    def _mm(self, x, w, stride, pad, packed):
        acc = None
        for xa, wa, sign in self._terms(x, w.float(), packed):
            t = sign * F.conv2d(xa, wa, None, stride, pad)
            acc = t if acc is None else acc + t
        return acc

    def conv(self, v, w, shift, k, stride=1, pad=0, act=0, res=None, extra=None, inter=False, packed=False, dt=None, final=False):
        dt = dt or self.dt
        acc = self._mm(v.mid, w, stride, pad, packed)
        if final and self.fault == "drop":
            xa, wa, _ = self._terms(v.mid, w.float(), packed)[0]
            kc = w.shape[2] // 2 if pad else 0
            for oy in {0, acc.shape[2] - 1}:
                for ox in {0, acc.shape[3] - 1}:
                    px = xa[:, :, oy * stride - pad + kc, ox * stride - pad + kc]
                    for n in range(px.shape[0]):      # (behind a ReLU the last channel may be 0 there - a void fault: the last non-zero one)
                        nz = px[n].nonzero()
                        c = int(nz[-1]) if nz.numel() else -1
                        acc[n, :, oy, ox] -= px[n, c] * wa[:, c, kc, kc]
        if extra is not None:
            v2, w2, s2 = extra
            acc = acc + self._mm(v2.mid, w2, s2, 0, packed)
        sh = shift.float()[None, :, None, None]
        r = None if res is None else (res.mid if isinstance(res, V) else res.float())
        if final and self.fault == "late":
            if r is not None:
                y = _act(self._rnd(acc + sh, dt) + r, act)
            else:
                y = _act(self._rnd(acc, dt) + sh, act)
        else:
            y = _act(acc + sh + (0.0 if r is None else r), act)
        if inter and self.fault == "unrounded":
            return V(y)
        if final and self.fault == "trunc":
            assert dt == torch.bfloat16
            return V(truncate_bf16(y))
        return V(self._rnd(y, dt))

    def pool(self, v):
        return V(F.max_pool2d(v.mid, 3, 2, 1))

    def unshuffle(self, v):
        return V(F.pixel_unshuffle(v.mid, 2))


# ----------------------------------------------------------------------------------------------
# statistics
# ----------------------------------------------------------------------------------------------
BIAS_LIMIT, BIAS_MIN_N = 2.0 ** -11, 2000


def bias_stat(got, ref):
    """-> (mean of (got - ref) / ref over the elements with |ref| >= 2^-6 max|ref|, their number).  Round to nearest even to bf16: mean 0,
    standard deviation below 2^-8 / sqrt(3 N), so with N >= 2000 the limit 2^-11 is above 10 sigma; a truncating store gives about -2.8e-3"""
    sel = ref.abs() >= 2.0 ** -6 * ref.abs().max()
    return float(((got[sel] - ref[sel]) / ref[sel]).mean()), int(sel.sum())


def position(got, iv):
    """max |got - mid| / half-width over the elements with lo < hi (where lo == hi the only value inside has position 0)"""
    hw = (iv.hi - iv.lo) / 2
    sel = hw > 0
    if not bool(sel.any()):
        return 0.0
    return float(((got[sel] - (iv.lo[sel] + iv.hi[sel]) / 2).abs() / hw[sel]).max())


def error_over_e(got, iv):
    """max |got - ref| / e over the elements the ReLU does not cut: how much of the accumulation bound a kernel uses.  Meaningful for fp32
    stores, where the rounding of the store is below e; nan behind a max-pool (e belongs to the convolution in front of it)"""
    if iv.e is None:
        return float("nan")
    sel = iv.ref != 0
    return float(((got[sel] - iv.ref[sel]).abs() / iv.e[sel]).max()) if bool(sel.any()) else 0.0


def outside(got, iv):
    return int(((got < iv.lo) | (got > iv.hi)).sum())


# ----------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------
class FakeBN(object):
    def __init__(self, c, key):
        self.weight = 0.8 + 0.4 * procedural_input(key + ".w", (c,), 0, 0, 1)
        self.bias = procedural_input(key + ".b", (c,), 0, -0.2, 0.2)
        self.running_mean = procedural_input(key + ".m", (c,), 0, -0.3, 0.3)
        self.running_var = 0.6 + 0.8 * procedural_input(key + ".v", (c,), 0, 0, 1)
        self.eps = 1e-5


class Case(object):
    """name, kind (a key of BUILDERS), entry (the C symbol the case must launch), modes (the modes the entry point is built for), knobs
    (ops switches that force the route), stat (False: fewer than BIAS_MIN_N outputs, no bias statistic), packed (the modes in which the
    kernel takes the three-term / packed form of f32_matrix.hpp), a (the kind's arguments)"""

    def __init__(self, name, kind, entry, modes, knobs=None, stat=True, packed=(), hidden=(), **a):
        self.name, self.kind, self.entry, self.modes, self.knobs, self.stat, self.packed, self.a = name, kind, entry, modes, knobs or {}, stat, packed, a
        self.hidden = hidden

    def __repr__(self):
        return self.name


class knobs(object):
    def __init__(self, case):
        self.new = case.knobs

    def __enter__(self):
        self.old = {k: getattr(ops, k) for k in self.new}
        for k, v in self.new.items():
            setattr(ops, k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            setattr(ops, k, v)
        return False


def _w4(plan, table=None):
    """the folded weights as the plan stores them -> (Cout, Cin, k, k)"""
    t = plan.wgt if table is None else table
    return t.detach().cpu()[:, :plan.K].to(F64).reshape(plan.cout, plan.kh, plan.kw, plan.cin).permute(0, 3, 1, 2).contiguous()


def _shift(plan):
    return plan.bias.detach().cpu().to(F64) if plan.bias is not None else torch.zeros(plan.cout, dtype=F64)


def _conv(case, mode, device):
    a, dt = case.a, store_dtype(mode)
    n, cin, h, w, cout, k = a["n"], a["cin"], a["h"], a["w"], a["cout"], a["k"]
    if a.get("cin_fp32") and dt == torch.float32:
        cin = a["cin_fp32"]
    stride, pad, act, sm, smallc = a.get("stride", 1), a.get("pad", 0), a.get("act", 0), a.get("store_mode", 0), a.get("smallc", False)
    key = "cb." + case.name
    x = procedural_input(key + ".x", (n, cin, h, w), 0)
    wt = procedural_input(key + ".w", (cout, cin, k, k), 0) * math.sqrt(3.0 / (cin * k * k))
    b = procedural_input(key + ".b", (cout,), 0, -0.3, 0.3) if a.get("bias", True) else None
    bnm = FakeBN(cout, key + ".bn") if a.get("bn") else None
    pbn = FakeBN(cin, key + ".pbn") if a.get("pre_bn") else None
    plan = ops.ConvPlan(wt, b, bn=bnm, pre_bn=pbn, pre_relu=bool(pbn), stride=stride, pad=pad, act=act, upsample=a.get("upsample", False),
                        store_mode=sm, dtype=dt, device=device, smallc=smallc)
    xs = rne(x.to(F64), dt)             # (a small-Cin plan takes the fp32 image and rounds it to the storage dtype while it packs the tile)
    ho, wo = plan.out_hw(h, w)
    res = rne(procedural_input(key + ".res", (n, cout, ho, wo), 0).to(F64), dt) if a.get("residual") else None
    wk = plan.wgt_head.detach().cpu().to(F64).reshape(cout, 3, 3, cin).permute(0, 3, 1, 2) if a.get("head") else \
        _w4(plan, plan.wgt_rows) if a.get("rows") else _w4(plan)
    shift = _shift(plan)
    packed = mode in case.packed

    def net(B):
        v = B.input(xs)
        if pbn is not None:
            v = B.affine(v, plan.pre_scale.cpu(), plan.pre_shift.cpu(), True)
        if plan.upsample:
            v = B.up(v)
        out = B.conv(v, wk, shift, plan.K, stride, pad, act, res=res, packed=packed, dt=torch.float32 if sm == 2 else dt, final=True)
        return B.unshuffle(out) if sm == 1 else out
    return dict(net=net, plan=plan, x=x if smallc else xs.to(dt), res=None if res is None else res.to(dt), out_pad=a.get("out_pad"))


# ---- inputs of the fused cases.  With K = 576 .. 1152 and operands of random sign the sums cancel (S / |pre| ~ sqrt(K)) and e reaches the
# spacing of bf16: half the intermediates then straddle a rounding boundary and the propagated term carries the test.  So the fused
# cases take operands whose SIGNS are coherent and whose magnitudes are random: x = g(pixel) m with a smooth field g in [-1, 1] and
# m in [0.5, 1), weights W_k[co, ci] = tau_k[co] tau_(k-1)[ci] |u| with sign vectors tau (tau_0 = 1).  Stage k is then
# tau_k[co] sign(g) (a sum of positive terms): S / |pre| ~ 1, every channel lives on the pixels where tau_k[co] = sign(g) and is cut by
# the ReLU on the others, and every weight multiplies a non-zero activation somewhere.
def _field(n, h, w):
    y, x, i = torch.arange(h, dtype=F64)[None, :, None], torch.arange(w, dtype=F64)[None, None, :], torch.arange(n, dtype=F64)[:, None, None]
    return torch.sin(0.9 * y + 0.55 * x + 1.3 * i + 0.4).float()


def _coherent_x(key, g, c):
    n, h, w = g.shape
    return g[:, None] * (0.5 + 0.5 * procedural_input(key, (n, c, h, w), 0, 0.0, 1.0))


def _signs(key, c):
    return torch.where(procedural_input(key, (c,), 0) >= 0, 1.0, -1.0)


def _coherent_w(key, cout, cin, k, tau_out, tau_in=None):
    tau_in = torch.ones(cin) if tau_in is None else tau_in
    mag = 0.5 + 0.5 * procedural_input(key, (cout, cin, k, k), 0, 0.0, 1.0)
    return tau_out[:, None, None, None] * tau_in[None, :, None, None] * mag * (1.5 / (0.5625 * cin * k * k))


def _bb_plans(key, c, dt, device):
    t1, t2 = _signs(key + ".t1", c), _signs(key + ".t2", c)
    w1, w2 = _coherent_w(key + ".w1", c, c, 3, t1), _coherent_w(key + ".w2", c, c, 3, t2, t1)
    p1 = ops.ConvPlan(w1, None, bn=FakeBN(c, key + ".bn1"), stride=1, pad=1, act=1, dtype=dt, device=device)
    p2 = ops.ConvPlan(w2, None, bn=FakeBN(c, key + ".bn2"), stride=1, pad=1, act=1, dtype=dt, device=device)
    return p1, p2


def _basicblock(case, mode, device):
    """relu(conv2(round(relu(conv1(x)))) + x): the intermediate is rounded to the storage type exactly as the unfused path stores it
    (basicblock.hip); both convolutions in the three-term / packed form in the second / third library (kXPack3<T, 4> / kXPack<T, 4>)"""
    a, dt = case.a, store_dtype(mode)
    c, packed = a["c"], mode in case.packed
    p1, p2 = _bb_plans("cb.bb%d" % c, c, dt, device)
    xs = rne(_coherent_x("cb.bb.x", _field(a["n"], a["h"], a["w"]), c).to(F64), dt)
    w1, w2, b1, b2 = _w4(p1), _w4(p2), _shift(p1), _shift(p2)

    def net(B):
        v = B.input(xs)
        y1 = B.conv(v, w1, b1, 9 * c, 1, 1, 1, inter=True, packed=packed)
        return B.conv(y1, w2, b2, 9 * c, 1, 1, 1, res=xs, packed=packed, final=True)
    return dict(net=net, p1=p1, p2=p2, x=xs.to(dt))


def _dsblock(case, mode, device):
    """relu(conv2(round(relu(conv1/s2(x)))) + ds(x)): the shortcut is "four more k-groups into conv2's accumulators ... never rounded to
    bf16 on its own" (basicblock.hip), so K = 9 * 128 + 64"""
    a, dt = case.a, torch.bfloat16
    t1, t2 = _signs("cb.ds.t1", 128), _signs("cb.ds.t2", 128)
    w1, w2, wd = _coherent_w("cb.ds.w1", 128, 64, 3, t1), _coherent_w("cb.ds.w2", 128, 128, 3, t2, t1), _coherent_w("cb.ds.wd", 128, 64, 1, t2)
    p1 = ops.ConvPlan(w1, None, bn=FakeBN(128, "cb.ds.bn1"), stride=2, pad=1, act=1, dtype=dt, device=device)
    p2 = ops.ConvPlan(w2, None, bn=FakeBN(128, "cb.ds.bn2"), stride=1, pad=1, act=1, dtype=dt, device=device)
    pd = ops.ConvPlan(wd, None, bn=FakeBN(128, "cb.ds.bnd"), stride=2, pad=0, act=0, dtype=dt, device=device)
    xs = rne(_coherent_x("cb.ds.x", _field(a["n"], a["h"], a["w"]), 64).to(F64), dt)
    k1, k2, kd = _w4(p1), _w4(p2), _w4(pd, pd.wgt_rows)
    b1, b2 = _shift(p1), _shift(p2)
    # the shortcut's own fp32 shift enters as an exact additive map, so that S holds |b2| + |bd| and not |b2 + bd|
    bd = _shift(pd)[None, :, None, None].expand(a["n"], 128, a["h"] // 2, a["w"] // 2).contiguous()

    def net(B):
        v = B.input(xs)
        y1 = B.conv(v, k1, b1, 9 * 64, 2, 1, 1, inter=True)
        return B.conv(y1, k2, b2, 9 * 128 + 64, 1, 1, 1, res=bd, extra=(v, kd, 2), final=True)
    return dict(net=net, p1=p1, p2=p2, pd=pd, x=xs.to(dt))


def _conv3_ds(case, mode, device):
    """act(conv2(y) + b2 + round(ds(x) + bd)): "a wave holds the COMPLETE shortcut sum of its tiles, rounds it (+ its bias) to the storage
    type - exactly what the separate launch stores - and adds it to its partial sum" (conv3x3.hip): the shortcut is a stage of its own
    (K = Cin2) whose interval enters the second convolution as its residual; that one's K counts the shortcut's Cin as well"""
    a, dt = case.a, torch.bfloat16
    c, cin2, n, h2, w2 = a["c"], a["cin2"], a["n"], a["h2"], a["w2"]
    ho, wo = (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1
    key = "cb.c3ds%d_%d" % (c, cin2)
    # the shortcut is the stage with an intermediate: coherent signs (above); the 3x3 on y is a plain final stage: uniform operands, as in
    # the single-stage cases, so that one product of its K = 9 C is not hidden behind a sum of equal signs
    x = rne(_coherent_x(key + ".x", _field(n, h2, w2), cin2).to(F64), dt)
    y = rne(procedural_input(key + ".y", (n, c, ho, wo), 0).to(F64), dt)
    wt2 = procedural_input(key + ".w2", (c, c, 3, 3), 0) * math.sqrt(3.0 / (9 * c))
    wd = _coherent_w(key + ".wd", c, cin2, 1, _signs(key + ".t", c)) * 0.5
    p1 = ops.ConvPlan(torch.zeros(c, cin2, 3, 3), None, bn=FakeBN(c, key + ".bn1"), stride=2, pad=1, act=1, dtype=dt, device=device)
    p2 = ops.ConvPlan(wt2, None, bn=FakeBN(c, key + ".bn2"), stride=1, pad=1, act=1, dtype=dt, device=device)
    pd = ops.ConvPlan(wd, None, bn=FakeBN(c, key + ".bnd"), stride=2, pad=0, act=0, dtype=dt, device=device)
    k2, kd, b2, bd = _w4(p2), _w4(pd, pd.wgt_rows), _shift(p2), _shift(pd)

    def net(B):
        sc = B.conv(B.input(x), kd, bd, cin2, 2, 0, 0, inter=True)
        return B.conv(B.input(y), k2, b2, 9 * c + cin2, 1, 1, 1, res=sc, final=True)
    return dict(net=net, p1=p1, p2=p2, pd=pd, x=x.to(dt), y=y.to(dt))


class _Bneck(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(128, 32, 1, bias=False), nn.BatchNorm2d(32)
        self.conv2, self.bn2 = nn.Conv2d(32, 32, 3, 1, 1, bias=False), nn.BatchNorm2d(32)
        self.conv3, self.bn3 = nn.Conv2d(32, 128, 1, bias=False), nn.BatchNorm2d(128)


def _bneck_module():
    m = _Bneck().eval()
    t1, t2, t3 = _signs("cb.bnk.t1", 32), _signs("cb.bnk.t2", 32), _signs("cb.bnk.t3", 128)
    ws = (_coherent_w("cb.bnk.w1", 32, 128, 1, t1), _coherent_w("cb.bnk.w2", 32, 32, 3, t2, t1), _coherent_w("cb.bnk.w3", 128, 32, 1, t3, t2))
    with torch.no_grad():
        for i, (conv, bn, w) in enumerate(zip((m.conv1, m.conv2, m.conv3), (m.bn1, m.bn2, m.bn3), ws)):
            conv.weight.copy_(w)
            f = FakeBN(w.shape[0], "cb.bnk.bn%d" % i)
            bn.weight.copy_(f.weight), bn.bias.copy_(f.bias), bn.running_mean.copy_(f.running_mean), bn.running_var.copy_(f.running_var)
    return m


def bottleneck_weights(plan):
    """BottleneckPlan's MFMA fragments back to (W1 (32, 128, 1, 1), W2 (32, 32, 3, 3), W3 (128, 32, 1, 1)): the inverse of the index
    maps its constructor documents"""
    lane, j = torch.arange(64), torch.arange(8)
    row, half = lane % 32, lane // 32
    g, u = torch.arange(8), torch.arange(2)
    f1, f2, f3 = (t.detach().cpu().to(F64) for t in (plan.w1, plan.w2, plan.w3))
    w1, w2, w3 = torch.zeros(32, 128, dtype=F64), torch.zeros(32, 32, 9, dtype=F64), torch.zeros(128, 32, dtype=F64)
    k1 = 16 * g[:, None, None] + 8 * half[None, :, None] + j[None, None, :]
    w1[row[None, :, None].expand(8, 64, 8), k1] = f1
    k2 = 16 * u[:, None, None] + 8 * half[None, :, None] + j[None, None, :]
    k3 = 16 * u[:, None, None] + (j & 3)[None, None, :] + 8 * (j >> 2)[None, None, :] + 4 * half[None, :, None]
    r2 = row[None, :, None].expand(2, 64, 8)
    for t in range(9):
        w2[:, :, t][r2, k2] = f2[t]
    for ct in range(4):
        w3[32 * ct:32 * ct + 32][r2, k3] = f3[ct]
    return w1.reshape(32, 128, 1, 1), w2.reshape(32, 32, 3, 3), w3.reshape(128, 32, 1, 1)


def _bneck_net(xs, ws, bs, y1=None):
    (w1, w2, w3), (b1, b2, b3) = ws, bs

    def net(B):
        v = B.input(xs)
        v1 = B.input(y1) if y1 is not None else B.conv(v, w1, b1, 128, 1, 0, 1, inter=True)
        v2 = B.conv(v1, w2, b2, 9 * 32, 1, 1, 1, inter=True)
        return B.conv(v2, w3, b3, 32, 1, 0, 1, res=xs, final=True)
    return net


def _bottleneck(case, mode, device):
    """relu(conv3(round(relu(conv2(round(relu(conv1(x))))))) + x), bf16 (bottleneck.hip)"""
    a = case.a
    m = _bneck_module()
    plan = ops.BottleneckPlan(m.conv1, m.bn1, m.conv2, m.bn2, m.conv3, m.bn3, device=device)
    xs = rne(_coherent_x("cb.bnk.x", _field(a["n"], a["h"], a["w"]), 128).to(F64), torch.bfloat16)
    bs = [t.detach().cpu().to(F64) for t in (plan.b1, plan.b2, plan.b3)]
    return dict(net=_bneck_net(xs, bottleneck_weights(plan), bs), plan=plan, x=xs.to(torch.bfloat16))


def _bottleneck_f32(case, mode, device):
    """the same block in fp32 storage (bottleneck_f32.hip), conv1 computed by the kernel or its result y1 taken from the producer (then an
    exact operand: here a CPU fp32 evaluation of relu(conv1(x)))"""
    a, f32 = case.a, torch.float32
    m = _bneck_module()
    p1 = ops.ConvPlan(m.conv1.weight, None, bn=m.bn1, act=1, dtype=f32, device=device)
    p2 = ops.ConvPlan(m.conv2.weight, None, bn=m.bn2, stride=1, pad=1, act=1, dtype=f32, device=device)
    p3 = ops.ConvPlan(m.conv3.weight, None, bn=m.bn3, act=1, dtype=f32, device=device)
    xs = _coherent_x("cb.bnk.x", _field(a["n"], a["h"], a["w"]), 128).to(F64)
    ws, bs = (_w4(p1, p1.wgt_rows), _w4(p2), _w4(p3, p3.wgt_rows)), (_shift(p1), _shift(p2), _shift(p3))
    y1 = None
    if a["with_y1"]:
        y1 = torch.relu(F.conv2d(xs.float(), ws[0].float(), bs[0].float())).to(F64)
    return dict(net=_bneck_net(xs, ws, bs, y1), p1=p1, p2=p2, p3=p3, x=xs.float(), y1=None if y1 is None else y1.float())


def _stem(case, mode, device):
    """conv 7x7 / s2 + BN + ReLU (+ max-pool 3 / 2 / 1) on the fp32 image or on uint8 frames through the (3, 256) normalisation table"""
    a, dt = case.a, store_dtype(mode)
    n, h, w = a["n"], a["h"], a["w"]
    wt = procedural_input("cb.st.w", (64, 3, 7, 7), 0) * math.sqrt(3.0 / 147)
    plan = ops.ConvPlan(wt, None, bn=FakeBN(64, "cb.st.bn"), stride=2, pad=3, act=1, dtype=dt, device=device, smallc=True)
    x8 = lut = None
    if a.get("u8"):
        x8 = (procedural_input("cb.st.x8", (n, h, w, 3), 0, 0.0, 1.0) * 255).round().clamp(0, 255).to(torch.uint8)
        lut = torch.stack([(torch.arange(256, dtype=F64) / 255 - mu) / sd for mu, sd in ((0.485, 0.229), (0.456, 0.224), (0.406, 0.225))]).float()
        x = torch.stack([lut[c][x8[..., c].long()] for c in range(3)], 1)
    else:
        x = procedural_input("cb.st.x", (n, 3, h, w), 0)
    xs, wk, shift = rne(x.to(F64), dt), _w4(plan), _shift(plan)

    def net(B):
        out = B.conv(B.input(xs), wk, shift, 147, 2, 3, 1, final=True)
        return B.pool(out) if a.get("pool") else out
    return dict(net=net, plan=plan, x=x, x8=x8, lut=lut)


BUILDERS = {"conv": _conv, "basicblock": _basicblock, "dsblock": _dsblock, "conv3_ds": _conv3_ds, "bottleneck": _bottleneck,
            "bottleneck_f32": _bottleneck_f32, "stem": _stem}


def build(case, mode, device="cpu"):
    return BUILDERS[case.kind](case, mode, device)


_REFS = {}


def reference(case, mode):
    """-> (the output's Interval (N, C, H, W), the intermediates' Intervals, the final convolution's Interval - the output's but for a
    max-pool or a PixelUnshuffle behind it), computed once per (case, mode)"""
    key = (case.name, mode)
    if key not in _REFS:
        B = Ref(mode)
        out = build(case, mode)["net"](B)
        _REFS[key] = (out.iv, B.inter, B.final)
    return _REFS[key]


def emulate(case, mode, fault=None):
    return build(case, mode)["net"](Emul(mode, fault)).mid.to(F64)


def _cases():
    out = []
    all_off = dict(USE_CONV3X3=False, USE_GEMM_ROWS=False, USE_STEM=False, USE_HEAD_CONV=False)
    ig = lambda name, **a: out.append(Case("igemm_" + name, "conv", "cobevt_conv2d_nhwc", MODES, all_off, **a))         # noqa: E731
    ig("3x3_24to40", n=2, cin=24, h=9, w=11, cout=40, k=3, pad=1, act=1)                           # the gather path, a K tail (216 of 224)
    ig("3x3s2_16to24", n=4, cin=16, h=15, w=13, cout=24, k=3, stride=2, pad=1, bias=False, bn=True, act=1, residual=True)
    ig("1x1s2_64to128", n=1, cin=64, h=16, w=16, cout=128, k=1, stride=2, bias=False, bn=True)
    ig("7x7s2_smallc", n=1, cin=3, h=32, w=32, cout=64, k=7, stride=2, pad=3, bias=False, bn=True, act=1, smallc=True)
    ig("1x1_preact_padded", n=1, cin=56, h=14, w=15, cout=128, k=1, bias=False, pre_bn=True, out_pad=(18, 24))
    ig("3x3_upsample", n=2, cin=32, h=8, w=8, cout=16, k=3, pad=1, bn=True, act=1, upsample=True)
    ig("3x3_unshuffle", n=2, cin=32, h=16, w=16, cout=8, k=3, pad=1, bias=False, store_mode=1)
    epi = dict(k=3, pad=1, bias=False, bn=True, act=1, residual=True)
    # hidden "late" at Cin 256: K = 2304 with operands of random sign puts e near one bf16 ulp of the result, and a residual added after the
    # rounding leaves the interval at a handful of elements only (4 on the CPU that wrote this) - no basis for an assertion; Cin 64 asserts it
    for cin, cout, h, w in ((64, 64, 9, 12), (256, 192, 9, 21)):
        out.append(Case("conv3_lds_%d_%d" % (cin, cout), "conv", "cobevt_conv3x3_nhwc", MODES, dict(USE_CONV3_WFRAG=False),
                        hidden=("late",) if cin == 256 else (), n=2, cin=cin, h=h, w=w, cout=cout, **epi))
    # the strip kernel: every tile variant; channel chunks are 64 (bf16) / 32 (fp32) wide, so fp32 storage takes half the channels for
    # the same 1 - 3 chunks.  128-cout tiles (variant % 10 == 0): a wave owns two k-groups per tap -> three-term / packed form
    for variant in (130, 131, 140, 141, 150, 151, 160, 161, 113, 123, 133, 143, 153):
        four_wave = variant % 10 == 3
        modes = ("bf16",) if four_wave else MODES                                                  # the four-wave 32-cout form is built for bf16 only
        packed = ("fp32_split", "fp32_fast") if variant % 10 == 0 else ()
        for i, (nch, h, w, cout, kw) in enumerate([(1, 19, 37, 32 if four_wave else 160, dict(bn=True, act=1, residual=True)),
                                                   (3, 9, 12, 72 if four_wave else 160, dict(bias=False, upsample=True, act=1)),
                                                   (2, 12, 20, 24 if four_wave else 160, dict(bias=False, store_mode=1))]):
            out.append(Case("strips_v%d_%d" % (variant, i), "conv", "cobevt_conv3x3_wfrag_nhwc", modes, dict(CONV3_VARIANT=variant), packed=packed,
                            n=1 if i == 0 else 2, cin=64 * nch, cin_fp32=32 * nch, h=h, w=w, cout=cout, k=3, pad=1, **kw))
    # stride 2 through the strip kernel; the second library routes these to the implicit GEMM (ops.conv_route), so no fp32_split
    for cin, cout, h, w in ((64, 128, 17, 37), (64, 64, 9, 64)):
        out.append(Case("strips_s2_%d_%d" % (cin, cout), "conv", "cobevt_conv3x3_wfrag_nhwc", ("bf16", "fp32", "fp32_fast"), {},
                        packed=("fp32_fast",) if cout > 64 else (), n=2, cin=cin, h=h, w=w, cout=cout, stride=2, **epi))
    for variant in (130, 131, 140, 141, 150, 151):
        # (256, 256): K = 9 * 256 + 256 = 2560 with operands of random sign puts e at two bf16 ulps of the result (median e / |ref| 8.8e-3),
        # so a term added after the rounding or an unrounded shortcut stays inside; the kernel's four-chunk limits are reached at fewer channels by (64, 256),
        # K = 832, where every fault is seen
        for c, cin2, n, h2, w2 in ((128, 64, 1, 19, 37), (256, 256, 1, 12, 12), (64, 256, 2, 15, 21)):
            out.append(Case("conv3_ds_v%d_%d_%d" % (variant, c, cin2), "conv3_ds", "cobevt_conv3x3_ds_wfrag_nhwc", ("bf16",), dict(CONV3_VARIANT=variant),
                            hidden=("late", "unrounded") if c == 256 else (), variant=variant, c=c, cin2=cin2, n=n, h2=h2, w2=w2))
    out.append(Case("stem_38x50", "stem", "cobevt_stem_conv7x7s2", MODES, n=1, h=38, w=50))
    out.append(Case("stem_pool_36x52", "stem", "cobevt_stem_conv7x7s2_pool", MODES, n=1, h=36, w=52, pool=True))
    out.append(Case("stem_pool_u8_36x52", "stem", "cobevt_stem_conv7x7s2_pool_u8", MODES, n=1, h=36, w=52, pool=True, u8=True))
    # hidden "unrounded": an intermediate kept unrounded moves the next stage's sum by a random walk of its K roundings, about
    # sqrt(K) 2^-9 |x||w|, while that stage's own e is K 2^-23 S ~ K^2 2^-23 |x||w|: the ratio 2^14 / K^1.5 is 1.2 at K = 576 and 0.4 at
    # K = 1152, and a move smaller than e crosses a rounding boundary only where the interval is open.  The kernels fix K there
    # (128-channel BasicBlock: 9 * 128; layer2's block: 9 * 128 + 64), so fault (c) is asserted for the 64-channel block only
    for c, n, h, w in ((64, 1, 13, 21), (128, 2, 9, 35)):
        out.append(Case("basicblock_%d" % c, "basicblock", "cobevt_basicblock_nhwc", MODES, packed=("fp32_split", "fp32_fast"),
                        hidden=() if c == 64 else ("unrounded",), c=c, n=n, h=h, w=w))
    out.append(Case("dsblock_26x44", "dsblock", "cobevt_dsblock_nhwc", ("bf16",), hidden=("unrounded",), n=1, h=26, w=44))
    out.append(Case("dsblock_2x2", "dsblock", "cobevt_dsblock_nhwc", ("bf16",), stat=False, hidden=("unrounded", "late"), n=1, h=2, w=2))   # one output pixel: 128 values, too few for "late" (5 leave)
    for rows in (0, 8, 16):
        out.append(Case("bottleneck_r%d_21x37" % rows, "bottleneck", "cobevt_bottleneck_nhwc", ("bf16",), n=1, h=21, w=37, tile_rows=rows))
        out.append(Case("bottleneck_r%d_5x3" % rows, "bottleneck", "cobevt_bottleneck_nhwc", ("bf16",), stat=False, n=1, h=5, w=3, tile_rows=rows))
    for with_y1 in (False, True):
        for h, w in ((21, 37), (5, 3)):
            out.append(Case("bottleneck_f32_%s_%dx%d" % ("y1" if with_y1 else "x", h, w), "bottleneck_f32", "cobevt_bottleneck_f32_nhwc",
                            ("fp32", "fp32_split", "fp32_fast"), n=1, h=h, w=w, with_y1=with_y1))
    # the direct head kernel keeps its weights in fp32 in both storage types (plan.wgt_head) and stores fp32 NCHW; one pixel's channels fit
    # 256 bytes, so fp32 storage takes 64 input channels where bf16 takes 128.  postprocess.hip is no per-library source: bf16 and fp32
    for cout, cin, cin32, n, h, w in ((3, 32, 32, 2, 37, 21), (4, 128, 64, 1, 20, 33), (1, 64, 64, 1, 23, 9), (2, 32, 32, 1, 5, 18)):
        out.append(Case("head_%dx%d" % (cout, cin), "conv", "cobevt_conv3x3_head_nchw", ("bf16", "fp32"), stat=False, n=n, cin=cin, cin_fp32=cin32,
                        h=h, w=w, cout=cout, k=3, pad=1, store_mode=2, head=True))
    # 1x1 / stride 1 (a Linear: rows as a (1, 1, rows, K) map) on the 32-row kernel and on the 128 x 128 dense-row kernel
    for entry, kn in (("cobevt_linear_rows_small_k", {}), ("cobevt_linear_rows", dict(USE_GEMM_ROWS3=False, USE_GEMM_ROWS3_F32=False))):
        for kk, nn_, rows, kw in ((32, 128, 257, dict(residual=True)), (128, 96, 130, dict(act=1)), (256, 128, 257, dict())):
            out.append(Case("%s_%d_%d" % (entry[len("cobevt_linear_"):], kk, nn_), "conv", entry, MODES, kn, n=1, cin=kk, h=1, w=rows, cout=nn_, k=1,
                            rows=True, **kw))
    return out


CASES = _cases()
CASE_MODES = [(c, m) for c in CASES for m in c.modes]


def case_id(cm):
    return "%s-%s" % (cm[0].name, cm[1])
