"""Float64 interval reference of the row-local kernels (tests/test_rows_bounds.py on the CPU, tests/test_rows_bounds_gpu.py on the device).

The machinery is conv_bounds_ref's: a row map (M, K) is the (1, K, 1, M) map its table already uses for
linear_rows, every GEMM is Ref.conv with a 1 x 1 kernel and contraction length K (same S, same e = K 2^-23 S + 2^-23 |pre| + the mode
term of csrc/f32_matrix.hpp, unpacked form: none of these kernels takes the three-term / packed form), and every network is written
once against a backend, RowsRef (the intervals) or RowsEmul (a correct kernel on the CPU, which also injects the faults).  This file
adds the three stages the family has and the convolutions have not.  U = 2^-23 throughout: one ulp of fp32, twice the unit roundoff,
so "one rounding" below is a relative U whether the kernel contracts an fma or not.

normalise(v, eps) - rc_normalise of row_chain.hip and its copies in row_chain64 / row_chain_f32 / proj_chain128 / proj_chain_k /
ln_linear64 / gemm_rows3*.hip:  mu = sum x / C,  d_i = x_i - mu,  q = sum d_i^2,  r = rsqrtf(q / C + eps),  x^_i = d_i r,  no affine.
  (a) the input's half-width delta (|Dx_i| <= delta_i).  The Jacobian is  dx^_i/dx_j = r (1[i = j] - 1/C) - x^_i x^_j r / C,  so to
      first order |Dx^_i| <= r (delta_i + mean delta) + |x^_i| r mean_j(|x^_j| delta_j).  The remainder is bounded, not dropped: by the
      mean value theorem Dx^_i = grad x^_i(xi) . Dx at some point xi of the box, so it is enough to bound the Jacobian over the box.
      There d_j moves by at most eta_j = delta_j + mean delta, the rms of d by at most s = rms(eta), and sigma = sqrt(rms^2 + eps)
      is 1-Lipschitz in the rms, so with t = r s (asserted < 1/4):  r(xi) <= R = r / (1 - t),  |x^_j(xi)| <= X_j = (|x^_j| + r eta_j) / (1 - t)
      and   |Dx^_i| <= R (delta_i + mean delta) + X_i R mean_j(X_j delta_j).
  (b) the fp32 evaluation, at any point of the box (|x_i| <= |x_i| + delta_i, |d_i| <= D_i = |d_i| + eta_i, r <= R).  The sum of C terms in
      ANY order: C U mean|x| on mu; ONE rounding of the mean: U |mu| - which costs U |mu| R on every x^ of the row, the term that rows
      far from zero pay; the subtraction: |Dd_i| <= dd_i = Dmu + U (D_i + Dmu).  q: the perturbed squares mean(2 D dd + dd^2), their C
      roundings and the C-term sum, the division and the addition of eps: a relative rho on q / C + eps, measured against its lower
      bound (sigma - s)^2; r: rho / 2 (1 - rho)^-3/2 + U for a v_rsq_f32 of 1 ulp; the product: one more U.  Together
          e_fp_i = R ((D_i + dd_i) (1 + rho_r) (1 + U) - D_i).
  The result is closed (rounded to the storage type) wherever the kernel stores it in that type, else it travels as (x^, e).
ln_affine - the post-LayerNorm's x^ g + b:  |g| e (1 + 2 U) + U |x^ g| + U |pre|, two roundings, which covers both contraction choices.
pre_affine / relu - conv_bounds_ref's affine (the pre-activation BatchNorm -> ReLU of the projection chains), unchanged.

gelu(v) - bf16 kernels: gelu_bf16 of csrc/common.hpp, whose comment documents |error| <= 6.2e-5 against x Phi(x) for x >= -8 (below: the
  result is below 1e-9 in magnitude, and so is x Phi(x)) and <= 0.38 of 2^-9 max(|gelu|, 0.01); fp32 kernels: gelu_erf over erf_as,
  |erf error| <= 1.5e-7, i.e. 0.75e-7 |x| on the GELU.  tests/test_rows_bounds.py scans both formulas in float64, exactly as written, and
  asserts these constants.  e of the stage = the documented term (the smaller of the two bf16 ones) + L e_in with L = |gelu'(p)| + 0.8 e_in
  (|gelu''| = phi(x) |2 - x^2| <= 2 phi(0) < 0.8: the remainder again explicit) + the fp32 evaluation of the formula as written: every
  fma / multiply / add one U, and v_exp_f32, v_rcp_f32 (and v_rsq_f32 above) taken as 1 ulp each.  That 1-ulp figure is AMD's
  documented accuracy of the three instructions; NOBODY HAS CHECKED IT IN THIS PROJECT - the `used` figure the GPU file prints
  (max |got - ref| / e on fp32 stores) shows what the kernels leave of it.  The evaluation term is taken at both ends and the middle
  of the incoming interval (and at 0 where it holds 0: s (1 - s) peaks there).

mean_rows - cobevt_mean_linear_rows_small_k: a stage of its own with K = L: (L - 1) U sum|x| / L for the sequential sum, 2 U |mean| for the
  rounded reciprocal and the product; L = 1 is exact (the kernel has no averaging code on that path).

Cutting the chain at HBM: row_chain.hip's phase F feeds the next projection "`out` rows exactly as stored", so the reference of out_next
starts from the tensor the kernel wrote to `out`, as an exact operand (next_reference) - valid only after that tensor passed its own
interval test, which the GPU test asserts first.  The propagated width is one chain's, not two.

Width control: with K = 128 and operands of random sign about 4 % of y = a Wp^T + bp + skip would straddle a bf16 boundary.  The bf16
cases put the projection's operands on dyadic grids (a on 1/2, Wp in {0, +-1/8}, bp and skip on 1/16 and 1/8; the builder asserts that
y is exactly representable wherever |y| > 2^10 e - most of it, K = 512 included), so the width starts at the first LayerNorm; test_rows_bounds.py checks for every bf16 case that the
median of (hi - lo) / |ref| is <= 2^-6 and that at most 5 % of the elements are wider than 2^-5 |ref| + 2^-8 max|ref|.

The operands are the plan's: weights and biases are read back from plan.wgt_rows / plan.bias with the LayerNorm affine already folded by
ConvPlan (W' = W g, b' = b + W beta), the convention of section 3t.  An error in the folding is invisible to the intervals;
test_rows_bounds.py::test_layernorm_folding_of_the_plans checks it on its own against a float64 fold.

Left out, by name:
  bev_embed / bev_query (gemm_rows3_kernel<true, 32>, bev_query_kernel<4>): the embedding's geometry needs another reference;
      test_bev_query_wave_level_kernel stays.
  swap_stage.hip: it has an attention inside.  The attention bound it was waiting for now exists for the backward kernels (DESIGN.md
      section 3z, tests/attn_bwd_ref.py); the forward families, this one among them, are still without one.
  swish and sigmoid epilogues (act 3, 4): no derivation yet.
  row_chain64_kernel<NNT, 6, true> and <NNT, 6, false> (NNT 0, 2, 4, 6): reached only through COBEVT_RC64_PREFETCH, an environment gate
      read once per process.
  row_chain_f32_kernel behind a post-LayerNorm in the third library ("fp32_fast"): no bound exists (the table's comment has the figures).
  a broadcast residual of cobevt_proj_chain: ops.proj_chain always passes skip_rows = 0, the C entry is not reachable with another value.
"""
import math

import torch

from cobevt_amd import ops
from cobevt_amd.synth import procedural_input
from conv_bounds_ref import (Ref, Emul, V, Interval, rne, bias_stat, position, outside, error_over_e, knobs, Case,  # noqa: F401
                             U, F64, LIB, BIAS_LIMIT, BIAS_MIN_N, store_dtype, truncate_bf16)

BF16, F32 = torch.bfloat16, torch.float32
F32_MODES = ("fp32", "fp32_split", "fp32_fast")
GELU_BF16_ABS, GELU_BF16_REL, GELU_BF16_FLOOR, GELU_BF16_TAIL = 6.2e-5, 0.38, 0.01, 1e-9       # csrc/common.hpp, the comment of gelu_bf16
ERF_AS_ABS = 1.5e-7                                                                          # ... of erf_as
SQRT1_2 = 0.70710678118654752440


def rows4(t):
    """(M, K) -> (1, K, 1, M)"""
    return t.t()[None, :, None, :].contiguous()


def rows2(t):
    """(1, K, 1, M) -> (M, K)"""
    return t[0, :, 0, :].t().contiguous()


# ----------------------------------------------------------------------------------------------
# the two GELU formulas of csrc/common.hpp, exactly as written, in the dtype of x (float64: the scan; float32: the emulator)
# ----------------------------------------------------------------------------------------------
def gelu_exact(x):
    """x Phi(x) in float64 (erfc keeps the negative tail)"""
    return 0.5 * x * torch.special.erfc(-x * SQRT1_2)


def gelu_prime(x):
    return 0.5 * torch.special.erfc(-x * SQRT1_2) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_bf16_formula(x):
    xc = x.clamp(-8.0, 8.0)
    u = xc * xc
    w = u * 0.0011102325515821576 + -0.10751112550497055
    w = w * u + -2.3001456260681152
    return x * (1.0 / (1.0 + torch.exp2(xc * w)))


def erf_as_formula(x):
    ax = x.abs()
    t = 1.0 / (0.3275911 * ax + 1.0)
    poly = 1.061405429 * t + -1.453152027
    poly = poly * t + 1.421413741
    poly = poly * t + -0.284496736
    poly = poly * t + 0.254829592
    e = torch.exp2(-ax * ax * 1.4426950408889634)
    return torch.copysign(-poly * t * e + 1.0, x)


def gelu_erf_formula(x):
    return 0.5 * x * (1.0 + erf_as_formula(x * SQRT1_2))


def _fp_gelu_bf16(x):
    """bound of the fp32 evaluation of gelu_bf16 at x (float64)"""
    xc = x.clamp(-8.0, 8.0)
    u = xc * xc
    du = U * u
    w1 = u * 0.0011102325515821576 - 0.10751112550497055
    dw1 = 0.0011102325515821576 * du + U * w1.abs()
    w2 = w1 * u - 2.3001456260681152
    dw2 = dw1 * u + w1.abs() * du + U * w2.abs()
    arg = xc * w2
    darg = xc.abs() * dw2 + U * arg.abs()
    s = 1.0 / (1.0 + torch.exp2(arg))
    kappa = math.log(2.0) * darg * (1.0 + math.log(2.0) * darg) + U
    return x.abs() * s * ((1.0 - s) * kappa + 3.0 * U)


def _fp_gelu_erf(x):
    """bound of the fp32 evaluation of gelu_erf at x (float64)"""
    xs = x * SQRT1_2
    ax = xs.abs()
    dxs = 1.5 * U * ax
    den = 0.3275911 * ax + 1.0
    t = 1.0 / den
    dt = t * (2.0 * U + 0.3275911 * dxs / den)
    poly = (((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592
    dpoly = 4.0 * 4.476 * U + 11.7 * dt             # four fmas on partial sums below sum|c| = 4.476; |poly'| <= 11.7 on [0, 1]
    arg = ax * ax * 1.4426950408889634
    darg = 3.0 * U * arg + 2.0 * ax * dxs * 1.4426950408889634
    e = torch.exp2(-arg)
    kappa = math.log(2.0) * darg * (1.0 + math.log(2.0) * darg) + U
    pt = poly * t
    dpt = dpoly * t + poly.abs() * dt + U * pt.abs()
    y = 1.0 - pt * e
    dy = dpt * e + pt.abs() * e * kappa + U * y.abs()
    g = 0.5 * x.abs() * (1.0 + y)
    return 0.5 * x.abs() * (dy + U * (1.0 + y.abs())) + U * g


# ----------------------------------------------------------------------------------------------
# LayerNorm without affine: the float64 bound and an fp32 evaluation in several summation orders
# ----------------------------------------------------------------------------------------------
def normalise_bound(x, dl, eps):
    """x, dl (rows, C) float64: the mid-points and half-widths -> (x^, e): the module docstring's (a) + (b)"""
    C = x.shape[1]
    mu = x.mean(1, keepdim=True)
    d = x - mu
    var = (d * d).mean(1, keepdim=True)
    sig = torch.sqrt(var + eps)
    r = 1.0 / sig
    xh = d * r
    mdl = dl.mean(1, keepdim=True)
    eta = dl + mdl
    s = torch.sqrt((eta * eta).mean(1, keepdim=True))
    t = r * s
    assert float(t.max()) < 0.25, "the incoming interval is as wide as the row's spread: %.3f" % float(t.max())
    R = r / (1.0 - t)
    X = (xh.abs() + r * eta) / (1.0 - t)
    prop = R * eta + X * R * (X * dl).mean(1, keepdim=True)
    av = (x.abs() + dl).mean(1, keepdim=True)
    dmu = C * U * av + U * (mu.abs() + mdl)
    D = d.abs() + eta
    dd = dmu + U * (D + dmu)
    m2 = (2.0 * D * dd + dd * dd).mean(1, keepdim=True)
    var_up = (D * D).mean(1, keepdim=True) + m2
    dv = m2 + (C + 2.0) * U * var_up + U * (var_up + eps)
    rho = dv / (sig - s) ** 2
    assert float(rho.max()) < 0.01
    rho_r = 0.5 * rho / (1.0 - rho) ** 1.5 + U
    e_fp = R * ((D + dd) * (1.0 + rho_r) * (1.0 + U) - D)
    return xh, prop + e_fp


def _sum32(t, order):
    """fp32 sum over the last axis: 0 torch's pairwise sum, 1 left to right, 2 right to left, 3 the kernels' (8 lanes of consecutive
    runs, each left to right, then a butterfly over the lanes)"""
    if order == 0:
        return t.sum(-1, keepdim=True)
    if order == 1:
        return t.cumsum(-1)[..., -1:]
    if order == 2:
        return t.flip(-1).cumsum(-1)[..., -1:]
    c = t.shape[-1]
    pad = (-c) % 8
    tt = torch.nn.functional.pad(t, (0, pad)).reshape(t.shape[:-1] + (8, (c + pad) // 8))
    lanes = tt.cumsum(-1)[..., -1]
    for step in (1, 2, 4):
        lanes = lanes + lanes[..., torch.arange(8) ^ step]
    return lanes[..., :1]


def normalise_f32(x, eps, order=0):
    """x (rows, C) fp32 -> rc_normalise in fp32"""
    c = x.shape[-1]
    mean = _sum32(x, order) / torch.tensor(float(c), dtype=F32)
    d = x - mean
    q = _sum32(d * d, order)
    return d * torch.rsqrt(q / torch.tensor(float(c), dtype=F32) + torch.tensor(eps, dtype=F32))


# ----------------------------------------------------------------------------------------------
# backends
# ----------------------------------------------------------------------------------------------
class RowsRef(Ref):
    def gemm(self, v, w, b, act=0, res=None, raw=False, inter=False, final=False, tag=None, pad=None):
        """w (N, K) float64 as the plan stores it, b (N,) or None, res a V or an exact map.  raw: the fp32 accumulator travels on
        (mid = ref, d = e); else it is closed in the storage type behind act (0 none, 1 ReLU)"""
        shift = torch.zeros(w.shape[0], dtype=F64) if b is None else b
        out = self.conv(v, w[:, :, None, None], shift, w.shape[1], 1, 0, act, res=res, inter=inter and not raw, dt=F32 if raw else None,
                        final=final and not raw)
        if raw:
            return V(out.iv.ref, out.iv.e, out.iv)
        return out

    def rows_index(self, m, skip_rows, tile):
        return torch.arange(m) % skip_rows

    def store(self, v, final=True):
        iv = Interval(v.mid, None, v.d, rne(v.mid - v.d, self.dt), rne(v.mid + v.d, self.dt))
        if final:
            self.final = iv
        return V((iv.lo + iv.hi) / 2, (iv.hi - iv.lo) / 2, iv)

    def normalise(self, v, eps, store, slot=None):
        xh, e = normalise_bound(rows2(v.mid), rows2(v.d), eps)
        out = V(rows4(xh), rows4(e))
        if not store:
            return out
        out = self.store(out, final=False)
        self.inter.append(out.iv)
        return out

    def ln_affine(self, v, g, b):
        g, b = g.to(F64)[None, :, None, None], b.to(F64)[None, :, None, None]
        pre = v.mid * g + b
        return self.store(V(pre, g.abs() * v.d * (1.0 + 2.0 * U) + U * (v.mid * g).abs() + U * pre.abs()))

    def gelu(self, v, final=False):
        p, ein = v.mid, v.d
        ref = gelu_exact(p)
        prop = (gelu_prime(p).abs() + 0.8 * ein) * ein
        pts = [p - ein, p, p + ein, torch.where((p.abs() <= ein), torch.zeros_like(p), p)]
        if self.dt == BF16:
            approx = torch.minimum(torch.full_like(p, GELU_BF16_ABS), GELU_BF16_REL * 2.0 ** -9 * (ref.abs() + prop).clamp_min(GELU_BF16_FLOOR))
            fp = torch.stack([_fp_gelu_bf16(q) for q in pts]).max(0).values
        else:
            approx = 0.5 * ERF_AS_ABS * (p.abs() + ein)
            fp = torch.stack([_fp_gelu_erf(q) for q in pts]).max(0).values
        out = self.store(V(ref, approx + prop + fp), final=final)
        if not final:
            self.inter.append(out.iv)
        return out

    def mean_rows(self, x):
        """x (L, M, K) exact -> the fp32 mean over L as (mid, e)"""
        L = x.shape[0]
        m = x.mean(0)
        e = torch.zeros_like(m) if L == 1 else (L - 1.0) * U * x.abs().sum(0) / L + 2.0 * U * m.abs()
        return V(rows4(m), rows4(e))


FAULTS = ("drop", "eps", "skip_shift", "late", "pad", "trunc")


class RowsEmul(Emul):
    """a correct kernel on the CPU (fp32 torch on the same operands, one round-to-nearest-even per stored stage, the GELU formula of
    common.hpp in fp32), or one with `fault`:
      drop        one product missing: fc2's (tag "fc2") / the only GEMM's (tag "lin") on the last row of the map; the next projection's
                  (tag "next") in its last 128-column pass.  These are the most visible forms of "one product missing": the operand
                  dropped is the row's LARGEST (behind a GELU the last non-zero one, which conv_bounds_ref drops, is next to 0 as
                  often as not), and the next projection loses its product on every row of the pass - the shares the CPU file
                  prints say that a lost product of typical-to-large size is seen, not how small a one would be
      eps:<slot>  1e-5 in the LayerNorm slot "1" / "post" / "next" / "ln" where the case passes another eps
      skip_shift  skip[(m + 1) % skip_rows] for the rows of the second tile
      late        b2 (tag "fc2": no post-LayerNorm behind it; "fc2p" with one, where nothing is rounded in between) / the bias (tag "lin", no
                  GELU behind it) added after the rounding
      pad         the hidden columns [Hd, Hdp) the last k-group reads hold GELU(b1[j - Hd]) and meet W2[:, j - Hd] (a pad that aliases
                  live entries: against the zero pad the plans write, a non-zero hidden pad column alone changes nothing)
      trunc       the final bf16 store truncates
    order: the summation order of the LayerNorm sums (_sum32)"""

    def __init__(self, mode, fault=None, order=0):
        super().__init__(mode, fault)
        self.order, self.late = order, None

    def _store(self, y, final=False):
        if self.late is not None and final:
            y, self.late = self._rnd(y, self.dt) + self.late, None
            return V(y)
        if final and self.fault == "trunc":
            assert self.dt == BF16
            return V(truncate_bf16(y))
        return V(self._rnd(y, self.dt))

    def gemm(self, v, w, b, act=0, res=None, raw=False, inter=False, final=False, tag=None, pad=None):
        w4 = w.float()[:, :, None, None]
        acc = self._mm(v.mid, w4, 1, 0, False)
        x2 = v.mid[0, :, 0, :]                         # (K, M)
        if self.fault == "drop" and tag in ("fc2", "fc2p", "lin"):
            k = int(x2[:, -1].abs().argmax())           # (the row's largest operand: behind a GELU many are next to 0, a void fault)
            acc[0, :, 0, -1] -= x2[k, -1] * w.float()[:, k]
        if self.fault == "drop" and tag == "next":
            c0 = (w.shape[0] - 1) // 128 * 128
            acc[0, c0:, 0, :] -= w.float()[c0:, -1:] * x2[-1:, :]
        if self.fault == "pad" and tag in ("fc2", "fc2p") and pad is not None:
            b1, n = pad
            g = self.gelu_f32(b1.float()[:n])
            acc[0, :, 0, :] += (w.float()[:, :n] * self._rnd(g, self.dt)[None, :]).sum(1, keepdim=True)
        y = acc
        late = self.fault == "late" and b is not None and (tag == "fc2" or (tag == "lin" and not raw))
        if b is not None and not late:
            y = y + b.float()[None, :, None, None]
        if res is not None:
            y = y + (res.mid if isinstance(res, V) else res.float())
        if late:
            self.late = b.float()[None, :, None, None]
        if raw:
            return V(y)
        y = torch.relu(y) if act == 1 else y
        return self._store(y, final)

    def rows_index(self, m, skip_rows, tile):
        idx = torch.arange(m) % skip_rows
        if self.fault == "skip_shift":
            second = (torch.arange(m) >= tile) & (torch.arange(m) < 2 * tile)
            idx = torch.where(second, (torch.arange(m) + 1) % skip_rows, idx)
        return idx

    def store(self, v, final=True):
        return self._store(v.mid, final)

    def normalise(self, v, eps, store, slot=None):
        if self.fault == "eps:%s" % slot:
            eps = 1e-5
        y = rows4(normalise_f32(rows2(v.mid), eps, self.order))
        return self._store(y) if store else V(y)

    def ln_affine(self, v, g, b):
        return self._store(v.mid * g.float()[None, :, None, None] + b.float()[None, :, None, None], True)

    def gelu_f32(self, x):
        return gelu_bf16_formula(x) if self.dt == BF16 else gelu_erf_formula(x)

    def gelu(self, v, final=False):
        return self._store(self.gelu_f32(v.mid), final)

    def mean_rows(self, x):
        x = x.float()
        acc = x[0].clone()
        for l in range(1, x.shape[0]):
            acc += x[l]
        if x.shape[0] > 1:
            acc = acc * (torch.tensor(1.0, dtype=F32) / torch.tensor(float(x.shape[0]), dtype=F32))
        return V(rows4(acc))


# ----------------------------------------------------------------------------------------------
# operands
# ----------------------------------------------------------------------------------------------
class _LN(object):
    def __init__(self, key, c, eps):
        self.weight = 0.8 + 0.4 * procedural_input(key + ".g", (c,), 0, 0, 1)
        self.bias = procedural_input(key + ".b", (c,), 0, -0.2, 0.2)
        self.eps = eps


def _grid(key, shape, lo, hi, step):
    return torch.round(procedural_input(key, shape, 0, lo, hi) / step) * step


def _sparse_w(key, n, k, keep):
    """(n, k) weights in {0, +-1/8}: about `keep` of them non-zero"""
    u = procedural_input(key, (n, k), 0)
    return torch.where(u.abs() < keep, torch.sign(u) * 0.125, torch.zeros_like(u))


def _uniform_w(key, n, k, scale=1.0):
    return procedural_input(key, (n, k), 0) * math.sqrt(3.0 / k) * scale


def _w(plan, k):
    return plan.wgt_rows.detach().cpu()[:, :k].to(F64)


def _b(plan):
    return None if plan.bias is None else plan.bias.detach().cpu().to(F64)


def _exact(iv, what):
    nz = iv.e < 2.0 ** -10 * iv.ref.abs()            # (a value below 2^10 e keeps an open interval: bf16 is dense towards 0)
    assert float(nz.double().mean()) > 0.5
    # (behind a ReLU a 0 of the pre-activation map is the interval [0, round(e)], whose mid-point moves ref by less than e)
    assert torch.equal(iv.lo[nz], iv.hi[nz]) and bool(((iv.lo - iv.ref).abs() <= iv.e)[nz].all()), "%s: the dyadic operands do not give a representable map" % what


SMALL = 2.0 ** -7          # small-variance cases: every operand of y (and of z) scaled by this, the row variance about 1e-4


def _chain(case, mode, device):
    """cobevt_attn_mlp_chain: y = a Wp^T (+ bp) (+ skip[m % skip_rows]); z = y + fc2(GELU(fc1(normalise(y)))); out = postLN?(z);
    next = act(normalise?(out) Wn'^T + bn') from `out` as stored"""
    a_, dt = case.a, store_dtype(mode)
    M, C, Hd, Nn, batch = a_["M"], a_["C"], a_["Hd"], a_.get("Nn", 0), a_.get("batch", 1)
    eps = a_.get("eps", 1e-5)
    sc = SMALL if a_.get("small") else 1.0
    key = "rb." + case.name
    rows = M // batch
    if dt == BF16:
        a = _grid(key + ".a", (M, C), -2, 2, 0.5) * sc
        wp = _sparse_w(key + ".wp", C, C, 0.5)
        bp = _grid(key + ".bp", (C,), -0.2, 0.2, 1.0 / 16) * sc if a_.get("bp") else None
        sk = _grid(key + ".s", (rows if batch > 1 else M, C), -1, 1, 0.125) * sc if a_.get("skip", True) else None
    else:
        off = a_.get("offset", 0.0)
        a = procedural_input(key + ".a", (M, C), 0, -2, 2) * sc
        wp = _uniform_w(key + ".wp", C, C)
        bp = procedural_input(key + ".bp", (C,), 0, -0.2, 0.2) * sc if a_.get("bp") else None
        sk = (procedural_input(key + ".s", (rows if batch > 1 else M, C), 0, -1, 1) * sc + off) if a_.get("skip", True) else None
    ln1, lnn = _LN(key + ".ln1", C, eps), _LN(key + ".lnn", C, eps)
    pp = ops.ConvPlan(wp, bp, dtype=dt, device=device)
    p1 = ops.ConvPlan(_uniform_w(key + ".w1", Hd, C), procedural_input(key + ".b1", (Hd,), 0, -0.2, 0.2), act=2, dtype=dt, device=device, ln=ln1)
    # (bf16: fc2 at half the usual scale - every hidden value on a rounding boundary widens z by |w2| half an ulp of it)
    p2 = ops.ConvPlan(_uniform_w(key + ".w2", C, Hd, sc * (0.5 if dt == BF16 else 1.0)), procedural_input(key + ".b2", (C,), 0, -0.2, 0.2) * sc, dtype=dt, device=device)
    pn = None
    if Nn:
        pn = ops.ConvPlan(_uniform_w(key + ".wn", Nn, C), procedural_input(key + ".bn", (Nn,), 0, -0.2, 0.2), act=a_.get("next_act", 0), dtype=dt,
                          device=device, ln=lnn if a_.get("next_ln") else None)
    post = None
    if a_.get("post"):
        post = (0.8 + 0.4 * procedural_input(key + ".g2", (C,), 0, 0, 1), procedural_input(key + ".be2", (C,), 0, -0.2, 0.2), eps)
    a64 = rne(a.to(F64), dt)
    sk64 = None if sk is None else rne(sk.to(F64), dt)
    skip_rows = rows if (batch > 1 and sk is not None) else M
    tile = 64 if case.knobs.get("ROW_CHAIN_ROWS") == 64 else 32
    ws = [(_w(p, p.K), _b(p)) for p in (pp, p1, p2)]
    hdp = p2.kp_rows
    npad = 0 if Hd == hdp else (min(hdp, (Hd + 15) // 16 * 16) - Hd if Hd <= 128 else hdp - Hd)

    def net(B):
        res = None if sk64 is None else rows4(sk64[B.rows_index(M, skip_rows, tile)])
        y = B.gemm(B.input(rows4(a64)), ws[0][0], ws[0][1], res=res, inter=True, tag="proj")
        if dt == BF16 and isinstance(B, RowsRef):
            _exact(y.iv, case.name)
        xh = B.normalise(y, eps, True, slot="1")
        h = B.gelu(B.gemm(xh, ws[1][0], ws[1][1], raw=True, tag="fc1"))
        z = B.gemm(h, ws[2][0], ws[2][1], res=y, raw=True, tag="fc2" if post is None else "fc2p", pad=(ws[1][1], npad) if npad else None)
        if post is None:
            return B.store(z)
        return B.ln_affine(B.normalise(z, eps, False, slot="post"), post[0], post[1])

    def next_net(B, out):
        """out: (M, C) float64, the chain's output as stored"""
        v = B.input(rows4(out))
        if pn.has_ln:
            v = B.normalise(v, eps, True, slot="next")
        wn, bn = _w(pn, C), _b(pn)
        if pn.act == 2:
            return B.gelu(B.gemm(v, wn, bn, raw=True, tag="next"), final=True)
        return B.gemm(v, wn, bn, act=pn.act, final=True, tag="next")
    skd = None
    if sk is not None:
        skd = sk64.to(dt).to(device)
        skd = skd[None].expand(batch, rows, C) if batch > 1 else skd
    ad = a64.to(dt).to(device)
    return dict(net=net, next_net=next_net if Nn else None, a=ad.reshape(batch, rows, C) if batch > 1 else ad, skip=skd, plans=(pp, p1, p2), post=post, pn=pn,
                slots=["1"] + (["post"] if post else []) + (["next"] if Nn and a_.get("next_ln") else []), npad=npad)


def _pre_affine(plan, k, relu, scale=1.0):
    """dyadic pre-activation scale / shift written over the plan's (the BatchNorm's own are of no interest here): scale in {1, 2},
    shift on the 1/2 grid, so that the affine of a dyadic map is exact"""
    sc = 2.0 ** torch.round(procedural_input("rb.pre.sc%d" % k, (k,), 0, -0.4, 1.4))
    sh = _grid("rb.pre.sh%d" % k, (k,), -1, 1, 0.5) * scale             # (a power of two: ReLU(s (x sc + sh)) = s ReLU(x sc + sh), still exact)
    plan.pre_scale.copy_(sc.to(plan.pre_scale.device))
    plan.pre_shift.copy_(sh.to(plan.pre_shift.device))
    return sc.to(F64), sh.to(F64)


class _BN(object):
    def __init__(self, c):
        self.weight, self.bias, self.running_mean, self.running_var, self.eps = torch.ones(c), torch.zeros(c), torch.zeros(c), torch.ones(c), 1e-5


def _proj_side(key, K, M, Nn, pre, relu, res, next_ln, next_act, eps, device, keep, sc=1.0):
    """one projection chain: y = ReLU?(x sc + sh) Wp^T + bp (+ res), next = act(normalise?(y) Wn'^T + bn'); bf16"""
    wp = _sparse_w(key + ".wp", 128, K, keep)
    bp = _grid(key + ".bp", (128,), -0.2, 0.2, 1.0 / 16) * sc
    pp = ops.ConvPlan(wp, bp, pre_bn=_BN(K) if pre else None, pre_relu=bool(pre and relu), dtype=BF16, device=device)
    aff = _pre_affine(pp, K, relu, sc) if pre else None
    pn = ops.ConvPlan(_uniform_w(key + ".wn", Nn, 128), procedural_input(key + ".bn", (Nn,), 0, -0.2, 0.2), act=next_act, dtype=BF16, device=device,
                      ln=_LN(key + ".lnn", 128, eps) if next_ln else None)
    r64 = None if not res else (_grid(key + ".r", (M, 128), -1, 1, 0.125) * sc).to(F64)
    wp64, bp64, wn64, bn64 = _w(pp, K), _b(pp), _w(pn, 128), _b(pn)

    def side(B, x):
        v = B.input(x)
        if aff is not None:
            v = B.affine(v, aff[0], aff[1], bool(relu))
        y = B.gemm(v, wp64, bp64, res=None if r64 is None else rows4(r64), inter=True, tag="proj")
        if isinstance(B, RowsRef):
            _exact(y.iv, key)
        if next_ln:
            y = B.normalise(y, eps, True, slot="next")
        if next_act == 2:
            return B.gelu(B.gemm(y, wn64, bn64, raw=True, tag="next"), final=True)
        return B.gemm(y, wn64, bn64, act=next_act, final=True, tag="next")
    return side, pp, pn, r64


def _proj(case, mode, device):
    """cobevt_proj_chain (K = 128)"""
    a_ = case.a
    M, Nn, eps = a_["M"], a_["Nn"], a_.get("eps", 1e-5)
    key = "rb." + case.name
    sc = SMALL if a_.get("small") else 1.0
    x = (_grid(key + ".x", (M, 128), -2, 2, 0.5) * sc).to(F64)
    side, pp, pn, r64 = _proj_side(key, 128, M, Nn, a_.get("pre"), a_.get("relu"), a_.get("res"), a_.get("next_ln", True), a_.get("next_act", 0), eps,
                                   device, 0.25, sc)
    return dict(net=lambda B: side(B, rows4(x)), x=x.to(BF16).to(device), res=None if r64 is None else r64.to(BF16).to(device), plans=(pp, pn),
                slots=["next"] if a_.get("next_ln", True) else [])


def _kv(case, mode, device):
    """cobevt_proj_chain_kv: the key side (with the residual) and the value side of one launch, Nn = 256 behind a LayerNorm"""
    a_ = case.a
    M, K, eps = a_["M"], a_["K"], a_.get("eps", 1e-5)
    key = "rb." + case.name
    sc = SMALL if a_.get("small") else 1.0
    x = (_grid(key + ".x", (M, K), -2, 2, 0.5) * sc).to(F64)
    ks, ppk, pnk, r64 = _proj_side(key + ".k", K, M, 256, True, True, True, True, 0, eps, device, 32.0 / K, sc)
    vs, ppv, pnv, _ = _proj_side(key + ".v", K, M, 256, True, True, False, True, 0, eps, device, 32.0 / K, sc)
    return dict(net=lambda B: ks(B, rows4(x)), net_v=lambda B: vs(B, rows4(x)), x=x.to(BF16).to(device), res=r64.to(BF16).to(device),
                plans=(ppk, ppv, pnk, pnv), slots=["next"])


def _lin(case, mode, device):
    """cobevt_linear_rows_small_k behind a LayerNorm: out = act(normalise(x) W'^T + b' (+ residual))"""
    a_, dt = case.a, store_dtype(mode)
    M, K, N, act, eps = a_["M"], a_["K"], a_["N"], a_.get("act", 0), a_.get("eps", 1e-5)
    key = "rb." + case.name
    sc = SMALL if a_.get("small") else 1.0
    x = rne((procedural_input(key + ".x", (M, K), 0, -2, 3) * sc).to(F64), dt)
    plan = ops.ConvPlan(_uniform_w(key + ".w", N, K), procedural_input(key + ".b", (N,), 0, -0.2, 0.2), act=act, dtype=dt, device=device,
                        ln=_LN(key + ".ln", K, eps))
    res = rne(procedural_input(key + ".r", (M, N), 0).to(F64), dt) if a_.get("res") else None
    w64, b64 = _w(plan, K), _b(plan)

    def net(B):
        v = B.normalise(B.input(rows4(x)), eps, True, slot="ln")
        r4 = None if res is None else rows4(res)
        if act == 2:
            return B.gelu(B.gemm(v, w64, b64, res=r4, raw=True, tag="lin"), final=True)
        return B.gemm(v, w64, b64, act=act, res=r4, final=True, tag="lin")
    return dict(net=net, x=x.to(dt).to(device), res=None if res is None else res.to(dt).to(device), plan=plan, slots=["ln"])


def _mean(case, mode, device):
    """cobevt_mean_linear_rows_small_k: out = act(normalise?(mean_l x[b, l, r, :]) W'^T + b')"""
    a_ = case.a
    B_, L, R, K, N, act, eps = a_["B"], a_["L"], a_["R"], a_["K"], a_["N"], a_.get("act", 0), a_.get("eps", 1e-5)
    key = "rb." + case.name
    x = rne(procedural_input(key + ".x", (B_, L, R, K), 0, -2, 3).to(F64), BF16)
    plan = ops.ConvPlan(_uniform_w(key + ".w", N, K), procedural_input(key + ".b", (N,), 0, -0.2, 0.2), act=act, dtype=BF16, device=device,
                        ln=_LN(key + ".ln", K, eps) if a_.get("ln") else None)
    w64, b64 = _w(plan, K), _b(plan)
    xl = x.permute(1, 0, 2, 3).reshape(L, B_ * R, K)

    def net(B):
        v = B.mean_rows(xl)
        v = B.normalise(v, eps, True, slot="ln") if a_.get("ln") else B.store(v, final=False)
        if act == 2:
            return B.gelu(B.gemm(v, w64, b64, raw=True, tag="lin"), final=True)
        return B.gemm(v, w64, b64, act=act, final=True, tag="lin")
    return dict(net=net, x=x.to(BF16).to(device), plan=plan, slots=["ln"] if a_.get("ln") else [])


BUILDERS = {"chain": _chain, "proj": _proj, "kv": _kv, "lin": _lin, "mean": _mean}
_OPS, _REFS = {}, {}


def build(case, mode, device="cpu"):
    return BUILDERS[case.kind](case, mode, device)


def cpu_op(case, mode):
    key = (case.name, mode)
    if key not in _OPS:
        _OPS[key] = build(case, mode)
    return _OPS[key]


def reference(case, mode, net="net"):
    """-> (the output's Interval (1, N, 1, M), the intermediates' Intervals), computed once per (case, mode, net)"""
    key = (case.name, mode, net)
    if key not in _REFS:
        B = RowsRef(mode)
        out = cpu_op(case, mode)[net](B)
        _REFS[key] = (out.iv, B.inter)
    return _REFS[key]


def emulate(case, mode, fault=None, order=0, net="net"):
    return cpu_op(case, mode)[net](RowsEmul(mode, fault, order)).mid.to(F64)


def outputs(case, mode, fault=None, order=0):
    """-> [(label, Interval, emulated)] for every destination of the case: "net" (out; the key side), "net_v" (the value side), "next" (the
    chain's next projection: its Interval from the HONEST emulator's `out` as stored, its emulation from the same rows)"""
    op = cpu_op(case, mode)
    res = [(n, reference(case, mode, n)[0], emulate(case, mode, fault, order, n)) for n in (("net", "net_v") if case.kind == "kv" else ("net",))]
    if case.kind == "chain" and op["next_net"] is not None:
        key = (case.name, mode, "next")
        if key not in _REFS:
            stored = rows2(emulate(case, mode))
            _REFS[key] = (stored, next_reference(op, mode, stored))
        stored, iv = _REFS[key]
        res.append(("next", iv, next_emulate(op, mode, stored, fault)))
    return res


def next_reference(op, mode, out):
    """the next projection's Interval from `out` (M, C) as stored"""
    B = RowsRef(mode)
    return op["next_net"](B, out.to(F64)).iv


def next_emulate(op, mode, out, fault=None):
    return op["next_net"](RowsEmul(mode, fault), out.to(F64)).mid.to(F64)


# ----------------------------------------------------------------------------------------------
# the table: what the entry point receives (dims, null-ness of its pointers) and the instantiation it must select
# ----------------------------------------------------------------------------------------------
def case_dims(case, mode):
    a, code = case.a, 0 if mode == "bf16" else 1
    if case.kind == "chain":
        hd = a["Hd"]
        batch = a.get("batch", 1)
        return [code, a["M"], a["C"], hd, (hd + 127) // 128 * 128, a.get("Nn", 0), int(bool(a.get("Nn") and a.get("next_ln"))),
                a.get("next_act", 0) if a.get("Nn") else 0, case.knobs.get("ROW_CHAIN_ROWS", 0), a["M"] // batch if batch > 1 else 0]
    if case.kind == "proj":
        return [0, a["M"], 128, a["Nn"], int(a.get("next_ln", True)), a.get("next_act", 0), 0, int(bool(a.get("pre") and a.get("relu"))), 0]
    if case.kind == "kv":
        return [0, a["M"], a["K"], 256, 1, 2, 1, 0, 1, 0]
    if case.kind == "lin":
        return [code, a["M"], a["N"], a["K"], a["K"], 0, a.get("act", 0), 1, 1, 1, a["M"], 1, a["M"], 64 if case.knobs.get("GEMM_ROWS3_ROWS64_MIN_M") else 32]
    return [0, a["B"], a["L"], a["R"], a["K"], a["N"], int(bool(a.get("ln"))), a.get("act", 0)]


def select_line(case, mode):
    """the case in the line format of tests/golden/rows_select/cases.txt (None: cobevt_proj_chain_kv is not routed by rows_select.hpp)"""
    a, dims = case.a, case_dims(case, mode)
    if case.kind == "chain":
        entry, flags = "chain", [1, int(a.get("skip", True)), int(bool(a.get("post"))), int(bool(a.get("post"))), int(bool(a.get("Nn"))), int(bool(a.get("Nn")))]
    elif case.kind == "proj":
        entry, flags = "proj", [1, int(bool(a.get("pre"))), int(bool(a.get("pre"))), int(bool(a.get("res")))]
    elif case.kind == "lin":
        entry, flags = "small_k", [1, int(bool(a.get("res"))), 0, 0]
    elif case.kind == "mean":
        entry, flags = "mean", [1]
    else:
        return None
    return " ".join(str(t) for t in ["%s-%s" % (case.name, mode), entry, len(dims)] + dims + [len(flags)] + flags + [1, 1, 1536])


def _cases():
    out = []
    gen = lambda npass, rows, full: "row_chain_kernel<%d, %d, %s, true>" % (npass, rows, "true" if full else "false")      # noqa: E731

    def chain(name, modes=("bf16",), kernel=None, rows=0, **a):
        tile = 64 if rows == 64 else 32
        kernel = kernel or gen(2 if a["Hd"] > 128 else 1, tile, a["C"] == 128)
        out.append(Case("chain_%s%s" % (name, "_r64" if rows == 64 else ""), "chain", "cobevt_attn_mlp_chain", modes, dict(ROW_CHAIN_ROWS=rows) if rows or modes == ("bf16",) else {},
                        kernel=kernel, stat=a["M"] * a["C"] >= 4000, **a))
    # the generic kernel: all eight <NPASS, ROWS, FULL, true>; widths with and without padded hidden columns (Hd 200, 72), rows around
    # a 32- and a 64-row tile, a broadcast skip whose modulo wraps inside both, every switch, one to six passes of the next projection
    for rows in (32, 64):
        chain("c128_h256_m130_post", rows=rows, M=130, C=128, Hd=256, bp=True, post=True)
        chain("c128_h256_m33_n384", rows=rows, M=33, C=128, Hd=256, Nn=384, next_ln=True)
        chain("c128_h200_m31_n768_relu", rows=rows, M=31, C=128, Hd=200, bp=True, Nn=768, next_act=1, post=True)
        chain("c128_h128_m150_bcast_n200_gelu", rows=rows, M=150, batch=3, C=128, Hd=128, Nn=200, next_ln=True, next_act=2)
        chain("c128_h72_m1_noskip", rows=rows, M=1, C=128, Hd=72, skip=False, bp=True)
        chain("c64_h200_m130_n8", rows=rows, M=130, C=64, Hd=200, Nn=8, post=True, next_ln=True)
        chain("c64_h128_m150_bcast", rows=rows, M=150, batch=3, C=64, Hd=128, bp=True)
        chain("c40_h72_m33_n200", rows=rows, M=33, C=40, Hd=72, Nn=200, next_act=1)
        chain("c40_h256_m31_post", rows=rows, M=31, C=40, Hd=256, post=True, skip=False)
        chain("c8_h16_m130_n8_gelu", rows=rows, M=130, C=8, Hd=16, bp=True, Nn=8, next_act=2)
        # small-variance rows (about 1e-4) and an eps that is not 1e-5: eps1 + eps_post, eps1 + eps_next
        chain("c128_h256_m130_small_post", rows=rows, M=130, C=128, Hd=256, bp=True, post=True, small=True, eps=3e-5)
        chain("c64_h128_m130_small_next", rows=rows, M=130, C=64, Hd=128, Nn=200, next_ln=True, small=True, eps=3e-5)
    # row_chain64_kernel<NNT, 4, true>: the threshold, a ragged tail, a block count (515) that is no multiple of the four waves, and a map
    # of more blocks (2,052) than the 512 x 4 waves of the capped grid, where a wave walks a second block
    c64 = lambda nnt: "row_chain64_kernel<%d, 4, true>" % nnt                              # noqa: E731
    chain("rc64_m16384_n0_post", kernel=c64(0), M=16384, C=64, Hd=128, bp=True, post=True)
    chain("rc64_m16424_n64_relu", kernel=c64(2), M=16384 + 40, C=64, Hd=128, Nn=64, next_act=1, post=True)
    chain("rc64_m16480_n128_gelu", kernel=c64(4), M=16480, C=64, Hd=128, bp=True, Nn=128, next_ln=True, next_act=2)
    chain("rc64_m65639_n192", kernel=c64(6), M=65536 + 103, C=64, Hd=128, Nn=192, next_ln=True)
    chain("rc64_m16384_small_n64", kernel=c64(2), M=16384, C=64, Hd=128, Nn=64, next_ln=True, small=True, eps=3e-5)
    # row_chain_f32_kernel, in every fp32-storage mode it is built for
    # Third library ("fp32_fast"): the weights' 2^-11 rounding, propagated through four GEMMs, gives the chain's own `out` a width of
    # about 1.9 |ref| (measured: F32_FAST_OUT_WIDTH below; the interval is asserted, and says next to nothing), while `out_next`, one
    # LayerNorm and one GEMM from the stored `out`, stays 1.2 - 1.3 % of |ref| wide and sees the dropped product.  The three rows with
    # a post-LayerNorm stay out of that library: the same propagation reaches the post-LayerNorm as an interval wider than the row's own
    # spread (normalise_bound's t = 2.2 for f32_m130_post, 1.5 for f32_m31_n768_relu, 1.2 for f32_m130_small_post against the
    # asserted 1/4), so no bound exists there
    # hidden there ("fault/destination@mode"): one product of fc2, and eps1 on small-variance rows, stay inside that `out` interval (0 of the
    # touched elements leave); `out_next` sees its own dropped product (74 - 100 %) and its own eps (95 %), `out` still a shifted skip row
    f32 = dict(modes=F32_MODES, kernel="row_chain_f32_kernel", C=128, Hd=256, hidden=("drop/net@fp32_fast", "eps/net@fp32_fast"))
    f32p = dict(f32, modes=("fp32", "fp32_split"))
    chain("f32_m130_post", M=130, bp=True, post=True, **f32p)
    chain("f32_m33_n384", M=33, Nn=384, next_ln=True, **f32)
    chain("f32_m31_n768_relu", M=31, bp=True, Nn=768, next_act=1, post=True, **f32p)
    chain("f32_m150_bcast_n200_gelu", M=150, batch=3, Nn=200, next_ln=True, next_act=2, **f32)
    chain("f32_m1_noskip_n8", M=1, skip=False, Nn=8, **f32)
    # rows N(100, 1): the next projection's LayerNorm, on `out` as stored, carries the U |mu| r term of the single mean (behind a post-
    # LayerNorm the rows would be centred again; the chain's own `out` interval is wide here, |skip| = 100 sits in every S)
    # hidden "drop" on `out`: e of y and z is K 2^-23 S with |skip| = 100 in S, a hundred times the other cases', and one product of fc2
    # stays inside it (2 / 1 of the last row's 128 elements leave in fp32 / fp32_split); `next` sees its own dropped product (78 %)
    chain("f32_m130_offset100", M=130, offset=100.0, Nn=200, next_ln=True, **dict(f32, hidden=("drop/net",)))
    chain("f32_m130_small_post", M=130, bp=True, post=True, small=True, eps=3e-5, **f32p)
    chain("f32_m130_small_next", M=130, Nn=200, next_ln=True, small=True, eps=3e-5, **f32)

    def proj(name, kernel, **a):
        out.append(Case("proj_" + name, "proj", "cobevt_proj_chain", ("bf16",), {}, kernel=kernel, **a))
    pg = "row_chain_kernel<1, 32, true, false>"
    proj("m130_pre_relu_res", pg, M=130, Nn=256, pre=True, relu=True, res=True)
    proj("m33_plain_n200_gelu", pg, M=33, Nn=200, next_act=2, stat=False)
    proj("m1000_pre_noln_relu", pg, M=1000, Nn=384, pre=True, next_ln=False, next_act=1)
    proj("m32767_res", pg, M=32767, Nn=128, res=True)
    proj("m130_small", pg, M=130, Nn=256, res=True, small=True, eps=3e-5)
    proj("w128_m32768_pre_relu_res", "proj_chain128_kernel<4, 8>", M=32768, Nn=128, pre=True, relu=True, res=True)
    proj("w128_m32845", "proj_chain128_kernel<4, 8>", M=32768 + 77, Nn=128, next_ln=False)
    proj("w256_m32768_pre", "proj_chain128_kernel<8, 8>", M=32768, Nn=256, pre=True)
    proj("w256_m32845_res", "proj_chain128_kernel<8, 8>", M=32768 + 77, Nn=256, res=True)
    proj("w256_m65613_pre_relu_res", "proj_chain128_kernel<8, 8>", M=65536 + 77, Nn=256, pre=True, relu=True, res=True)     # a wave's second block
    for k, m in ((256, 31), (384, 77), (512, 1000), (256, 1000)):
        out.append(Case("kv_k%d_m%d" % (k, m), "kv", "cobevt_proj_chain_kv", ("bf16",), {}, kernel=None, K=k, M=m))
    out.append(Case("kv_k384_m130_small", "kv", "cobevt_proj_chain_kv", ("bf16",), {}, kernel=None, K=384, M=130, small=True, eps=3e-5))

    def lin(name, kernel, modes=("bf16",), rows64=False, **a):
        out.append(Case("lin_" + name, "lin", "cobevt_linear_rows_small_k", modes, dict(GEMM_ROWS3_ROWS64_MIN_M=1) if rows64 else {}, kernel=kernel,
                        stat=a["M"] * a["N"] >= 4000, **a))
    for r64 in (False, True):
        g3 = "gemm_rows3_kernel<false, %d>" % (64 if r64 else 32)
        sfx = "_r64" if r64 else ""
        lin("k8_n40_m130" + sfx, g3, rows64=r64, M=130, K=8, N=40)
        lin("k64_n200_m33_res_relu" + sfx, g3, rows64=r64, M=33, K=64, N=200, res=True, act=1)
        lin("k128_n384_m130_gelu" + sfx, g3, rows64=r64, M=130, K=128, N=384, act=2)
        lin("k128_n128_m130_small_res" + sfx, g3, rows64=r64, M=130, K=128, N=128, res=True, small=True, eps=3e-5)
    lin("f32_k128_n200_m130_res_gelu", "gemm_rows3_f32_kernel", modes=F32_MODES, M=130, K=128, N=200, res=True, act=2)
    lin("f32_k128_n128_m33_relu", "gemm_rows3_f32_kernel", modes=F32_MODES, M=33, K=128, N=128, act=1)
    # ln_linear64_kernel<NNT, 4>: N = 32 NNT at the threshold, once ragged, once on a map of more blocks than the capped grid's waves
    for nnt in range(1, 7):
        m = 65536 + 37 if nnt == 6 else 65536
        lin("ln64_n%d_m%d" % (32 * nnt, m), "ln_linear64_kernel<%d, 4>" % nnt, M=m, K=64, N=32 * nnt, act=2 if nnt == 2 else 0)
    lin("ln64_n32_m196645", "ln_linear64_kernel<1, 4>", M=196608 + 37, K=64, N=32)
    lin("ln64_n64_m65536_small", "ln_linear64_kernel<2, 4>", M=65536, K=64, N=64, small=True, eps=3e-5)
    for L, ln, act in ((1, True, 0), (5, True, 2), (64, True, 0), (1, False, 2), (5, False, 1), (64, False, 0)):
        out.append(Case("mean_l%d%s_act%d" % (L, "_ln" if ln else "", act), "mean", "cobevt_mean_linear_rows_small_k", ("bf16",), {},
                        kernel="gemm_rows3_kernel<false, 32>", B=2, L=L, R=35, K=64 if L == 5 else 128, N=72, ln=ln, act=act))
    return out


CASES = _cases()
# median (hi - lo) / |ref| of the fp32 chain's own `out` in the third library, measured on the CPU (test_rows_bounds.py recomputes it): the
# rows that cannot meet a useful width at the precision their library fixes, by name
F32_FAST_OUT_WIDTH = {"chain_f32_m33_n384": 1.90, "chain_f32_m150_bcast_n200_gelu": 1.86, "chain_f32_m1_noskip_n8": 2.20,
                      "chain_f32_m130_offset100": 0.030, "chain_f32_m130_small_next": 1.55}
CASE_MODES = [(c, m) for c in CASES for m in c.modes]
COVERED = sorted({c.a["kernel"] for c in CASES if c.a["kernel"]})
LEFT_OUT = {"gemm_rows3_kernel<true, 32>": "bev_embed: the embedding's geometry needs another reference",
            "bev_query_kernel<4>": "bev_query: the same; test_bev_query_wave_level_kernel stays"}
LEFT_OUT.update({"row_chain64_kernel<%d, 6, %s>" % (nnt, pf): "reached only through COBEVT_RC64_PREFETCH, read once per process"
                 for nnt in (0, 2, 4, 6) for pf in ("true", "false")})


def case_id(cm):
    return "%s-%s" % (cm[0].name, cm[1])
