"""Float64 restatement and per-element intervals of the typed agent attention (host.HGTCavAttention, RTE, RelTemporalEncoding,
CavPositionalEncoding; csrc/att_fuse.hip: cobevt_typed_linear, cobevt_hgt_attention_nhwc).  tests/test_hgt.py uses it on the CPU,
tests/test_hgt_gpu.py on the device, tools/hgt_probe.py as the torch baseline it times.

The restatement.  Every function takes a state dict and tensors of ONE dtype and is vectorised: no loop over agents, no host read.
  unfolded(sd, x, mask, types, heads)      the reference's procedure: q, k, v by the row's type; score_ij = scale q_i^T R_att[e] k_j,
                                           message = R_msg[e]^T v_j with e = types_i T + types_j; key mask; softmax over j; a_linears by
                                           the row's type.  fault= plants one of FAULTS.
  fold64(sd, ln)                           the algebra of ops.hgt_fold written a second time: for a row of type b, as seen by a query of
                                           type a:  k' = blockdiag_m(R_att[a T + b, m]) (Wk_b x + bk_b),  v' = blockdiag_m(R_msg[a T + b, m]^T)
                                           (Wv_b x + bv_b); the LayerNorm affine last (W' = W g, b' = b + W beta).
  folded(fold, x, mask, types, ...)        the three stages the kernels run: typed_rows -> attention_rows -> typed_rows.

The intervals.  U = 2^-23 (one ulp of fp32, twice the unit roundoff), gamma(n) = n U / (1 - n U).
GEMM (typed_linear_interval): the construction of conv_bounds_ref / rows_bounds_ref, imported, one RowsRef.gemm per group with the
  weights of that group's type: e = K U S + U |pre| (+ the propagated width of the normalised row: rows_bounds_ref.normalise_bound,
  closed in the storage type where the kernel stores it - it writes the normalised row to LDS in that type).  fp32 storage runs on
  the exact v_mfma_f32_32x32x2_f32 in all three libraries, so every fp32 mode takes the "fp32" term (none).
Attention (attention_interval), per (pixel, head, query i) over the unmasked keys j, from the operands as stored:
  score     s_j = scale sum_c q_c k_jc: 32 products and their sum in ANY order, then the scale: |ds_j| <= gamma(33) scale sum_c |q_c k_jc|.
  weights   the kernel keeps a running maximum m and folds key j in as  den = den a + w, acc = acc a + w v_j  with a = exp(m_old - m_new),
            w = exp(s_j - m_new).  The SAME a and w enter den and acc, so the weight the kernel gives key j - exp(s_j - m) with its
            errors - is common to numerator and denominator: out~ = sum_j P_j (1 + theta_j) v_j / sum_j P_j (1 + theta_j), hence
                out~ - out = sum_j P_j theta_j (v_j - out) / (1 + sum_j P_j theta_j),   |.| <= sum_j P_j Theta_j |v_j - out| / (1 - max Theta).
            theta_j collects: the score error, e^(ds_j); the roundings of the exponents' subtractions, which telescope along the chain of
            rescalings to at most U (m - s_j) - taken with the float64 D_j = max_k s_k - s_j plus 2 max ds for the computed maximum; and
            at most L evaluations of expf at 1 ulp each: (1 + U)^L.  THE 1 ulp OF expf IS ASSUMED, as DESIGN.md 3u assumes it of v_exp_f32
            and says so; the `used` figures the GPU file prints show what the kernel leaves of it.
                Theta_j = expm1(ds_j + U (D_j + 2 max ds) + L U).
  sums      acc: a product w v, a product acc a and an addition per key: gamma(3 L) sum_j P_j |v_j| (first order, times
            (1 + max Theta) / (1 - max Theta)); den, all terms positive: gamma(2 L) relative; 1 / den and the final product: 2 U.
                e = weights term + gamma(3 L) A + gamma(2 L + 2) (|out| + weights term + gamma(3 L) A),   A = sum_j P_j |v_j| (1 + Th) / (1 - Th).
  Then ONE rounding to the storage type: [rne(out - e), rne(out + e)].  A query without a key: exactly 0.  D_j < 80 is asserted (no
  weight underflows).  No constant here is fitted to the kernel.
"""
import math
import os

import numpy as np
import torch

from cobevt_amd.synth import fill_module_, procedural_input
from conv_bounds_ref import Interval, rne, U, F64, store_dtype
from rows_bounds_ref import RowsRef, rows4, rows2

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FILE = os.path.join(HERE, "golden", "gv31_hgt.npz")
FAULTS = ("relation_index", "msg_not_transposed", "mask_queries", "value_by_key_type")
RELATION_GAIN = 1.5


def gamma(n):
    return n * U / (1.0 - n * U)


# ----------------------------------------------------------------------------------------------
# weights
# ----------------------------------------------------------------------------------------------
@torch.no_grad()
def fill_hgt_(module, seed=0):
    """synth.fill_module_, then the relation matrices of every HGTCavAttention inside at unit gain per 32 x 32 block times RELATION_GAIN
    (the state-dict fill scales them by the fan-in of the whole (heads, 32, 32) slab, and xavier's are as small: scores near 0, a
    softmax that is a plain mean).  A function of (key, shape, seed) like the rest."""
    fill_module_(module, seed)
    for key, t in module.state_dict().items():
        if key.endswith("relation_att") or key.endswith("relation_msg"):
            t.copy_(procedural_input("hgt." + key, t.shape, seed) * math.sqrt(3.0 / t.shape[-1]) * RELATION_GAIN)
    return module


def state64(module):
    return {k: v.detach().clone().double() for k, v in module.state_dict().items()}


def num_types(sd):
    return len([k for k in sd if k.startswith("q_linears.") and k.endswith(".weight")])


def _stack(sd, name):
    t = num_types(sd)
    return (torch.stack([sd["%s_linears.%d.weight" % (name, i)] for i in range(t)]),
            torch.stack([sd["%s_linears.%d.bias" % (name, i)] for i in range(t)]))


# ----------------------------------------------------------------------------------------------
# the four modules, vectorised, in the dtype of their arguments
# ----------------------------------------------------------------------------------------------
def rel_temporal(sd, x, t, ratio):
    """RelTemporalEncoding: x (H, W, C) or any (..., C), t an integer scalar tensor"""
    enc = sd["emb.weight"][t.long() * ratio] @ sd["lin.weight"].t() + sd["lin.bias"]
    return x + enc[None, None]


def rte(sd, x, dts, ratio):
    """RTE: x (B, L, H, W, C), dts (B, L) integer"""
    enc = sd["emb.emb.weight"][dts.long() * ratio] @ sd["emb.lin.weight"].t() + sd["emb.lin.bias"]
    return x + enc[:, :, None, None, :]


def cav_pos(sd, x):
    return x + sd["pos_table"][None, :, None, None, :]


def layer_norm(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps) * g + b


def unfolded(sd, x, mask, types, heads, fault=None):
    """x (B, L, H, W, C); mask broadcastable to (B, H, W, 1, L) (0 = key masked) or None; types (B, L) integer -> (B, L, H, W, C)"""
    T = num_types(sd)
    B, L, H, W, _ = x.shape
    ty = types.long()
    (wq, bq), (wk, bk), (wv, bv), (wa, ba) = (_stack(sd, n) for n in "qkva")
    proj = lambda w, b: (torch.einsum("blhwc,blnc->blhwn", x, w[ty]) + b[ty][:, :, None, None, :]).reshape(B, L, H, W, heads, -1)   # noqa: E731
    q, k, v = proj(wq, bq), proj(wk, bk), proj(wv, bv)
    ti, tj = ty[:, :, None], ty[:, None, :]
    e = ti * T + tj
    e_att = tj * T + ti if fault == "relation_index" else e
    e_msg = tj * T + tj if fault == "value_by_key_type" else e_att
    w_att, w_msg = sd["relation_att"][e_att], sd["relation_msg"][e_msg]          # (B, Li, Lj, M, 32, 32)
    if fault == "msg_not_transposed":
        w_msg = w_msg.transpose(-1, -2)
    score = torch.einsum("bihwmp,bijmpq,bjhwmq->bhwmij", q, w_att, k) * (q.shape[-1] ** -0.5)
    if mask is not None:
        mk = mask.to(x.dtype).expand(B, H, W, 1, L)
        mk = mk.reshape(B, H, W, 1, L, 1) if fault == "mask_queries" else mk.reshape(B, H, W, 1, 1, L)
        score = score.masked_fill(mk == 0, -float("inf"))
    att = torch.softmax(score, -1)
    if fault == "mask_queries":
        att = torch.nan_to_num(att, nan=0.0)                                       # (a kernel with this fault writes zeros there)
    v_msg = torch.einsum("bijmpc,bjhwmp->bhwmijc", w_msg, v)
    out = torch.einsum("bhwmij,bhwmijc->bihwmc", att, v_msg).reshape(B, L, H, W, -1)
    return torch.einsum("blhwn,blcn->blhwc", out, wa[ty]) + ba[ty][:, :, None, None, :]


class LN(object):
    def __init__(self, weight, bias, eps=1e-5):
        self.weight, self.bias, self.eps = weight, bias, eps


def fold64(sd, ln=None, fault=None):
    """-> (w_in (T, (1 + 2 T) inner, dim), b_in, w_out (T, dim, inner), b_out) in the dtype of sd (float64 in the tests)"""
    T = num_types(sd)
    ratt, rmsg = sd["relation_att"], sd["relation_msg"]
    heads, dh = ratt.shape[1], ratt.shape[2]
    bd = lambda r: torch.block_diag(*[r[m] for m in range(heads)])                # noqa: E731
    w_in, b_in = [], []
    for b in range(T):
        ws, bs = [sd["q_linears.%d.weight" % b]], [sd["q_linears.%d.bias" % b]]
        for a in range(T):
            e = b * T + a if fault == "relation_index" else a * T + b
            r = bd(ratt[e])
            ws.append(r @ sd["k_linears.%d.weight" % b])
            bs.append(r @ sd["k_linears.%d.bias" % b])
        for a in range(T):
            e = b * T + a if fault == "relation_index" else a * T + b
            r = bd(rmsg[e]) if fault == "msg_not_transposed" else bd(rmsg[e]).t()
            ws.append(r @ sd["v_linears.%d.weight" % b])
            bs.append(r @ sd["v_linears.%d.bias" % b])
        w, bb = torch.cat(ws, 0), torch.cat(bs, 0)
        if ln is not None:
            bb = bb + w @ ln.bias.to(w.dtype)
            w = w * ln.weight.to(w.dtype)[None, :]
        w_in.append(w)
        b_in.append(bb)
    wa, ba = _stack(sd, "a")
    return torch.stack(w_in), torch.stack(b_in), wa, ba


def normalise(x, eps):
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    return d * torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)


def typed_rows(x, w, b, types, ln_eps=None, residual=None, store=None):
    """cobevt_typed_linear: x (B, L, ..., K), types (B, L) (clamped like the kernel's), w (T, N, K), b (T, N); store = the storage dtype the
    normalised row is rounded to (None: not rounded)"""
    ty = types.long().clamp(0, w.shape[0] - 1)
    if ln_eps is not None:
        x = normalise(x, ln_eps)
        if store is not None:
            x = x.to(store).to(w.dtype)
    wt, bt = w[ty], b[ty]
    extra = x.dim() - 3
    y = torch.einsum("bl...k,blnk->bl...n", x, wt) + bt.reshape(bt.shape[:2] + (1,) * extra + bt.shape[2:])
    return y if residual is None else y + residual


def attention_rows(proj, types, mask, heads, T, fault=None):
    """cobevt_hgt_attention_nhwc: proj (B, L, H, W, (1 + 2 T) inner), mask (B, H, W, L) or None -> (B, L, H, W, inner); plain softmax in
    the dtype of proj, zeros where no key is left"""
    B, L, H, W, _ = proj.shape
    inner = heads * 32
    ty = types.long().clamp(0, T - 1)
    q = proj[..., :inner].reshape(B, L, H, W, heads, 32)
    kall = proj[..., inner:(1 + T) * inner].reshape(B, L, H, W, T, heads, 32)
    vall = proj[..., (1 + T) * inner:].reshape(B, L, H, W, T, heads, 32)
    bidx = torch.arange(B)[:, None]
    # [b, i, j] = the variant a_i of agent j's keys / values
    ksel = kall.permute(0, 4, 1, 2, 3, 5, 6)[bidx, ty]                             # (B, Li, Lj, H, W, M, 32)
    if fault == "value_by_key_type":
        vsel = vall[bidx, torch.arange(L)[None, :], :, :, ty][:, None].expand(B, L, L, H, W, heads, 32)
    else:
        vsel = vall.permute(0, 4, 1, 2, 3, 5, 6)[bidx, ty]
    score = torch.einsum("bihwmc,bijhwmc->bihwmj", q, ksel) * (32 ** -0.5)
    if mask is not None:
        if fault == "mask_queries":
            on = (mask != 0).permute(0, 3, 1, 2)[:, :, :, :, None, None].expand(B, L, H, W, heads, L)
        else:
            on = (mask != 0)[:, None, :, :, None, :].expand(B, L, H, W, heads, L)
        score = score.masked_fill(~on, -float("inf"))
        dead = ~on.any(-1, keepdim=True)
        score = torch.where(dead, torch.zeros_like(score), score)
    p = torch.softmax(score, -1)
    if mask is not None:
        p = torch.where(dead, torch.zeros_like(p), p)
    return torch.einsum("bihwmj,bijhwmc->bihwmc", p, vsel).reshape(B, L, H, W, inner)


def key_mask(mask, B, L, H, W):
    return None if mask is None else mask.to(torch.float32).expand(B, H, W, 1, L).reshape(B, H, W, L)


def folded(fold, x, mask, types, heads, T, ln_eps=None, residual=None, fault=None):
    """the three stages in the dtype of the operands, nothing rounded in between"""
    w_in, b_in, w_out, b_out = fold
    B, L, H, W, _ = x.shape
    proj = typed_rows(x, w_in, b_in, types, ln_eps)
    att = attention_rows(proj, types, key_mask(mask, B, L, H, W), heads, T, fault)
    return typed_rows(att, w_out, b_out, types, residual=residual)


def layer_restatement(sd, ln, x, mask, prior, heads):
    """PreNorm(HGTCavAttention)(x) + x by the reference's procedure, in the dtype of the operands (tools/hgt_probe.py's baseline)"""
    types = prior[:, :, 0, 0, 2].to(torch.int)
    return unfolded(sd, layer_norm(x, ln.weight, ln.bias, ln.eps), mask, types, heads) + x


# ----------------------------------------------------------------------------------------------
# intervals
# ----------------------------------------------------------------------------------------------
def _cat(ivs):
    return Interval(*[None if ivs[0][f] is None else torch.cat([iv[f] for iv in ivs], 3) for f in range(5)])


def typed_linear_interval(x, w, b, types, rows, mode, ln_eps=None, residual=None):
    """x (G rows, K), w (T, N, K), b (T, N), residual (G rows, N) or None: float64 values the storage type holds exactly; types (G,) ->
    Interval with (G rows, N) fields.  mode "bf16" or "fp32" (every fp32-storage library: the kernel's matrix path does not change)"""
    ty = types.long().clamp(0, w.shape[0] - 1)
    ivs = []
    for g in range(ty.numel()):
        B = RowsRef(mode)
        sl = slice(g * rows, (g + 1) * rows)
        v = B.input(rows4(x[sl]))
        if ln_eps is not None:
            v = B.normalise(v, ln_eps, True, slot="ln")
        out = B.gemm(v, w[ty[g]], b[ty[g]], res=None if residual is None else rows4(residual[sl]), final=True, tag="lin")
        ivs.append(out.iv)
    iv = _cat(ivs)
    return Interval(*[None if f is None else rows2(f) for f in iv])


def attention_interval(proj, types, mask, heads, T, dt):
    """proj (B, L, H, W, (1 + 2 T) inner) float64 as stored, mask (B, H, W, L) or None -> Interval with (B, L, H, W, inner) fields"""
    B, L, H, W, _ = proj.shape
    inner = heads * 32
    scale = 32 ** -0.5
    ty = types.long().clamp(0, T - 1)
    q = proj[..., :inner].reshape(B, L, H, W, heads, 32)
    kall = proj[..., inner:(1 + T) * inner].reshape(B, L, H, W, T, heads, 32)
    vall = proj[..., (1 + T) * inner:].reshape(B, L, H, W, T, heads, 32)
    bidx = torch.arange(B)[:, None]
    ksel = kall.permute(0, 4, 1, 2, 3, 5, 6)[bidx, ty]                             # (B, Li, Lj, H, W, M, 32)
    vsel = vall.permute(0, 4, 1, 2, 3, 5, 6)[bidx, ty]
    s = torch.einsum("bihwmc,bijhwmc->bihwmj", q, ksel) * scale
    ds = gamma(33) * scale * torch.einsum("bihwmc,bijhwmc->bihwmj", q.abs(), ksel.abs())
    on = torch.ones_like(s, dtype=torch.bool) if mask is None else (mask != 0)[:, None, :, :, None, :].expand_as(s)
    alive = on.any(-1, keepdim=True)
    neg = torch.full_like(s, -float("inf"))
    smax = torch.where(on, s, neg).max(-1, keepdim=True).values
    smax = torch.where(alive, smax, torch.zeros_like(smax))
    D = torch.where(on, smax - s, torch.zeros_like(s))
    assert float(D.max()) < 80.0, "a softmax weight would underflow in fp32"
    p = torch.where(on, torch.exp(-D), torch.zeros_like(s))
    p = p / p.sum(-1, keepdim=True).clamp_min(1e-300)
    dsmax = torch.where(on, ds, torch.zeros_like(ds)).max(-1, keepdim=True).values
    theta = torch.where(on, torch.expm1(ds + U * (D + 2.0 * dsmax) + L * U), torch.zeros_like(s))
    thmax = theta.max(-1, keepdim=True).values
    assert float(thmax.max()) < 0.01
    out = torch.einsum("bihwmj,bijhwmc->bihwmc", p, vsel)                            # (B, L, H, W, M, 32)
    dv = (vsel.permute(0, 1, 3, 4, 5, 2, 6) - out[..., None, :]).abs()               # (B, Li, H, W, M, Lj, 32)
    wterm = torch.einsum("bihwmj,bihwmjc->bihwmc", p * theta, dv) / (1.0 - thmax)
    A = torch.einsum("bihwmj,bijhwmc->bihwmc", p, vsel.abs()) * (1.0 + thmax) / (1.0 - thmax)
    e = wterm + gamma(3 * L) * A
    e = e + gamma(2 * L + 2) * (out.abs() + e)
    e = torch.where(alive.expand_as(e), e, torch.zeros_like(e))
    out = torch.where(alive.expand_as(out), out, torch.zeros_like(out))
    shp = (B, L, H, W, inner)
    out, e = out.reshape(shp), e.reshape(shp)
    return Interval(out, None, e, rne(out - e, dt), rne(out + e, dt))


def used(got, iv):
    """max |got - ref| / e over the elements with e > 0 (meaningful for fp32 stores, where the store's rounding is below e)"""
    sel = iv.e > 0
    return float(((got[sel] - iv.ref[sel]).abs() / iv.e[sel]).max()) if bool(sel.any()) else 0.0


def outside(got, iv):
    return int(((got < iv.lo) | (got > iv.hi)).sum())


# ----------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------
def make_types(kind, B, L, T):
    """(B, L) int32: "equal" all T - 1, "mixed" a cycle that starts at the sample's index, "oor" mixed with a negative and a too large one"""
    if kind == "equal":
        return torch.full((B, L), T - 1, dtype=torch.int32)
    ty = ((torch.arange(L)[None, :] + torch.arange(B)[:, None]) % T).to(torch.int32)
    if kind == "oor":
        ty = ty.clone()
        ty[0, 0], ty[-1, -1] = -3, T + 5
    return ty


def make_mask(kind, B, L, H, W):
    """None | "padded": the last agent of sample 0 (the last two where L >= 4) is masked at every pixel, (B, 1, 1, 1, L) | "pixel": one
    pixel's key 1 (key L - 1 for L = 2) | "dead": as "pixel", and one pixel with every key masked.  Key 0 stays on except in "dead"."""
    if kind is None:
        return None
    if kind == "padded":
        m = torch.ones(B, 1, 1, 1, L)
        m[0, ..., L - (2 if L >= 4 else 1):] = 0.0 if L > 1 else 1.0
        return m
    m = torch.ones(B, H, W, 1, L)
    if L > 1:
        m[0, H // 2, W // 2, 0, 1] = 0.0
        m[-1, 0, 0, 0, L - 1] = 0.0
    if kind == "dead":
        m[-1, H - 1, W - 1, 0, :] = 0.0
    return m


# module cases of the golden file: name -> dict
MODULE_CASES = {
    "d64": dict(dim=64, heads=2, T=2, R=4, B=2, L=3, H=3, W=5, types="mixed", mask="pixel"),
    "d128": dict(dim=128, heads=8, T=3, R=9, B=1, L=5, H=2, W=3, types="mixed", mask="padded"),
}
RTE_CASE = dict(dim=64, ratio=2, B=2, L=3, H=3, W=5)
POS_CASE = dict(dim=64, cav_num=3, B=2, H=3, W=5)


def module_inputs(name):
    c = MODULE_CASES[name]
    B, L, H, W = c["B"], c["L"], c["H"], c["W"]
    x = procedural_input("hgt.%s.x" % name, (B, L, H, W, c["dim"]), 0, -2.0, 2.0)
    types = make_types(c["types"], B, L, c["T"])
    prior = torch.zeros(B, L, H, W, 3)
    prior[..., 0] = procedural_input("hgt.%s.vel" % name, (B, L, 1, 1), 0, 0.0, 5.0)
    prior[..., 1] = (torch.arange(L)[None, :] % 4).float()[:, :, None, None]
    prior[..., 2] = types.float()[:, :, None, None]
    return x, make_mask(c["mask"], B, L, H, W), prior, types


def rte_inputs():
    c = RTE_CASE
    x = procedural_input("hgt.rte.x", (c["B"], c["L"], c["H"], c["W"], c["dim"]), 0, -2.0, 2.0)
    dts = torch.tensor([[0, 3, 1], [2, 0, 7]], dtype=torch.int32)
    return x, dts


def pos_inputs():
    c = POS_CASE
    return procedural_input("hgt.pos.x", (c["B"], c["cav_num"], c["H"], c["W"], c["dim"]), 0, -2.0, 2.0)


def load_golden():
    return np.load(GOLDEN_FILE, allow_pickle=False)


# kernel cases: the smallest shapes at which each kernel can go wrong.  rows = H W: 1, 15 and 33 (a 32-row tile and a one-row tail; with
# G > 1 a tile that ignored the group boundary would straddle two agents); N / 32 = 6 (one pass), 3 (odd: the unstored twin tile), 40 and
# 10 (a second pass of the wave's column loop needs more than 8 tiles); K = 64, 96, 128, 256; T = 1, 2, 3; out-of-range types.
LINEAR_CASES = {
    #  name            B  L  H  W   K    N    T  types     ln     res
    "q64_t1_1x1":     (1, 1, 1, 1, 64, 192, 1, "equal", True, False),
    "q64_t2_3x5":     (2, 3, 3, 5, 64, 320, 2, "mixed", True, False),
    "q64_t2_33":      (2, 2, 33, 1, 64, 320, 2, "mixed", True, False),
    "q128_t2_33":     (1, 5, 3, 11, 128, 1280, 2, "mixed", True, False),
    "q128_t3_oor":    (2, 3, 3, 5, 128, 96, 3, "oor", True, False),
    "q96_t2_33":      (1, 3, 3, 11, 96, 480, 2, "mixed", True, False),
    "a256_t3_res":    (2, 5, 3, 5, 256, 128, 3, "mixed", False, True),
    "a64_t2_33_res":  (2, 3, 33, 1, 64, 64, 2, "mixed", False, True),
    "a64_t1_noln":    (1, 2, 3, 5, 64, 96, 1, "equal", False, False),
}
ATTENTION_CASES = {
    #  name              B  L  H  W  heads T  types    mask
    "l1_1x1":           (1, 1, 1, 1, 2, 1, "equal", None),
    "l2_3x5_pixel":     (2, 2, 3, 5, 2, 2, "mixed", "pixel"),
    "l3_33_padded":     (2, 3, 33, 1, 2, 2, "mixed", "padded"),
    "l5_3x5_h8_t3":     (2, 5, 3, 5, 8, 3, "mixed", "padded"),
    "l5_33_h8_dead":    (1, 5, 3, 11, 8, 2, "mixed", "dead"),
    "l3_3x5_equal":     (2, 3, 3, 5, 2, 2, "equal", None),
    "l3_3x5_oor":       (2, 3, 3, 5, 2, 3, "oor", "pixel"),
    "l8_3x5_t2":        (1, 8, 3, 5, 2, 2, "mixed", "pixel"),
    # 4 heads lanes per row that do not divide the 256 of a workgroup: a row's lanes straddle two workgroups (33 > 256 / 12, 15 > 256 / 24)
    "l3_33_h3":         (1, 3, 3, 11, 3, 2, "mixed", "pixel"),
    "l2_3x5_h6":        (2, 2, 3, 5, 6, 2, "mixed", "padded"),
}


def linear_operands(name, dt):
    """-> dict of float64 operands the storage type holds exactly (x, w, residual) and fp32 bias, types int32, rows, ln_eps"""
    B, L, H, W, K, N, T, kind, ln, res = LINEAR_CASES[name]
    key = "hgt.lin." + name
    x = rne(procedural_input(key + ".x", (B * L * H * W, K), 0, -2.0, 3.0).to(F64), dt)
    w = rne((procedural_input(key + ".w", (T, N, K), 0) * math.sqrt(3.0 / K)).to(F64), dt)
    b = procedural_input(key + ".b", (T, N), 0, -0.2, 0.2).to(F64)
    r = rne(procedural_input(key + ".r", (B * L * H * W, N), 0).to(F64), dt) if res else None
    return dict(x=x, w=w, b=b, residual=r, types=make_types(kind, B, L, T).reshape(-1), rows=H * W, ln_eps=1e-5 if ln else None, shape=(B, L, H, W))


def attention_operands(name, dt):
    B, L, H, W, heads, T, kind, mk = ATTENTION_CASES[name]
    key = "hgt.att." + name
    proj = rne(procedural_input(key + ".p", (B, L, H, W, (1 + 2 * T) * heads * 32), 0, -2.0, 2.0).to(F64), dt)
    mask = key_mask(make_mask(mk, B, L, H, W), B, L, H, W)
    return dict(proj=proj, types=make_types(kind, B, L, T), mask=None if mask is None else mask.contiguous(), heads=heads, T=T)


_IVS = {}


def linear_interval(name, mode):
    if (name, mode) not in _IVS:
        o = linear_operands(name, store_dtype(mode))
        _IVS[name, mode] = typed_linear_interval(o["x"], o["w"], o["b"], o["types"], o["rows"], mode, o["ln_eps"], o["residual"])
    return _IVS[name, mode]


def attention_case_interval(name, mode):
    if ("att", name, mode) not in _IVS:
        dt = store_dtype(mode)
        o = attention_operands(name, dt)
        _IVS["att", name, mode] = attention_interval(o["proj"], o["types"], o["mask"], o["heads"], o["T"], dt)
    return _IVS["att", name, mode]
