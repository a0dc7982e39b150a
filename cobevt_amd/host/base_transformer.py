"""PreNormResidual / FeedForward — mirror of opv2v/opencood/models/base_transformer.py:102-124 (the parts of that file on
the FAX hot path) - and PreNorm / CavAttention / BaseEncoder / BaseTransformer (:91-99,127-172,321-362), the per-pixel agent
attention of the CVT + AttFuse baseline.  RelTemporalEncoding / RTE / CavPositionalEncoding (:14-89) and
HGTCavAttention (:175-319), the agent-wise half of V2X-ViT, complete the file: the encodings are broadcast adds from device-side
gathers, the typed attention is three launches (typed projection, attention, typed output projection: DESIGN.md 3y)."""
import math

import numpy as np
import torch
import torch.nn as nn

from ..lib import CobevtHipError

from .. import ops
from . import runtime as rt
from . import training
from .runtime import HipModule


class PreNormResidual(HipModule):
    """fn(LayerNorm(x)) + x.  The residual add is fused into fn's last GEMM when fn offers `forward_fused`."""

    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn

    def forward_fused(self, x, **kwargs):
        """x: contiguous channels-last tensor in the compute dtype."""
        return self.fn.forward_fused(x, residual=x, ln=self.norm, **kwargs)

    def forward(self, x, **kwargs):
        if self.training:
            if isinstance(self.fn, FeedForward):
                return training.feed_forward(self.fn, x, norm=self.norm)
            return training.swap_attention(self.fn, x, kwargs.get("mask"), 2, norm=self.norm)
        self._require_inference(x)
        return rt.like_input(self.forward_fused(rt.as_compute(x), **kwargs), x)


class FeedForward(HipModule):
    """Linear -> GELU -> Dropout -> Linear -> Dropout (dropout is identity at inference)."""

    def __init__(self, dim, hidden_dim, dropout=0.):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, hidden_dim), nn.GELU(), nn.Dropout(dropout),
                                 nn.Linear(hidden_dim, dim), nn.Dropout(dropout))

    def forward_fused(self, x, residual=None, ln=None):
        t = ops.linear(x, rt.linear_plan(self, "fc1", self.net[0], act=2, ln=ln))
        return ops.linear(t, rt.linear_plan(self, "fc2", self.net[3]), residual=residual)

    def forward(self, x):
        if self.training:
            return training.feed_forward(self, x)
        self._require_inference(x)
        return rt.like_input(self.forward_fused(rt.as_compute(x)), x)


class PreNorm(HipModule):
    """fn(LayerNorm(x)) (base_transformer.py:91-99); the residual is added by the caller (BaseEncoder)."""

    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn

    def forward(self, x, **kwargs):
        self._require_inference(x)
        return rt.like_input(self.fn.forward_fused(rt.as_compute(x), ln=self.norm, **kwargs), x)


class CavAttention(HipModule):
    """At every BEV pixel, multi-head attention over the agents (base_transformer.py:127-172).  It is the gathered window
    attention kernel with 1 x 1 windows: tokens of a window = the L agents' features at that pixel, key mask = com_mask."""

    def __init__(self, dim, heads, dim_head=64, dropout=0.1):
        super().__init__()
        if dim_head != 32:
            raise CobevtHipError("the HIP attention kernel is built for dim_head = 32")
        inner_dim = heads * dim_head
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.attend = nn.Softmax(dim=-1)
        self.to_qkv = nn.Linear(dim, inner_dim * 3, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner_dim, dim), nn.Dropout(dropout))

    def forward_fused(self, x, residual=None, ln=None, mask=None):
        """x (b, l, h, w, c) compute dtype (raw, with ln = the PreNorm LayerNorm to fold into to_qkv); mask (b, h, w, 1, l) or
        (b, l)-broadcastable; -> to_out(attention) (+ residual)"""
        b, l, h, w, c = x.shape
        inner = self.heads * 32
        qkv = ops.linear(x, rt.linear_plan(self, "qkv", self.to_qkv, ln=ln))
        out = torch.empty((b, l, h, w, inner), device=x.device, dtype=x.dtype)
        m = ops.tokmap(0, l, h, w, 1, 1)
        mk = None
        if mask is not None:
            mk = mask.to(torch.float32).expand(b, h, w, 1, l).reshape(b, h, w, l).contiguous()
        ops.window_attention(qkv, qkv, qkv, out, m, m, m, b, self.heads, self.scale, 3 * inner, 3 * inner, 3 * inner, inner,
                             koff=inner, voff=2 * inner, mask=mk)
        return ops.linear(out, rt.linear_plan(self, "out", self.to_out[0]), residual=residual)

    def forward(self, x, mask, prior_encoding=None):
        """x (B, L, H, W, C); mask (B, H, W, 1, L) (or (B, 1, 1, 1, L)) -> (B, L, H, W, C)"""
        self._require_inference(x, mask)
        return rt.like_input(self.forward_fused(rt.as_compute(x), mask=mask), x)


class RelTemporalEncoding(HipModule):
    """x + lin(emb[t * RTE_ratio]) (base_transformer.py:14-37): a sinusoid table of max_len delays behind a Linear.  t is a device
    integer tensor: (), one agent's delay as in the reference, or (B, L), every agent's at once; the gather stays on the device."""

    def __init__(self, n_hid, RTE_ratio, max_len=100, dropout=0.2):
        super().__init__()
        position = torch.arange(0., max_len).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, n_hid, 2) * -(math.log(10000.0) / n_hid))
        emb = nn.Embedding(max_len, n_hid)
        emb.weight.data[:, 0::2] = torch.sin(position * div_term) / math.sqrt(n_hid)
        emb.weight.data[:, 1::2] = torch.cos(position * div_term) / math.sqrt(n_hid)
        emb.requires_grad = False
        self.RTE_ratio = RTE_ratio
        self.emb = emb
        self.lin = nn.Linear(n_hid, n_hid)

    def encoding(self, t):
        """t integer tensor of any shape -> lin(emb[t * RTE_ratio]) (..., n_hid) fp32; indices outside the table are clamped into it"""
        idx = (t.long() * self.RTE_ratio).clamp(0, self.emb.num_embeddings - 1)
        return self.lin(self.emb(idx))

    def forward(self, x, t):
        enc = self.encoding(t)
        enc = enc[:, :, None, None, :] if t.dim() == 2 else enc.unsqueeze(0).unsqueeze(1)
        return x + enc.to(x.dtype)


class RTE(HipModule):
    """base_transformer.py:40-58 without its B x L Python loop: x (B, L, H, W, C) + the delay encoding of dts (B, L), one gather"""

    def __init__(self, dim, RTE_ratio=2):
        super().__init__()
        self.RTE_ratio = RTE_ratio
        self.emb = RelTemporalEncoding(dim, RTE_ratio=self.RTE_ratio)

    def forward(self, x, dts):
        if x.dim() != 5 or dts.dim() != 2 or tuple(dts.shape) != tuple(x.shape[:2]):
            raise CobevtHipError("RTE: x must be (B, L, H, W, C) and dts (B, L), got %s and %s" % (tuple(x.shape), tuple(dts.shape)))
        return self.emb(x, dts.to(torch.int))


class CavPositionalEncoding(HipModule):
    """x + pos_table[None, :, None, None, :] (base_transformer.py:61-89).  The reference adds the whole table, so L must be cav_num."""

    def __init__(self, d_hid, cav_num=5):
        super().__init__()
        self.register_buffer('pos_table', self._get_sinusoid_encoding_table(cav_num, d_hid))

    @staticmethod
    def _get_sinusoid_encoding_table(cav_num, d_hid):
        hid = np.arange(d_hid)
        table = np.arange(cav_num, dtype=np.float64)[:, None] / np.power(10000, 2 * (hid // 2) / d_hid)[None, :]
        table[:, 0::2] = np.sin(table[:, 0::2])
        table[:, 1::2] = np.cos(table[:, 1::2])
        return torch.from_numpy(table).float()

    def forward(self, x):
        if x.dim() != 5 or x.shape[1] != self.pos_table.shape[0] or x.shape[4] != self.pos_table.shape[1]:
            raise CobevtHipError("CavPositionalEncoding: x must be (B, L=%d, H, W, C=%d): the whole table is added, got %s"
                                 % (self.pos_table.shape[0], self.pos_table.shape[1], tuple(x.shape)))
        return x + self.pos_table[:x.shape[1]][None, :, None, None, :].to(x.dtype)


class HGTCavAttention(HipModule):
    """Per-pixel attention over the agents with projections chosen by agent type and a 32 x 32 relation matrix per (query type, key
    type, head) inside the score and the message (base_transformer.py:175-319).  The relation matrices fold into the key / value
    projections (ops.hgt_fold), so a row's own type selects ONE projection of width (1 + 2 T) inner, and the forward is three
    launches: ops.typed_linear (with the PreNorm LayerNorm), ops.hgt_attention, ops.typed_linear (with the residual).  The types are
    read on the device.  Inference only."""

    def __init__(self, dim, heads, num_types=2, num_relations=4, dim_head=64, dropout=0.1):
        super().__init__()
        if dim_head != 32:
            raise CobevtHipError("the HIP attention kernel is built for dim_head = 32")
        if num_types < 1 or num_relations < num_types * num_types:
            raise CobevtHipError("HGTCavAttention: num_relations=%d must be at least num_types^2 = %d (relation index a T + b)"
                                 % (num_relations, num_types * num_types))
        inner_dim = heads * dim_head
        if dim % 32 or dim > 512:
            raise CobevtHipError("HGTCavAttention: dim=%d must be a multiple of 32, at most 512 (ops.typed_linear)" % dim)
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.num_types = num_types
        self.attend = nn.Softmax(dim=-1)
        self.drop_out = nn.Dropout(dropout)
        self.k_linears = nn.ModuleList()
        self.q_linears = nn.ModuleList()
        self.v_linears = nn.ModuleList()
        self.a_linears = nn.ModuleList()
        self.norms = nn.ModuleList()
        for _ in range(num_types):
            self.k_linears.append(nn.Linear(dim, inner_dim))
            self.q_linears.append(nn.Linear(dim, inner_dim))
            self.v_linears.append(nn.Linear(dim, inner_dim))
            self.a_linears.append(nn.Linear(inner_dim, dim))
        self.relation_att = nn.Parameter(torch.Tensor(num_relations, heads, dim_head, dim_head))
        self.relation_msg = nn.Parameter(torch.Tensor(num_relations, heads, dim_head, dim_head))
        torch.nn.init.xavier_uniform_(self.relation_att)
        torch.nn.init.xavier_uniform_(self.relation_msg)

    @staticmethod
    def key_mask(mask, b, l, h, w):
        """mask in what CavAttention accepts - broadcastable to (B, H, W, 1, L) - -> contiguous fp32 (B, H, W, L); the reference's
        commented (B, H, W, L, 1) masks whole QUERY rows (NaN there) and is refused"""
        if mask.dim() >= 2 and mask.shape[-1] == 1 and mask.shape[-2] == l and l > 1:
            raise CobevtHipError("HGTCavAttention: a mask of shape %s ends in (L, 1): it would mask whole query rows (NaN in the "
                                 "reference); pass the key mask, broadcastable to (B, H, W, 1, L)" % (tuple(mask.shape),))
        try:
            return mask.to(torch.float32).expand(b, h, w, 1, l).reshape(b, h, w, l).contiguous()
        except RuntimeError:
            raise CobevtHipError("HGTCavAttention: mask of shape %s is not broadcastable to (B, H, W, 1, L) = %s"
                                 % (tuple(mask.shape), (b, h, w, 1, l))) from None

    def forward_fused(self, x, residual=None, ln=None, mask=None, prior_encoding=None):
        """x (B, L, H, W, C) compute dtype (raw, with ln = the PreNorm LayerNorm to fold into the projection); mask broadcastable to
        (B, H, W, 1, L); prior_encoding (B, L, H, W, 3) = [velocity, delay, type] -> a_linears[type](attention) (+ residual)"""
        if self.training:
            raise CobevtHipError("HGTCavAttention is inference-only: call .eval() first (training it is not built)")
        if prior_encoding is None or prior_encoding.dim() != 5 or prior_encoding.shape[-1] != 3 or tuple(prior_encoding.shape[:2]) != tuple(x.shape[:2]):
            raise CobevtHipError("HGTCavAttention: prior_encoding must be (B, L, H, W, 3) = [velocity, delay, type] for x %s, got %s"
                                 % (tuple(x.shape), None if prior_encoding is None else tuple(prior_encoding.shape)))
        b, l, h, w, c = x.shape
        types = prior_encoding[:, :, 0, 0, 2].to(torch.int32).contiguous()          # device slice + cast: no host read
        fold = ops.hgt_fold(self, ln=ln, dtype=x.dtype, device=x.device)
        mk = None if mask is None else self.key_mask(mask, b, l, h, w)
        proj = ops.typed_linear(x, fold.w_in, fold.b_in, types, h * w, ln_eps=None if ln is None else ln.eps)
        att = ops.hgt_attention(proj, types, self.heads, self.num_types, mask=mk)
        return ops.typed_linear(att, fold.w_out, fold.b_out, types, h * w, residual=residual)

    def forward(self, x, mask, prior_encoding):
        """x (B, L, H, W, C); mask broadcastable to (B, H, W, 1, L); prior_encoding (B, L, H, W, 3) -> (B, L, H, W, C)"""
        self._require_inference(x, mask, prior_encoding)
        return rt.like_input(self.forward_fused(rt.as_compute(x), mask=mask, prior_encoding=prior_encoding), x)


class BaseEncoder(HipModule):
    """base_transformer.py:321-339: depth x [PreNorm(CavAttention) + x, PreNorm(FeedForward) + x]"""

    def __init__(self, dim, depth, heads, dim_head, mlp_dim, dropout=0.):
        super().__init__()
        self.layers = nn.ModuleList([])
        for _ in range(depth):
            self.layers.append(nn.ModuleList([PreNorm(dim, CavAttention(dim, heads=heads, dim_head=dim_head, dropout=dropout)),
                                              PreNorm(dim, FeedForward(dim, mlp_dim, dropout=dropout))]))

    def forward_blhwc(self, x, mask):
        for attn, ff in self.layers:
            x = attn.fn.forward_fused(x, residual=x, ln=attn.norm, mask=mask)
            x = ff.fn.forward_fused(x, residual=x, ln=ff.norm)
        return x

    def forward(self, x, mask):
        self._require_inference(x, mask)
        return rt.like_input(self.forward_blhwc(rt.as_compute(x), mask), x)


class BaseTransformer(HipModule):
    """base_transformer.py:342-362: the encoder, then the ego agent's map.  x (B, L, H, W, C) -> (B, H, W, C)"""

    def __init__(self, args):
        super().__init__()
        self.encoder = BaseEncoder(args["dim"], args["depth"], args["heads"], args["dim_head"], args["mlp_dim"], args["dropout"])

    def forward_blhwc(self, x, mask):
        return self.encoder.forward_blhwc(x, mask)[:, 0]

    def forward(self, x, mask):
        self._require_inference(x, mask)
        return rt.like_input(self.forward_blhwc(rt.as_compute(x), mask), x)
