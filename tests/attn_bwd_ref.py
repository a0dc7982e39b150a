"""Float64 interval reference of the window-attention backward kernels (tests/test_attn_bwd_bounds.py on the CPU,
tests/test_attn_bwd_bounds_gpu.py on the device).

The function under test, cut at HBM.  cobevt_window_attention_bwd is a function of its operands exactly as stored: q, k, v, out, lse
(base 2, [B][L][heads][Nq]), dout, optionally dlse, bias_table and mask, the token maps, scale, drop_p and the seed.  `out` and `lse` are
OPERANDS: the case builder evaluates the forward in float64, rounds `out` to the storage type and `lse` to fp32, and the backward
reference takes the rounded tensors as exact inputs - P = exp2(z log2e - lse) is not renormalised, D = rowsum(dO o O) - dlse uses the
stored O.  No forward kernel runs in any of these tests.  For one (batch, window, head), in float64:
    z2 = (Q K^T) scale log2e + bias[rel(q, k)] log2e      P = exp2(z2 - lse) on the visible keys, 0 on the others
    dP = dO V^T     D = rowsum(dO o O) - dlse     dZ = P (keep' dP - D)     keep' = keep / (1 - p)
    dV = (P keep')^T dO     dK = scale dZ^T Q     dQ = scale dZ K     dbias[rel(q, k), head] += dZ
The index arithmetic is restated below from csrc/attn_common.hpp (tok_coord, tok_pixel, tok_row, the two relative-bias terms,
key_visible of attention_bwd.hip for modes 0, 1 and 2, attn_keep with its murmur finaliser); the GPU file ties the restatement to the
library's hooks bit for bit, once.

The bound: the conventions of section 3t / conv_bounds_ref.  U = 2^-23 (one ulp of fp32, twice the unit roundoff: "one rounding" is a
relative U whether or not the compiler contracts an fma); a contraction of n terms in ANY order costs n U sum|a||b|; operand errors
propagate as sum(|a| e_b + e_a |b| + e_a e_b); an interval is closed by `rne` wherever the kernel rounds.  Stage by stage, as the four
kernels of attention_bwd.hip are written:
  S, dP    32-term products: e_S = 32 U |Q||K|^T, e_dP = 32 U |dO||V|^T.  On the bf16 matrix path the tiles are rounded to bf16 as they
           are staged (pack8f4 / pack_bf2: Q, K, V and dO, every use of them in the five products).  That rounding is deterministic: the
           reference applies it to the operands - it is part of the specification, not of the width - and bf16 x bf16 products are exact
           in the fp32 accumulator, so the same 32 U covers the accumulation alone.
  z - lse  sl2 = scale * log2e (the fp32 constant within 2^-24 of log2e, one rounding of the product), z = S sl2 (one), bias_col =
           bias * log2e (constant + one), z += bias_col (one), z - lse (one).  An ABSOLUTE error on a base-2 exponent,
               delta = c e_S + 2 U |S c| + 2 U |b| + U |S c + b| + U |z2 - lse|,   c = scale log2e, b = bias log2e
           which grows with |z| and |lse|.
  P        e_P = P (2^delta - 1) + U P 2^delta + 2^-126: v_exp_f32 taken at 1 ulp - AMD's documented figure, the assumption of section 3u
           and equally UNCHECKED here (the GPU file prints how much of the bound the kernels use) - and a result below the normal range
           may be flushed.
  D        32 products summed in two halves with one cross-lane add (kv / kv2: 16 + 16 per lane pair; q / q4: 16 + 16 per half-wave),
           minus dlse: e_D = 32 U sum|dO||O| + U |D|.  With 0x400 kv2 reads the value q4 stored: the same bound, both being covered.
           On the bf16 matrix path D is still formed from the fp32 values as loaded (bf16 storage: the bf16 values stored).
  dZ       keep' = 1 / (1 - p) in fp32: two roundings, 3 U keep' (exactly 1 without dropout).  t1 = keep' dP, t2 = t1 - D, dZ = P t2:
               e_1 = keep' e_dP + e_k |dP| + U |t1|,  e_2 = e_1 + e_D + U |t2|,  e_dZ = P e_2 + e_P |t2| + e_P e_2 + U |dZ|
           and P keep' likewise: e_P keep' + e_k P + U P keep'.
  bf16     path: P keep' and dZ are rounded to bf16 before the row-contracting products (pack_acc8).  Their intervals are closed there,
           [rne(x - e), rne(x + e)], as Ref._close does, and travel as (mid, half-width).
  dV, dK, dQ   dV = sum_q (P keep') dO, dK = scale sum_q dZ Q, dQ = scale sum_k dZ K: n = Nq resp. Nk (the zero rows of a ragged tile add
           nothing), cross-wave (LDS) and cross-tile sums included in the any-order bound: n U sum(|a| + d_a)|b| + sum d_a |b|; the final
           multiply by scale is one rounding, U |result|.
  stores   fp32: [rne32(ref - e), rne32(ref + e)]; bf16 storage: [rne(lo), rne(hi)], and O / dO enter D as the bf16 values stored.
  dbias    sum of dZ (the fp32 value, before any bf16 rounding) over all (batch, window, query, key) pairs of a table row and head; the
           atomics add in any order and on two levels (LDS copy, then global): n U sum|dZ| + sum e_dZ with n = the contributing pairs.

AttnBwdEmul is a correct kernel on the CPU: fp32 torch arithmetic with the same roundings at the same points, the summation order of
every contraction a parameter (ORDERS), and `fault=` one of FAULTS (tests/test_attn_bwd_bounds.py shows each leaving the interval).

Left out by name: fully masked query rows (lse = -inf, no defined gradient: the builder asserts every row has a visible key); the
forward families (cobevt_window_attention_lse, attention.hip, attention_resident.hip, and swap_stage.hip's inner attention), whose
gates stay as they are."""
import math
import zlib

import numpy as np
import torch

from conv_bounds_ref import (U, F64, Interval, rne, bias_stat, position, outside, error_over_e, truncate_bf16,  # noqa: F401
                             BIAS_LIMIT, BIAS_MIN_N)

F32, BF16 = torch.float32, torch.bfloat16
LOG2E = 1.4426950408889634
FP32_CODE, BF16_CODE = 1, 0                                   # ops.FP32 / ops.BF16, restated: dims[0] & 0xff
# path -> (dims[0], reference key).  The kernels reached, from reading the entry: DESIGN.md section 3z
PATHS = {"fp32": (FP32_CODE, "fp32"), "bf16mm": (FP32_CODE | 0x100, "bf16mm"), "bf16mm_1tile": (FP32_CODE | 0x300, "bf16mm"),
         "bf16st": (BF16_CODE | 0x100, "bf16st"), "bf16st_scr": (BF16_CODE | 0x100 | 0x400, "bf16st")}
ORDERS = ("forward", "reverse", "tile", "perm")
FAULTS = ("drop_last_q_tile", "pad_keys_visible", "mask_cam_ignored", "bias_qmap_window", "dlse_sign", "lse_natural", "dv_without_keep",
          "dk_no_scale", "trunc_bf16", "dbias_second_window", "dscr_next_head", "mask_mode0_index")
WIDTH_MEDIAN, WIDTH_SHARE = 2.0 ** -6, 0.05                   # the bf16 width condition of section 3u


def store_of(refkey):
    return BF16 if refkey == "bf16st" else F32


# ----------------------------------------------------------------------------------------------
# the index arithmetic of csrc/attn_common.hpp, restated (numpy int64; a map is (mode, ncam, HH, WW, w1, w2, X, Y))
# ----------------------------------------------------------------------------------------------
def ntok(m):
    return m[1] * m[4] * m[5]


def nwin(m):
    return m[6] * m[7]


def tok_coord(m, t):
    ws = m[4] * m[5]
    cam = t // ws
    rem = t - cam * ws
    i = rem // m[5]
    return cam, i, rem - i * m[5]


def tok_pixel(m, l, i, j):
    x = l // m[7]
    y = l - x * m[7]
    if m[0] == 1:
        return i * m[6] + x, j * m[7] + y
    return x * m[4] + i, y * m[5] + j


def tok_row(m, b, l, cam, i, j):
    if m[0] == 2:
        return (((b * m[1] + cam) * (m[6] * m[7]) + l) * m[4] + i) * m[5] + j
    ph, pw = tok_pixel(m, l, i, j)
    return ((b * m[1] + cam) * m[2] + ph) * m[3] + pw


def map_rows(m, batch):
    return batch * m[1] * (nwin(m) * m[4] * m[5] if m[0] == 2 else m[2] * m[3])


def index_map(m, batch):
    """int64 (batch, L, N): the row of token t of window l of batch b"""
    b = np.arange(batch, dtype=np.int64)[:, None, None]
    l = np.arange(nwin(m), dtype=np.int64)[None, :, None]
    cam, i, j = tok_coord(m, np.arange(ntok(m), dtype=np.int64)[None, None, :])
    return tok_row(m, b, l, cam, i, j)


def rel_bias_query_term(km, bias_L, cam, i, j):
    return ((cam + bias_L - 1) * (2 * km[4] - 1) + i + km[4] - 1) * (2 * km[5] - 1) + j + km[5] - 1


def rel_bias_key_term(km, cam, i, j):
    return (cam * (2 * km[4] - 1) + i) * (2 * km[5] - 1) + j


def bias_index(qmap, kmap, bias_L, wmap=None, nk_pad=0):
    """int64 (Nq, Nk [+ pad]): the table row of every (query, key) pair; the window extents are the KEY map's (wmap: the fault that takes
    another map's).  A pad key has the coordinates of token 0, as the kernels evaluate it."""
    wm = kmap if wmap is None else wmap
    tk = np.arange(ntok(kmap) + nk_pad, dtype=np.int64)
    tk = np.where(tk < ntok(kmap), tk, 0)
    qt = rel_bias_query_term(wm, bias_L, *tok_coord(qmap, np.arange(ntok(qmap), dtype=np.int64)))
    kt = rel_bias_key_term(wm, *tok_coord(kmap, tk))
    return qt[:, None] - kt[None, :]


def bias_rows(kmap, bias_L):
    return (2 * bias_L - 1) * (2 * kmap[4] - 1) * (2 * kmap[5] - 1)


def key_visible(mask, kmap, batch, mode0_index=False):
    """bool (batch, L, Nk) from the fp32 mask: (B, HH, WW, ncam) for modes 0 / 1, (B, L, w1, w2, ncam) for mode 2"""
    flat = np.asarray(mask, dtype=np.float32).reshape(-1)
    b = np.arange(batch, dtype=np.int64)[:, None, None]
    l = np.arange(nwin(kmap), dtype=np.int64)[None, :, None]
    cam, i, j = tok_coord(kmap, np.arange(ntok(kmap), dtype=np.int64)[None, None, :])
    if kmap[0] == 2 and not mode0_index:
        idx = (((b * nwin(kmap) + l) * kmap[4] + i) * kmap[5] + j) * kmap[1] + cam
    else:
        m0 = (0,) + tuple(kmap[1:]) if kmap[0] == 2 else kmap
        ph, pw = tok_pixel(m0, l, i, j)
        idx = ((b * kmap[2] + ph) * kmap[3] + pw) * kmap[1] + cam
    return flat[idx] != 0


_M32 = np.uint64(0xFFFFFFFF)


def mix32(x):
    """murmur3 finaliser on uint64 arrays holding 32-bit values"""
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & _M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & _M32
    return x ^ (x >> np.uint64(16))


def attn_keep(batch, L, heads, nq, nk, drop_p, seed):
    """bool (batch, L, heads, nq, nk): uniform 32-bit hash >= p 2^32, the comparison in fp32 as the kernel makes it; seed = the host seed
    plus the device word, modulo 2^32"""
    bl = np.arange(batch * L * heads, dtype=np.uint64).reshape(batch, L, heads, 1)
    row = bl * np.uint64(nq) + np.arange(nq, dtype=np.uint64)[None, None, None, :]
    hrow = mix32((row & _M32) ^ mix32((row >> np.uint64(32)) ^ np.uint64(seed & 0xFFFFFFFF)))
    tk = (np.arange(nk, dtype=np.uint64) * np.uint64(0x9E3779B1)) & _M32
    u = mix32(hrow[..., None] ^ tk)
    return u.astype(np.float32) * np.float32(2.3283064365386963e-10) >= np.float32(drop_p)


def kv_nsplit(case, path):
    """the entry's window split, restated: about 2048 workgroups in all, nsplit of them share the windows of one (head, key tile position)"""
    nkt = (case.Nk + 31) // 32
    flags, ref = PATHS[path]
    kv2 = bool(flags & 0x100) and (nkt >= 2 or ref == "bf16st") and not flags & 0x200
    per = case.heads * ((nkt + 1) // 2 if kv2 else nkt) * case.B
    return max(1, min(case.L, (2048 + per - 1) // per))


# ----------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------
class Case(object):
    """name, the query / key token maps (the output map is the query map), B, heads, the paths the row runs in, bias_L (0: no bias), mask,
    dropout (drop_p, host seed, device seed word), dlse, layout (None | "a" | "b"), outlier (logits of case 8), coherent (dout and v
    of many_windows, see _coherent_dp)"""

    def __init__(self, name, qmap, kmap, B, heads, paths, bias_L=0, mask=False, drop_p=0.0, seed=0, seed_dev=0, dlse=False, layout=None,
                 outlier=False, coherent=False):
        self.name, self.qmap, self.kmap, self.omap, self.B, self.heads, self.paths = name, tuple(qmap), tuple(kmap), tuple(qmap), B, heads, paths
        self.bias_L, self.mask, self.drop_p, self.seed, self.seed_dev, self.dlse = bias_L, mask, drop_p, seed, seed_dev, dlse
        self.layout, self.outlier, self.coherent = layout, outlier, coherent
        self.L, self.Nq, self.Nk, self.d = nwin(self.qmap), ntok(self.qmap), ntok(self.kmap), heads * 32
        self.Rq, self.Rk = map_rows(self.qmap, B), map_rows(self.kmap, B)
        self.bias_rows = bias_rows(self.kmap, bias_L) if bias_L else 0
        self.scale = float(np.float32(32.0 ** -0.5))
        assert nwin(self.kmap) == self.L

    def __repr__(self):
        return self.name


def _win(mode, ncam, hh, ww, w1, w2):
    return (mode, ncam, hh, ww, w1, w2, hh // w1, ww // w2)


def _cases():
    r90 = _win(0, 3, 12, 20, 6, 5)
    one64 = _win(0, 1, 8, 8, 8, 8)
    return [
        Case("one_tile_25", _win(0, 1, 10, 10, 5, 5), _win(0, 1, 10, 10, 5, 5), 1, 1, ("fp32", "bf16mm", "bf16mm_1tile", "bf16st", "bf16st_scr")),
        Case("ragged_90", r90, r90, 2, 2, ("fp32", "bf16mm", "bf16mm_1tile", "bf16st", "bf16st_scr"), bias_L=3, mask=True),
        Case("grid_245", _win(1, 5, 14, 14, 7, 7), _win(1, 5, 14, 14, 7, 7), 2, 4, ("fp32", "bf16mm", "bf16st_scr"), bias_L=5, mask=True),
        Case("cross_48_108", _win(0, 3, 8, 8, 4, 4), _win(0, 3, 12, 12, 6, 6), 2, 2, ("fp32", "bf16mm"), bias_L=3, dlse=True),
        Case("stored_partition", _win(2, 2, 8, 8, 4, 4), _win(2, 2, 8, 8, 4, 4), 2, 2, ("fp32", "bf16mm", "bf16st"), mask=True),
        Case("dropout_64", one64, one64, 2, 2, ("fp32", "bf16mm_1tile"), bias_L=1, drop_p=0.3, seed=0x5EED1234, seed_dev=77),
        Case("dropout_64_128", one64, _win(0, 2, 8, 8, 8, 8), 2, 2, ("bf16mm",), bias_L=2, drop_p=0.3, seed=0xFFFFFFF0, seed_dev=0x31),
        Case("many_windows", _win(0, 1, 192, 192, 4, 4), _win(0, 1, 192, 192, 4, 4), 1, 1, ("fp32", "bf16st"), bias_L=1, coherent=True),
        Case("outlier_logits", r90, r90, 2, 2, ("fp32", "bf16mm"), bias_L=3, mask=True, outlier=True),
        Case("layout_a", r90, r90, 2, 2, ("fp32", "bf16st_scr"), bias_L=3, mask=True, layout="a"),
        Case("layout_b", r90, r90, 2, 2, ("fp32", "bf16st_scr"), bias_L=3, mask=True, layout="b"),
    ]


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
CASE_PATHS = [(c, p) for c in CASES for p in c.paths]
# restatement of the entry's ceil(2048 / (heads nkt B)): many_windows is the row whose workgroups walk a second window
assert kv_nsplit(BY_NAME["many_windows"], "fp32") == 2048 < BY_NAME["many_windows"].L and BY_NAME["many_windows"].L % 2048 != 0
assert kv_nsplit(BY_NAME["many_windows"], "bf16st") == 2048
assert all(kv_nsplit(c, p) == c.L for c, p in CASE_PATHS if c.name != "many_windows")


def case_id(cp):
    return "%s-%s" % (cp[0].name, cp[1])


def layout_offsets(case, path):
    """(ld, (qoff, koff, voff, ooff)) of layout b: dims[4..7] and dims[8..11]"""
    return case.d + 32, ((8, 16, 8, 16) if PATHS[path][1] == "bf16st" else (4, 8, 12, 16))


def case_dims(case, path):
    """the dims array the entry must receive (include/cobevt_hip.h: dtype | flags, B, L, heads, the four row strides, the four column
    offsets, bias mode / rows / L, mean_q, the three maps)"""
    d = case.d
    ld, off = (d, d, d, d), (0, 0, 0, 0)
    if case.layout == "a":
        ld = (3 * d, 3 * d, 3 * d, d)
    elif case.layout == "b":
        w, off = layout_offsets(case, path)
        ld = (w, w, w, w)
    return ([PATHS[path][0], case.B, case.L, case.heads] + list(ld) + list(off)
            + [1 if case.bias_L else 0, case.bias_rows, case.bias_L if case.bias_L else 1, 0] + list(case.qmap) + list(case.kmap) + list(case.omap))


def _gather(rows, idx, heads):
    """(R, heads * 32), (B, L, N) -> (B, L, heads, N, 32)"""
    b, l, n = idx.shape
    return rows[idx.reshape(-1)].reshape(b, l, n, heads, 32).permute(0, 1, 3, 2, 4).contiguous()


def _scatter(g, idx, nrows):
    b, l, h, n, _ = g.shape
    out = torch.full((nrows, h * 32), float("nan"), dtype=g.dtype)
    out[idx.reshape(-1)] = g.permute(0, 1, 3, 2, 4).reshape(b * l * n, h * 32)
    return out


def _coherent_dp(case, gen):
    """dout and v of many_windows, gathered.  A table row of that case sums dZ over 2,304 windows x up to 16 pairs; with operands of random
    sign the sum cancels (sum_k dZ = 0 in every query row) while the any-order bound n U sum|dZ| does not, and the interval is 0.3 |ref|
    wide in the median.  So dP is made a function of the RELATIVE position, which is what a table row collects: with
        dout_q = s (a0 qi', a0 qj', a0, noise),   v_k = s (a, b, -(a ki' + b kj'), noise),   i' = i - (w - 1) / 2,   s = +-1 per window
    dP[q, k] = a0 (a (qi - ki) + b (qj - kj)) + noise: dZ = P (dP - D) then has one sign per table row wherever |dP| stands clear of D,
    and dout keeps a random sign and O(1) size.  (The section 3u device: operands chosen so that the width starts where the kernel rounds.)"""
    B, L, H = case.B, case.L, case.heads
    rnd = lambda n: torch.randn(B, L, H, n, 32, generator=gen, dtype=F64) * 0.1      # noqa: E731
    s = torch.where(torch.rand(B, L, 1, 1, generator=gen) < 0.5, -1.0, 1.0).to(F64)
    a0, a, b = 0.5, 0.5, 2.0
    _, qi, qj = (torch.from_numpy(t).to(F64) for t in tok_coord(case.qmap, np.arange(case.Nq)))
    _, ki, kj = (torch.from_numpy(t).to(F64) for t in tok_coord(case.kmap, np.arange(case.Nk)))
    ci, cj = (case.kmap[4] - 1) / 2, (case.kmap[5] - 1) / 2
    dO, V = rnd(case.Nq), rnd(case.Nk)
    dO[..., 0], dO[..., 1], dO[..., 2] = a0 * (qi - ci), a0 * (qj - cj), a0
    V[..., 0], V[..., 1], V[..., 2] = a, b, -(a * (ki - ci) + b * (kj - cj))
    return dO * s[..., None], V * s[..., None]


_OPS = {}


def operands(case, store):
    """the entry's operands as stored (row matrices in `store`, fp32 lse / dlse / table / mask), the index tables, and the builder's
    conditions asserted; computed once per (case, storage type)"""
    key = (case.name, store)
    if key in _OPS:
        return _OPS[key]
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    B, L, H, Nq, Nk, d = case.B, case.L, case.heads, case.Nq, case.Nk, case.d
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)          # noqa: E731
    st = lambda t: t.to(F32).to(store)                                 # noqa: E731
    qidx, kidx = torch.from_numpy(index_map(case.qmap, B)), torch.from_numpy(index_map(case.kmap, B))
    for idx, n in ((qidx, case.Rq), (kidx, case.Rk)):                  # a partition: every row of the map belongs to one (window, token)
        assert idx.numel() == n and bool((torch.sort(idx.reshape(-1))[0] == torch.arange(n)).all())
    a = math.sqrt(1.3)
    q, k, v = st(rnd(case.Rq, d) * a), st(rnd(case.Rk, d) * a), st(rnd(case.Rk, d))
    if case.coherent:
        dO_c, V_c = _coherent_dp(case, g)
        v = st(_scatter(V_c, kidx, case.Rk))
    table = (rnd(case.bias_rows, H) * 0.5).to(F32) if case.bias_L else None
    mask = vis = None
    if case.mask:
        km = case.kmap
        shape = (B, L, km[4], km[5], km[1]) if km[0] == 2 else (B, km[2], km[3], km[1])
        mask = (torch.rand(*shape, generator=g) < 0.7).to(F32)
        mask[..., 0] = 1.0                                            # the ego camera is visible: every query row has a visible key
        vis = torch.from_numpy(key_visible(mask.numpy(), km, B))
    else:
        vis = torch.ones(B, L, Nk, dtype=torch.bool)
    bidx = torch.from_numpy(bias_index(case.qmap, case.kmap, case.bias_L)) if case.bias_L else None
    if bidx is not None:
        assert int(bidx.min()) >= 0 and int(bidx.max()) < case.bias_rows
    if case.outlier:
        # a tenth of the query rows point at one visible key (of the ego camera) with z log2e ~ 60: P > 0.999 there, dP - D cancels
        Qg, Kg = _gather(q.to(F64), qidx, H), _gather(k.to(F64), kidx, H)
        hot = torch.rand(B, L, H, Nq, generator=g) < 0.1
        tgt = torch.randint(0, case.kmap[4] * case.kmap[5], (B, L, H, Nq), generator=g)
        kt = torch.gather(Kg, 3, tgt[..., None].expand(B, L, H, Nq, 32))
        Qg = torch.where(hot[..., None], kt * (60.0 / LOG2E / case.scale) / (kt * kt).sum(-1, keepdim=True), Qg)
        q = st(_scatter(Qg, qidx, case.Rq))
    keep = None
    if case.drop_p > 0:
        keep = torch.from_numpy(attn_keep(B, L, H, Nq, Nk, case.drop_p, case.seed + case.seed_dev))
    # ---- the forward in float64 from the operands as stored; out and lse are then operands of the backward
    Qg, Kg, Vg = _gather(q.to(F64), qidx, H), _gather(k.to(F64), kidx, H), _gather(v.to(F64), kidx, H)
    z2 = (Qg @ Kg.transpose(-1, -2)) * (case.scale * LOG2E)
    if bidx is not None:
        z2 = z2 + table.to(F64).t()[:, bidx.reshape(-1)].reshape(1, 1, H, Nq, Nk) * LOG2E
    visb = vis[:, :, None, None, :]
    assert bool(vis.any(-1).all()), "a fully masked query row: lse = -inf, no defined gradient (left out by name)"
    z2m = torch.where(visb, z2, torch.full_like(z2, -float("inf")))
    mx = z2m.max(-1, keepdim=True)[0]
    lse64 = mx[..., 0] + torch.log2(torch.exp2(z2m - mx).sum(-1))
    P = torch.exp2(z2m - lse64[..., None])
    kp = 1.0 if keep is None else keep.to(F64) / (1.0 - float(np.float32(case.drop_p)))
    out = st(_scatter((P * kp) @ Vg, qidx, case.Rq))
    lse = lse64.to(F32)
    dout = st(_scatter(dO_c, qidx, case.Rq)) if case.coherent else st(rnd(case.Rq, d))
    dlse = rnd(B, L, H, Nq).to(F32) if case.dlse else None
    sd = float((z2[visb.expand_as(z2)] / LOG2E).std())
    if case.outlier:
        top, share = float(z2[visb.expand_as(z2)].abs().max()), float((P.max(-1)[0] > 0.999).double().mean())
        assert 50.0 <= top <= 75.0 and 0.08 <= share <= 0.13, (top, share)
    else:
        assert 1.0 <= sd <= 2.0, sd
    if store == BF16:
        assert all(t.dtype == BF16 for t in (q, k, v, out, dout))
    o = dict(q=q, k=k, v=v, out=out, dout=dout, lse=lse, dlse=dlse, table=table, mask=mask, qidx=qidx, kidx=kidx, vis=vis, bidx=bidx, keep=keep,
             logit_std=sd)
    _OPS[key] = o
    return o


# ----------------------------------------------------------------------------------------------
# the float64 reference with its intervals
# ----------------------------------------------------------------------------------------------
def _bf(t):
    return t.to(F32).to(BF16).to(F64)


def _iv(ref, e, store):
    return Interval(ref, None, e, rne(ref - e, store), rne(ref + e, store))


_REFS = {}


def reference(case, path):
    """-> {"dq", "dk", "dv": Interval of (rows, heads * 32) matrices, "dbias": Interval (table rows, heads) | None}, once per (case, key)"""
    refkey = PATHS[path][1]
    key = (case.name, refkey)
    if key in _REFS:
        return _REFS[key]
    store, bfmm = store_of(refkey), refkey != "fp32"
    op = operands(case, store)
    B, L, H, Nq, Nk = case.B, case.L, case.heads, case.Nq, case.Nk
    T = lambda t: t.transpose(-1, -2)                                  # noqa: E731
    Q, dO, O = (_gather(op[n].to(F64), op["qidx"], H) for n in ("q", "dout", "out"))
    K, V = (_gather(op[n].to(F64), op["kidx"], H) for n in ("k", "v"))
    Qm, Km, Vm, dOm = (_bf(t) for t in (Q, K, V, dO)) if bfmm else (Q, K, V, dO)
    vis = op["vis"][:, :, None, None, :].to(F64)
    lse = op["lse"].to(F64)[..., None]
    c = case.scale * LOG2E
    S, eS = Qm @ T(Km), 32 * U * (Qm.abs() @ T(Km.abs()))
    dP, edP = dOm @ T(Vm), 32 * U * (dOm.abs() @ T(Vm.abs()))
    zs = S * c
    b = 0.0
    if case.bias_L:
        b = op["table"].to(F64).t()[:, op["bidx"].reshape(-1)].reshape(1, 1, H, Nq, Nk) * LOG2E
    z = zs + b
    t = z - lse
    delta = c * eS + 2 * U * zs.abs() + 2 * U * abs(b) + U * z.abs() + U * t.abs()
    P = torch.exp2(t) * vis
    eP = (P * (torch.exp2(delta) - 1) + U * P * torch.exp2(delta) + 2.0 ** -126) * vis
    D = (dO * O).sum(-1)
    eD = 32 * U * (dO.abs() * O.abs()).sum(-1)
    if op["dlse"] is not None:
        D = D - op["dlse"].to(F64)
    eD = (eD + U * D.abs())[..., None]
    D = D[..., None]
    if case.drop_p > 0:
        kp = op["keep"].to(F64) / (1.0 - float(np.float32(case.drop_p)))
        ek = 3 * U * kp
        t1 = kp * dP
        e1 = kp * edP + ek * dP.abs() + U * t1.abs()
        Pk, ePk = P * kp, eP * kp + ek * P + U * P * kp
    else:
        t1, e1, Pk, ePk = dP, edP, P, eP
    t2 = t1 - D
    e2 = e1 + eD + U * t2.abs()
    dZ = P * t2
    edZ = P * e2 + eP * t2.abs() + eP * e2 + U * dZ.abs()
    if bfmm:                                                           # pack_acc8: closed in bf16 before the row-contracting products
        def close(x, e):
            lo, hi = _bf(x - e), _bf(x + e)
            return (lo + hi) / 2, (hi - lo) / 2
        (Pc, dPc), (Zc, dZc) = close(Pk, ePk), close(dZ, edZ)
    else:
        Pc, dPc, Zc, dZc = Pk, ePk, dZ, edZ
    sc = case.scale
    dV = T(Pc) @ dOm
    edV = Nq * U * (T(Pc.abs() + dPc) @ dOm.abs()) + T(dPc) @ dOm.abs()
    dK = sc * (T(Zc) @ Qm)
    edK = sc * (Nq * U * (T(Zc.abs() + dZc) @ Qm.abs()) + T(dZc) @ Qm.abs())
    edK = edK + U * dK.abs()
    dQ = sc * (Zc @ Km)
    edQ = sc * (Nk * U * ((Zc.abs() + dZc) @ Km.abs()) + dZc @ Km.abs())
    edQ = edQ + U * dQ.abs()
    r = {}
    for name, val, e, idx, n in (("dq", dQ, edQ, op["qidx"], case.Rq), ("dk", dK, edK, op["kidx"], case.Rk), ("dv", dV, edV, op["kidx"], case.Rk)):
        r[name] = _iv(_scatter(val, idx, n), _scatter(e, idx, n), store)
    r["dbias"] = None
    if case.bias_L:
        flat = (op["bidx"].reshape(1, Nq * Nk) * H + torch.arange(H).reshape(H, 1)).reshape(1, 1, H, Nq, Nk).expand(B, L, H, Nq, Nk).reshape(-1)
        acc = lambda x: torch.zeros(case.bias_rows * H, dtype=F64).index_add_(0, flat, (x * vis).reshape(-1)).reshape(case.bias_rows, H)   # noqa: E731
        n = acc(torch.ones_like(dZ))
        ref = acc(dZ)
        r["dbias"] = _iv(ref, n * U * acc(dZ.abs()) + acc(edZ) + U * ref.abs(), F32)
    _REFS[key] = r
    return r


def width_stats(iv):
    """(median of (hi - lo) / |ref|, share of the elements wider than 2^-5 |ref| + 2^-8 max|ref|)"""
    w, a = iv.hi - iv.lo, iv.ref.abs()
    return float((w / a.clamp_min(1e-300)).median()), float((w > 2.0 ** -5 * a + 2.0 ** -8 * a.max()).double().mean())


# ----------------------------------------------------------------------------------------------
# a correct kernel on the CPU, and the faults
# ----------------------------------------------------------------------------------------------
class AttnBwdEmul(object):
    """fp32 torch arithmetic with the kernels' roundings at the kernels' points.  order: "forward" | "reverse" | "tile" (32 at a time, the
    tiles dealt round robin to four accumulators that meet as a0 + ((a1 + a2) + a3), as the waves of the kv / q kernels do; a 32-term
    product in pairs, as one MFMA step takes them) | "perm" (a seeded permutation).  fault: one of FAULTS."""

    def __init__(self, order="forward", fault=None, seed=1):
        assert order in ORDERS and (fault is None or fault in FAULTS)
        self.order, self.fault, self.gen = order, fault, torch.Generator().manual_seed(seed)

    def _sum(self, term, n):
        if self.order == "tile":
            if n == 32:
                acc = None
                for i in range(0, 32, 2):
                    p = term(i) + term(i + 1)
                    acc = p if acc is None else acc + p
                return acc
            acc = [None] * 4
            for i in range(n):
                w = (i // 32) % 4
                acc[w] = term(i) if acc[w] is None else acc[w] + term(i)
            live = [a for a in acc if a is not None]
            if len(live) == 1:
                return live[0]
            rest = live[1]
            for a in live[2:]:
                rest = rest + a
            return live[0] + rest
        idx = list(range(n))
        if self.order == "reverse":
            idx.reverse()
        elif self.order == "perm":
            idx = torch.randperm(n, generator=self.gen).tolist()
        acc = None
        for i in idx:
            acc = term(i) if acc is None else acc + term(i)
        return acc

    def run(self, case, path):
        """-> {"dq", "dk", "dv", "dbias"}: the stored values as float64"""
        refkey, fault = PATHS[path][1], self.fault
        store, bfmm = store_of(refkey), refkey != "fp32"
        op = operands(case, store)
        B, L, H, Nq, Nk = case.B, case.L, case.heads, case.Nq, case.Nk
        pad = (-Nk) % 32
        Nkp = Nk + pad
        padk = lambda t: torch.nn.functional.pad(t, (0, 0, 0, pad))      # noqa: E731
        rb = (lambda t: t.to(BF16).to(F32)) if bfmm else (lambda t: t)     # noqa: E731
        Q, dO, O = (_gather(op[n].to(F32), op["qidx"], H) for n in ("q", "dout", "out"))
        K, V = (padk(_gather(op[n].to(F32), op["kidx"], H)) for n in ("k", "v"))
        Qm, Km, Vm, dOm = rb(Q), rb(K), rb(V), rb(dO)
        vis = op["vis"]
        if fault == "mask_cam_ignored":
            cam = tok_coord(case.kmap, np.arange(Nk))[0]
            vis = vis | torch.from_numpy(cam == case.kmap[1] - 1)[None, None, :]
        if fault == "mask_mode0_index":
            vis = torch.from_numpy(key_visible(op["mask"].numpy(), case.kmap, B, mode0_index=True))
        vis = torch.nn.functional.pad(vis, (0, pad), value=(fault == "pad_keys_visible"))[:, :, None, None, :]
        S = self._sum(lambda i: Qm[..., :, None, i] * Km[..., None, :, i], 32)
        dP = self._sum(lambda i: dOm[..., :, None, i] * Vm[..., None, :, i], 32)
        sl2 = torch.tensor(case.scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
        z = S * sl2
        bflat = None
        if case.bias_L:
            wmap = case.qmap if fault == "bias_qmap_window" else None
            bidx = torch.from_numpy(bias_index(case.qmap, case.kmap, case.bias_L, wmap, pad))
            bidx = bidx.clamp(0, case.bias_rows - 1)
            col = op["table"] * torch.tensor(LOG2E, dtype=F32)
            z = z + col.t()[:, bidx.reshape(-1)].reshape(1, 1, H, Nq, Nkp)
            bflat = (bidx.reshape(1, Nq * Nkp) * H + torch.arange(H).reshape(H, 1)).reshape(1, 1, H, Nq, Nkp)
        lse = op["lse"][..., None]
        if fault == "lse_natural":
            lse = lse * torch.tensor(LOG2E, dtype=F32)
        zero = torch.zeros((), dtype=F32)
        P = torch.where(vis, torch.exp2(z - lse), zero)
        prod = dO * O
        if self.order == "tile":
            D = self._sum(lambda i: prod[..., i], 16) + self._sum(lambda i: prod[..., 16 + i], 16)
        else:
            D = self._sum(lambda i: prod[..., i], 32)
        if op["dlse"] is not None:
            D = D + op["dlse"] if fault == "dlse_sign" else D - op["dlse"]
        if fault == "dscr_next_head":
            D = torch.roll(D, -1, 2)
        D = D[..., None]
        if case.drop_p > 0:
            p32 = torch.tensor(case.drop_p, dtype=F32)
            kp = torch.where(torch.nn.functional.pad(op["keep"], (0, pad), value=False), 1.0 / (1.0 - p32), zero)
            Pk, t1 = P * kp, kp * dP
        else:
            Pk, t1 = P, dP
        dZ = P * (t1 - D)
        if fault == "dv_without_keep":
            Pk = P
        Pb, Zb = Pk, dZ
        if bfmm:
            Pb, Zb = (truncate_bf16(Pk), truncate_bf16(dZ)) if fault == "trunc_bf16" else (rb(Pk), rb(dZ))
        Pkv, Zkv = Pb, Zb
        if fault == "drop_last_q_tile":
            live = (torch.arange(Nq) < 32 * ((Nq + 31) // 32 - 1)).to(F32)[:, None]
            Pkv, Zkv = Pb * live, Zb * live
        dV = self._sum(lambda i: Pkv[..., i, :, None] * dOm[..., i, None, :], Nq)
        dK = self._sum(lambda i: Zkv[..., i, :, None] * Qm[..., i, None, :], Nq)
        dQ = self._sum(lambda i: Zb[..., :, i, None] * Km[..., i, None, :], Nkp)
        sc = torch.tensor(case.scale, dtype=F32)
        if fault != "dk_no_scale":
            dK = dK * sc
        dQ = dQ * sc
        st = lambda t: t.to(store).to(F64)                                 # noqa: E731
        r = dict(dq=st(_scatter(dQ, op["qidx"], case.Rq)), dk=st(_scatter(dK[..., :Nk, :], op["kidx"], case.Rk)),
                 dv=st(_scatter(dV[..., :Nk, :], op["kidx"], case.Rk)), dbias=None)
        if case.bias_L:
            zb = torch.where(vis, dZ, zero)
            if fault == "dbias_second_window":
                zb = zb * (torch.arange(L) < kv_nsplit(case, path)).to(F32)[None, :, None, None, None]
            n = case.bias_rows * H
            if self.order == "tile":                                      # two levels: a table per (batch, window), then their sum
                fl = (bflat + (torch.arange(B * L) * n).reshape(B, L, 1, 1, 1)).reshape(-1)
                acc = torch.zeros(B * L * n, dtype=F32).index_add_(0, fl, zb.reshape(-1)).reshape(B * L, n).sum(0)
            else:
                fl, val = bflat.expand(B, L, H, Nq, Nkp).reshape(-1), zb.reshape(-1)
                if self.order == "reverse":
                    fl, val = fl.flip(0), val.flip(0)
                elif self.order == "perm":
                    pm = torch.randperm(fl.numel(), generator=self.gen)
                    fl, val = fl[pm], val[pm]
                acc = torch.zeros(n, dtype=F32).index_add_(0, fl, val)
            r["dbias"] = acc.reshape(case.bias_rows, H).to(F64)
        return r


_EMUL = {}


def emulate(case, path, order="forward", fault=None):
    key = (case.name, PATHS[path][1], order, fault, kv_nsplit(case, path) if fault == "dbias_second_window" else 0)
    if key not in _EMUL:
        _EMUL[key] = AttnBwdEmul(order, fault).run(case, path)
    return _EMUL[key]
