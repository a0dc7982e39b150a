"""GPU: the four window-attention backward kernels inside the per-element float64 interval of tests/attn_bwd_ref.py.

One test per (case, path) of attn_bwd_ref.CASES - the table of DESIGN.md section 3z.  Each test calls cobevt_window_attention_bwd through
the project's call path (autograd._call with autograd._attn_dims, the path's flags or-ed into dims[0]) on the case's operands as stored -
`out` and `lse` come from the builder's float64 forward, no forward kernel runs - with dq / dk / dv in sentinel-filled buffers that have
64 guard rows behind them and a zero-filled dbias, and asserts
  - exactly one call of the entry, with the dims of the table row, returning COBEVT_OK,
  - every gradient element of every row of the partition overwritten (the kernels' header: each row is written once), nothing written in
    the guard rows, in the pad columns of layout b, or - layout a, one (rows, 3 d) gradient - outside the three column blocks,
  - lo <= got <= hi per element of dq, dk, dv and dbias,
  - for bf16 stores of >= 2000 elements the signed rounding bias within +-2^-11,
  - two runs of the same call bit-identical in dq, dk, dv (dbias goes through atomics and is exempt),
and prints the worst position in the interval and, for fp32 stores, max |got - ref| / e: how much of the derived bound - the 1-ulp
assumption for v_exp_f32 in it - the kernels use.  The restated index arithmetic is tied to the library's hooks first, bit for bit.

Figures of one run on an MI355X: the comment at the end."""
import ctypes

import numpy as np
import pytest
import torch

import attn_bwd_ref as ab
from cobevt_amd import autograd as ag
from cobevt_amd import lib, ops
from test_bev_backbone_gpu import SENTINEL

pytestmark = pytest.mark.gpu

GUARD = 64
ENTRY = "cobevt_window_attention_bwd"
COBEVT_OK, COBEVT_ERR_UNSUPPORTED = 0, 4                      # include/cobevt_hip.h
NAMES = ("dq", "dk", "dv")
_WORST = {}


class _Launches(object):
    """records (symbol, library variant, the int dims array, the status returned) of every lib.call made inside"""

    def __enter__(self):
        self.records, self._call = [], lib.call

        def call(name, *args, variant=None):
            dims = [list(a) for a in args if isinstance(a, ctypes.Array) and a._type_ is ctypes.c_int]
            rc = getattr(lib.load(variant), name)(*args)
            self.records.append((name, variant, dims[0] if len(dims) == 1 else dims, rc))
            lib.check(rc, name)
        lib.call = call
        return self

    def __exit__(self, *exc):
        lib.call = self._call
        return False


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    for path, (pos, used) in sorted(_WORST.items()):
        print("worst position in the interval  %-13s %.3f   max |got - ref| / e (fp32 stores)  %.3f" % (path, pos, used))


def test_restatement_equals_the_hooks(cuda):
    """attn_bwd_ref's token maps, bias index and dropout hash against ops.attention_index_map, ops.attention_bias_index and
    autograd.attention_dropout_mask, bit for bit, at one small shape each; after this only the restatement is used"""
    for mode in (0, 1, 2):
        m = (mode, 2, 4, 6, 2, 3, 2, 2)
        assert np.array_equal(ops.attention_index_map(m, 2, cuda).cpu().numpy().astype(np.int64), ab.index_map(m, 2))
    c = ab.BY_NAME["cross_48_108"]
    assert np.array_equal(ops.attention_bias_index(c.qmap, c.kmap, 3, cuda).cpu().numpy().astype(np.int64), ab.bias_index(c.qmap, c.kmap, 3))
    seed = (0xFFFFFFF0 + 0x31) & 0xFFFFFFFF
    assert np.array_equal(ag.attention_dropout_mask(2, 3, 2, 5, 7, 0.3, seed, cuda).cpu().numpy(), ab.attn_keep(2, 3, 2, 5, 7, 0.3, seed))


class _Grad(object):
    """a sentinel-filled (rows + GUARD, width) buffer; the gradient lives in columns [col, col + d) of its first `rows` rows"""

    def __init__(self, buf, rows, col, d, own):
        self.buf, self.rows, self.col, self.d, self.own = buf, rows, col, d, own
        self.view = buf[:rows, col:col + d]

    def raw(self):
        return self.buf.view(SENTINEL[self.buf.dtype][0]).cpu()

    def check(self):
        bits = SENTINEL[self.buf.dtype][1]
        raw = self.raw()
        assert not bool((raw[:self.rows, self.col:self.col + self.d] == bits).any()), "a gradient element was not written"
        assert bool((raw[self.rows:] == bits).all()), "guard rows were written"
        if self.own:                                                          # the columns beside the block belong to nobody
            assert bool((raw[:self.rows, :self.col] == bits).all()) and bool((raw[:self.rows, self.col + self.d:] == bits).all()), "pad columns were written"


def _sentinel(rows, width, dt, cuda):
    idt, bits = SENTINEL[dt]
    return torch.full((rows + GUARD, width), bits, dtype=idt, device=cuda).view(dt)


def _setup(case, path, cuda):
    """-> (the argument tensors of the entry, the three _Grad, dbias, the ctypes dims)"""
    store = ab.store_of(ab.PATHS[path][1])
    op = ab.operands(case, store)
    d, nan = case.d, float("nan")
    t = {n: op[n].to(cuda) for n in ("q", "k", "v", "out", "dout")}
    rows = {"q": case.Rq, "k": case.Rk, "v": case.Rk}
    off = (0, 0, 0, 0)
    if case.layout == "a":                                                      # q | k | v as the column blocks of one (rows, 3 d) tensor
        qkv = torch.cat([t["q"], t["k"], t["v"]], 1).contiguous()
        t["q"], t["k"], t["v"] = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
        g = _sentinel(case.Rq, 3 * d, store, cuda)
        grads = [_Grad(g, case.Rq, i * d, d, False) for i in range(3)]
        ld = (3 * d, 3 * d, 3 * d, d)
    elif case.layout == "b":                                                    # ld = d + 32, the blocks at column offsets, NaN in the gaps
        w, off = ab.layout_offsets(case, path)
        for n, o in zip(("q", "k", "v", "out", "dout"), off + (off[3],)):
            buf = torch.full((t[n].shape[0], w), nan, dtype=store, device=cuda)
            buf[:, o:o + d] = t[n]
            t[n] = buf
        grads = [_Grad(_sentinel(rows[n], w, store, cuda), rows[n], o, d, True) for n, o in zip(("q", "k", "v"), off)]
        ld = (w, w, w, w)
    else:
        grads = [_Grad(_sentinel(rows[n], d, store, cuda), rows[n], 0, d, True) for n in ("q", "k", "v")]
        ld = (d, d, d, d)
    lse = op["lse"].to(cuda)
    if ab.PATHS[path][0] & 0x400:                                               # [0] the log-sum-exp, [1] the D scratch: written before it is read
        lse = torch.cat([lse[None], torch.full_like(lse, nan)[None]], 0).contiguous()
    t["lse"] = lse
    for n in ("dlse", "table", "mask"):
        t[n] = None if op[n] is None else op[n].to(cuda)
    t["seed_dev"] = torch.tensor([case.seed_dev], dtype=torch.int32, device=cuda) if case.drop_p > 0 and case.seed_dev else None
    dbias = None if t["table"] is None else torch.zeros_like(t["table"])
    dims = ag._attn_dims(case.B, case.heads, ld[0], ld[1], ld[2], ld[3], t["table"], max(case.bias_L, 1), case.qmap, case.kmap, case.omap)
    dims[0] = ab.PATHS[path][0]
    for i in range(4):
        dims[8 + i] = off[i]
    return t, grads, dbias, dims


def _launch(case, t, grads, dbias, dims, drop_p=None):
    p = ops._p
    ptr = [p(g.buf) if g.own else p(g.view) for g in grads]      # layout a: the block's own pointer, offsets 0; else the base and dims[8..11]
    ag._call(ENTRY, p(t["q"]), p(t["k"]), p(t["v"]), p(t["out"]), p(t["lse"]), p(t["dout"]), p(t["dlse"]), ptr[0], ptr[1], ptr[2], p(dbias),
             p(t["table"]), p(t["mask"]), dims, ctypes.c_float(case.scale), ctypes.c_float(case.drop_p if drop_p is None else drop_p),
             ctypes.c_uint(case.seed), p(t["seed_dev"]), ops._stream())


def _check(case, path, name, got, iv, bf16_store):
    assert got.shape == iv.ref.shape and bool(torch.isfinite(got).all()), name
    pos, out, used = ab.position(got, iv), ab.outside(got, iv), ab.error_over_e(got, iv)
    if not bf16_store:
        old = _WORST.get(path, (0.0, 0.0))
        _WORST[path] = (max(pos, old[0]), max(used, old[1]))
    print("%s %s %s: max (got - mid) / half-width %.3f, max |got - ref| / e %.3f, %d of %d elements outside, max|ref| %.3g"
          % (case.name, path, name, pos, used, out, got.numel(), float(iv.ref.abs().max())))
    if out:
        bad = ((got < iv.lo) | (got > iv.hi)).nonzero()
        i = tuple(bad[0].tolist())
        assert out == 0, "%s: %d elements outside; first at row %d, column %d: got %.9g, interval [%.9g, %.9g], ref %.9g, e %.3g; rows %s, columns %s" % (
            name, out, i[0], i[1], float(got[i]), float(iv.lo[i]), float(iv.hi[i]), float(iv.ref[i]), float(iv.e[i]),
            sorted(set(bad[:, 0].tolist()))[:16], sorted(set(bad[:, 1].tolist()))[:16])
    if bf16_store:
        mean, n = ab.bias_stat(got, iv.ref)
        if n >= ab.BIAS_MIN_N:
            print("%s %s %s: signed rounding bias %.3e over %d elements (limit %.3e)" % (case.name, path, name, mean, n, ab.BIAS_LIMIT))
            assert abs(mean) <= ab.BIAS_LIMIT, (mean, n)


@pytest.mark.parametrize("cp", ab.CASE_PATHS, ids=[ab.case_id(cp) for cp in ab.CASE_PATHS])
def test_attention_backward_within_its_interval(cuda, cp):
    case, path = cp
    ref = ab.reference(case, path)
    runs = []
    for _ in range(2):
        t, grads, dbias, dims = _setup(case, path, cuda)
        with _Launches() as rec:
            _launch(case, t, grads, dbias, dims)
        torch.cuda.synchronize()
        assert rec.records == [(ENTRY, "", ab.case_dims(case, path), COBEVT_OK)], rec.records
        runs.append((grads, dbias))
    grads, dbias = runs[0]
    for g in grads:
        g.check()
    for name, g, g2 in zip(NAMES, grads, runs[1][0]):
        assert torch.equal(g.raw(), g2.raw()), "%s differs between two runs of the same call" % name
    bf16_store = ab.store_of(ab.PATHS[path][1]) == torch.bfloat16
    for name, g in zip(NAMES, grads):
        _check(case, path, name, g.view.detach().cpu().to(torch.float64), ref[name], bf16_store)
    if ref["dbias"] is not None:
        _check(case, path, "dbias", dbias.cpu().to(torch.float64), ref["dbias"], False)


def test_unsupported_combinations_are_refused(cuda):
    """dlse with probability dropout, and bf16 storage with probability dropout: COBEVT_ERR_UNSUPPORTED before any launch"""
    case = ab.BY_NAME["cross_48_108"]
    for path in ("fp32", "bf16st"):
        t, grads, dbias, dims = _setup(case, path, cuda)
        if path == "bf16st":
            t["dlse"] = None
        with _Launches() as rec, pytest.raises(lib.CobevtHipError):
            _launch(case, t, grads, dbias, dims, drop_p=0.25)
        torch.cuda.synchronize()
        assert [r[0] for r in rec.records] == [ENTRY] and rec.records[0][3] == COBEVT_ERR_UNSUPPORTED, rec.records
        bits = SENTINEL[grads[0].buf.dtype][1]
        assert all(bool((g.raw() == bits).all()) for g in grads), "a refused call wrote a gradient"


# A record, not a gate: one run of this file on an MI355X, 31 tests in 3.65 s (all passed, on the first run of every row; no kernel had to be
# changed).  The slowest: test_restatement_equals_the_hooks 0.21 s, many_windows-bf16st 0.16 s, grid_245-fp32 0.16 s (the float64 references
# of 2,304 windows of 16 x 16 and of 32 (batch, window, head) of 245 x 245); every other test at or under 0.13 s.
# Per path, the worst position in the interval and `used` = max |got - ref| / e on fp32 stores (how much of the derived bound - the 1-ulp
# assumption for v_exp_f32 in it - the kernels use):
#     path            position   used
#     fp32            0.055      0.056    dq / dk / dv (the largest: dq of many_windows; dv of outlier_logits 0.050); dbias 0.020
#     bf16mm          0.998      0.998    dq / dk / dv; dbias 0.012
#     bf16mm_1tile    0.998      0.998    dq / dk / dv; dbias 0.009
#     bf16st          0.005      0.005    dbias only (dq / dk / dv are bf16 stores: position 1.000, the interval being one to two values wide)
#     bf16st_scr      0.009      0.009    dbias only
#   0.998 on the bf16 matrix path is no use of the accumulation bound: where P keep' or dZ straddles a bf16 rounding boundary the
#   reference travels at the midpoint of the two candidates and the kernel - like the CPU emulator, which shows the same 0.998 - holds
#   one of them, so an element that one such term dominates sits at the end of its interval.  Where nothing straddles, the kernels are as
#   close as on the fp32 path.
# Signed rounding bias of the bf16 stores (27 destinations of N >= 2000): within -3.9e-5 .. +6.4e-5 against the limit 4.9e-4.
