"""GPU: every row-local kernel inside the per-element float64 interval of tests/rows_bounds_ref.py.

One test per (case, mode) of rows_bounds_ref.CASES - the table DESIGN.md section 3u names; a new row-local kernel, epilogue or
instantiation gets a row there.  Each test builds the plans through ops, runs the op inside ops.LaunchProfile() with lib.call recorded,
and asserts
  - that exactly one launch was made, that it was the case's C entry point in the mode's library, and that the `dims` array lib.call
    received equals the case's dims element for element - the dims for which tests/test_rows_bounds.py proved, on the CPU and through
    csrc/rows_select.hpp itself, the instantiation the row names,
  - where the op takes its destination (proj_chain, proj_chain_kv, linear), on a sentinel-filled buffer with 64 guard rows behind it,
    that every destination element was written and nothing behind row M,
  - lo <= got <= hi for every element of `out`, and then of `out_next` from the `out` the kernel stored (rows_bounds_ref's docstring:
    "Cutting the chain at HBM"),
  - for bf16 stores with N >= 2000 elements of size, the signed rounding bias within +-2^-11,
and prints the position in the interval and, for fp32 stores, max |got - ref| / e: how much of the derived bound - the 1-ulp
assumption for v_exp_f32 / v_rcp_f32 / v_rsq_f32 included - the kernel uses.

Left out by name: rows_bounds_ref's docstring (bev_embed / bev_query, swap_stage, swish / sigmoid epilogues, the six-wave and
no-prefetch forms of row_chain64, the fp32 chain behind a post-LayerNorm in the third library, a broadcast residual of
cobevt_proj_chain).

Figures of one run on an MI355X: the comment below."""
import ctypes

import pytest
import torch

import rows_bounds_ref as rb
from cobevt_amd import lib, ops
from test_bev_backbone_gpu import SENTINEL, _mode

pytestmark = pytest.mark.gpu

# A record, not a gate: one run of this file on an MI355X, 93 tests in 28.7 s (all passed; no kernel had to be changed).  The slowest:
# chain_rc64_m65639_n192 6.0 s, proj_w256_m65613_pre_relu_res 3.4 s, lin_ln64_n64_m65536 1.9 s (float64 references of 65,536 and
# more rows: the thresholds of the persistent kernels and the smallest maps on which a wave walks a second block), every other test under 2 s.
# Worst position in the interval: 1.000 for every entry point in bf16 storage (an open bf16 interval is one to three values wide, so
# a correct value sits on an end: the figure says "inside", no more).  fp32 stores, per entry point and mode, worst position and
# max |got - ref| / e (how much of the derived bound - the 1-ulp assumption for v_exp_f32 / v_rcp_f32 / v_rsq_f32 in it - is used):
#     entry point                       fp32            fp32_split      fp32_fast
#     cobevt_attn_mlp_chain             1.000  0.082    1.000  0.082    0.202  0.202
#     cobevt_linear_rows_small_k        0.075  0.075    0.066  0.066    1.000  0.204
#   (position 1.000 in fp32: an interval a ReLU clips to [0, hi]).  Of the chain's 0.082, `out` uses 0.000 - 0.001 (its e is the
#   worst case of four GEMMs in a row, every element's interval open: median width 5 - 23 % of |ref|) and `out_next`, one LayerNorm
#   and one GEMM from the stored `out`, 0.003 - 0.082 (the largest behind a GELU epilogue).
#   chain_f32_m130_offset100, whose next LayerNorm sees rows N(100, 1) and carries the U |mu| r term of the single mean: 0.001 in
#   the first two libraries, 0.044 in the third.  Third library (the five rows without a post-LayerNorm): `out` 0.001 - 0.002 of an
#   interval about 1.9 |ref| wide (rows_bounds_ref.F32_FAST_OUT_WIDTH), `out_next` 0.044 - 0.202 of one 1.2 - 1.3 % wide.
# Signed rounding bias of the bf16 stores (77 destinations of N >= 2000): within +-5.0e-5 against the limit 4.9e-4.

GUARD = 64
_WORST = {}


class _Launches(object):
    """records (symbol, library variant, the integer dims array among the arguments) of every lib.call made inside"""

    def __enter__(self):
        self.records, self._call = [], lib.call

        def call(name, *args, variant=None):
            dims = [list(a) for a in args if isinstance(a, ctypes.Array) and a._type_ in (ctypes.c_int, ctypes.c_long)]
            self.records.append((name, lib.get_variant() if variant is None else variant, dims[0] if len(dims) == 1 else dims))
            return self._call(name, *args, variant=variant)
        lib.call = call
        return self

    def __exit__(self, *exc):
        lib.call = self._call
        return False


class _Guarded(object):
    """a sentinel-filled (M + GUARD, N) buffer whose first M rows are the op's destination"""

    def __init__(self, m, n, dt, cuda):
        self.idt, self.bits = SENTINEL[dt]
        self.m, self.buf = m, torch.full((m + GUARD, n), self.bits, dtype=self.idt, device=cuda).view(dt)
        self.out = self.buf[:m]

    def check(self):
        raw = self.buf.view(self.idt).cpu()
        assert not bool((raw[:self.m] == self.bits).any()), "a destination element was not written"
        assert bool((raw[self.m:] == self.bits).all()), "rows behind the result were written"


def _run_chain(case, op, cuda, dt):
    post = None if op["post"] is None else (op["post"][0].to(cuda), op["post"][1].to(cuda), op["post"][2])
    r = ops.attn_mlp_chain(op["a"], op["skip"], *op["plans"], post, next_plan=op["pn"])
    m, c = case.a["M"], case.a["C"]
    if op["pn"] is None:
        return {"net": r.reshape(m, c)}, []
    return {"net": r[0].reshape(m, c), "next": r[1].reshape(m, -1)}, []


def _run_proj(case, op, cuda, dt):
    pp, pn = op["plans"]
    assert ops.proj_chain_fusable(op["x"], pp, pn, op["res"])
    g = _Guarded(case.a["M"], pn.cout, dt, cuda)
    assert ops.proj_chain(op["x"], pp, pn, residual=op["res"], out_next=g.out) is g.out
    return {"net": g.out}, [g]


def _run_kv(case, op, cuda, dt):
    ppk, ppv, pnk, pnv = op["plans"]
    assert ops.proj_chain_kv_fusable(op["x"], ppk, ppv, pnk, pnv, op["res"])
    gk, gv = _Guarded(case.a["M"], 256, dt, cuda), _Guarded(case.a["M"], 256, dt, cuda)
    ops.proj_chain_kv(op["x"], ppk, ppv, pnk, pnv, residual=op["res"], out_k=gk.out, out_v=gv.out)
    return {"net": gk.out, "net_v": gv.out}, [gk, gv]


def _run_lin(case, op, cuda, dt):
    m, n, k, plan = case.a["M"], case.a["N"], case.a["K"], op["plan"]
    g = _Guarded(m, n, dt, cuda)
    if dt == torch.float32:
        # ops.linear never asks gemm_rows3_f32_kernel for its LayerNorm: ops.ln_fusable stops at K = 64 in fp32 storage and the kernel
        # has the K = 128 form only, so the product runs cobevt_layernorm first.  The kernel's own LayerNorm is launched the way
        # ops.conv2d launches the entry point, with ln = 1
        r4 = None if op["res"] is None else op["res"].reshape(1, 1, m, n)
        with ops._timed("gemm_rows|ln f32 %d->%d M=%d" % (k, n, m), lambda: (2.0 * m * n * k, 4.0 * (m * k + m * n + n * k))):
            ops._launch_rows(op["x"].reshape(1, 1, m, k), plan.wfrag_rows, plan.bias, r4, None, None, g.out.reshape(1, 1, m, n), kp=plan.kp_rows,
                             rows=32, act=plan.act, ln=1, ln_eps=plan.ln_eps)
    else:
        assert ops.linear(op["x"], plan, residual=op["res"], out=g.out) is g.out
    return {"net": g.out}, [g]


def _run_mean(case, op, cuda, dt):
    y = ops.mean_ln_linear(op["x"], op["plan"])
    assert y is not None
    return {"net": y.reshape(-1, case.a["N"])}, []


RUN = {"chain": _run_chain, "proj": _run_proj, "kv": _run_kv, "lin": _run_lin, "mean": _run_mean}


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    for (entry, mode), (pos, used) in sorted(_WORST.items()):
        print("worst position in the interval  %-34s %-10s %.3f   max |got - ref| / e (fp32 stores)  %.3f" % (entry, mode, pos, used))


def _check(case, mode, label, y, iv):
    got = rb.rows4(y.detach().cpu().to(torch.float64))
    assert got.shape == iv.ref.shape and bool(torch.isfinite(got).all())
    pos, out, used = rb.position(got, iv), rb.outside(got, iv), rb.error_over_e(got, iv)
    old = _WORST.get((case.entry, mode), (0.0, 0.0))
    _WORST[case.entry, mode] = (max(pos, old[0]), max(used, old[1]) if y.dtype == torch.float32 else old[1])
    print("%s %s %s: max (got - mid) / half-width %.3f, max |got - ref| / e %.3f, %d of %d elements outside, max|ref| %.3g"
          % (case.name, mode, label, pos, used, out, got.numel(), float(iv.ref.abs().max())))
    if out:
        bad = ((got < iv.lo) | (got > iv.hi)).nonzero()
        i = tuple(bad[0].tolist())
        assert out == 0, "%s: %d elements outside; first at column %d, row %d: got %.9g, interval [%.9g, %.9g], ref %.9g, e %.3g; columns %s, rows %s" % (
            label, out, i[1], i[3], float(got[i]), float(iv.lo[i]), float(iv.hi[i]), float(iv.ref[i]), float(iv.e[i]) if iv.e is not None else -1.0,
            sorted(set(bad[:, 1].tolist()))[:16], sorted(set(bad[:, 3].tolist()))[:16])
    if y.dtype == torch.bfloat16:
        mean, n = rb.bias_stat(got, iv.ref)
        if n >= rb.BIAS_MIN_N:
            print("%s %s %s: signed rounding bias %.3e over %d elements (limit %.3e)" % (case.name, mode, label, mean, n, rb.BIAS_LIMIT))
            assert abs(mean) <= rb.BIAS_LIMIT, (mean, n)


@pytest.mark.parametrize("cm", rb.CASE_MODES, ids=[rb.case_id(cm) for cm in rb.CASE_MODES])
def test_rows_kernel_within_its_interval(cuda, cm):
    case, mode = cm
    dt = rb.store_dtype(mode)
    with _mode(mode), rb.knobs(case):
        op = rb.build(case, mode, cuda)
        with _Launches() as rec, ops.LaunchProfile() as prof:
            outs, guarded = RUN[case.kind](case, op, cuda, dt)
        calls = sum(d["calls"] for d in prof.summary().values())
    torch.cuda.synchronize()
    assert [r[:2] for r in rec.records] == [(case.entry, rb.LIB[mode])], rec.records
    assert calls == 1
    assert rec.records[0][2] == rb.case_dims(case, mode), (rec.records[0][2], rb.case_dims(case, mode))
    for g in guarded:
        g.check()
    for label in ("net", "net_v"):
        if label in outs:
            _check(case, mode, label, outs[label], rb.reference(case, mode, label)[0])
    if "next" in outs:           # from `out` as the kernel stored it, which has just passed its own interval
        _check(case, mode, "next", outs["next"], rb.next_reference(rb.cpu_op(case, mode), mode, outs["net"].detach().cpu()))
