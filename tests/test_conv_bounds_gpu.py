"""GPU: every convolution entry point inside the per-element float64 interval of tests/conv_bounds_ref.py.

One test per (case, mode) of conv_bounds_ref.CASES - the table DESIGN.md section 3t names; a new convolution
kernel or epilogue gets a row there.  Each test builds the plan through ops, runs the op inside ops.LaunchProfile() with lib.call
recorded, and asserts
  - that exactly one launch was made and that it was the case's C entry point in the mode's library,
  - that every destination element was written and, for a padded `out`, nothing outside (NaN-payload sentinels, where the op takes `out`),
  - lo <= got <= hi for every element: what a kernel that accumulates in fp32 and rounds once may store (conv_bounds_ref's docstring
    derives e; tests/test_conv_bounds.py shows on the CPU that a correct kernel is inside and that a dropped product, a term added
    after the rounding, an unrounded intermediate are not),
  - for bf16 stores, the signed rounding bias: the mean of (got - ref) / ref over the elements with |ref| >= 2^-6 max|ref| within
    +-2^-11 (N >= 2000; a truncating store gives about -2.8e-3),
and prints max |got - mid| / half-width over the elements whose interval is open (1.000 wherever an open interval is one ulp wide or
is clipped by the ReLU, which is the rule: the figure says "inside", no more) and, more telling for fp32 stores, max |got - ref| / e
over the elements the ReLU does not cut.

Kernels left out by name, because they are not built for the mode: the four-wave 32-cout strip variants (113 .. 153), the projection-
shortcut strip kernel, cobevt_dsblock_nhwc and cobevt_bottleneck_nhwc are bf16 only; cobevt_bottleneck_f32_nhwc is fp32 storage only;
the stride-2 strip variants are not reached in the split-bf16 library (ops.conv_route sends them to the implicit GEMM there); the
head kernel (postprocess.hip) is not a per-library source.  GELU / swish epilogues stay on their gates in test_kernels_gpu.py.

Worst position in the interval per entry point and mode, and the run time of this file, from one run on an MI355X: the comment below."""
import pytest
import torch

import conv_bounds_ref as cb
from cobevt_amd import lib, ops
from test_bev_backbone_gpu import SENTINEL, _mode

pytestmark = pytest.mark.gpu

# A record, not a gate: one run of this file on an MI355X, 243 tests in 5.5 s (all passed; no kernel had to be changed).
# Worst position in the interval per entry point and mode: 1.000 for every entry point in every mode (an open bf16 interval is one ulp
# wide and a ReLU clips many fp32 ones to [0, hi], so a correct value sits on an end), except
#     cobevt_conv3x3_head_nchw          bf16 0.005   fp32 0.005
#     cobevt_linear_rows                fp32 0.045   fp32_split 0.283
#     cobevt_linear_rows_small_k        fp32 0.040
#     cobevt_stem_conv7x7s2_pool        fp32 0.014   fp32_split 0.061
#     cobevt_stem_conv7x7s2_pool_u8     fp32 0.010   fp32_split 0.065   fp32_fast 0.355
# max |got - ref| / e, fp32 stores (how much of the derived accumulation bound the kernel uses):
#     entry point                       fp32     fp32_split   fp32_fast
#     cobevt_conv2d_nhwc                0.028    0.264        0.389
#     cobevt_conv3x3_nhwc               0.002    0.010        0.094
#     cobevt_conv3x3_wfrag_nhwc         0.004    0.030        0.183
#     cobevt_stem_conv7x7s2             0.011    0.086        0.214
#     cobevt_basicblock_nhwc            0.004    0.006        0.040
#     cobevt_bottleneck_f32_nhwc        0.039    0.060        0.157
#     cobevt_linear_rows                0.047    0.283        0.450
#     cobevt_linear_rows_small_k        0.039    0.271        0.392
#     cobevt_conv3x3_head_nchw          0.005 (and 0.005 on bf16 input)

_WORST = {}


class _Launches(object):
    """records (symbol, library variant) of every lib.call made inside"""

    def __enter__(self):
        self.records, self._call = [], lib.call

        def call(name, *args, variant=None):
            self.records.append((name, lib.get_variant() if variant is None else variant))
            return self._call(name, *args, variant=variant)
        lib.call = call
        return self

    def __exit__(self, *exc):
        lib.call = self._call
        return False


def _nhwc(t, cuda, dt=None):
    t = t.permute(0, 2, 3, 1).contiguous().to(cuda)
    return t if dt is None else t.to(dt)


def _sentinel(shape, dt, cuda):
    idt, bits = SENTINEL[dt]
    return torch.full(shape, bits, dtype=idt, device=cuda).view(dt)


def _written(out, dt, ho, wo):
    """every element of out[:, :ho, :wo] written, none outside"""
    idt, bits = SENTINEL[dt]
    raw = out.view(idt).cpu()
    assert not bool((raw[:, :ho, :wo] == bits).any()), "a destination element was not written"
    mask = torch.ones(raw.shape[1:3], dtype=torch.bool)
    mask[:ho, :wo] = False
    assert bool((raw[:, mask] == bits).all()), "elements outside the result were written"


def _run_conv(case, op, cuda, dt):
    plan, a = op["plan"], case.a
    xd = _nhwc(op["x"], cuda, None if plan.smallc else dt)
    rd = None if op["res"] is None else _nhwc(op["res"], cuda, dt)
    ho, wo = plan.out_hw(a["h"], a["w"])
    if plan.store_mode != 0:
        y = ops.conv2d(xd, plan, residual=rd)
        return (y if plan.store_mode == 2 else y.permute(0, 3, 1, 2)), None
    out = _sentinel((a["n"],) + tuple(op["out_pad"] or (ho, wo)) + (plan.cout,), dt, cuda)
    y = ops.conv2d(xd, plan, residual=rd, out=out)
    assert y is out
    return out[:, :ho, :wo].permute(0, 3, 1, 2), lambda: _written(out, dt, ho, wo)


def _run_basicblock(case, op, cuda, dt):
    xd = _nhwc(op["x"], cuda)
    assert ops.basicblock_fusable(xd, op["p1"], op["p2"])
    return ops.basicblock(xd, op["p1"], op["p2"]).permute(0, 3, 1, 2), None


def _run_dsblock(case, op, cuda, dt):
    xd = _nhwc(op["x"], cuda)
    assert ops.dsblock_fusable(xd, op["p1"], op["p2"], op["pd"])
    return ops.dsblock(xd, op["p1"], op["p2"], op["pd"]).permute(0, 3, 1, 2), None


def _run_conv3_ds(case, op, cuda, dt):
    xd, yd, variant = _nhwc(op["x"], cuda), _nhwc(op["y"], cuda), case.a["variant"]
    assert ops.conv3_ds_fusable(xd, op["p1"], op["p2"], op["pd"]) == variant
    return ops.conv3_ds(yd, xd, op["p2"], op["pd"], variant).permute(0, 3, 1, 2), None


def _run_bottleneck(case, op, cuda, dt):
    xd = _nhwc(op["x"], cuda)
    assert ops.bottleneck_fusable(xd)
    return ops.bottleneck(xd, op["plan"], case.a["tile_rows"]).permute(0, 3, 1, 2), None


def _run_bottleneck_f32(case, op, cuda, dt):
    xd = _nhwc(op["x"], cuda)
    y1 = None if op["y1"] is None else _nhwc(op["y1"], cuda)
    assert ops.bottleneck_f32_fusable(xd, op["p1"], op["p2"], op["p3"], y1)
    return ops.bottleneck_f32(xd, op["p1"], op["p2"], op["p3"], y1).permute(0, 3, 1, 2), None


def _run_stem(case, op, cuda, dt):
    plan, a = op["plan"], case.a
    if a.get("u8"):
        return ops.stem_pool_u8(op["x8"].to(cuda), op["lut"].to(cuda), plan).permute(0, 3, 1, 2), None
    xd = _nhwc(op["x"], cuda)
    if a.get("pool"):
        return ops.stem_pool(xd, plan).permute(0, 3, 1, 2), None
    ho, wo = plan.out_hw(a["h"], a["w"])
    out = _sentinel((a["n"], ho, wo, 64), dt, cuda)
    assert ops.conv2d(xd, plan, out=out) is out
    return out.permute(0, 3, 1, 2), lambda: _written(out, dt, ho, wo)


RUN = {"conv": _run_conv, "basicblock": _run_basicblock, "dsblock": _run_dsblock, "conv3_ds": _run_conv3_ds, "bottleneck": _run_bottleneck,
       "bottleneck_f32": _run_bottleneck_f32, "stem": _run_stem}


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    for (entry, mode), (pos, used) in sorted(_WORST.items()):
        print("worst position in the interval  %-32s %-10s %.3f   max |got - ref| / e (fp32 stores in front of no pool)  %.3f" % (entry, mode, pos, used))


@pytest.mark.parametrize("cm", cb.CASE_MODES, ids=[cb.case_id(cm) for cm in cb.CASE_MODES])
def test_conv_kernel_within_its_interval(cuda, cm):
    case, mode = cm
    dt = cb.store_dtype(mode)
    iv, _, _ = cb.reference(case, mode)
    with _mode(mode), cb.knobs(case):
        op = cb.build(case, mode, cuda)
        with _Launches() as rec, ops.LaunchProfile() as prof:
            y, written = RUN[case.kind](case, op, cuda, dt)
        calls = sum(d["calls"] for d in prof.summary().values())
    torch.cuda.synchronize()
    assert rec.records == [(case.entry, cb.LIB[mode])], rec.records
    assert calls == 1
    if written is not None:
        written()
    got = y.detach().cpu().to(torch.float64)
    assert got.shape == iv.ref.shape and bool(torch.isfinite(got).all())
    pos, out, used = cb.position(got, iv), cb.outside(got, iv), cb.error_over_e(got, iv)
    old = _WORST.get((case.entry, mode), (0.0, 0.0))
    _WORST[case.entry, mode] = (max(pos, old[0]), max(used, old[1]) if (used == used and y.dtype == torch.float32) else old[1])
    print("%s %s: max (got - mid) / half-width %.3f, max |got - ref| / e %.3f, %d of %d elements outside, max|ref| %.3f"
          % (case.name, mode, pos, used, out, got.numel(), float(iv.ref.abs().max())))
    if out:
        bad = ((got < iv.lo) | (got > iv.hi)).nonzero()
        i = tuple(bad[0].tolist())
        assert out == 0, "%d elements outside; first at %s: got %.9g, interval [%.9g, %.9g], ref %.9g, e %.3g; outside at channels %s" % (
            out, i, float(got[i]), float(iv.lo[i]), float(iv.hi[i]), float(iv.ref[i]), float(iv.e[i]) if iv.e is not None else -1.0,
            sorted(set(bad[:, 1].tolist()))[:16])
    if y.dtype == torch.bfloat16 and case.stat:
        mean, n = cb.bias_stat(got, iv.ref)
        print("%s %s: signed rounding bias %.3e over %d elements (limit %.3e)" % (case.name, mode, mean, n, cb.BIAS_LIMIT))
        assert n >= cb.BIAS_MIN_N and abs(mean) <= cb.BIAS_LIMIT, (mean, n)
