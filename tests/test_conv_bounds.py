"""CPU: the float64 interval reference of the convolution kernels (tests/conv_bounds_ref.py) is neither too tight nor vacuous.

For every case and mode of tests/test_conv_bounds_gpu.py: a CPU model of a correct kernel lies inside [lo, hi] everywhere; the same
model with one injected fault leaves it at one element at least - (a) one product dropped at the four corner pixels, (b) the residual
(else the shift) added after the rounding, (c) a fused kernel's intermediate kept unrounded; a truncating bf16 store fails the signed
bias statistic; and the case itself is a fair one (outputs of size, a ReLU that cuts some but not all, few intermediates on a rounding
boundary, the route the GPU test expects).

(b) and (c) are bf16 statements: in fp32 storage the accumulator already has the storage type, so "rounded, then added" and "kept
unrounded" are what a correct kernel does."""
import pytest
import torch

import conv_bounds_ref as cb
from cobevt_amd import ops

FUSED = ("basicblock", "dsblock", "conv3_ds", "bottleneck")
PARAMS = dict(argnames="cm", argvalues=cb.CASE_MODES, ids=[cb.case_id(cm) for cm in cb.CASE_MODES])
BF16 = dict(argnames="case", argvalues=[c for c in cb.CASES if "bf16" in c.modes], ids=[c.name for c in cb.CASES if "bf16" in c.modes])


def _has_term(case):
    a = case.a            # (the head kernel stores fp32 in bf16 mode as well: nothing is rounded before its shift)
    return (case.kind != "conv" or (bool(a.get("residual") or a.get("bias", True) or a.get("bn")) and not a.get("head"))) and "late" not in case.hidden


def _has_intermediate(case):
    return (case.kind in FUSED or bool(case.a.get("pre_bn"))) and "unrounded" not in case.hidden


@pytest.mark.parametrize(**PARAMS)
def test_honest_model_is_inside(cm):
    case, mode = cm
    iv, _, _ = cb.reference(case, mode)
    got = cb.emulate(case, mode)
    assert got.shape == iv.ref.shape and bool((iv.lo <= iv.hi).all())
    print("%s %s: position in the interval %.3f" % (case.name, mode, cb.position(got, iv)))
    assert cb.outside(got, iv) == 0, "%d of %d elements of a correct kernel outside" % (cb.outside(got, iv), got.numel())


@pytest.mark.parametrize(**PARAMS)
def test_dropped_product_leaves_the_interval(cm):
    case, mode = cm
    iv, _, _ = cb.reference(case, mode)
    assert cb.outside(cb.emulate(case, mode, "drop"), iv) >= 1, "the bound is too loose for this case's K"


@pytest.mark.parametrize(**dict(BF16, argvalues=[c for c in BF16["argvalues"] if _has_term(c)],          # (cases with neither are left out)
                                ids=[c.name for c in BF16["argvalues"] if _has_term(c)]))
def test_term_added_after_the_rounding_leaves_the_interval(case):
    iv, _, _ = cb.reference(case, "bf16")
    assert cb.outside(cb.emulate(case, "bf16", "late"), iv) >= 1


@pytest.mark.parametrize(**dict(BF16, argvalues=[c for c in BF16["argvalues"] if _has_intermediate(c)],
                                ids=[c.name for c in BF16["argvalues"] if _has_intermediate(c)]))
def test_unrounded_intermediate_leaves_the_interval(case):
    iv, _, _ = cb.reference(case, "bf16")
    assert cb.outside(cb.emulate(case, "bf16", "unrounded"), iv) >= 1


@pytest.mark.parametrize(**dict(BF16, argvalues=[c for c in BF16["argvalues"] if c.stat], ids=[c.name for c in BF16["argvalues"] if c.stat]))
def test_truncating_store_fails_the_bias_statistic(case):
    iv, _, _ = cb.reference(case, "bf16")
    mean, n = cb.bias_stat(cb.emulate(case, "bf16"), iv.ref)
    assert n >= cb.BIAS_MIN_N, "%d elements: too few for the statistic - enlarge the case or set stat=False" % n
    assert abs(mean) <= cb.BIAS_LIMIT, mean
    mean_t, _ = cb.bias_stat(cb.emulate(case, "bf16", "trunc"), iv.ref)
    print("%s: signed bias %.2e honest, %.2e truncating (limit %.2e, N = %d)" % (case.name, mean, mean_t, cb.BIAS_LIMIT, n))
    assert mean_t < -cb.BIAS_LIMIT, mean_t


@pytest.mark.parametrize(**PARAMS)
def test_case_conditions(cm):
    case, mode = cm
    iv, inter, conv = cb.reference(case, mode)
    assert float(iv.ref.abs().max()) > 0.1
    relu = case.kind != "conv" or case.a.get("act", 0) == 1
    if relu:
        cut = float((conv.ref == 0).double().mean())            # (in front of the max-pool, where there is one)
        assert 0.05 < cut < 0.95, "%.0f %% of the outputs cut by the ReLU" % (100 * cut)
    # in fp32 storage e is several ulps of the storage type, so lo < hi nearly everywhere and d1 is of the order of the next stage's own
    # K 2^-23 S: the share says something in bf16 storage only, where one ulp is 2^15 times e's unit
    for k, mid in enumerate(inter if mode == "bf16" else []):
        open_ = float((mid.lo < mid.hi).double().mean())
        assert open_ < 0.25, "intermediate %d: %.0f %% of the elements straddle a rounding boundary" % (k, 100 * open_)
    if not case.stat:
        assert cb.bias_stat(iv.ref, iv.ref)[1] < cb.BIAS_MIN_N or store_is_fp32_only(case), "stat=False on a case large enough for the statistic"


def store_is_fp32_only(case):
    return bool(case.a.get("head"))          # the head kernel stores fp32 in both modes


@pytest.mark.parametrize(**dict(PARAMS, argvalues=[cm for cm in cb.CASE_MODES if cm[0].kind == "conv"],
                                ids=[cb.case_id(cm) for cm in cb.CASE_MODES if cm[0].kind == "conv"]))
def test_route_is_the_entry_point(cm):
    """ops.conv_route is a pure function: under the case's switches the plan takes the entry point the GPU test asserts, and the strip
    kernel's three-term / packed form is marked exactly where a wave owns two k-groups per tap (128-cout tiles)"""
    case, mode = cm
    op = cb.build(case, mode)
    plan, a = op["plan"], case.a
    with cb.knobs(case):
        r = ops.conv_route(plan, a["n"], a["h"], a["w"], op["out_pad"], op["res"] is not None, cb.LIB[mode])
    assert ops.CONV_SYMBOLS[r.kernel] == case.entry, r
    if r.kernel == "strips":
        assert (mode in case.packed) == (r.variant % 10 == 0 and mode in ("fp32_split", "fp32_fast")), r
        if "CONV3_VARIANT" in case.knobs:
            assert r.variant == case.knobs["CONV3_VARIANT"]


def test_bottleneck_fragments_invert():
    """bottleneck_weights undoes BottleneckPlan's fragment order: the folded weights, rounded to bf16"""
    m = cb._bneck_module()
    plan = ops.BottleneckPlan(m.conv1, m.bn1, m.conv2, m.bn2, m.conv3, m.bn3, device="cpu")
    for conv, bn, w in zip((m.conv1, m.conv2, m.conv3), (m.bn1, m.bn2, m.bn3), cb.bottleneck_weights(plan)):
        sc, _ = ops.bn_affine(bn)
        want = (conv.weight.detach().double() * sc[:, None, None, None]).float().to(torch.bfloat16).double()
        assert torch.equal(w, want)
