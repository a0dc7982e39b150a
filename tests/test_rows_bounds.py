"""CPU: the float64 interval reference of the row-local kernels (tests/rows_bounds_ref.py) is neither too tight nor vacuous.

  - the constants csrc/common.hpp documents for its two GELU formulas hold on a float64 scan of the formulas as written;
  - the LayerNorm bound holds under random corner perturbations of its input and fp32 evaluations in four summation orders;
  - for every case and mode of tests/test_rows_bounds_gpu.py a CPU model of a correct kernel lies inside [lo, hi] everywhere;
  - the same model with one injected fault (rows_bounds_ref.RowsEmul) leaves the interval at >= 1 % of the elements the fault
    touches, in at least one case of every entry point it applies to (the cases that hide a fault say so, with the measured share),
    and a truncating bf16 store fails the signed bias statistic;
  - every bf16 case keeps a useful interval (the width condition of the module docstring);
  - every case selects, through csrc/rows_select.hpp, the instantiation its row of the table names, and the table and the list of
    what is left out together are test_rows_select.KERNELS.

The faults are shown on the maps of up to 2,000 rows; the big-map cases (the wave-level kernels' thresholds) repeat their arithmetic."""
import json
import os
import subprocess

import pytest
import torch

import rows_bounds_ref as rb
from test_attn_select import _cxx
from test_rows_select import KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
PARAMS = dict(argnames="cm", argvalues=rb.CASE_MODES, ids=[rb.case_id(cm) for cm in rb.CASE_MODES])
SMALL = [c for c in rb.CASES if c.a.get("M", 0) <= 2000]
ENTRIES = sorted({c.entry for c in rb.CASES})
MIN_SHARE = 0.01


# ----------------------------------------------------------------------------------------------
# the documented constants
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan_points():
    return torch.cat([torch.linspace(-100.0, 100.0, 4000001, dtype=F64), torch.linspace(-10.0, 10.0, 2000001, dtype=F64)])


def test_gelu_bf16_constants(scan_points):
    """gelu_bf16 against x Phi(x): <= 6.2e-5 for x >= -8, below 1e-9 in magnitude under -8, <= 0.38 of 2^-9 max(|gelu|, 0.01)"""
    x = scan_points
    exact, got = rb.gelu_exact(x), rb.gelu_bf16_formula(x)
    err = (got - exact).abs()
    i = int(err.argmax())
    ratio = err / (2.0 ** -9 * exact.abs().clamp_min(rb.GELU_BF16_FLOOR))
    tail = x < -8.0
    print("gelu_bf16: max |error| %.4e at x = %.3f, %.4f of the bf16 rounding, %.2e in magnitude below -8" % (
        float(err[i]), float(x[i]), float(ratio.max()), float(got[tail].abs().max())))
    assert float(err[~tail].max()) <= rb.GELU_BF16_ABS
    assert float(got[tail].abs().max()) < rb.GELU_BF16_TAIL and float(exact[tail].abs().max()) < rb.GELU_BF16_TAIL
    assert float(ratio.max()) <= rb.GELU_BF16_REL


def test_gelu_erf_constants(scan_points):
    """erf_as against erf: <= 1.5e-7, so gelu_erf against x Phi(x): <= 0.75e-7 |x|"""
    x = scan_points
    e_erf = (rb.erf_as_formula(x) - torch.erf(x)).abs()
    e_gelu = (rb.gelu_erf_formula(x) - rb.gelu_exact(x)).abs()
    print("erf_as: max |error| %.3e; gelu_erf: %.3e absolute, %.3e |x| relative" % (
        float(e_erf.max()), float(e_gelu.max()), float((e_gelu / x.abs().clamp_min(1e-300)).max())))
    assert float(e_erf.max()) <= rb.ERF_AS_ABS
    assert bool((e_gelu <= 0.5 * rb.ERF_AS_ABS * x.abs() + 1e-18).all())


def test_gelu_evaluation_bounds_cover_an_fp32_evaluation():
    """the fp32 evaluation term of the GELU stage: an fp32 torch evaluation of either formula lies within it of the float64 one"""
    x = torch.linspace(-12.0, 12.0, 400001, dtype=F64).float().double()
    for formula, bound in ((rb.gelu_bf16_formula, rb._fp_gelu_bf16), (rb.gelu_erf_formula, rb._fp_gelu_erf)):
        d = (formula(x.float()).double() - formula(x)).abs()
        assert bool((d <= bound(x)).all()), float((d / bound(x).clamp_min(1e-300)).max())


LN_CASES = [("c128_var1", 128, 1.0, 0.0, 1e-5, 2.0 ** -9), ("c128_exact_input", 128, 1.0, 0.0, 1e-5, 0.0), ("c64_var1", 64, 1.0, 0.5, 1e-5, 2.0 ** -9),
            ("c40_small", 40, 1e-2, 0.0, 3e-5, 2.0 ** -9), ("c8", 8, 1.0, 0.0, 1e-5, 2.0 ** -9), ("c128_offset100", 128, 1.0, 100.0, 1e-5, 0.0),
            ("c128_wide", 128, 1.0, 0.0, 1e-5, 2.0 ** -5)]


@pytest.mark.parametrize("name,c,std,offset,eps,rel", LN_CASES, ids=[t[0] for t in LN_CASES])
def test_layernorm_bound_holds_at_the_corners(name, c, std, offset, eps, rel):
    """8 rows, 1,000 draws each of delta_i = +- its half-width (rel |x_i|: half a bf16 ulp and wider; 0: an exact input), the perturbed
    rows normalised in fp32 in four summation orders: every result inside x^ +- e"""
    g = torch.Generator().manual_seed(len(name) * 1000 + c)
    x = (torch.randn(8, c, generator=g, dtype=F64) * std + offset).float().double()
    dl = rel * x.abs()
    xh, e = rb.normalise_bound(x, dl, eps)
    sign = torch.where(torch.rand(1000, 8, c, generator=g) < 0.5, -1.0, 1.0).double()
    xp = (x[None] + sign * dl[None]).float()
    worst = 0.0
    for order in range(4):
        got = rb.normalise_f32(xp, eps, order).double()
        ratio = ((got - xh[None]).abs() / e[None]).max()
        worst = max(worst, float(ratio))
    print("%s: max |x^ - ref| / e over 1000 corners x 4 orders: %.3f" % (name, worst))
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------
# the emulator and the faults
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**PARAMS)
def test_honest_model_is_inside(cm):
    case, mode = cm
    for label, iv, got in rb.outputs(case, mode):
        assert got.shape == iv.ref.shape and bool((iv.lo <= iv.hi).all()) and bool(torch.isfinite(iv.lo).all() & torch.isfinite(iv.hi).all())
        print("%s %s %s: position in the interval %.3f" % (case.name, mode, label, rb.position(got, iv)))
        assert rb.outside(got, iv) == 0, "%s: %d of %d elements of a correct kernel outside" % (label, rb.outside(got, iv), got.numel())


def _touched(case, mode, fault, label, iv):
    """the elements of destination `label` the fault touches (None: it does not apply)"""
    a, kind = case.a, case.kind
    n, m = iv.ref.shape[1], iv.ref.shape[3]
    mask = torch.zeros(n, m, dtype=torch.bool)
    op = rb.cpu_op(case, mode)
    behind_next = label == "next" or kind in ("proj", "kv")              # the destination of a GEMM with the tag "next"
    if fault == "drop":
        if behind_next:
            mask[(n - 1) // 128 * 128:] = True
        else:
            mask[:, -1] = True
    elif fault.startswith("eps:"):
        slot = fault[4:]
        if slot not in op["slots"] or a.get("eps", 1e-5) == 1e-5 or (slot == "next") != behind_next:
            return None
        mask[:] = True
    elif fault == "skip_shift":
        tile = 64 if case.knobs.get("ROW_CHAIN_ROWS") == 64 else 32
        if kind != "chain" or label != "net" or not a.get("skip", True) or a["M"] <= tile:
            return None
        mask[:, tile:2 * tile] = True
    elif fault == "late":
        ok = (kind == "chain" and label == "net" and not a.get("post")) or (kind in ("lin", "mean") and a.get("act", 0) != 2)
        if not ok or mode != "bf16":
            return None
        mask[:] = True
    elif fault == "pad":
        if kind != "chain" or label != "net" or not op["npad"]:
            return None
        mask[:] = True
    return mask[None, :, None, :]


FAULTS = ["drop", "eps:1", "eps:post", "eps:next", "eps:ln", "skip_shift", "late", "pad"]


@pytest.mark.parametrize("fault", FAULTS)
def test_fault_leaves_the_interval(fault):
    seen = {}
    for case in SMALL:
        for mode in case.modes:
            for label, iv, got in rb.outputs(case, mode, fault):
                mask = _touched(case, mode, fault, label, iv)
                if mask is None:
                    continue
                share = float(((got < iv.lo) | (got > iv.hi))[mask].double().mean())
                base = fault.split(":")[0]
                hidden = base in case.hidden or "%s/%s" % (base, label) in case.hidden or "%s/%s@%s" % (base, label, mode) in case.hidden
                print("%-10s %-44s %-10s %-5s %6.1f %% of %d touched elements outside%s" % (fault, case.name, mode, label, 100 * share, int(mask.sum()),
                                                                                    "  (hidden)" if hidden else ""))
                if not hidden:
                    assert share >= MIN_SHARE, "%s %s %s: the bound is too loose to see %s (%.2f %%)" % (case.name, mode, label, fault, 100 * share)
                    seen.setdefault(case.entry, []).append(case.name)
    applies = {"skip_shift": ["cobevt_attn_mlp_chain"], "pad": ["cobevt_attn_mlp_chain"], "eps:1": ["cobevt_attn_mlp_chain"],
               "eps:post": ["cobevt_attn_mlp_chain"], "eps:next": ["cobevt_attn_mlp_chain", "cobevt_proj_chain", "cobevt_proj_chain_kv"],
               "eps:ln": ["cobevt_linear_rows_small_k"], "late": ["cobevt_attn_mlp_chain", "cobevt_linear_rows_small_k", "cobevt_mean_linear_rows_small_k"],
               "drop": ENTRIES}[fault]
    for entry in applies:
        assert seen.get(entry), "%s is hidden in every case of %s" % (fault, entry)


BF16_STAT = [c for c in SMALL if "bf16" in c.modes and c.stat]


@pytest.mark.parametrize("case", BF16_STAT, ids=[c.name for c in BF16_STAT])
def test_truncating_store_fails_the_bias_statistic(case):
    honest = rb.outputs(case, "bf16")
    for (label, iv, got), (_, _, got_t) in zip(honest, rb.outputs(case, "bf16", "trunc")):
        mean, n = rb.bias_stat(got, iv.ref)
        if n < rb.BIAS_MIN_N:
            continue                                  # (the GPU test applies the statistic under the same condition)
        mean_t, _ = rb.bias_stat(got_t, iv.ref)
        print("%s %s: signed bias %.2e honest, %.2e truncating (limit %.2e, N = %d)" % (case.name, label, mean, mean_t, rb.BIAS_LIMIT, n))
        assert abs(mean) <= rb.BIAS_LIMIT, mean
        assert mean_t < -rb.BIAS_LIMIT, mean_t


def test_every_entry_point_has_a_case_for_the_bias_statistic():
    for entry in ENTRIES:
        assert any(rb.bias_stat(got, iv.ref)[1] >= rb.BIAS_MIN_N for c in BF16_STAT if c.entry == entry for _, iv, got in rb.outputs(c, "bf16")), entry


# ----------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------
BF16_CM = [cm for cm in rb.CASE_MODES if cm[1] == "bf16"]


@pytest.mark.parametrize(**dict(PARAMS, argvalues=BF16_CM, ids=[rb.case_id(cm) for cm in BF16_CM]))
def test_width_condition(cm):
    """the reference alone keeps the final interval useful: median (hi - lo) / |ref| <= 2^-6, at most 5 % wider than 2^-5 |ref| + 2^-8 max|ref|"""
    case, mode = cm
    for label, iv, _ in rb.outputs(case, mode):
        width = iv.hi - iv.lo
        nz = iv.ref != 0
        median = float((width[nz] / iv.ref[nz].abs()).median())
        wide = float((width > 2.0 ** -5 * iv.ref.abs() + 2.0 ** -8 * iv.ref.abs().max()).double().mean())
        print("%s %s: median width %.2e |ref|, %.2f %% wide" % (case.name, label, median, 100 * wide))
        assert float(iv.ref.abs().max()) > 0.01
        assert median <= 2.0 ** -6 and wide <= 0.05, (median, wide)


def test_fp32_fast_chain_rows_are_listed_with_their_width():
    """the fp32 chain's own `out` in the third library cannot meet a useful width; every such row stands in F32_FAST_OUT_WIDTH with the
    measured median, and `out_next`, from the stored `out`, is at most 2^-6 |ref| wide but for the N(100, 1) rows (listed: 0.061)"""
    rows = [c for c in rb.CASES if c.kind == "chain" and "fp32_fast" in c.modes]
    assert {c.name for c in rows} == set(rb.F32_FAST_OUT_WIDTH)
    for case in rows:
        for label, iv, _ in rb.outputs(case, "fp32_fast"):
            nz = iv.ref != 0
            median = float(((iv.hi - iv.lo)[nz] / iv.ref[nz].abs()).median())
            print("%s fp32_fast %s: median width %.3g |ref|" % (case.name, label, median))
            if label == "net":
                assert abs(median / rb.F32_FAST_OUT_WIDTH[case.name] - 1.0) < 0.05, median
            else:
                assert median <= (0.0625 if case.a.get("offset") else 2.0 ** -6), median


def test_layernorm_folding_of_the_plans():
    """the intervals take W' and b' from the plan; here the fold itself against float64: W' = round(W g), b' = b + W beta"""
    from cobevt_amd import ops
    from cobevt_amd.synth import procedural_input
    for dt, tol in ((torch.bfloat16, 2.0 ** -8), (torch.float32, 2.0 ** -23)):
        for n, k in ((72, 40), (200, 128), (32, 64)):
            w, b = rb._uniform_w("rb.fold.w%d" % n, n, k), procedural_input("rb.fold.b%d" % n, (n,), 0, -0.2, 0.2)
            ln = rb._LN("rb.fold.ln%d" % n, k, 3e-5)
            plan = ops.ConvPlan(w, b, act=2, dtype=dt, device="cpu", ln=ln)
            want_w, want_b = w.double() * ln.weight.double()[None, :], b.double() + w.double() @ ln.bias.double()
            assert plan.has_ln and plan.ln_eps == 3e-5
            assert bool(((rb._w(plan, k) - want_w).abs() <= tol * want_w.abs()).all())
            assert bool(((rb._b(plan) - want_b).abs() <= 2.0 ** -22 * (want_b.abs() + (w.double().abs() @ ln.bias.double().abs()))).all())
            assert float(plan.wgt_rows.detach().double()[:, k:].abs().max()) == 0.0 if plan.wgt_rows.shape[1] > k else True


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rows_bounds") / "rows_select_main")
    _cxx(["-O1", os.path.join(ROOT, "tests", "rows_select_main.cpp"), "-o", exe])
    return exe


def test_every_case_selects_the_instantiation_its_row_names(program):
    routed = [(c, m) for c, m in rb.CASE_MODES if rb.select_line(c, m) is not None]
    lines = "\n".join(rb.select_line(c, m) for c, m in routed) + "\n"
    p = subprocess.run([program], input=lines.encode(), stdout=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    got = [json.loads(ln) for ln in p.stdout.decode().splitlines()]
    assert len(got) == len(routed)
    for (case, mode), rec in zip(routed, got):
        assert rec["name"] == rb.case_id((case, mode)) and rec["status"] == 0, rec
        assert rec["kernel"] == case.a["kernel"], (rec, case.a["kernel"])
    assert all(c.kind == "kv" for c in rb.CASES if c.a["kernel"] is None)


def test_table_and_left_out_are_every_instantiation():
    assert not set(rb.COVERED) & set(rb.LEFT_OUT)
    assert set(rb.COVERED) | set(rb.LEFT_OUT) == set(KERNELS)
    assert all(rb.LEFT_OUT.values())
