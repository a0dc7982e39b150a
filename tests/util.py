"""Shared helpers for the test-suite."""
import copy
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"))


def rel_err(got, ref):
    """max |got - ref| / max |ref|  (the north-star's "rel" on the output scale)"""
    got = torch.as_tensor(got).detach().float().cpu()
    ref = torch.as_tensor(ref).detach().float().cpu()
    assert got.shape == ref.shape, "shape %s vs %s" % (tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), "non-finite values"
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


def rms_rel_err(got, ref):
    """||got - ref||_2 / ||ref||_2: the AVERAGE error on the output's own scale.  The max-norm above cannot see an error that sits
    on low-magnitude entries (small logits); this one cannot see a single bad entry - the gates use both."""
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).square().sum().sqrt() / ref.square().sum().sqrt().clamp_min(1e-30)).item()


def class_margin_stats(got, ref, class_dim):
    """logit tensors (classes along `class_dim`): arg-max agreement over all positions, over the positions whose REFERENCE
    top-1 / top-2 margin exceeds 2 % of the logit scale ("decisive" positions: a flip there is an error, not a tie), and the
    largest reference margin at which the arg-max flipped (0.0 if none did), as a fraction of the logit scale."""
    got = torch.as_tensor(got).detach().float().cpu().movedim(class_dim, -1)
    ref = torch.as_tensor(ref).detach().float().cpu().movedim(class_dim, -1)
    scale = ref.abs().max().clamp_min(1e-12)
    top2 = ref.topk(2, dim=-1).values
    margin = (top2[..., 0] - top2[..., 1]) / scale
    same = got.argmax(-1) == ref.argmax(-1)
    decisive = margin > 0.02
    flipped = margin[~same]
    return {"agreement": same.float().mean().item(),
            "decisive_agreement": same[decisive].float().mean().item() if decisive.any() else 1.0,
            "decisive_fraction": decisive.float().mean().item(),
            "worst_flipped_margin": flipped.max().item() if flipped.numel() else 0.0}


# bf16 gates.  Fixed numbers that do not come from anything measured on the HIP path:
#   * BF16_FLOOR = 1e-2: the bf16 gate BASELINE.md section 2 states ("bf16 perf mode is gated at 1e-2 + argmax/mIoU agreement");
#   * tests/golden/gv18_reference_bf16_autocast.npz: how far the REFERENCE's own bf16 run - the same module / model inside
#     torch.autocast(bfloat16), its mixed-precision mode (opv2v/opencood/tools/train_camera.py:157-160,
#     nuscenes/scripts/benchmark.py:45) - moves away from its fp32 forward, on the tests' inputs, as the envelope over the
#     procedural weight sets 0..3 (tests/golden/make_golden.py gv18; the reference's deviation moves by +-40 % between weight
#     sets: it is one realisation of accumulated rounding noise).
# A bf16 result of the HIP path may deviate from the fp32 reference / oracle by max(BF16_FLOOR, the reference's own deviation)
# in the max norm and by max(0.9 * BF16_FLOOR, the reference's own rms deviation) in the rms norm - never by more.
# `BF16` as a tolerance means "look the gate up under the comparison's case name"; comparisons whose module the reference
# fixture does not hold (restated third-party EfficientNet, fusion operators in isolation) name the fixture case of the
# model they belong to or run at the floor.
BF16_FLOOR = 1e-2
BF16 = "bf16: reference-derived gate"
RMS_FRACTION = {True: 0.9, False: 1.0}           # keyed by "tol is a bf16 gate" (tol > 2e-3)
_REF_BF16 = None
_REPORT = os.environ.get("COBEVT_PARITY_REPORT")
# Headroom policy.  Gates are never re-derived from what the HIP path measures: fp32 modes 1e-3 (north-star),
# bf16 max(1e-2, the reference's own bf16-autocast deviation).  A comparison may therefore sit close to its gate - in round 5
# CrossViewModule (0.98), resnet34[2] (0.95) and FAXModule (0.92) did - and a change of summation order moves a bf16 max-norm by
# +-30 % (profiles/r04_level0_error_probe.txt).  So every assert_close records measured / gate here and tests/conftest.py prints the
# ten largest ratios at the end of the run: a near-miss is visible in a GREEN run, before a kernel change turns it into a red one.
GATE_RATIOS = []                                 # (ratio, "max" | "rms", measured, gate, what, test id)


def reference_bf16_deviation(case):
    """[max-rel, rms-rel, arg-max agreement] of the reference's bf16-autocast run for `case` (gv18 fixture)"""
    global _REF_BF16
    if _REF_BF16 is None:
        _REF_BF16 = golden("gv18_reference_bf16_autocast")
    if case not in _REF_BF16:
        raise KeyError("no reference bf16-autocast deviation recorded for %r (tests/golden/make_golden.py gv18)" % case)
    return [float(v) for v in _REF_BF16[case]]


def bf16_gate(case=None):
    """(max-rel gate, rms-rel gate) for a bf16 comparison; case=None: no reference counterpart -> the floor"""
    if case is None:
        return BF16_FLOOR, RMS_FRACTION[True] * BF16_FLOOR
    r = reference_bf16_deviation(case)
    return max(BF16_FLOOR, r[0]), max(RMS_FRACTION[True] * BF16_FLOOR, r[1])


def assert_close(got, ref, tol, what, case=None):
    """tol: a number (max-rel gate; the rms-rel gate is tol itself, 0.9 * tol for a bf16-sized gate) or BF16 (gates looked up
    in the reference's bf16-autocast fixture under `case`, default: `what`)"""
    if tol is BF16 or tol == BF16:
        tol, rms_gate = bf16_gate(what if case is None else case)
    else:
        rms_gate = tol * RMS_FRACTION[tol > 2e-3]
    e = rel_err(got, ref)
    r = rms_rel_err(got, ref)
    if _REPORT:                      # measured values next to their gates
        with open(_REPORT, "a") as f:
            f.write("%s\t%s\tmax_rel=%.3e\trms_rel=%.3e\tgate=%.2e\trms_gate=%.2e\n"
                    % (os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], what, e, r, tol, rms_gate))
    tid = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    if tol > 0 and rms_gate > 0:              # (a zero gate is a bit-exact comparison: nothing to rank)
        GATE_RATIOS.append((e / tol, "max", e, tol, what, tid))
        GATE_RATIOS.append((r / rms_gate, "rms", r, rms_gate, what, tid))
    assert e <= tol, "%s: rel err %.3e > %.2e" % (what, e, tol)
    assert r <= rms_gate, "%s: rms rel err %.3e > %.2e" % (what, r, rms_gate)
    return e


def cfg_copy(cfg):
    return copy.deepcopy(cfg)


def focal_reference(pred, label, vis, label_indices, min_visibility, alpha, gamma, reduction="mean"):
    """torch restatement of BinarySegmentationLoss / CenterLoss (nuscenes losses.py:27-84) over fvcore's published sigmoid_focal_loss,
    in the type of `pred` (fp32 on the device: torch's own arithmetic; float64 on the CPU: the reference of the kernel-level tests).
    reduction "sum": the sum over the kept elements instead of their mean."""
    F = torch.nn.functional
    if label_indices is not None:
        label = torch.stack([label[:, idx].max(1)[0] for idx in label_indices], 1)
    p = torch.sigmoid(pred)
    ce = F.binary_cross_entropy_with_logits(pred, label, reduction="none")
    pt = p * label + (1 - p) * (1 - label)
    loss = ce * (1 - pt) ** gamma
    if alpha >= 0:
        loss = (alpha * label + (1 - alpha) * (1 - label)) * loss
    if min_visibility is not None:
        mask = (vis >= min_visibility)[:, None].expand_as(loss)
        loss = loss[mask]
    return loss.sum() if reduction == "sum" else loss.mean()
