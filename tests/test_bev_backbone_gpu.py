"""GPU: cobevt_deconv_nhwc at kernel level (ops.DeconvPlan / ops.deconv_into) in the four compute modes, host.BaseBEVBackbone against
the reference's output (fixture gv25) and against the torch restatement tests/bev_backbone_ref.mirror for the reference's other
branches, and PointPillarFuseBEVT with the backbone and the detection head.

Kernel-level gates are derived per output element from a float64 evaluation of the operands the kernel gets (bev_backbone_ref.deconv_f64:
BatchNorm folded in float64, weights and input rounded to the storage dtype by the test), with S = sum_k |x_k| |w'_k| and K = Cin:
    fp32 (native)  K 2^-23 S + 2^-23 |ref|         fp32 accumulation of K exact products in any order, one rounding for the shift add
    bf16           ... + 2^-8 |ref|                the rounding of the stored result (bf16 products are exact in the fp32 accumulator)
    fp32_split     ... + 2^-17 S                   operands as hi + lo bf16 halves, |x - hi - lo| <= 2^-17 |x| (csrc/f32_matrix.hpp)
    fp32_fast      ... + 2^-11 S                   the encoder's library: weights as ONE fp16 term, 11 significand bits

Module-level gates cannot be derived (9 - 17 layers), so they are measured on the CPU with the mirror: d32 = max-norm deviation of the
fp32 mirror from the float64 mirror, d16 = that of the mirror with weights and every layer's output rounded to bf16; the gates are
4 d32 and 4 d16 (the MFMA accumulation order differs from a CPU dot product and both numbers are one sample), relative to max|out|:

    configuration      d32        d16        max|out|   fp32 gate   bf16 gate
    golden (gv25)      3.404e-07  5.936e-03  1.2126     1.123e-06   1.958e-02
    down_deblock       3.647e-07  7.166e-03  1.6194     9.007e-07   1.770e-02
    trailing_deblock   1.576e-07  2.173e-03  0.5341     1.180e-06   1.627e-02
    no_deblocks        4.818e-07  8.110e-03  1.8975     1.016e-06   1.710e-02
"""
import copy

import pytest
import torch

import bev_backbone_ref as br
import cases_detect as cd
import launch_trace_bev_backbone as ltb
from cobevt_amd import host, lib, ops
from cobevt_amd.synth import fill_module_, procedural_input

pytestmark = pytest.mark.gpu

# name -> (d32, d16, max|out|), measured on the CPU (bev_backbone_ref.deviations; make_golden_bev_backbone.py prints the first row)
DEVIATIONS = {"golden": (3.404e-07, 5.936e-03, 1.2126), "down_deblock": (3.647e-07, 7.166e-03, 1.6194),
              "trailing_deblock": (1.576e-07, 2.173e-03, 0.5341), "no_deblocks": (4.818e-07, 8.110e-03, 1.8975)}
FACTOR = 4.0
SENTINEL = {torch.bfloat16: (torch.int16, 0x7FC1), torch.float32: (torch.int32, 0x7FC12345)}        # two NaN payloads no kernel produces


class _mode(object):
    """the compute mode; "fp32_fast" additionally inside lib.encoder_scope(), where that mode's third library serves the launches"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.ctx = [host.compute_dtype(self.mode)] + ([lib.encoder_scope()] if self.mode == "fp32_fast" else [])
        for c in self.ctx:
            c.__enter__()
        assert lib.get_variant() == {"bf16": "", "fp32": "", "fp32_split": "f32s", "fp32_fast": "f32h"}[self.mode]

    def __exit__(self, *exc):
        for c in reversed(self.ctx):
            c.__exit__(*exc)
        return False


def _bound(mode, k, mag, ref):
    b = k * 2.0 ** -23 * mag + 2.0 ** -23 * ref.abs()
    if mode == "bf16":
        b = b + 2.0 ** -8 * ref.abs()
    elif mode == "fp32_split":
        b = b + 2.0 ** -17 * mag
    elif mode == "fp32_fast":
        b = b + 2.0 ** -11 * mag
    return b


@pytest.fixture(scope="module")
def kernel_refs():
    """(case, storage dtype) -> the case's operands and float64 reference, computed once"""
    out = {}
    for case in br.KERNEL_CASES:
        weight, bn, x = br.kernel_case(case)
        for dt in (torch.bfloat16, torch.float32):
            out[case, dt] = (weight, bn, x) + br.deconv_f64(weight, bn, x, dt)
    return out


@pytest.mark.parametrize("mode", ["bf16", "fp32", "fp32_split", "fp32_fast"])
@pytest.mark.parametrize("case", br.KERNEL_CASES, ids=lambda c: "s%d_%dto%d_n%d_%dx%d_off%d_ldc%d" % c)
def test_deconv_kernel(cuda, kernel_refs, case, mode):
    s, cin, cout, n, h, w, c_off, ldc = case
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    weight, bn, x, ref, mag = kernel_refs[case, dt]
    idt, bits = SENTINEL[dt]
    out = torch.full((n, s * h, s * w, ldc), bits, dtype=idt, device=cuda).view(dt)
    with _mode(mode):
        plan = ops.DeconvPlan(weight, br.bn_module(bn), s, dt, cuda)
        res = ops.deconv_into(x.to(dt).to(cuda).contiguous(), plan, out, c_off)
    torch.cuda.synchronize()
    assert res is out
    raw = out.view(idt).cpu()
    outside = torch.cat([raw[..., :c_off], raw[..., c_off + cout:]], dim=-1)
    assert bool((outside == bits).all()), "channels outside [c_off, c_off + Cout) were written"
    assert not bool((raw[..., c_off:c_off + cout] == bits).any()), "a destination element of the slice was not written"
    got = out.cpu()[..., c_off:c_off + cout].double()
    assert bool(torch.isfinite(got).all())
    err, bound = (got - ref).abs(), _bound(mode, cin, mag, ref)
    ratio = float((err / bound.clamp_min(1e-30)).max())
    print("deconv %s %s: max|err| %.3e, max err / bound %.3f, max|ref| %.3f, %.0f %% cut by the ReLU"
          % (mode, case, float(err.max()), ratio, float(ref.abs().max()), 100 * float((ref == 0).double().mean())))
    assert float(ref.abs().max()) > 0.1 and 0.05 < float((ref == 0).double().mean()) < 0.95
    assert bool((err <= bound).all()), "max err / bound = %.3f" % ratio


def _module_check(cuda, name, sd, cfg, x, want, mode):
    d32, d16, scale = DEVIATIONS[name]
    gate = FACTOR * (d16 if mode == "bf16" else d32) / scale
    model = host.BaseBEVBackbone(copy.deepcopy(cfg), x.shape[1]).eval()
    model.load_state_dict(sd, strict=True)
    model = model.to(cuda)
    with torch.no_grad(), host.compute_dtype(mode):
        data = {"spatial_features": x.to(cuda)}
        out = model(data)
        assert out is data
        y = out["spatial_features_2d"]
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(want.shape) and y.shape[1] == model.num_bev_features
    err = float((y.cpu().double() - want.double()).abs().max()) / float(want.abs().max())
    print("BaseBEVBackbone %s %s: max-norm rel err %.3e (gate %.3e)" % (name, mode, err, gate))
    assert abs(float(want.abs().max()) - scale) < 1e-3 * scale
    assert err <= gate, "%s %s: %.3e > %.3e" % (name, mode, err, gate)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_backbone_matches_the_reference(cuda, mode):
    """the reference's own output (fixture gv25)"""
    sd, x, want = br.load_golden()
    _module_check(cuda, "golden", sd, br.GOLDEN_CFG, x, want, mode)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(br.MIRROR_CFGS))
def test_backbone_branches_match_the_mirror(cuda, name, mode):
    """a strided-conv deblock (upsample stride 0.5), the trailing deblock, no deblocks: against the float64 mirror"""
    cfg = br.MIRROR_CFGS[name]
    sd = fill_module_(host.BaseBEVBackbone(copy.deepcopy(cfg), br.INPUT_CHANNELS), 0).state_dict()
    x = procedural_input("gv25.spatial_features", br.INPUT_SHAPE, 0, -1.0, 1.0)
    with torch.no_grad():
        want = br.mirror(sd, cfg, x, torch.float64)
    _module_check(cuda, name, sd, cfg, x, want, mode)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_model_with_backbone_and_head(cuda, mode):
    """PointPillarFuseBEVT + backbone + anchor_number = 2 on a 16 x 24 grid, one sample of two agents (40 pillars): the head's maps
    come out at the backbone's 8 x 12 and equal the 1 x 1 heads applied (float64) to the module's own spatial_features_2d, with the
    kernel-level bound for K = 96; VoxelPostprocessor's default feature_stride = 2 then fits the maps"""
    model = fill_module_(host.PointPillarFuseBEVT(ltb.model_args()), 0).eval().to(cuda)
    batch = {"processed_lidar": {k: v.to(cuda) for k, v in ltb.voxels().items()}, "record_len": torch.tensor([2], dtype=torch.int32, device=cuda)}
    with torch.no_grad(), host.compute_dtype(mode):
        out = model(batch)
    torch.cuda.synchronize()
    assert set(out) == {"fused_feature", "spatial_features_2d", "psm", "rm"}
    assert tuple(out["fused_feature"].shape) == (1, 64, 16, 24) and tuple(out["spatial_features_2d"].shape) == (1, 96, 8, 12)
    assert tuple(out["psm"].shape) == (1, 2, 8, 12) and tuple(out["rm"].shape) == (1, 14, 8, 12)
    assert out["psm"].dtype == out["rm"].dtype == torch.float32 and out["psm"].is_contiguous() and out["rm"].is_contiguous()
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    feat = out["spatial_features_2d"].cpu().double()                   # exactly what the head kernel read (bf16 values in bf16 mode)
    assert float(feat.abs().max()) > 0.05
    for key, head in (("psm", model.cls_head), ("rm", model.reg_head)):
        w = head.weight.detach().cpu().flatten(1).to(dt).double()
        ref = torch.einsum("nchw,oc->nohw", feat, w) + head.bias.detach().cpu().double()[None, :, None, None]
        mag = torch.einsum("nchw,oc->nohw", feat.abs(), w.abs())
        bound = 96 * 2.0 ** -23 * mag + 2.0 ** -23 * ref.abs() + (2.0 ** -8 * ref.abs() if mode == "bf16" else 0.0)
        err = (out[key].cpu().double() - ref).abs()
        print("head %s %s: max err / bound %.3f" % (key, mode, float((err / bound.clamp_min(1e-30)).max())))
        assert bool((err <= bound).all())
    post = host.VoxelPostprocessor(cd.anchor_params((8, 12), "hwl", 4.8, 3.2), train=False)
    anchors = post.generate_anchor_box()
    assert "feature_stride" not in post.params["anchor_args"] and anchors.shape == (8, 12, 2, 7)
    data = {0: {"anchor_box": anchors, "transformation_matrix": torch.eye(4)}}
    boxes, scores = post.post_process(data, {0: {"psm": out["psm"], "rm": out["rm"]}})
    assert (boxes is None and scores is None) or (boxes.shape[0] == scores.shape[0] <= 1000 and tuple(boxes.shape[1:]) == (8, 3))
