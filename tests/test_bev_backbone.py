"""CPU: host.BaseBEVBackbone's state_dict against the reference's (fixture gv25), its constructor branches and errors, the tap-major
weight layout of ops.DeconvPlan, the preconditions of ops.deconv_into, PointPillarFuseBEVT's state_dict with and without the
backbone, and the launch sequence of the model with the backbone in the four compute modes (tests/launch_trace_bev_backbone.py)."""
import copy
import json
import os

import pytest
import torch
import torch.nn.functional as F

import bev_backbone_ref as br
import cases_pillar as cp
import launch_trace as lt
import launch_trace_bev_backbone as ltb
from cobevt_amd import host, ops
from cobevt_amd.lib import CobevtHipError

HERE = os.path.dirname(os.path.abspath(__file__))


def test_state_dict_is_the_references():
    sd, _, _ = br.load_golden()
    model = host.BaseBEVBackbone(copy.deepcopy(br.GOLDEN_CFG), br.INPUT_CHANNELS)
    own = model.state_dict()
    assert list(own) == list(sd)
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert "blocks.0.1.weight" in own and "blocks.0.2.running_mean" in own and "deblocks.2.0.weight" in own
    model.load_state_dict(sd, strict=True)
    assert torch.equal(model.deblocks[2][0].weight, sd["deblocks.2.0.weight"])
    assert model.blocks[0][2].eps == model.deblocks[0][1].eps == 1e-3


@pytest.mark.parametrize("cfg, want, n_deblocks", [
    (br.GOLDEN_CFG, 96, 3), (br.STANDARD_CFG, 384, 3), (br.MIRROR_CFGS["down_deblock"], 96, 3),
    (br.MIRROR_CFGS["trailing_deblock"], 96, 3), (br.MIRROR_CFGS["no_deblocks"], 96, 0),
    (dict(layer_nums=[2], layer_strides=[1], num_filters=[64], upsample_strides=[2], num_upsample_filter=[32]), 32, 1),
    (dict(layer_nums=[2], layer_strides=[2], num_filters=[64]), 64, 0)])
def test_num_bev_features(cfg, want, n_deblocks):
    model = host.BaseBEVBackbone(copy.deepcopy(cfg), 64)
    assert model.num_bev_features == want and len(model.deblocks) == n_deblocks and len(model.blocks) == len(cfg["layer_nums"])
    for i, block in enumerate(model.blocks):
        assert len(block) == 4 + 3 * cfg["layer_nums"][i] and isinstance(block[0], torch.nn.ZeroPad2d)
        assert block[1].stride == (cfg["layer_strides"][i],) * 2 and block[1].padding == (0, 0) and block[4].padding == (1, 1)
    if cfg is br.MIRROR_CFGS["down_deblock"]:
        conv = model.deblocks[0][0]
        assert isinstance(conv, torch.nn.Conv2d) and conv.kernel_size == conv.stride == (2, 2)
    if cfg is br.MIRROR_CFGS["trailing_deblock"]:
        conv = model.deblocks[2][0]
        assert isinstance(conv, torch.nn.ConvTranspose2d) and (conv.in_channels, conv.out_channels, conv.stride) == (96, 96, (2, 2))


@pytest.mark.parametrize("s", [1, 2, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_deconv_plan_layout(s, dtype):
    """the plan's matrix times a row vector, un-shuffled, is conv_transpose2d + BatchNorm on a 1 x 1 input: float64 arithmetic on the
    STORED weights, so the only difference is their rounding to the storage dtype - per output at most u * sum_k |x_k| |w'_k| with
    u = 2^-24 (fp32) / 2^-9 + 2^-23 (bf16: rounded to fp32, then to bf16) from the unit roundoffs of round-to-nearest, plus 2^-24 |shift| for
    the fp32 shift"""
    cin, cout = 40, 64
    weight, bn, _ = br.kernel_case((s, cin, cout, 1, 1, 1, 0, cout))
    plan = ops.DeconvPlan(weight, br.bn_module(bn), s, dtype, "cpu")
    kpad = {torch.float32: 48, torch.bfloat16: 64}[dtype]
    assert tuple(plan.wgt.shape) == (s * s * cout, kpad) and plan.wgt.dtype == dtype and plan.wgt.is_contiguous()
    assert tuple(plan.shift.shape) == (cout,) and plan.shift.dtype == torch.float32
    assert (plan.cin, plan.cout, plan.stride, plan.kpad, plan.act) == (cin, cout, s, kpad, 1)
    assert not plan.wgt[:, cin:].any()
    x = (torch.rand(cin, generator=torch.Generator().manual_seed(s)) - 0.5).double()
    got = (plan.wgt.double()[:, :cin] @ x + plan.shift.double().repeat(s * s)).reshape(s, s, cout).permute(2, 0, 1)       # (co, dy, dx)
    scale, shift = br.fold({"b." + k: v for k, v in bn.items()}, "b.")
    ref = F.conv_transpose2d(x.reshape(1, cin, 1, 1), weight.double(), stride=s)[0] * scale[:, None, None] + shift[:, None, None]
    mag = F.conv_transpose2d(x.abs().reshape(1, cin, 1, 1), weight.double().abs(), stride=s)[0] * scale.abs()[:, None, None]
    u = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -9 + 2.0 ** -23
    assert bool(((got - ref).abs() <= u * mag + 2.0 ** -24 * shift.abs()[:, None, None]).all())
    assert float((got - ref).abs().max()) < 1e-2 and float(ref.abs().max()) > 0.1


def test_deconv_plan_preconditions():
    w = torch.zeros(32, 48, 2, 2)
    with pytest.raises(CobevtHipError, match="Cout=48"):
        ops.DeconvPlan(w, None, 2, torch.bfloat16, "cpu")
    with pytest.raises(CobevtHipError, match="stride 9"):
        ops.DeconvPlan(torch.zeros(32, 32, 9, 9), None, 9, torch.bfloat16, "cpu")
    with pytest.raises(CobevtHipError, match="kernel = stride"):
        ops.DeconvPlan(torch.zeros(32, 32, 3, 3), None, 2, torch.bfloat16, "cpu")
    with pytest.raises(CobevtHipError, match="Cin=36"):
        ops.DeconvPlan(torch.zeros(36, 32, 2, 2), None, 2, torch.bfloat16, "cpu")
    ops.DeconvPlan(torch.zeros(36, 32, 2, 2), None, 2, torch.float32, "cpu")             # a multiple of 4 is enough in fp32


def test_deconv_into_preconditions():
    """all raised before the device check and before any launch: CPU tensors reach them"""
    plan = ops.DeconvPlan(torch.zeros(32, 32, 2, 2), None, 2, torch.bfloat16, "cpu")
    x = torch.zeros(1, 3, 4, 32, dtype=torch.bfloat16)
    out = torch.zeros(1, 6, 8, 64, dtype=torch.bfloat16)
    with pytest.raises(CobevtHipError, match="c_off=4"):
        ops.deconv_into(x, plan, out, 4)
    with pytest.raises(CobevtHipError, match=r"\[40, 72\) do not fit the destination's 64"):
        ops.deconv_into(x, plan, out, 40)
    with pytest.raises(CobevtHipError, match=r"must be contiguous \(1, 6, 8, ldc\)"):
        ops.deconv_into(x, plan, torch.zeros(1, 6, 7, 64, dtype=torch.bfloat16), 0)
    with pytest.raises(CobevtHipError, match="do not match the plan"):
        ops.deconv_into(x.float(), plan, out, 0)
    with pytest.raises(CobevtHipError, match="bad input"):
        ops.deconv_into(torch.zeros(1, 3, 4, 64, dtype=torch.bfloat16), plan, out, 0)
    with pytest.raises(CobevtHipError, match="ROCm device"):                                # valid arguments: only the device is missing
        ops.deconv_into(x, plan, out, 32)


def test_backbone_constructor_errors():
    base = dict(layer_nums=[1, 1], layer_strides=[2, 2], num_filters=[32, 64])
    with pytest.raises(CobevtHipError, match="multiple of 32"):
        host.BaseBEVBackbone(dict(base, upsample_strides=[1, 2], num_upsample_filter=[48, 48]), 32)
    with pytest.raises(CobevtHipError, match=r"upsample_strides\[1\] = 9"):
        host.BaseBEVBackbone(dict(base, upsample_strides=[1, 9], num_upsample_filter=[32, 32]), 32)
    with pytest.raises(CobevtHipError, match=r"num_upsample_filter\[-1\] must be 0"):
        host.BaseBEVBackbone(dict(base, upsample_strides=[1, 2, 2], num_upsample_filter=[32, 32, 64]), 32)
    with pytest.raises(CobevtHipError, match="one entry per level"):
        host.BaseBEVBackbone(dict(base, layer_strides=[2]), 32)


def test_mismatched_level_sizes_raise_before_any_launch(monkeypatch):
    rec = lt.Recorder()
    lt.install(monkeypatch.setattr, rec)
    cfg = dict(layer_nums=[1, 1], layer_strides=[2, 2], num_filters=[32, 32], upsample_strides=[1, 1], num_upsample_filter=[32, 32])
    model = host.BaseBEVBackbone(cfg, 32).eval()
    with pytest.raises(CobevtHipError, match="a 16 x 24 input gives 8 x 12, 4 x 6"):
        model.forward_nhwc(torch.zeros(1, 16, 24, 32, dtype=torch.bfloat16))
    # an odd size: level 2 of the standard strides rounds up, its x 2 deblock no longer meets level 1
    model = host.BaseBEVBackbone(copy.deepcopy(br.GOLDEN_CFG), 32).eval()
    with pytest.raises(CobevtHipError, match="a 10 x 24 input gives 5 x 12, 6 x 12, 8 x 12"):
        model.forward_nhwc(torch.zeros(1, 10, 24, 32, dtype=torch.bfloat16))
    assert rec.records == []


def test_train_mode_forward_raises():
    model = host.BaseBEVBackbone(copy.deepcopy(br.GOLDEN_CFG), 32).train()
    with pytest.raises(CobevtHipError, match="inference path"):
        model({"spatial_features": torch.zeros(1, 32, 16, 24)})
    args = ltb.model_args()
    del args["anchor_number"]
    with pytest.raises(CobevtHipError, match="base_bev_backbone.*inference only"):
        host.PointPillarFuseBEVT(args).train()({"processed_lidar": ltb.voxels(), "record_len": torch.tensor([2], dtype=torch.int32)})


def test_point_pillar_state_dict_with_and_without_the_backbone():
    """without the argument: the keys recorded from the commit before the backbone existed (tests/golden/point_pillar_state_dict_keys.json);
    with it: more keys only under backbone., and the heads resized to num_bev_features"""
    with open(os.path.join(HERE, "golden", "point_pillar_state_dict_keys.json")) as f:
        recorded = json.load(f)
    args = cp.model_args()
    plain = host.PointPillarFuseBEVT(copy.deepcopy(args))
    assert list(plain.state_dict()) == recorded["plain"] and plain.backbone is None
    args["anchor_number"] = 2
    det = host.PointPillarFuseBEVT(copy.deepcopy(args)).state_dict()
    assert list(det) == recorded["anchor_number"]
    args["base_bev_backbone"] = copy.deepcopy(br.GOLDEN_CFG)
    model = host.PointPillarFuseBEVT(args)
    both = model.state_dict()
    extra = [k for k in both if k not in det]
    assert extra and all(k.startswith("backbone.") for k in extra) and set(det) <= set(both)
    assert [k[len("backbone."):] for k in extra] == list(host.BaseBEVBackbone(copy.deepcopy(br.GOLDEN_CFG), 64).state_dict())
    resized = {k for k in det if det[k].shape != both[k].shape}
    assert resized == {"cls_head.weight", "reg_head.weight"}
    assert tuple(both["cls_head.weight"].shape) == (2, 96, 1, 1) and tuple(both["reg_head.weight"].shape) == (14, 96, 1, 1)
    assert model.backbone.num_bev_features == 96


@pytest.mark.parametrize("mode", lt.MODES)
def test_launch_trace_with_backbone(mode, monkeypatch):
    """the model with the backbone and the head against its fixture; each deblock is ONE cobevt_deconv_nhwc launch into its slice of
    the 96-channel map, nothing of torch between them, and the head's product follows"""
    got = json.loads(json.dumps(ltb.trace(mode, monkeypatch.setattr)))
    want = ltb.read_fixture(mode)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: launch %d differs from the fixture\n  traced:  %s\n  fixture: %s" % (mode, i, json.dumps(g), json.dumps(w))
    assert len(got) == len(want)
    code = 0 if mode == "bf16" else 1
    kpad = (lambda c: -(-c // 32) * 32) if mode == "bf16" else (lambda c: -(-c // 16) * 16)
    deconvs = [r for r in got if r[1] == "cobevt_deconv_nhwc"]
    # dims: dtype, N, H, W, Cin, Cout, Kpad, s, c_off, ldc, act
    assert [r[2][4] for r in deconvs] == [[code, 1, 8, 12, 32, 32, kpad(32), 1, 0, 96, 1], [code, 1, 4, 6, 32, 32, kpad(32), 2, 32, 96, 1],
                                          [code, 1, 2, 3, 64, 32, kpad(64), 4, 64, 96, 1]]
    assert {r[0] for r in deconvs} == {"" if mode in ("bf16", "fp32") else "f32s"}
    names = [r[1] for r in got]
    first = names.index("cobevt_deconv_nhwc")
    # FuseBEVT first, then the six block convs interleaved with the three deblocks, then the head's one product
    assert len(names) - first == 3 + 3 * 2 - 2 + 1 and names[-2] == "cobevt_deconv_nhwc"


def test_existing_point_pillar_traces_launch_nothing_new():
    """without the argument nothing of the new path is launched (the existing fixtures replay unchanged in test_launch_traces.py)"""
    for mode in lt.MODES:
        assert "cobevt_deconv_nhwc" not in {name for _, name, _ in lt.read_fixture("point_pillar.%s" % mode)}
