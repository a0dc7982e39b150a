"""CPU: host.AttBEVBackbone's and host.AutoEncoder's state_dicts against the reference's (fixtures gv26), their constructor branches and
errors, the preconditions of ops.att_fuse and of its C entry point, PointPillarIntermediate's keys and registry name, and the launch sequence of that model in
the four compute modes (tests/launch_trace_att_backbone.py)."""
import copy
import ctypes
import json

import pytest
import torch

import att_backbone_ref as ar
import bev_backbone_ref as br
import launch_trace as lt
import launch_trace_att_backbone as lta
import launch_trace_bev_backbone as ltb
from cobevt_amd import host, lib, ops
from cobevt_amd.lib import CobevtHipError
from cobevt_amd.registry import create_model


def _shapes(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


def _recorded(z, prefix):
    return {k: tuple(int(d) for d in s.split(",") if d) for k, s in zip(z[prefix + "/keys"].tolist(), z[prefix + "/shapes"].tolist())}


def test_state_dict_is_the_references():
    sd, _, _, z = ar.load_golden()
    model = host.AttBEVBackbone(copy.deepcopy(ar.GOLDEN_CFG), ar.INPUT_CHANNELS)
    own = model.state_dict()
    assert len(own) == 54 and list(own) == list(sd) and _shapes(own) == _shapes(sd)
    model.load_state_dict(sd, strict=True)
    assert [type(m).__name__ for m in model.fuse_modules] == ["AttFusion"] * 3 and not list(model.fuse_modules.parameters())
    assert not model.compress and not hasattr(model, "compression_modules")
    # the same keys as the backbone without fusion: the fusion has no parameters
    assert list(own) == list(host.BaseBEVBackbone(copy.deepcopy(ar.GOLDEN_CFG), ar.INPUT_CHANNELS).state_dict())
    # compression 2: AutoEncoder(64, 2) at level 0, AutoEncoder(64, 1) at level 1, none at level 2
    own2 = host.AttBEVBackbone(copy.deepcopy(ar.COMPRESSION2_CFG), ar.INPUT_CHANNELS).state_dict()
    want2 = _recorded(z, "compression2")
    assert len(own2) == 126 and list(own2) == list(want2) and _shapes(own2) == want2
    assert "compression_modules.0.decoder.1.0.0.weight" in own2 and "compression_modules.1.encoder.0.4.weight" in own2
    assert not any(k.startswith("compression_modules.2.") for k in own2)


def test_compression_state_dict_and_autoencoder_keys():
    sd, _, _, _ = ar.load_golden(ar.GOLDEN_COMPRESSION)
    model = host.AttBEVBackbone(copy.deepcopy(ar.COMPRESSION_CFG), ar.INPUT_CHANNELS)
    own = model.state_dict()
    assert list(own) == list(sd) and _shapes(own) == _shapes(sd)
    model.load_state_dict(sd, strict=True)
    ae = host.AutoEncoder(64, 1)
    pre = "compression_modules.0."
    assert list(ae.state_dict()) == [k[len(pre):] for k in sd if k.startswith(pre)]
    assert tuple(ae.decoder[0][0][0].weight.shape) == (32, 64, 2, 2) and ae.encoder[0][1].stride == (2, 2)
    assert ae.out_size(8, 8) == (8, 8) and ae.out_size(5, 7) == (6, 8) and host.AutoEncoder(128, 2).out_size(8, 12) == (8, 12)


@pytest.mark.parametrize("cfg, want", [
    (ar.GOLDEN_CFG, 96), (ar.COMPRESSION_CFG, 32), (ar.COMPRESSION2_CFG, 96), (br.STANDARD_CFG, 384),
    (ar.MIRROR_CFGS["down_deblock"], 96), (ar.MIRROR_CFGS["trailing_deblock"], 96), (ar.MIRROR_CFGS["no_deblocks"], 96)])
def test_num_bev_features(cfg, want):
    model = host.AttBEVBackbone(copy.deepcopy(cfg), 64)
    assert model.num_bev_features == want and len(model.fuse_modules) == len(model.blocks) == len(cfg["layer_nums"])
    assert [m.feature_dim for m in model.fuse_modules] == list(cfg["num_filters"])


def test_constructor_errors():
    base = dict(layer_nums=[1, 1], layer_strides=[2, 2], num_filters=[32, 64])
    # AutoEncoder(32, 2): its second decoder is a transposed conv 8 -> 16, which the deconv kernel (32 output channels per tile) cannot take
    with pytest.raises(CobevtHipError, match=r"AutoEncoder\(32, 2\): decoder 1 is a transposed conv 8 -> 16"):
        host.AutoEncoder(32, 2)
    with pytest.raises(CobevtHipError, match=r"AutoEncoder\(32, 2\)"):
        host.AttBEVBackbone(dict(base, upsample_strides=[1, 2], num_upsample_filter=[32, 32], compression=2), 32)
    # BaseBEVBackbone's checks hold for the subclass
    with pytest.raises(CobevtHipError, match="multiple of 32"):
        host.AttBEVBackbone(dict(base, upsample_strides=[1, 2], num_upsample_filter=[48, 48]), 32)
    with pytest.raises(CobevtHipError, match="AttBEVBackbone: layer_nums, layer_strides and num_filters"):
        host.AttBEVBackbone(dict(base, layer_strides=[2]), 32)
    # a level whose width the fusion kernel cannot take (8 x a power of two)
    with pytest.raises(CobevtHipError, match="feature_dim=48"):
        host.AttBEVBackbone(dict(layer_nums=[1], layer_strides=[2], num_filters=[48]), 32)
    with pytest.raises(CobevtHipError, match="feature_dim=1024"):
        host.AttFusion(1024)


def test_att_fuse_preconditions(monkeypatch):
    """all raised before the device check and before any launch: CPU tensors reach them"""
    rec = lt.Recorder()
    monkeypatch.setattr("cobevt_amd.lib.load", rec.load)
    x = torch.zeros(3, 2, 5, 64, dtype=torch.bfloat16)
    rl = torch.tensor([2, 1], dtype=torch.int32)
    with pytest.raises(CobevtHipError, match="C=24"):
        ops.att_fuse(torch.zeros(3, 2, 5, 24, dtype=torch.bfloat16), rl)
    with pytest.raises(CobevtHipError, match="C=1024"):
        ops.att_fuse(torch.zeros(3, 2, 5, 1024, dtype=torch.bfloat16), rl)
    with pytest.raises(CobevtHipError, match="contiguous"):
        ops.att_fuse(torch.zeros(3, 2, 64, 5, dtype=torch.bfloat16).permute(0, 1, 3, 2), rl)
    with pytest.raises(CobevtHipError, match=r"\(N, H, W, C\)"):
        ops.att_fuse(x[0], rl)
    with pytest.raises(CobevtHipError, match="compute dtype"):
        ops.att_fuse(x.to(torch.float16), rl)
    with pytest.raises(CobevtHipError, match="record_len must be a contiguous int32"):
        ops.att_fuse(x, rl.long())
    with pytest.raises(CobevtHipError, match="record_len must be a contiguous int32"):
        ops.att_fuse(x, torch.zeros(0, dtype=torch.int32))
    with pytest.raises(CobevtHipError, match="out= must be a contiguous torch.bfloat16 tensor of shape"):
        ops.att_fuse(x, rl, out=torch.zeros(3, 2, 5, 64, dtype=torch.bfloat16))
    with pytest.raises(CobevtHipError, match="out= must be"):
        ops.att_fuse(x, rl, out=torch.zeros(2, 2, 5, 64))
    with pytest.raises(CobevtHipError, match="ROCm device"):                                # valid arguments: only the device is missing
        ops.att_fuse(x, rl)
    assert rec.records == []


def test_c_abi_validates_arguments_before_any_launch():
    """cobevt_att_fuse_nhwc rejects null pointers and an unknown dtype (COBEVT_ERR_ARG = 1) and unsupported shapes (COBEVT_ERR_SHAPE = 2)
    without touching a device, in all three libraries (one shared object)"""
    buf = (ctypes.c_float * 16)()                               # host memory: only its address is looked at
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    for variant in ("", "f32s", "f32h"):
        f = lib.load(variant).cobevt_att_fuse_nhwc

        def call(x=ptr, rl=ptr, out=ptr, dtype=0, b=1, n=2, hw=4, c=64):
            return f(x, rl, out, dtype, b, n, hw, c, ctypes.c_float(0.125), None)
        assert call(x=None) == 1 and call(rl=None) == 1 and call(out=None) == 1 and call(dtype=2) == 1
        for bad in (dict(c=24), dict(c=12), dict(c=0), dict(c=1024), dict(b=0), dict(b=65536), dict(n=0), dict(hw=0), dict(hw=-1)):
            assert call(**bad) == 2, bad


def test_train_mode_forward_raises():
    model = host.AttBEVBackbone(copy.deepcopy(ar.GOLDEN_CFG), 32).train()
    with pytest.raises(CobevtHipError, match="inference path"):
        model({"spatial_features": torch.zeros(2, 32, 16, 24), "record_len": torch.tensor([2])})
    with pytest.raises(CobevtHipError, match="inference path"):
        host.AttFusion(32).train()(torch.zeros(2, 32, 4, 4), torch.tensor([2]))
    with pytest.raises(CobevtHipError, match="inference path"):
        host.AutoEncoder(64, 1).train()(torch.zeros(1, 64, 8, 8))
    with pytest.raises(CobevtHipError, match="inference path"):
        host.PointPillarIntermediate(ar.pillar_args()).train()({"processed_lidar": ar.pillar_voxels(), "record_len": [2]})


def test_mismatched_level_sizes_raise_before_any_launch(monkeypatch):
    rec = lt.Recorder()
    lt.install(monkeypatch.setattr, rec)
    model = host.AttBEVBackbone(copy.deepcopy(ar.GOLDEN_CFG), 32).eval()
    with pytest.raises(CobevtHipError, match="AttBEVBackbone: .* a 10 x 24 input gives 5 x 12, 6 x 12, 8 x 12"):
        model.forward_nhwc(torch.zeros(2, 10, 24, 32, dtype=torch.bfloat16), torch.tensor([2], dtype=torch.int32))
    assert rec.records == []


def test_point_pillar_intermediate_layout_and_registry():
    _, _, _, z = ar.load_golden()
    want = _recorded(z, "pillar")
    model = create_model({"model": {"core_method": "point_pillar_intermediate", "args": ar.pillar_args()}})
    assert type(model) is host.PointPillarIntermediate
    own = model.state_dict()
    assert list(own) == list(want) and _shapes(own) == want
    assert [n for n, _ in model.named_children()] == ["pillar_vfe", "scatter", "backbone", "cls_head", "reg_head"]
    assert tuple(own["cls_head.weight"].shape) == (2, 96, 1, 1) and tuple(own["reg_head.weight"].shape) == (14, 96, 1, 1)
    assert isinstance(model.backbone, host.AttBEVBackbone) and model.backbone.num_bev_features == 96
    # the canvas's agent count comes from the host: a host record_len, or num_agents next to a device one
    assert model.num_agents({"record_len": [2, 3]}) == 5 and model.num_agents({"record_len": torch.tensor([1, 2])}) == 3
    assert model.num_agents({"record_len": None, "num_agents": 4}) == 4
    args = ar.pillar_args()
    args["anchor_number"] = 0
    with pytest.raises(CobevtHipError, match="anchor_number must be at least 1"):
        host.PointPillarIntermediate(args)


@pytest.mark.parametrize("mode", lt.MODES)
def test_launch_trace(mode, monkeypatch):
    """the model against its fixture: per level the block's convs on the N = 2 agent maps, ONE cobevt_att_fuse_nhwc launch to B = 1 map,
    ONE cobevt_deconv_nhwc launch into the level's slice of the 96-channel map; nothing of torch between them; the heads' one product"""
    got = json.loads(json.dumps(lta.trace(mode, monkeypatch.setattr)))
    want = lta.read_fixture(mode)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: launch %d differs from the fixture\n  traced:  %s\n  fixture: %s" % (mode, i, json.dumps(g), json.dumps(w))
    assert len(got) == len(want)
    code = 0 if mode == "bf16" else 1
    fuses = [r for r in got if r[1] == "cobevt_att_fuse_nhwc"]
    # x, record_len, out, dtype, B, N, HW, C, scale
    assert [r[2][3:8] for r in fuses] == [[code, 1, 2, 96, 32], [code, 1, 2, 24, 32], [code, 1, 2, 6, 64]]
    assert [r[2][8] for r in fuses] == pytest.approx([32 ** -0.5, 32 ** -0.5, 64 ** -0.5], rel=1e-6)
    assert all(r[2][:3] == ["ptr", "ptr", "ptr"] for r in fuses)
    # the fusion has no matrix product: the shared object's kernel, whichever library serves the mode
    assert {r[0] for r in fuses} == {"" if mode in ("bf16", "fp32") else "f32s"}
    names = [r[1] for r in got]
    assert names[0] == "cobevt_pillar_vfe" and names.count("cobevt_pillar_vfe") == 1
    at = [i for i, n in enumerate(names) if n == "cobevt_att_fuse_nhwc"]
    assert all(names[i + 1] == "cobevt_deconv_nhwc" for i in at) and len(names) == 1 + 3 * 4 + 1
    deconvs = [r[2][4] for r in got if r[1] == "cobevt_deconv_nhwc"]
    # dims: dtype, N, H, W, Cin, Cout, Kpad, s, c_off, ldc, act: the deblocks read B = 1 fused map
    assert [(d[1], d[7], d[8], d[9]) for d in deconvs] == [(1, 1, 0, 96), (1, 2, 32, 96), (1, 4, 64, 96)]


def test_existing_traces_launch_nothing_new(monkeypatch):
    """BaseBEVBackbone's launch sequence is unchanged by the shared level loop (its fixtures replay in test_bev_backbone.py; here once
    more for one mode), and no existing fixture launches the new kernel"""
    got = json.loads(json.dumps(ltb.trace("bf16", monkeypatch.setattr)))
    assert got == ltb.read_fixture("bf16")
    fixtures = [lt.read_fixture(name) for name in sorted(lt.CASES)] + [ltb.read_fixture(mode) for mode in lt.MODES]
    assert len(fixtures) == len(lt.CASES) + 4
    for fixture in fixtures:
        assert "cobevt_att_fuse_nhwc" not in {name for _, name, _ in fixture}
