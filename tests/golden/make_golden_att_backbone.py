"""Generate gv26_att_bev_backbone.npz and gv26_att_bev_backbone_compression.npz by running the REFERENCE's AttBEVBackbone
(opencood/models/backbones/att_bev_backbone.py with fusion_modules/self_attn.py AttFusion and sub_modules/auto_encoder.py AutoEncoder)
in eval mode on the CPU, in the build container like make_golden.py:

    python tests/golden/make_golden_att_backbone.py

Main case: tests/att_backbone_ref.GOLDEN_CFG (three levels, layer_strides [2, 2, 2], upsample_strides [1, 2, 4]) on 32 input channels,
input (5, 32, 16, 24) of amplitude +-2 as record_len [3, 2].  The amplitude matters: at +-1 the deeper levels' softmax is nearly
uniform and a backbone that fused by the plain mean would sit close to the real one.  Asserted on the spot: the test-side restatement
(att_backbone_ref.mirror) matches the reference to 1e-5; between 10 % and 90 % of the outputs are cut by the ReLU; the restatement
with the attention replaced by the mean misses the bf16 gate by a factor of 10 or more.

Compression case (second file): one level, 32 -> 64 channels, compression 1 (AutoEncoder(64, 1)), upsample [1] -> 32, input
(3, 32, 16, 16) as record_len [2, 1]; also the AutoEncoder's own input and output.  After the autoencoder the features are tiny and
the attention is close to a mean: this case pins the wiring, not the attention.

Also stored in the main file: the reference's state_dict keys and shapes with compression 2 (COMPRESSION2_CFG, 126 keys), and the
golden of PointPillarIntermediate - not a class of the reference tree: the generator's own composition of the reference's PillarVFE,
PointPillarScatter and AttBEVBackbone with two nn.Conv2d heads under OpenCOOD's attribute names, on cases_pillar voxels of two agents.

Weights, BatchNorm affine and running statistics are procedural (synth.fill_module_, seed 0), inputs seeded.  Prints the deviations
d32 / d16 the module-level GPU gates are made of and the fp32 restatement's deviation per kernel case (the kernel-level gates)."""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn as nn

import make_golden as mg                      # first: puts the repository, this directory and the stand-ins in place
import cases_pillar as cp
from cobevt_amd.synth import fill_module_, procedural_input

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import att_backbone_ref as ar  # noqa: E402

from opencood.models.backbones.att_bev_backbone import AttBEVBackbone as R_AttBEVBackbone  # noqa: E402
from opencood.models.sub_modules.pillar_vfe import PillarVFE as R_PillarVFE  # noqa: E402
from opencood.models.sub_modules.point_pillar_scatter import PointPillarScatter as R_PointPillarScatter  # noqa: E402


def _report(name, d32, d16, scale):
    print("  %-18s d32 %.3e  d16 %.3e  max|out| %.4f  -> gates %.3e / %.3e (relative)" % (name, d32, d16, scale, 4 * d32 / scale, 4 * d16 / scale))


def _run(cfg, channels, x, record_len):
    model = fill_module_(R_AttBEVBackbone(copy.deepcopy(cfg), channels), 0).eval()
    out = model({"spatial_features": x.clone(), "record_len": torch.tensor(record_len)})["spatial_features_2d"]
    return model, {k: v.clone() for k, v in model.state_dict().items()}, out


class Composition(nn.Module):
    """the reference's modules under OpenCOOD's PointPillarIntermediate attribute names"""

    def __init__(self, args):
        super().__init__()
        self.pillar_vfe = R_PillarVFE(copy.deepcopy(args["pillar_vfe"]), 4, args["voxel_size"], args["lidar_range"])
        self.scatter = R_PointPillarScatter(copy.deepcopy(args["point_pillar_scatter"]))
        self.backbone = R_AttBEVBackbone(copy.deepcopy(args["base_bev_backbone"]), 64)
        self.cls_head = nn.Conv2d(self.backbone.num_bev_features, args["anchor_number"], kernel_size=1)
        self.reg_head = nn.Conv2d(self.backbone.num_bev_features, 7 * args["anchor_number"], kernel_size=1)

    def forward(self, vox, record_len):
        bd = self.scatter(self.pillar_vfe({k: v.clone() for k, v in vox.items()}))
        bd["record_len"] = record_len
        feat = self.backbone(bd)["spatial_features_2d"]
        return self.cls_head(feat), self.reg_head(feat), feat


def gv26():
    out = {}
    # ---- main case
    x = procedural_input("gv26.spatial_features", ar.INPUT_SHAPE, 0, -ar.AMPLITUDE, ar.AMPLITUDE)
    model, sd, want = _run(ar.GOLDEN_CFG, ar.INPUT_CHANNELS, x, ar.RECORD_LEN)
    assert tuple(want.shape) == (2, 96, 8, 12) and model.num_bev_features == 96 and len(sd) == 54
    mg._close("AttBEVBackbone (mirror, fp32)", ar.mirror(sd, ar.GOLDEN_CFG, x, ar.RECORD_LEN, torch.float32), want, tol=1e-5)
    zero = float((want == 0).float().mean())
    print("  %.0f %% of the outputs are cut by the ReLU, max|out| %.3f" % (100 * zero, float(want.abs().max())))
    assert 0.1 <= zero <= 0.9
    d32, d16, scale = ar.deviations(sd, ar.GOLDEN_CFG, x, ar.RECORD_LEN)
    _report("golden", d32, d16, scale)
    ref = ar.mirror(sd, ar.GOLDEN_CFG, x, ar.RECORD_LEN)
    miss = float((ar.mirror(sd, ar.GOLDEN_CFG, x, ar.RECORD_LEN, fuse="mean") - ref).abs().max())
    print("  a mean-fusion backbone is %.3e away: %.1f x the bf16 gate %.3e" % (miss, miss / (4 * d16), 4 * d16))
    assert miss >= 10 * 4 * d16, "the inputs do not tell the attention from a mean: change the amplitude, not the gate"
    out.update(input=mg._np(x), output=mg._np(want), **{"sd/" + k: mg._np(v) for k, v in sd.items()})
    # ---- keys and shapes with compression 2
    sd2 = R_AttBEVBackbone(copy.deepcopy(ar.COMPRESSION2_CFG), ar.INPUT_CHANNELS).state_dict()
    assert len(sd2) == 126
    out["compression2/keys"] = np.array(list(sd2.keys()))
    out["compression2/shapes"] = np.array([",".join(str(int(d)) for d in t.shape) for t in sd2.values()])
    # ---- PointPillarIntermediate
    args, vox = ar.pillar_args(), ar.pillar_voxels()
    comp = fill_module_(Composition(args), 0).eval()
    psm, rm, feat = comp(vox, torch.tensor(ar.PILLAR_RECORD_LEN))
    psd = {k: v.clone() for k, v in comp.state_dict().items()}
    got = ar.pillar_intermediate(psd, args, vox, ar.PILLAR_RECORD_LEN, torch.float32)
    for name, g, w in zip(("psm", "rm", "spatial_features_2d"), got, (psm, rm, feat)):
        mg._close("PointPillarIntermediate %s (mirror, fp32)" % name, g, w, tol=1e-5)
    r64 = ar.pillar_intermediate(psd, args, vox, ar.PILLAR_RECORD_LEN, torch.float64)
    r16 = ar.pillar_intermediate(psd, args, vox, ar.PILLAR_RECORD_LEN, torch.float64, bf16=True)
    for i, name in enumerate(("psm", "rm")):
        _report("pillar " + name, float((got[i].double() - r64[i]).abs().max()), float((r16[i] - r64[i]).abs().max()), float(r64[i].abs().max()))
    out.update({"pillar/psm": mg._np(psm), "pillar/rm": mg._np(rm), "pillar/keys": np.array(list(psd.keys())),
                "pillar/shapes": np.array([",".join(str(int(d)) for d in t.shape) for t in psd.values()])})
    mg.save("gv26_att_bev_backbone", **out)
    # ---- compression case
    xc = procedural_input("gv26.compression", ar.COMPRESSION_SHAPE, 0, -ar.AMPLITUDE, ar.AMPLITUDE)
    seen = {}
    model, sdc, wantc = None, None, None
    model = fill_module_(R_AttBEVBackbone(copy.deepcopy(ar.COMPRESSION_CFG), ar.INPUT_CHANNELS), 0).eval()
    h = model.compression_modules[0].register_forward_hook(lambda mod, i, o: seen.update(ae_in=i[0].clone(), ae_out=o.clone()))
    wantc = model({"spatial_features": xc.clone(), "record_len": torch.tensor(ar.COMPRESSION_RECORD_LEN)})["spatial_features_2d"]
    h.remove()
    sdc = {k: v.clone() for k, v in model.state_dict().items()}
    assert tuple(wantc.shape) == (2, 32, 8, 8) and len(sdc) == 18 + 24
    mg._close("AttBEVBackbone compression (mirror, fp32)", ar.mirror(sdc, ar.COMPRESSION_CFG, xc, ar.COMPRESSION_RECORD_LEN, torch.float32), wantc, tol=1e-5)
    mg._close("AutoEncoder (mirror, fp32)", ar.auto_encoder(sdc, "compression_modules.0.", seen["ae_in"], torch.float32), seen["ae_out"], tol=1e-5)
    zero = float((wantc == 0).float().mean())
    print("  compression: %.0f %% of the outputs are cut by the ReLU, max|out| %.3f, max|autoencoder out| %.3f"
          % (100 * zero, float(wantc.abs().max()), float(seen["ae_out"].abs().max())))
    assert 0.1 <= zero <= 0.9
    _report("compression", *ar.deviations(sdc, ar.COMPRESSION_CFG, xc, ar.COMPRESSION_RECORD_LEN))
    _report("autoencoder", *ar.auto_encoder_deviations(sdc, "compression_modules.0.", seen["ae_in"]))
    mg.save("gv26_att_bev_backbone_compression", input=mg._np(xc), output=mg._np(wantc), ae_input=mg._np(seen["ae_in"]),
            ae_output=mg._np(seen["ae_out"]), **{"sd/" + k: mg._np(v) for k, v in sdc.items()})


def branches():
    """d32 / d16 of the restatement on BaseBEVBackbone's other branches with the fusion in them (no reference run: np.int)"""
    from cobevt_amd import host
    x = procedural_input("gv26.spatial_features", ar.INPUT_SHAPE, 0, -ar.AMPLITUDE, ar.AMPLITUDE)
    for name in sorted(ar.MIRROR_CFGS):
        sd = fill_module_(host.AttBEVBackbone(copy.deepcopy(ar.MIRROR_CFGS[name]), ar.INPUT_CHANNELS), 0).state_dict()
        _report(name, *ar.deviations(sd, ar.MIRROR_CFGS[name], x, ar.RECORD_LEN))


def kernel_gates():
    """the fp32 restatement's own deviation from float64 per kernel case and storage dtype -> gv26_att_fuse_kernel_d32.json"""
    import json
    table = {}
    for dt in (torch.float32, torch.bfloat16):
        for c, hw, rl in ar.KERNEL_CASES + [ar.EMPTY_SAMPLE_CASE, ar.MODULE_CASE]:
            table[ar.case_key(c, hw, rl, dt)] = ar.kernel_d32(ar.kernel_input(c, hw, rl), rl, dt)
        c, hw, rl = ar.LARGE_SCORE_CASE
        x = ar.large_score_input()
        table["large_score_" + ar.case_key(c, hw, rl, dt)] = ar.kernel_d32(x, rl, dt)
        score = float((x.to(dt).double()[0] ** 2).sum(-1).min()) / c ** 0.5
        print("  large scores (%s): smallest ego self-score %.1f, d32 %.3e" % (dt, score, table["large_score_" + ar.case_key(c, hw, rl, dt)]))
    # (a sample of one agent is reproduced exactly by every implementation: record_len [1, 1] has d32 = 0, and so its fp32 gate)
    assert all((v > 0.0) == ("rl1-1_" not in k) for k, v in table.items())
    assert len(table) == 2 * (len(ar.KERNEL_CASES) + 3)
    with open(ar.KERNEL_D32_FILE, "w") as f:
        json.dump({k: float("%.4e" % v) for k, v in table.items()}, f, indent=0, sort_keys=True)
        f.write("\n")
    for dt in ("fp32", "bf16"):
        vals = [v for k, v in table.items() if k.endswith(dt) and not k.startswith("large") and "rl1-1_" not in k]
        print("  kernel d32 (%s): %.3e .. %.3e over %d cases" % (dt, min(vals), max(vals), len(vals)))


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    if sys.argv[1:] != ["gates"]:
        gv26()
    branches()
    kernel_gates()
