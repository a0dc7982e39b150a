"""Test-side torch restatement of AttFusion, AutoEncoder and AttBEVBackbone (our own code, pure functions of a state_dict, built on
tests/bev_backbone_ref.py's layer), the configurations the attentive-backbone tests share, the cobevt_att_fuse_nhwc kernel cases and
their float64 reference.

att_fusion(x, record_len, dtype) restates the reference's procedure (self_attn.py: per sample (HW, n, C) rows, bmm / sqrt(C), softmax,
bmm, row 0) in `dtype`; mirror(sd, cfg, x, record_len, dtype, bf16) is bev_backbone_ref.mirror with the compression and the fusion
between a block and its deblock; bf16=True rounds the folded weights, the input and every layer's and fusion's output to bfloat16 -
the storage roundings of the bf16 compute mode, with exact arithmetic in between.  fuse="mean" replaces the attention by the plain
mean over the agents: the wrong backbone the golden's generator measures its inputs against."""
import os

import numpy as np
import torch

import bev_backbone_ref as br
from bev_backbone_ref import _layer, _rd, fold

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gv26_att_bev_backbone.npz")
GOLDEN_COMPRESSION = os.path.join(HERE, "golden", "gv26_att_bev_backbone_compression.npz")

# the main case (tests/golden/make_golden_att_backbone.py): BaseBEVBackbone's golden configuration on five agents in two samples
GOLDEN_CFG = br.GOLDEN_CFG
INPUT_CHANNELS = 32
INPUT_SHAPE = (5, 32, 16, 24)
RECORD_LEN = [3, 2]
AMPLITUDE = 2.0
# the compression case: one level; AutoEncoder(64, 1) = 64 -> 64 (stride 2) -> 32, transposed conv 32 -> 64, 64 -> 64
COMPRESSION_CFG = dict(layer_nums=[1], layer_strides=[2], num_filters=[64], upsample_strides=[1], num_upsample_filter=[32], compression=1)
COMPRESSION_SHAPE = (3, 32, 16, 16)
COMPRESSION_RECORD_LEN = [2, 1]
# keys and shapes only: three levels wide enough for compression 2 (AutoEncoder(64, 2) and AutoEncoder(64, 1))
COMPRESSION2_CFG = dict(layer_nums=[1, 1, 1], layer_strides=[2, 2, 2], num_filters=[64, 64, 128], upsample_strides=[1, 2, 4],
                        num_upsample_filter=[32, 32, 32], compression=2)
# BaseBEVBackbone's other branches with the fusion in them, against the mirror
MIRROR_CFGS = br.MIRROR_CFGS
# PointPillarIntermediate's golden: cases_pillar voxels of two agents on a 16 x 24 grid, one sample
PILLAR_GRID = (16, 24)
PILLAR_COUNTS = [150, 130]
PILLAR_RECORD_LEN = [2]
ANCHOR_NUMBER = 2


def load_golden(path=GOLDEN):
    z = np.load(path)
    sd = {k[len("sd/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return sd, torch.from_numpy(z["input"]), torch.from_numpy(z["output"]), z


def offsets(record_len):
    return [int(sum(record_len[:b])) for b in range(len(record_len))]


def att_fusion(x, record_len, dtype=torch.float64, mean=False):
    """(N, C, H, W) -> (B, C, H, W) in `dtype`: the reference's AttFusion.forward, sample by sample"""
    x = x.to(dtype)
    n_all, c, h, w = x.shape
    out = []
    for off, n in zip(offsets(record_len), record_len):
        if n <= 0:
            out.append(torch.zeros(1, c, h, w, dtype=dtype))
            continue
        xx = x[off:off + n].reshape(n, c, -1).permute(2, 0, 1)                    # (HW, n, C)
        if mean:
            ctx = xx.mean(dim=1, keepdim=True).expand_as(xx)
        else:
            score = torch.bmm(xx, xx.transpose(1, 2)) / float(np.sqrt(c))
            ctx = torch.bmm(torch.softmax(score, -1), xx)
        out.append(ctx.permute(1, 2, 0).reshape(n, c, h, w)[0:1])
    return torch.cat(out, dim=0)


def auto_encoder(sd, prefix, x, dtype=torch.float64, bf16=False):
    layers = len({k[len(prefix + "encoder."):].split(".")[0] for k in sd if k.startswith(prefix + "encoder.")})
    for i in range(layers):
        p = "%sencoder.%d." % (prefix, i)
        x = _layer(x, sd[p + "1.weight"], *fold(sd, p + "2."), dtype, bf16, 2, pad=1)
        x = _layer(x, sd[p + "4.weight"], *fold(sd, p + "5."), dtype, bf16, 1, pad=1)
    for i in range(layers - 1, -1, -1):
        p = "%sdecoder.%d." % (prefix, i)
        x = _layer(x, sd[p + "0.0.weight"], *fold(sd, p + "0.1."), dtype, bf16, 2, transposed=True)
        x = _layer(x, sd[p + "1.0.weight"], *fold(sd, p + "1.1."), dtype, bf16, 1, pad=1)
    return x


def mirror(sd, cfg, x, record_len, dtype=torch.float64, bf16=False, fuse="att"):
    """(N, C, H, W) -> spatial_features_2d (B, C', H', W') in `dtype`"""
    nums, strides = cfg.get("layer_nums", []), cfg.get("layer_strides", [])
    ups = cfg.get("upsample_strides", [])
    comp = int(cfg.get("compression", 0) or 0)
    x = _rd(x.to(dtype), dtype, bf16)
    outs = []
    for i in range(len(nums)):
        for k in range(nums[i] + 1):
            idx = 1 + 3 * k
            x = _layer(x, sd["blocks.%d.%d.weight" % (i, idx)], *fold(sd, "blocks.%d.%d." % (i, idx + 1)), dtype, bf16,
                       strides[i] if k == 0 else 1, pad=1)
        if comp - i > 0:
            x = auto_encoder(sd, "compression_modules.%d." % i, x, dtype, bf16)
        y = _rd(att_fusion(x, record_len, dtype, mean=fuse == "mean"), dtype, bf16)
        if ups:
            w, (sc, sh) = sd["deblocks.%d.0.weight" % i], fold(sd, "deblocks.%d.1." % i)
            if ups[i] >= 1:
                outs.append(_layer(y, w, sc, sh, dtype, bf16, int(ups[i]), transposed=True))
            else:
                outs.append(_layer(y, w, sc, sh, dtype, bf16, int(round(1.0 / ups[i]))))
        else:
            outs.append(y)
    y = torch.cat(outs, dim=1) if len(outs) > 1 else outs[0]
    if len(ups) > len(nums):
        i = len(nums)
        y = _layer(y, sd["deblocks.%d.0.weight" % i], *fold(sd, "deblocks.%d.1." % i), dtype, bf16, int(ups[-1]), transposed=True)
    return y


def deviations(sd, cfg, x, record_len):
    """-> (d32, d16, max|out|): max-norm deviation of the fp32 mirror / the bf16-rounded mirror from the float64 mirror"""
    ref = mirror(sd, cfg, x, record_len, torch.float64)
    d32 = float((mirror(sd, cfg, x, record_len, torch.float32).double() - ref).abs().max())
    d16 = float((mirror(sd, cfg, x, record_len, torch.float64, bf16=True) - ref).abs().max())
    return d32, d16, float(ref.abs().max())


def auto_encoder_deviations(sd, prefix, x):
    ref = auto_encoder(sd, prefix, x.double())
    d32 = float((auto_encoder(sd, prefix, x.float(), torch.float32).double() - ref).abs().max())
    d16 = float((auto_encoder(sd, prefix, _rd(x.double(), torch.float64, True), torch.float64, bf16=True) - ref).abs().max())
    return d32, d16, float(ref.abs().max())


def pillar_args():
    """PointPillarIntermediate's arguments of the golden (cases_pillar's front end on PILLAR_GRID, the golden backbone on its 64 channels)"""
    import copy
    import cases_pillar as cp
    args = cp.model_args(grid=PILLAR_GRID, max_cav=2)
    del args["fax_fusion"], args["max_cav"]
    args["base_bev_backbone"] = copy.deepcopy(GOLDEN_CFG)
    args["anchor_number"] = ANCHOR_NUMBER
    return args


def pillar_voxels():
    import cases_pillar as cp
    return cp.voxels(counts=PILLAR_COUNTS, grid=PILLAR_GRID, tag="gv26")


def pillar_intermediate(sd, args, vox, record_len, dtype=torch.float64, bf16=False):
    """PointPillarIntermediate on a state_dict -> (psm, rm, spatial_features_2d) in `dtype`: tests/pillar_ref.py's front end (one canvas
    per agent), mirror() on the backbone.* entries, both 1 x 1 heads"""
    import pillar_ref as pr
    cfg = args["pillar_vfe"]
    w, s = pr.fold(sd, "pillar_vfe.pfn_layers.0.", cfg["use_norm"])
    g = pr.geom(args["voxel_size"], args["lidar_range"])
    ny, nx = args["point_pillar_scatter"]["grid_size"][1], args["point_pillar_scatter"]["grid_size"][0]
    rows = pr.pillar_features(vox["voxel_features"].to(dtype), vox["voxel_num_points"], vox["voxel_coords"], w.to(dtype), s.to(dtype), g,
                              cfg["use_absolute_xyz"], cfg["with_distance"])
    canvas = pr.scatter(rows, vox["voxel_coords"], int(sum(record_len)), ny, nx).permute(0, 3, 1, 2)
    bsd = {k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}
    feat = mirror(bsd, args["base_bev_backbone"], canvas, record_len, dtype, bf16)
    heads = []
    for name in ("cls_head", "reg_head"):
        wh = _rd(sd[name + ".weight"].double().flatten(1), dtype, bf16)
        y = torch.einsum("nchw,oc->nohw", feat, wh) + sd[name + ".bias"].to(dtype)[None, :, None, None]
        heads.append(_rd(y, dtype, bf16))
    return heads[0], heads[1], feat


# ----------------------------------------------------------------------------------------------
# kernel cases: (C, HW, record_len).  C = 8 .. 512 gives groups of G = 1, 8, 32, 64 lanes; HW = 35 is a partial wave for every G;
# HW = 300 crosses a 256-thread block at G = 1 (and is several blocks for the others)
# ----------------------------------------------------------------------------------------------
KERNEL_CHANNELS = [8, 64, 256, 512]
KERNEL_HW = [35, 300]
KERNEL_RECORD_LENS = [[1, 3, 2], [5], [1, 1]]
KERNEL_CASES = [(c, hw, tuple(rl)) for c in KERNEL_CHANNELS for hw in KERNEL_HW for rl in KERNEL_RECORD_LENS]
# recorded with them: the case with a sample without agents, and the one host.AttFusion's contract test runs as a (5, 32, 6, 7) map
EMPTY_SAMPLE_CASE = (64, 35, (2, 0, 1))
MODULE_CASE = (32, 42, (3, 2))


def kernel_amplitude(c):
    """inputs uniform in +-a with a^2 sqrt(C) / 3 = 1.5: the ego's self-score is 1.5 on average whatever C is, the other agents' scores
    scatter around 0, so the softmax is neither uniform nor one-hot"""
    return (4.5 / c ** 0.5) ** 0.5


def kernel_input(c, hw, record_len, amplitude=None, seed=0):
    """-> x (N, HW, C) fp32, seeded"""
    a = kernel_amplitude(c) if amplitude is None else amplitude
    g = torch.Generator().manual_seed(1000 * seed + 31 * c + hw + 7 * len(record_len) + sum(record_len))
    return (torch.rand(max(sum(record_len), 1), hw, c, generator=g) - 0.5) * 2.0 * a


def att_fuse_f64(x, record_len, store_dtype):
    """float64 evaluation from the operand the kernel gets: x (N, HW, C) rounded to `store_dtype` by this function itself.
    -> (B, HW, C) float64; a sample without agents is zeros"""
    xs = x.to(store_dtype).double()
    out = []
    for off, n in zip(offsets(record_len), record_len):
        if n <= 0:
            out.append(torch.zeros_like(xs[0:1]))
            continue
        a = xs[off:off + n]                                                       # (n, HW, C)
        w = torch.softmax(torch.einsum("pc,npc->pn", a[0], a) / float(np.sqrt(a.shape[-1])), dim=-1)
        out.append(torch.einsum("pn,npc->pc", w, a)[None])
    return torch.cat(out, dim=0)


def att_fuse_fp32_restatement(x, record_len, store_dtype):
    """the fp32 torch restatement (att_fusion, the reference's procedure) on the same rounded operand -> (B, HW, C) fp32"""
    xs = x.to(store_dtype).float()
    n, hw, c = xs.shape
    return att_fusion(xs.permute(0, 2, 1).reshape(n, c, hw, 1), list(record_len), torch.float32).reshape(len(record_len), c, hw).permute(0, 2, 1)


def kernel_d32(x, record_len, store_dtype):
    """max deviation of the fp32 restatement from the float64 reference: a quarter of the kernel's fp32 gate"""
    return float((att_fuse_fp32_restatement(x, record_len, store_dtype).double() - att_fuse_f64(x, record_len, store_dtype)).abs().max())


LARGE_SCORE_CASE = (256, 35, (3, 2))            # C, HW, record_len
LARGE_SCORE_AMPLITUDE, LARGE_SCORE_SPREAD = 6.0, 0.5


def large_score_input(seed=0):
    """every agent = its sample's ego (uniform in +-6) + uniform +-0.5: all scores sit near the ego's self-score 36 * 256 / 3 / 16 = 192
    (exp overflows fp32 without the running maximum) and differ from it by about 1, so the softmax still mixes the agents"""
    c, hw, rl = LARGE_SCORE_CASE
    g = torch.Generator().manual_seed(1000 * seed + 77)
    x = (torch.rand(sum(rl), hw, c, generator=g) - 0.5) * 2.0 * LARGE_SCORE_SPREAD
    for off, n in zip(offsets(rl), rl):
        ego = (torch.rand(hw, c, generator=g) - 0.5) * 2.0 * LARGE_SCORE_AMPLITUDE
        x[off] = 0.0
        x[off:off + n] += ego
    return x


# the fp32 restatement's deviation from float64 per kernel case and storage dtype (kernel_d32), measured on the CPU and recorded by
# tests/golden/make_golden_att_backbone.py: a quarter of each case's fp32 gate (tests/golden/README_gv26.md)
KERNEL_D32_FILE = os.path.join(HERE, "golden", "gv26_att_fuse_kernel_d32.json")


def case_key(c, hw, record_len, store_dtype):
    return "C%d_HW%d_rl%s_%s" % (c, hw, "-".join(str(v) for v in record_len), "bf16" if store_dtype == torch.bfloat16 else "fp32")


def load_kernel_d32():
    import json
    with open(KERNEL_D32_FILE) as f:
        return json.load(f)
