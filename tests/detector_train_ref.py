"""Test-side references of the detectors' training path (our own code, differentiable torch in any dtype):

  * train-mode restatements of a deblock, BaseBEVBackbone, AttBEVBackbone (through att_backbone_ref.att_fusion) and the AutoEncoder as
    pure functions of a dict of parameters: batch statistics (biased variance in the normalisation, unbiased in the running update,
    eps 1e-3, momentum 0.01 as the modules build them), with optional FORCED ReLU masks per BatchNorm layer - the idea of
    tests/sparse_train_ref.py: a gradient is only comparable between two arithmetics when both cut the same pre-activations, so the
    float64 run is forced to the mask of the run under test and the disagreements are counted and bounded separately;
  * per-element float64 references of the transposed convolution's three kernels (weight gradient, raw forward, input gradient), each
    with its magnitude sum S = sum_k |a_k| |b_k|;
  * float64 / fp32 autograd of att_fusion for the attention kernel cases.

A Tape carries what a run records and what it is forced to.  Layers run in one fixed order (per level: the block's convs, the
compression's encoder and decoder layers, the level's deblock; the trailing deblock last), the order of host/training.py."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import att_backbone_ref as ar

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gv30_detector_train.npz")
ATT_BWD_D32_FILE = os.path.join(HERE, "golden", "gv30_att_fuse_bwd_d32.json")
EPS, MOMENTUM = 1e-3, 0.01
SAMPLE_CAP = 4096            # the golden keeps at most this many elements of a tensor: flat[::ceil(numel / SAMPLE_CAP)]
# seeds of fill_module_ at which the fp32 and the float64 restatement cut the same pre-activations (0 mask disagreements; asserted in
# tests/test_detector_train.py), per configuration of the module-level GPU tests
MODULE_SEEDS = {"golden": 0, "compression": 0, "down_deblock": 0, "trailing_deblock": 0, "no_deblocks": 0}


def sample(t):
    """the elements of `t` the golden records"""
    f = t.detach().reshape(-1)
    return f[::max(1, -(-f.numel() // SAMPLE_CAP))]


class Tape(object):
    """masks: None (free ReLU) or one bool tensor per BatchNorm layer in run order (forced); frozen: BatchNorm prefixes that use their
    running statistics.  A run appends every layer's pre-activation to .pre and its prefix to .names and puts the running statistics
    after the step into .running[prefix] = (mean, var)."""

    def __init__(self, masks=None, frozen=()):
        self.masks, self.frozen = masks, set(frozen)
        self.pre, self.names, self.running = [], [], {}

    def free_masks(self):
        return [a > 0 for a in self.pre]


def params_of(sd, dtype, grad=True):
    """state_dict -> {key: leaf tensor in `dtype`} (floating-point entries require a gradient unless they are running statistics)"""
    out = {}
    for k, v in sd.items():
        t = v.detach().clone()
        if torch.is_floating_point(t):
            t = t.to(dtype)
            if grad and not k.endswith(("running_mean", "running_var")):
                t.requires_grad_(True)
        out[k] = t
    return out


def bn_relu(z, p, prefix, tape):
    """BatchNorm2d(eps 1e-3, momentum 0.01) in train mode (or frozen) + ReLU on the pre-activation z (N, C, H, W)"""
    g, b = p[prefix + "weight"], p[prefix + "bias"]
    rm, rv = p[prefix + "running_mean"].to(z.dtype), p[prefix + "running_var"].to(z.dtype)
    if prefix in tape.frozen:
        mean, var = rm, rv
    else:
        mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
        n = z.numel() // z.shape[1]
        tape.running[prefix] = ((1 - MOMENTUM) * rm + MOMENTUM * mean.detach(), (1 - MOMENTUM) * rv + MOMENTUM * var.detach() * n / max(n - 1, 1))
    a = (z - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + EPS) * g[None, :, None, None] + b[None, :, None, None]
    i = len(tape.pre)
    tape.pre.append(a.detach())
    tape.names.append(prefix)
    return torch.relu(a) if tape.masks is None else a * tape.masks[i].to(a.dtype)


def conv_layer(x, p, wkey, bnprefix, tape, stride, pad):
    return bn_relu(F.conv2d(x, p[wkey], stride=stride, padding=pad), p, bnprefix, tape)


def deblock(x, p, prefix, tape, u):
    """prefix + '0.weight' / prefix + '1.': ConvTranspose2d(kernel = stride = u) for u >= 1, Conv2d(kernel = stride = 1 / u) below"""
    w = p[prefix + "0.weight"]
    if u >= 1:
        z = F.conv_transpose2d(x, w, stride=int(u))
    else:
        z = F.conv2d(x, w, stride=int(round(1.0 / u)))
    return bn_relu(z, p, prefix + "1.", tape)


def auto_encoder(x, p, prefix, tape):
    layers = len({k[len(prefix + "encoder."):].split(".")[0] for k in p if k.startswith(prefix + "encoder.")})
    for i in range(layers):
        q = "%sencoder.%d." % (prefix, i)
        x = conv_layer(x, p, q + "1.weight", q + "2.", tape, 2, 1)
        x = conv_layer(x, p, q + "4.weight", q + "5.", tape, 1, 1)
    for i in range(layers - 1, -1, -1):
        q = "%sdecoder.%d." % (prefix, i)
        x = deblock(x, p, q + "0.", tape, 2)
        x = conv_layer(x, p, q + "1.0.weight", q + "1.1.", tape, 1, 1)
    return x


def backbone(p, cfg, x, tape, record_len=None):
    """BaseBEVBackbone (record_len None) or AttBEVBackbone in train mode: (N, C, H, W) -> spatial_features_2d in x's dtype"""
    nums, strides = cfg.get("layer_nums", []), cfg.get("layer_strides", [])
    ups = cfg.get("upsample_strides", [])
    comp = int(cfg.get("compression", 0) or 0) if record_len is not None else 0
    outs = []
    for i in range(len(nums)):
        for k in range(nums[i] + 1):
            idx = 1 + 3 * k
            x = conv_layer(x, p, "blocks.%d.%d.weight" % (i, idx), "blocks.%d.%d." % (i, idx + 1), tape, strides[i] if k == 0 else 1, 1)
        y = x
        if record_len is not None:
            if comp - i > 0:
                x = auto_encoder(x, p, "compression_modules.%d." % i, tape)
            y = ar.att_fusion(x, list(record_len), x.dtype)
        outs.append(deblock(y, p, "deblocks.%d." % i, tape, ups[i]) if ups else y)
    y = torch.cat(outs, dim=1) if len(outs) > 1 else outs[0]
    if len(ups) > len(nums):
        y = deblock(y, p, "deblocks.%d." % len(nums), tape, ups[-1])
    return y


def run(sd, cfg, x, record_len=None, dtype=torch.float64, masks=None, frozen=(), weight=None, fn=backbone):
    """One forward + backward of sum(out * weight) -> dict(out, tape, grads {key: gradient}, dx); weight None: forward only"""
    p = params_of(sd, dtype)
    xi = x.detach().to(dtype).clone().requires_grad_(True)
    tape = Tape(masks, frozen)
    out = fn(p, cfg, xi, tape, record_len) if fn is backbone else fn(p, cfg, xi, tape)
    res = {"out": out.detach(), "tape": tape, "params": p}
    if weight is not None:
        (out * weight.to(dtype)).sum().backward()
        res["grads"] = {k: v.grad for k, v in p.items() if v.requires_grad and v.grad is not None}
        res["dx"] = xi.grad
    return res


def mask_disagreements(a, b):
    """elements at which two runs' ReLU masks differ, summed over the layers"""
    return int(sum(int(((u > 0) != (v > 0)).sum()) for u, v in zip(a.pre, b.pre)))


def loss_weight(shape, seed=0):
    """the procedural w of the scalar sum(out * w): uniform in +-1"""
    g = torch.Generator().manual_seed(4242 + seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) - 0.5) * 2.0


# ----------------------------------------------------------------------------------------------
# the transposed convolution's kernels per element in float64, with S = sum_k |a_k| |b_k| (K products each: N H W, Cin, s s Cout)
# x (N, H, W, Cin), dz (N, sH, sW, Cout), weight (Cin, Cout, s, s)
# ----------------------------------------------------------------------------------------------
EXTRA_WGRAD_CASE = (1, 32, 32, 1, 37, 53, 0, 32)          # 1961 pixels: several chunks and a ragged last one


def kernel_cases():
    import bev_backbone_ref as br
    return list(br.KERNEL_CASES) + [EXTRA_WGRAD_CASE]


def kernel_operands(case, seed=0):
    """-> (weight fp32, x fp32 (N, H, W, Cin), dz fp32 (N, sH, sW, Cout)), seeded"""
    import bev_backbone_ref as br
    s, cin, cout, n, h, w, _, _ = case
    weight, _, x = br.kernel_case(case, seed)
    g = torch.Generator().manual_seed(9000 + 1000 * seed + 17 * s + cin + cout + h)
    return weight, x, (torch.rand(n, s * h, s * w, cout, generator=g) - 0.5) * 2.0


def _taps(dz, s):
    n, sh, sw, co = dz.shape
    return dz.reshape(n, sh // s, s, sw // s, s, co)                  # [n, y, dy, x, dx, co]


def wgrad_f64(x, dz, s):
    xd, zd = x.double(), _taps(dz.double(), s)
    return torch.einsum("nyxc,nykxlo->cokl", xd, zd), torch.einsum("nyxc,nykxlo->cokl", xd.abs(), zd.abs())


def raw_f64(x, weight):
    s = weight.shape[2]
    n, h, w, _ = x.shape
    xd, wd = x.double(), weight.double()
    shape = (n, s * h, s * w, weight.shape[1])
    return torch.einsum("nyxc,cokl->nykxlo", xd, wd).reshape(shape), torch.einsum("nyxc,cokl->nykxlo", xd.abs(), wd.abs()).reshape(shape)


def dgrad_f64(dz, weight):
    s = weight.shape[2]
    zd, wd = _taps(dz.double(), s), weight.double()
    return torch.einsum("nykxlo,cokl->nyxc", zd, wd), torch.einsum("nykxlo,cokl->nyxc", zd.abs(), wd.abs())


def accumulation_gate(k, mag, ref):
    """the project's per-element bound for K fp32 products accumulated in any order: K 2^-23 S + 2^-23 |ref|"""
    return k * 2.0 ** -23 * mag + 2.0 ** -23 * ref.abs()


# ----------------------------------------------------------------------------------------------
# the agent attention's backward by autograd of att_backbone_ref.att_fusion
# ----------------------------------------------------------------------------------------------
def att_cases():
    """(name, x (N, HW, C) fp32, record_len): the forward's kernel cases, the empty sample, the module case, the large scores"""
    out = []
    for c, hw, rl in list(ar.KERNEL_CASES) + [ar.EMPTY_SAMPLE_CASE, ar.MODULE_CASE]:
        out.append((ar.case_key(c, hw, rl, torch.float32), ar.kernel_input(c, hw, rl), rl))
    c, hw, rl = ar.LARGE_SCORE_CASE
    out.append(("large_score", ar.large_score_input(), rl))
    return out


def att_dout(x, record_len, seed=0):
    g = torch.Generator().manual_seed(777 + seed + x.shape[1] + x.shape[2])
    return (torch.rand(len(record_len), x.shape[1], x.shape[2], generator=g) - 0.5) * 2.0


def att_fuse_bwd_ref(x, record_len, dout, dtype):
    """x (N, HW, C), dout (B, HW, C) -> dx (N, HW, C) in `dtype` by autograd of att_fusion; rows outside every sample are 0"""
    n, hw, c = x.shape
    xs = x.to(dtype).clone().requires_grad_(True)
    out = ar.att_fusion(xs.permute(0, 2, 1).reshape(n, c, hw, 1), list(record_len), dtype)          # (B, C, HW, 1)
    (out.reshape(len(record_len), c, hw).permute(0, 2, 1) * dout.to(dtype)).sum().backward()
    return xs.grad


def att_bwd_d32(x, record_len, dout):
    """max-norm deviation of fp32 autograd from float64 autograd, and max |dx_f64|"""
    ref = att_fuse_bwd_ref(x, record_len, dout, torch.float64)
    return float((att_fuse_bwd_ref(x, record_len, dout, torch.float32).double() - ref).abs().max()), float(ref.abs().max())


def load_att_bwd_d32():
    with open(ATT_BWD_D32_FILE) as f:
        return json.load(f)


def load_golden():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(z[k]) for k in z.files}


# ----------------------------------------------------------------------------------------------
# the module-level cases: name -> configuration, input shape, record_len; parameters by synth.fill_module_ at MODULE_SEEDS[name]
# ----------------------------------------------------------------------------------------------
def module_cases():
    cases = {"golden": (ar.GOLDEN_CFG, ar.INPUT_SHAPE, ar.RECORD_LEN), "compression": (ar.COMPRESSION_CFG, ar.COMPRESSION_SHAPE, ar.COMPRESSION_RECORD_LEN)}
    for name, cfg in ar.MIRROR_CFGS.items():
        cases[name] = (cfg, ar.INPUT_SHAPE, ar.RECORD_LEN)
    return cases


def module_case(name, att, seed=None):
    """-> (module in train() mode on the CPU with procedural parameters, cfg, x (N, C, H, W) fp32 of amplitude 2, record_len | None)"""
    import copy
    from cobevt_amd import host
    from cobevt_amd.synth import fill_module_, procedural_input
    cfg, shape, rl = module_cases()[name]
    cfg = copy.deepcopy(cfg)
    if not att:
        cfg.pop("compression", None)
    cls = host.AttBEVBackbone if att else host.BaseBEVBackbone
    module = fill_module_(cls(copy.deepcopy(cfg), shape[1]), MODULE_SEEDS[name] if seed is None else seed).train()
    x = procedural_input("gv26.spatial_features" if name != "compression" else "gv26.compression", shape, 0, -ar.AMPLITUDE, ar.AMPLITUDE)
    return module, cfg, x, (list(rl) if att else None)
