"""Test-side torch restatement of BaseBEVBackbone (our own code, a pure function of a state_dict) and of one transposed-conv deblock,
the configurations the backbone tests share, and the float64 reference of the cobevt_deconv_nhwc kernel cases.

mirror(sd, cfg, x, dtype, bf16): every layer as conv / conv_transpose with the eval BatchNorm folded into the weights in float64 (as
the plans do), + shift, ReLU, in `dtype`; bf16=True rounds the folded weights, the input and every layer's output to bfloat16 - the
storage roundings of the bf16 compute mode, with exact accumulation in between."""
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gv25_base_bev_backbone.npz")
EPS = 1e-3

# the golden's configuration (tests/golden/make_golden_bev_backbone.py) and input
GOLDEN_CFG = dict(layer_nums=[1, 1, 1], layer_strides=[2, 2, 2], num_filters=[32, 32, 64], upsample_strides=[1, 2, 4],
                  num_upsample_filter=[32, 32, 32])
INPUT_CHANNELS = 32
INPUT_SHAPE = (2, 32, 16, 24)
# the reference's other branches, against the mirror: a strided-conv deblock (upsample stride < 1), the trailing deblock, no deblocks
MIRROR_CFGS = {
    "down_deblock": dict(layer_nums=[1, 1, 1], layer_strides=[1, 2, 2], num_filters=[32, 32, 64], upsample_strides=[0.5, 1, 2],
                         num_upsample_filter=[32, 32, 32]),
    "trailing_deblock": dict(layer_nums=[1, 1], layer_strides=[2, 2], num_filters=[32, 64], upsample_strides=[1, 2, 2],
                             num_upsample_filter=[32, 64, 0]),
    "no_deblocks": dict(layer_nums=[1, 1], layer_strides=[2, 1], num_filters=[32, 64]),
}
# the standard OpenCOOD PointPillar backbone on a 64-channel canvas
STANDARD_CFG = dict(layer_nums=[3, 5, 8], layer_strides=[2, 2, 2], num_filters=[64, 128, 256], upsample_strides=[1, 2, 4],
                    num_upsample_filter=[128, 128, 128])


def load_golden():
    z = np.load(GOLDEN)
    sd = {k[len("sd/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return sd, torch.from_numpy(z["input"]), torch.from_numpy(z["output"])


def fold(sd, prefix):
    """eval BatchNorm `prefix` -> (scale, shift) in float64"""
    s = sd[prefix + "weight"].double() / torch.sqrt(sd[prefix + "running_var"].double() + EPS)
    return s, sd[prefix + "bias"].double() - sd[prefix + "running_mean"].double() * s


def _rd(t, dtype, bf16):
    return t.to(torch.bfloat16).to(dtype) if bf16 else t.to(dtype)


def _layer(x, w, scale, shift, dtype, bf16, stride, pad=0, transposed=False):
    wf = w.double() * (scale[None, :, None, None] if transposed else scale[:, None, None, None])
    wf = _rd(wf, dtype, bf16)
    y = F.conv_transpose2d(x, wf, stride=stride) if transposed else F.conv2d(x, wf, stride=stride, padding=pad)
    y = torch.relu(y + shift.to(dtype)[None, :, None, None])
    return _rd(y, dtype, bf16)


def mirror(sd, cfg, x, dtype=torch.float64, bf16=False):
    """(N, C, H, W) -> spatial_features_2d (N, C', H', W') in `dtype`"""
    nums, strides = cfg.get("layer_nums", []), cfg.get("layer_strides", [])
    ups = cfg.get("upsample_strides", [])
    x = _rd(x.to(dtype), dtype, bf16)
    outs = []
    for i in range(len(nums)):
        for k in range(nums[i] + 1):
            idx = 1 + 3 * k
            x = _layer(x, sd["blocks.%d.%d.weight" % (i, idx)], *fold(sd, "blocks.%d.%d." % (i, idx + 1)), dtype, bf16,
                       strides[i] if k == 0 else 1, pad=1)
        if ups:
            w, (sc, sh) = sd["deblocks.%d.0.weight" % i], fold(sd, "deblocks.%d.1." % i)
            if ups[i] >= 1:
                outs.append(_layer(x, w, sc, sh, dtype, bf16, int(ups[i]), transposed=True))
            else:
                outs.append(_layer(x, w, sc, sh, dtype, bf16, int(round(1.0 / ups[i]))))
        else:
            outs.append(x)
    y = torch.cat(outs, dim=1) if len(outs) > 1 else outs[0]
    if len(ups) > len(nums):
        i = len(nums)
        y = _layer(y, sd["deblocks.%d.0.weight" % i], *fold(sd, "deblocks.%d.1." % i), dtype, bf16, int(ups[-1]), transposed=True)
    return y


def deviations(sd, cfg, x):
    """-> (d32, d16, max|out|): max-norm deviation of the fp32 mirror / the bf16-rounded mirror from the float64 mirror"""
    ref = mirror(sd, cfg, x, torch.float64)
    d32 = float((mirror(sd, cfg, x, torch.float32).double() - ref).abs().max())
    d16 = float((mirror(sd, cfg, x, torch.float64, bf16=True) - ref).abs().max())
    return d32, d16, float(ref.abs().max())


# ----------------------------------------------------------------------------------------------
# kernel cases: (s, Cin, Cout, N, H, W, c_off, ldc)
# ----------------------------------------------------------------------------------------------
KERNEL_CASES = [
    (1, 64, 128, 1, 5, 7, 0, 384),        # M = 35: a partial pixel tile
    (2, 128, 128, 2, 3, 5, 128, 384),     # a pixel tile that spans two images, middle slice
    (4, 256, 128, 1, 9, 8, 256, 384),     # M = 72: full + partial tile, 16 taps, last slice
    (2, 32, 32, 3, 1, 1, 0, 32),          # smallest K and N, M = 3
    (2, 96, 96, 1, 4, 4, 0, 96),          # K not a multiple of 64 elements, the trailing-deblock form
]


def kernel_case(case, seed=0):
    """-> (weight (Cin, Cout, s, s) fp32, bn dict of fp32 tensors, x (N, H, W, Cin) fp32), seeded"""
    s, cin, cout, n, h, w, _, _ = case
    g = torch.Generator().manual_seed(1000 * seed + 17 * s + cin + cout)
    weight = (torch.rand(cin, cout, s, s, generator=g) - 0.5) * 2.0 * (3.0 / cin) ** 0.5
    bn = {"weight": 0.8 + 0.4 * torch.rand(cout, generator=g), "bias": (torch.rand(cout, generator=g) - 0.5) * 0.6,
          "running_mean": (torch.rand(cout, generator=g) - 0.5) * 0.4, "running_var": 0.6 + 0.8 * torch.rand(cout, generator=g)}
    x = (torch.rand(n, h, w, cin, generator=g) - 0.5) * 2.0
    return weight, bn, x


def bn_module(bn):
    m = torch.nn.BatchNorm2d(bn["weight"].numel(), eps=EPS)
    m.load_state_dict({**bn, "num_batches_tracked": torch.tensor(0)})
    return m.eval()


def deconv_f64(weight, bn, x, store_dtype):
    """float64 evaluation from the operands the kernel gets: the BatchNorm folded in float64, then weights and input rounded to
    `store_dtype` by this function itself.  -> (ref (N, s*H, s*W, Cout) float64 after the ReLU, mag = sum_k |x_k| |w'_k| per element)"""
    s = weight.shape[2]
    sc, sh = fold({"b." + k: v for k, v in bn.items()}, "b.")
    wf = (weight.double() * sc[None, :, None, None]).to(torch.float32).to(store_dtype).double()
    xs = x.to(store_dtype).double()
    n, h, w, cin = xs.shape
    cout = wf.shape[1]
    # out[n, y, dy, x, dx, co] = sum_ci x[n, y, x, ci] w[ci, co, dy, dx]
    pre = torch.einsum("nyxc,cokl->nykxlo", xs, wf).reshape(n, s * h, s * w, cout) + sh.float().double()
    mag = torch.einsum("nyxc,cokl->nykxlo", xs.abs(), wf.abs()).reshape(n, s * h, s * w, cout)
    return torch.relu(pre), mag
