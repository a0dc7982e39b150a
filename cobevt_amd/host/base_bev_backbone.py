"""BaseBEVBackbone — the 2-D backbone of OpenCOOD's PointPillar models between the scattered BEV canvas and the heads
(opencood/models/backbones/base_bev_backbone.py): per level ZeroPad2d(1) + 3 x 3 / stride-s conv + layer_nums[i] 3 x 3 convs, each with
BatchNorm(eps 1e-3) + ReLU; per level a "deblock" ConvTranspose2d(kernel = stride = u) + BN + ReLU whose outputs are concatenated on
channels into spatial_features_2d.  `blocks` / `deblocks` are ModuleLists of nn.Sequentials at the reference's indices, so the
state_dict has the reference's keys and shapes (blocks.0.1.weight, blocks.0.2.running_mean, ..., deblocks.2.0.weight, ...).

model_cfg: layer_nums, layer_strides, num_filters; optionally upsample_strides, num_upsample_filter.  The reference's branches:
  * upsample_strides[i] >= 1: one cobevt_deconv_nhwc launch per level (ops.deconv_into) that writes its channel slice of the ONE
    preallocated concatenated map - no pixel-shuffle copy, no BN / ReLU pass, no torch.cat.  A stride of 1 is the same kernel.
  * upsample_strides[i] < 1: Conv2d(kernel = stride = round(1 / u)) through ops.conv2d into a temporary, copied into its slice.
  * one more entry in upsample_strides than levels: a trailing deblock over the concatenated map (the same kernel, c_off = 0).
  * no upsample_strides: the levels' own outputs are concatenated (they must share one H x W, as for the reference's torch.cat).
The blocks run through ops.conv2d (the stride-s conv with pad 1 IS ZeroPad2d(1) + pad 0).  Levels whose deblock outputs do not share
one H x W raise CobevtHipError before anything is launched.

forward(data_dict) is the reference's contract: reads data_dict['spatial_features'] (N, C, H, W), writes and returns
data_dict['spatial_features_2d'] (N, sum(num_upsample_filter), H', W') fp32 (the reference's per-level 'spatial_features_%dx' entries
are not produced).  forward_nhwc(x) takes and returns NHWC tensors in the compute dtype; models use it.  No host synchronisation:
the forward can be captured in a HIP graph.

In train() mode on ROCm tensors both forwards take the differentiable graph of host/training.base_bev_backbone: every conv through
autograd.conv2d, every BatchNorm2d with batch statistics (or, with its own .training flag off, its frozen running statistics), every
transposed conv through autograd.deconv; the outputs are fp32.  On CPU tensors a train()-mode forward raises."""
import torch
import torch.nn as nn

from .. import ops
from ..lib import CobevtHipError
from . import runtime as rt
from . import training
from .runtime import HipModule


def _bn(c):
    return nn.BatchNorm2d(c, eps=1e-3, momentum=0.01)


class BaseBEVBackbone(HipModule):
    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        layer_nums = list(model_cfg.get("layer_nums", []))
        layer_strides = list(model_cfg.get("layer_strides", [])) if layer_nums else []
        num_filters = list(model_cfg.get("num_filters", [])) if layer_nums else []
        if not len(layer_nums) == len(layer_strides) == len(num_filters):
            raise CobevtHipError("%s: layer_nums, layer_strides and num_filters must have one entry per level" % type(self).__name__)
        up_strides = list(model_cfg.get("upsample_strides", []))
        up_filters = list(model_cfg.get("num_upsample_filter", [])) if up_strides else []
        if len(up_strides) != len(up_filters):
            raise CobevtHipError("%s: upsample_strides and num_upsample_filter must have the same length" % type(self).__name__)
        levels = len(layer_nums)
        if up_strides and len(up_strides) not in (levels, levels + 1):
            raise CobevtHipError("%s: %d upsample_strides for %d levels (one per level, or one more for a trailing deblock)"
                                 % (type(self).__name__, len(up_strides), levels))
        self.layer_strides, self.upsample_strides = [int(s) for s in layer_strides], up_strides
        c_in = [input_channels] + num_filters[:-1]
        self.blocks, self.deblocks = nn.ModuleList(), nn.ModuleList()
        c_off = 0
        for i in range(levels):
            layers = [nn.ZeroPad2d(1), nn.Conv2d(c_in[i], num_filters[i], 3, stride=self.layer_strides[i], padding=0, bias=False),
                      _bn(num_filters[i]), nn.ReLU()]
            for _ in range(layer_nums[i]):
                layers += [nn.Conv2d(num_filters[i], num_filters[i], 3, padding=1, bias=False), _bn(num_filters[i]), nn.ReLU()]
            self.blocks.append(nn.Sequential(*layers))
            if up_strides:
                u, c = up_strides[i], up_filters[i]
                if u >= 1:
                    self._check_deblock(i, u, c, c_off)
                    conv = nn.ConvTranspose2d(num_filters[i], c, int(u), stride=int(u), bias=False)
                else:
                    r = int(round(1.0 / u))
                    conv = nn.Conv2d(num_filters[i], c, r, stride=r, bias=False)
                self.deblocks.append(nn.Sequential(conv, _bn(c), nn.ReLU()))
                c_off += c
        # the reference sizes the trailing deblock sum(num_upsample_filter) -> the same, over ALL entries: its own entry has to be 0
        # for that to be the width of the concatenated map it reads (the reference's forward throws otherwise)
        total = sum(up_filters)
        if len(up_strides) > levels:
            if total != sum(up_filters[:levels]):
                raise CobevtHipError("%s: the trailing deblock is sum(num_upsample_filter) = %d channels wide, the map it reads "
                                     "%d: num_upsample_filter[-1] must be 0" % (type(self).__name__, total, sum(up_filters[:levels])))
            self._check_deblock(levels, up_strides[-1], total, 0)
            self.deblocks.append(nn.Sequential(nn.ConvTranspose2d(total, total, int(up_strides[-1]), stride=int(up_strides[-1]), bias=False),
                                               _bn(total), nn.ReLU()))
        # (without deblocks the reference reports sum([]) = 0; here it is the width of the map the forward returns)
        self.num_bev_features = total if up_strides else sum(num_filters)

    @classmethod
    def _check_deblock(cls, i, u, c, c_off):
        if int(u) != u or not 1 <= int(u) <= ops.DECONV_MAX_STRIDE:
            raise CobevtHipError("%s: upsample_strides[%d] = %r: the transposed-conv kernel takes integer strides 1 .. %d"
                                 % (cls.__name__, i, u, ops.DECONV_MAX_STRIDE))
        if c % 32 != 0 or c_off % 8 != 0:
            raise CobevtHipError("%s: deblock %d writes %d channels at channel %d of the concatenated map; the transposed-conv "
                                 "kernel needs a multiple of 32 channels at a multiple of 8" % (cls.__name__, i, c, c_off))

    # ---- plans
    def _conv_plan(self, name, conv, bn, pad):
        def build(dt, dev):
            return ops.ConvPlan(conv.weight, None, bn=bn, stride=conv.stride[0], pad=pad, act=1, dtype=dt, device=dev)
        return self._plan(name, rt.module_tensors(conv, bn), build)

    def _deconv_plan(self, name, conv, bn):
        def build(dt, dev):
            return ops.DeconvPlan(conv.weight, bn, conv.stride[0], dt, dev)
        return self._plan(name, rt.module_tensors(conv, bn), build)

    # ---- shapes
    def _level_sizes(self, h, w):
        sizes = []
        for s in self.layer_strides:
            h, w = (h - 1) // s + 1, (w - 1) // s + 1           # 3 x 3, stride s, one zero row / column on every side
            sizes.append((h, w))
        return sizes

    def _up_sizes(self, sizes):
        if not len(self.deblocks):
            return sizes
        out = []
        for (h, w), u in zip(sizes, self.upsample_strides):
            if u >= 1:
                out.append((h * int(u), w * int(u)))
            else:
                r = int(round(1.0 / u))
                out.append(((h - r) // r + 1, (w - r) // r + 1))
        return out

    def _concat_size(self, h, w):
        """the one H x W the levels' outputs share for an h x w input; raises when they do not (before anything is launched)"""
        ups = self._up_sizes(self._level_sizes(h, w))
        if any(hw != ups[0] for hw in ups) or min(ups[0]) < 1:
            raise CobevtHipError("%s: the levels' outputs must share one H x W to be concatenated; a %d x %d input gives %s"
                                 % (type(self).__name__, h, w, ", ".join("%d x %d" % hw for hw in ups)))
        return ups[0]

    def _trains(self, x):
        """a train()-mode forward on a ROCm tensor takes the differentiable graph; anything else the inference path (which refuses train())"""
        return self.training and torch.is_tensor(x) and x.is_cuda

    def forward_nhwc(self, x):
        """(N, H, W, C) in the compute dtype -> (N, H', W', num_bev_features) in the compute dtype (train(): fp32, differentiable)"""
        if self._trains(x):
            return training.base_bev_backbone(self, x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        return self._forward_levels(x, x.shape[0])

    def _forward_levels(self, x, n_out, after_block=None):
        """the levels' loop.  after_block(i, x) -> (the map the next level reads, the n_out maps the level's deblock reads) is the
        subclasses' hook between a block and its deblock (AttBEVBackbone: compression, agent fusion); without it both are x"""
        self._require_inference(x)
        _, h, w, _ = x.shape
        levels = len(self.blocks)
        if levels == 0:
            return x
        up = self._concat_size(h, w)
        widths = [(self.deblocks[i][0] if len(self.deblocks) else self.blocks[i][1]).out_channels for i in range(levels)]
        cat = None
        if levels > 1 or len(self.deblocks):
            cat = torch.empty((n_out, up[0], up[1], sum(widths)), device=x.device, dtype=x.dtype)
        c_off = 0
        for i, block in enumerate(self.blocks):
            x = ops.conv2d(x, self._conv_plan("b%d.0" % i, block[1], block[2], 1))
            for k in range(4, len(block), 3):
                x = ops.conv2d(x, self._conv_plan("b%d.%d" % (i, k), block[k], block[k + 1], 1))
            y = x
            if after_block is not None:
                x, y = after_block(i, x)
            if len(self.deblocks):
                conv, bn = self.deblocks[i][0], self.deblocks[i][1]
                if isinstance(conv, nn.ConvTranspose2d):
                    ops.deconv_into(y, self._deconv_plan("d%d" % i, conv, bn), cat, c_off)
                else:
                    cat[..., c_off:c_off + widths[i]] = ops.conv2d(y, self._conv_plan("d%d" % i, conv, bn, 0))
            elif cat is not None:
                cat[..., c_off:c_off + widths[i]] = y
            c_off += widths[i]
        y = y if cat is None else cat
        if len(self.deblocks) > levels:
            conv, bn = self.deblocks[-1][0], self.deblocks[-1][1]
            s = conv.stride[0]
            y = ops.deconv_into(y, self._deconv_plan("d%d" % levels, conv, bn),
                                torch.empty((n_out, s * y.shape[1], s * y.shape[2], conv.out_channels), device=y.device, dtype=y.dtype), 0)
        return y

    def forward(self, data_dict):
        x = data_dict["spatial_features"]
        if self._trains(x):
            data_dict["spatial_features_2d"] = training.base_bev_backbone(self, x).float()
            return data_dict
        self._require_inference(x)
        data_dict["spatial_features_2d"] = rt.nchw_view(self.forward_nhwc(rt.to_nhwc(x))).float()
        return data_dict
