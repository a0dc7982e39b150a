"""AutoEncoder — the optional feature compression of OpenCOOD's AttBEVBackbone (opencood/models/sub_modules/auto_encoder.py).
encoder[i]: ZeroPad2d(1) + 3 x 3 / stride-2 conv + BN + ReLU, then a 3 x 3 conv that halves the channels + BN + ReLU; decoder[i]:
ConvTranspose2d(kernel = stride = 2) that doubles them + BN + ReLU, then a 3 x 3 conv + BN + ReLU.  The forward runs the encoders
first to last and the decoders LAST TO FIRST, as the reference does.  The containers are the reference's, so the keys match
(encoder.0.1.weight, ..., decoder.0.0.0.weight, decoder.0.1.1.running_var, ...).

Convs run through ops.conv2d, the transposed convs through ops.deconv_into (cobevt_deconv_nhwc, c_off = 0).  That kernel writes 32
output channels per tile, so every decoder width feature_num / 2^i has to be a multiple of 32 (and its input a multiple of 8):
AutoEncoder(64, 1) and (128, 2) build, (32, 2) (a transposed conv 8 -> 16) raises CobevtHipError at construction.  In train() mode on
ROCm tensors the forwards take host/training.auto_encoder (fp32, differentiable); on CPU tensors a train()-mode forward raises."""
import torch
import torch.nn as nn

from .. import ops
from ..lib import CobevtHipError
from . import runtime as rt
from . import training
from .base_bev_backbone import _bn
from .runtime import HipModule


class AutoEncoder(HipModule):
    def __init__(self, feature_num, layer_num):
        super().__init__()
        self.feature_num, self.feature_stride = int(feature_num), 2
        self.encoder, self.decoder = nn.ModuleList(), nn.ModuleList()
        c = self.feature_num
        for _ in range(layer_num):
            self.encoder.append(nn.Sequential(
                nn.ZeroPad2d(1), nn.Conv2d(c, c, kernel_size=3, stride=2, padding=0, bias=False), _bn(c), nn.ReLU(),
                nn.Conv2d(c, c // 2, kernel_size=3, padding=1, bias=False), _bn(c // 2), nn.ReLU()))
            c //= 2
        c = self.feature_num
        for i in range(layer_num):
            if c % 32 != 0 or (c // 2) % 8 != 0:
                raise CobevtHipError("AutoEncoder(%d, %d): decoder %d is a transposed conv %d -> %d; the transposed-conv kernel needs a "
                                     "multiple of 32 output channels and a multiple of 8 input channels"
                                     % (self.feature_num, layer_num, i, c // 2, c))
            self.decoder.append(nn.Sequential(
                nn.Sequential(nn.ConvTranspose2d(c // 2, c, kernel_size=2, stride=2, bias=False), _bn(c), nn.ReLU()),
                nn.Sequential(nn.Conv2d(c, c, kernel_size=3, stride=1, bias=False, padding=1), _bn(c), nn.ReLU())))
            c //= 2

    def _conv_plan(self, name, conv, bn):
        def build(dt, dev):
            return ops.ConvPlan(conv.weight, None, bn=bn, stride=conv.stride[0], pad=1, act=1, dtype=dt, device=dev)
        return self._plan(name, rt.module_tensors(conv, bn), build)

    def _deconv_plan(self, name, conv, bn):
        def build(dt, dev):
            return ops.DeconvPlan(conv.weight, bn, conv.stride[0], dt, dev)
        return self._plan(name, rt.module_tensors(conv, bn), build)

    def out_size(self, h, w):
        """the H x W the forward returns for an h x w input (the same when both divide by 2^layers)"""
        for _ in self.encoder:
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        return h << len(self.decoder), w << len(self.decoder)

    def forward_nhwc(self, x):
        if self.training and torch.is_tensor(x) and x.is_cuda:
            return training.auto_encoder(self, x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        self._require_inference(x)
        for i, enc in enumerate(self.encoder):
            x = ops.conv2d(x, self._conv_plan("e%d.1" % i, enc[1], enc[2]))        # pad 1 = the ZeroPad2d(1) in front of pad 0
            x = ops.conv2d(x, self._conv_plan("e%d.4" % i, enc[4], enc[5]))
        for i in range(len(self.decoder) - 1, -1, -1):
            up, conv = self.decoder[i]
            n, h, w, _ = x.shape
            x = ops.deconv_into(x, self._deconv_plan("d%d.0" % i, up[0], up[1]),
                                torch.empty((n, 2 * h, 2 * w, up[0].out_channels), device=x.device, dtype=x.dtype), 0)
            x = ops.conv2d(x, self._conv_plan("d%d.1" % i, conv[0], conv[1]))
        return x

    def forward(self, x):
        if self.training and torch.is_tensor(x) and x.is_cuda:
            return training.auto_encoder(self, x)
        self._require_inference(x)
        return rt.like_input(rt.nchw_view(self.forward_nhwc(rt.to_nhwc(x))), x)
