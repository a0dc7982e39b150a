"""AttBEVBackbone — the 2-D backbone of OpenCOOD's attentive-fusion PointPillar (opencood/models/backbones/att_bev_backbone.py):
BaseBEVBackbone's blocks and deblocks, with the agents of a sample collapsed into the ego's map at every level.  Per level: the
block runs on all N = sum(record_len) maps; the optional AutoEncoder (model_cfg['compression'] = k: levels i < k get
AutoEncoder(num_filters[i], k - i)) compresses and restores them; AttFusion takes the N maps to B (ops.att_fuse, one launch); the
deblock upsamples the B fused maps into the level's channel slice of the one concatenated map (ops.deconv_into).  The UN-fused N maps
feed the next level, as in the reference.  `blocks` / `fuse_modules` / `deblocks` / `compression_modules` are the reference's
containers: 54 state_dict keys for three levels of one extra conv each, 126 with compression 2.

The level loop, the plans, the shape rules and the branches (upsample_strides < 1, a trailing deblock, no deblocks) are
BaseBEVBackbone's own code (this class only hooks in between a block and its deblock), and so are its two deliberate differences
from the reference (num_bev_features without deblocks; num_upsample_filter[-1] == 0 for a trailing deblock).

forward(data_dict) is the reference's contract: reads 'spatial_features' (N, C, H, W) and 'record_len' (B,), writes and returns
'spatial_features_2d' (B, num_bev_features, H', W') fp32 (the per-level 'spatial_features_%dx' entries are not produced).
forward_nhwc(x, record_len) takes NHWC in the compute dtype and an int32 device record_len; models use it.  No host synchronisation.
In train() mode on ROCm tensors both forwards take host/training.att_bev_backbone (fp32, differentiable: the agent attention has its
own backward kernel); on CPU tensors a train()-mode forward raises."""
import torch.nn as nn

from . import runtime as rt
from . import training
from .auto_encoder import AutoEncoder
from .base_bev_backbone import BaseBEVBackbone
from .self_attn import AttFusion, record_len_i32


class AttBEVBackbone(BaseBEVBackbone):
    def __init__(self, model_cfg, input_channels):
        super().__init__(model_cfg, input_channels)           # blocks, deblocks, num_bev_features and their checks
        num_filters = [block[1].out_channels for block in self.blocks]
        self.fuse_modules = nn.ModuleList(AttFusion(c) for c in num_filters)
        self.compress_layer = int(model_cfg.get("compression", 0) or 0)
        self.compress = self.compress_layer > 0
        if self.compress:
            self.compression_modules = nn.ModuleList(AutoEncoder(c, self.compress_layer - i) for i, c in enumerate(num_filters)
                                                     if self.compress_layer - i > 0)

    def _level_sizes(self, h, w):
        sizes = []
        for i, s in enumerate(self.layer_strides):
            h, w = (h - 1) // s + 1, (w - 1) // s + 1
            if self.compress and i < len(self.compression_modules):
                h, w = self.compression_modules[i].out_size(h, w)
            sizes.append((h, w))
        return sizes

    def forward_nhwc(self, x, record_len):
        """(N, H, W, C) in the compute dtype, record_len int32 (B,) on the device -> (B, H', W', num_bev_features)"""
        if self._trains(x):
            return training.att_bev_backbone(self, x.permute(0, 3, 1, 2), record_len).permute(0, 2, 3, 1)

        def fuse(i, x):
            if self.compress and i < len(self.compression_modules):
                x = self.compression_modules[i].forward_nhwc(x)
            return x, self.fuse_modules[i].forward_nhwc(x, record_len)
        if not len(self.blocks):
            self._require_inference(x)
            return x
        return self._forward_levels(x, record_len.shape[0], fuse)

    def forward(self, data_dict):
        x = data_dict["spatial_features"]
        if self._trains(x):
            data_dict["spatial_features_2d"] = training.att_bev_backbone(self, x, record_len_i32(data_dict["record_len"], x.device)).float()
            return data_dict
        self._require_inference(x)
        y = self.forward_nhwc(rt.to_nhwc(x), record_len_i32(data_dict["record_len"], x.device))
        data_dict["spatial_features_2d"] = rt.nchw_view(y).float()
        return data_dict
