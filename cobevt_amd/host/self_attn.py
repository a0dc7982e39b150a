"""AttFusion — OpenCOOD's attentive fusion (opencood/models/fusion_modules/self_attn.py): per pixel, scaled-dot-product attention
over the agents of a sample with the agents' feature vectors as queries, keys and values, of which the ego's row is kept.  The
reference splits the batch by record_len on the host, permutes every sample to (HW, n, C), runs two bmm's and a softmax and permutes
back; here it is ONE launch over all samples on the channels-last maps (ops.att_fuse, csrc/att_fuse.hip) that reads record_len on
the device.  No parameters.  In train() mode on ROCm tensors the forwards take host/training.att_fusion (autograd.att_fuse: fp32, with
the backward kernel cobevt_att_fuse_bwd_nhwc); on CPU tensors a train()-mode forward raises."""
import torch

from .. import ops
from ..lib import CobevtHipError
from . import runtime as rt
from . import training
from .runtime import HipModule


def record_len_i32(record_len, device):
    """record_len as the kernels read it: contiguous int32 (B,) on `device` (no synchronisation for a device tensor)"""
    return torch.as_tensor(record_len).to(device=device, dtype=torch.int32).contiguous()


class AttFusion(HipModule):
    def __init__(self, feature_dim):
        super().__init__()
        if not ops.att_fuse_group_ok(int(feature_dim)):
            raise CobevtHipError("AttFusion: feature_dim=%r must be 8 times a power of two, at most 512 (ops.att_fuse)" % (feature_dim,))
        self.feature_dim = int(feature_dim)

    def forward_nhwc(self, x, record_len):
        """(N, H, W, C) in the compute dtype, record_len int32 (B,) on the device -> (B, H, W, C)"""
        if self.training and torch.is_tensor(x) and x.is_cuda:
            return training.att_fusion(self, x.permute(0, 3, 1, 2), record_len).permute(0, 2, 3, 1)
        self._require_inference(x)
        if x.shape[-1] != self.feature_dim:
            raise CobevtHipError("AttFusion: %d channels, built for %d" % (x.shape[-1], self.feature_dim))
        return ops.att_fuse(x, record_len)

    def forward(self, x, record_len):
        """the reference's contract: x (sum(record_len), C, H, W), record_len (B,) -> (B, C, H, W) in x's dtype (train(): fp32)"""
        if self.training and torch.is_tensor(x) and x.is_cuda:
            return training.att_fusion(self, x, record_len_i32(record_len, x.device))
        self._require_inference(x)
        y = self.forward_nhwc(rt.to_nhwc(x), record_len_i32(record_len, x.device))
        return rt.like_input(rt.nchw_view(y), x)
