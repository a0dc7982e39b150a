"""PointPillarLoss — the detection loss behind a PointPillar head, after upstream OpenCOOD's opencood/loss/point_pillar_loss.py (the
reference tree of this package ships no detection loss, so the contract is written out here and in include/cobevt_hip.h):

    p_b        = max(1, positives of sample b),  t = pos_equal_one (neg_equal_one is not read: every non-positive anchor is a negative)
    conf_loss  = cls_weight / B * sum [0.25 t + 0.75 (1 - t)] pt^2 bce / p_b      (sigmoid focal loss, alpha 0.25, gamma 2)
    reg_loss   = reg / B * sum over positives of smooth_l1(d_k, beta = 1 / 9) / p_b, the yaw component as sin(rm - tgt) in its
                 sin / cos product form; a NaN target counts as d = 0
    total_loss = conf_loss + reg_loss

Same constructor argument (`args` with `cls_weight` and `reg`), same `forward(output_dict, target_dict)` -> total loss and
`loss_dict` entries.  One operator call (ops.pointpillar_loss, csrc/detect_targets.hip) computes the three scalars and, when psm or
rm requires grad, both gradients in the same launch; it sits behind a torch.autograd.Function, so `.backward()` hands the kernel's
gradients to the head maps.  `target_dict` is what VoxelPostprocessor.generate_label_batch returns (its `num_pos` saves the count
launch) or the reference's collate_batch dict (float64 labels are converted).  There is no CPU fallback."""
import torch

from .. import ops
from ..lib import CobevtHipError


class PointPillarLossFn(torch.autograd.Function):
    """(psm, rm, pos_equal_one, targets, num_pos | None, cls_weight, reg, want) -> (3,) [total, conf_loss, reg_loss]; want: have the
    launch write the gradients too (decided by the caller: grad mode is off inside forward)"""

    @staticmethod
    def forward(ctx, psm, rm, pos_equal_one, targets, num_pos, cls_weight, reg, want):
        loss, dpsm, drm = ops.pointpillar_loss(psm, rm, pos_equal_one, targets, cls_weight, reg, num_pos=num_pos, want_grad=want)
        if want:
            ctx.save_for_backward(dpsm, drm)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        dpsm, drm = ctx.saved_tensors
        # total = conf_loss + reg_loss is the one differentiable output: its cotangent scales the stored d total / d map
        g = dloss[0]
        return dpsm * g, drm * g, None, None, None, None, None, None


class PointPillarLoss(object):
    def __init__(self, args):
        self.cls_weight = args["cls_weight"]
        self.reg_coe = args["reg"]
        self.alpha = 0.25
        self.gamma = 2.0
        self.loss_dict = {}

    def __call__(self, output_dict, target_dict):
        return self.forward(output_dict, target_dict)

    @staticmethod
    def _label(t, dev, what):
        t = torch.as_tensor(t)
        if not t.is_cuda:
            raise CobevtHipError("PointPillarLoss: %s must be on a ROCm device (got a CPU tensor); there is no CPU fallback" % what)
        return t.to(device=dev, dtype=torch.float32).contiguous()

    def forward(self, output_dict, target_dict):
        """output_dict: psm (B, A, H, W), rm (B, 7A, H, W); target_dict: pos_equal_one (B, H, W, A), targets (B, H, W, 7A) and
        optionally num_pos (B,) int32"""
        psm, rm = output_dict["psm"], output_dict["rm"]
        ops._need_cuda(psm, rm)
        # explicit (differentiable) casts: a bf16 head output reaches the fp32 kernel as fp32
        psm, rm = psm.float().contiguous(), rm.float().contiguous()
        pos = self._label(target_dict["pos_equal_one"], psm.device, "pos_equal_one")
        targets = self._label(target_dict["targets"], psm.device, "targets")
        num_pos = target_dict.get("num_pos")
        want = (psm.requires_grad or rm.requires_grad) and torch.is_grad_enabled()       # the validation pass stores no gradient
        loss = PointPillarLossFn.apply(psm, rm, pos, targets, num_pos, self.cls_weight, self.reg_coe, want)
        total = loss[0]
        # values for logging: detached, so that the record of the last step does not keep that step's autograd graph alive
        d = loss.detach()
        self.loss_dict.update({"total_loss": d[0], "reg_loss": d[2], "conf_loss": d[1]})
        return total
