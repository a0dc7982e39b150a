"""VoxelPostprocessor — mirror of opv2v/opencood/data_utils/post_processor/voxel_postprocessor.py: the anchor generator and what turns a
PointPillar head's two maps (psm, rm) into scored 3-D boxes, with the box helpers of opencood/utils/box_utils.py it calls.

`generate_anchor_box` is host numpy, as in the reference's data loader.  `post_process` runs on the tensors the model just produced:
ONE operator call (ops.detect_post_process, csrc/detect_post.hip) decodes every cav's boxes, applies the box filters, cuts at the
1000 best scores, runs the rotated NMS and the range mask on the device; the host reads the count once.  `post_process_device` is the
same call without that read (fixed-capacity tensors plus a count: graph-capturable).

Not mirrored: generate_label (training targets; it needs the Cython box_overlaps extension), collate_batch and visualize."""
import math

import numpy as np
import torch

from .. import ops
from ..lib import CobevtHipError


class VoxelPostprocessor(object):
    def __init__(self, anchor_params, train):
        self.params = anchor_params
        self.bbx_dict = {}
        self.train = train
        self.anchor_num = self.params["anchor_args"]["num"]

    def generate_anchor_box(self):
        """(H / stride, W / stride, anchor_num, 7) float64: centres on a linspace grid inset by one voxel, z = -1, the three sizes in
        the configured order ('hwl' or 'lhw') and one yaw per anchor"""
        a = self.params["anchor_args"]
        yaws = [math.radians(deg) for deg in a["r"]]
        if self.anchor_num != len(yaws):
            raise CobevtHipError("VoxelPostprocessor: anchor_args.num = %d but %d yaw angles" % (self.anchor_num, len(yaws)))
        stride = a["feature_stride"] if "feature_stride" in a else 2
        rng = a["cav_lidar_range"]
        xs = np.linspace(rng[0] + a["vw"], rng[3] - a["vw"], a["W"] // stride)
        ys = np.linspace(rng[1] + a["vh"], rng[4] - a["vh"], a["H"] // stride)
        cx, cy = np.meshgrid(xs, ys)
        cx = np.tile(cx[..., np.newaxis], self.anchor_num)
        cy = np.tile(cy[..., np.newaxis], self.anchor_num)
        cz = np.ones_like(cx) * -1.0
        l, w, h = np.ones_like(cx) * a["l"], np.ones_like(cx) * a["w"], np.ones_like(cx) * a["h"]
        yaw = np.ones_like(cx)
        for i in range(self.anchor_num):
            yaw[..., i] = yaws[i]
        if self.params["order"] == "hwl":
            return np.stack([cx, cy, cz, h, w, l, yaw], axis=-1)
        if self.params["order"] == "lhw":
            return np.stack([cx, cy, cz, l, h, w, yaw], axis=-1)
        raise CobevtHipError("VoxelPostprocessor: unknown bbx order %r" % (self.params["order"],))

    @staticmethod
    def delta_to_boxes3d(deltas, anchors):
        """deltas (N, 7A, H, W) fp32 on the device, anchors (H, W, A, 7) -> (N, H W A, 7)"""
        return ops.delta_to_boxes3d(deltas, anchors)

    def _cavs(self, data_dict, output_dict):
        cavs = []
        for cav_id, cav_content in data_dict.items():
            if cav_id not in output_dict:
                raise CobevtHipError("VoxelPostprocessor: cav %r has no model output" % (cav_id,))
            psm, rm = output_dict[cav_id]["psm"], output_dict[cav_id]["rm"]
            if psm.shape[0] != 1 or rm.shape[0] != 1:
                raise CobevtHipError("VoxelPostprocessor: during validation / testing the batch size is 1 per cav, got %d for %r"
                                     % (rm.shape[0], cav_id))
            cavs.append((psm.float().contiguous(), rm.float().contiguous(), cav_content["anchor_box"], cav_content["transformation_matrix"]))
        return cavs

    def post_process_device(self, data_dict, output_dict, out=None, workspace=None):
        """-> boxes (1000, 8, 3), scores (1000), index (1000) int32, count (1) int32 on the device, without a host read"""
        return ops.detect_post_process(self._cavs(data_dict, output_dict), self.params["target_args"]["score_threshold"],
                                       self.params["nms_thresh"], self.params["order"], out=out, workspace=workspace)

    def post_process(self, data_dict, output_dict):
        """-> (pred_box3d_tensor (K, 8, 3), scores (K,)) in the ego frame after NMS and the range mask, best score first; (None, None)
        when no candidate passes the score threshold (the reference returns that before its box filters; when candidates pass it but
        none survives the filters, NMS or the range mask, both tensors are empty)"""
        cavs = self._cavs(data_dict, output_dict)
        thr = self.params["target_args"]["score_threshold"]
        boxes, scores, _, count = ops.detect_post_process(cavs, thr, self.params["nms_thresh"], self.params["order"])
        k = int(count.item())                                  # the one host read
        if k == 0:
            # rare: tell "nothing above the threshold" (None, None) from "nothing survived" (empty tensors), as the reference does;
            # sigmoid(x) > t as the kernel compares it
            above = any(bool((torch.sigmoid(c[0]) > thr).any()) for c in cavs)
            if not above:
                return None, None
        return boxes[:k].clone(), scores[:k].clone()
