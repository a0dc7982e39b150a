"""VoxelPostprocessor — mirror of opv2v/opencood/data_utils/post_processor/voxel_postprocessor.py: the anchor generator and what turns a
PointPillar head's two maps (psm, rm) into scored 3-D boxes, with the box helpers of opencood/utils/box_utils.py it calls.

`generate_anchor_box` is host numpy, as in the reference's data loader.  `post_process` runs on the tensors the model just produced:
ONE operator call (ops.detect_post_process, csrc/detect_post.hip) decodes every cav's boxes, applies the box filters, cuts at the
1000 best scores, runs the rotated NMS and the range mask on the device; the host reads the count once.  `post_process_device` is the
same call without that read (fixed-capacity tensors plus a count: graph-capturable).

`generate_label` / `generate_label_batch` build the training targets on the device (ops.boxes_standup + ops.detect_targets,
csrc/detect_targets.hip): the reference's anchor-to-ground-truth assignment with the `bbox_overlaps` of its Cython extension restated
as a kernel, bit-identical to that compiled C given the same standup boxes.  `generate_label` keeps the reference's
signature and types (numpy in, numpy float64 out, one host read); `generate_label_batch` takes the collated batch and returns device
tensors without a synchronisation, `num_pos` included for PointPillarLoss.  `collate_batch` is a plain mirror.

Two things to know about the targets:
  * mask.  IoU column k is the k-th VALID box (mask == 1) and the targets are taken from that same box.  The reference indexes the
    UNFILTERED gt array with the filtered index: the same thing for the prefix masks its datasets produce, and wrong otherwise.
  * ties.  With the `+1` convention a rotated gt's hull contains several anchors at exactly the same IoU, so the reference's
    "highest anchor" is decided by fp32 rounding noise in its torch-CPU corner arithmetic; the device's standup boxes can differ
    from those in the last ulp, and on such exact or near ties the chosen anchor may differ.  The rule here: the lowest anchor index
    of maximal IoU (np.argmax), applied to the device's own fp32 IoU.

Not mirrored: visualize."""
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
        self._anchor_cache = None       # (key, the anchor array, anchors fp32 on the device, their standup boxes)

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

    # ------------------------------------------------------------------------------------------ training targets
    def _device_anchors(self, anchors, dev):
        """(anchors (H, W, A, 7) fp32, standup boxes (H W A, 4)) on `dev`, cached per anchor array (identity and shape: the data
        loader generates the anchor box once and hands the same array to every call)"""
        key = (id(anchors), tuple(anchors.shape), str(dev))
        c = self._anchor_cache
        if c is not None and c[0] == key and c[1] is anchors:
            return c[2], c[3]
        a = torch.as_tensor(anchors)
        if a.dim() != 4 or a.shape[3] != 7 or a.shape[2] != self.anchor_num or not a.is_floating_point():
            raise CobevtHipError("VoxelPostprocessor: anchors must be floating point (H, W, %d, 7), got %s %s"
                                 % (self.anchor_num, a.dtype, tuple(a.shape)))
        a = a.to(device=dev, dtype=torch.float32).contiguous()
        st = ops.boxes_standup(a.reshape(-1, 7))
        self._anchor_cache = (key, anchors, a, st)
        return a, st

    def generate_label_batch(self, gt_box_center, mask, anchors):
        """gt_box_center (B, max_num, 7), mask (B, max_num), anchors (H, W, A, 7) -> {targets (B, H, W, 7A), pos_equal_one
        (B, H, W, A), neg_equal_one (B, H, W, A) fp32, num_pos (B,) int32} on the device: what collate_batch would deliver, without a
        host synchronisation.  gt_box_center and mask are device tensors (any float / integer type); max_num <= 128."""
        if self.params["order"] != "hwl":
            raise CobevtHipError("VoxelPostprocessor: generate_label supports the 'hwl' bbx order only, got %r" % (self.params["order"],))
        gt, mask = torch.as_tensor(gt_box_center), torch.as_tensor(mask)
        if gt.dim() != 3 or gt.shape[2] != 7 or tuple(mask.shape) != tuple(gt.shape[:2]):
            raise CobevtHipError("VoxelPostprocessor: gt_box_center must be (B, max_num, 7) with mask (B, max_num), got %s and %s"
                                 % (tuple(gt.shape), tuple(mask.shape)))
        if gt.shape[1] > ops.DETECT_MAX_GT:
            raise CobevtHipError("VoxelPostprocessor: at most %d ground-truth slots per sample are supported, got %d"
                                 % (ops.DETECT_MAX_GT, gt.shape[1]))
        ops._need_cuda(gt, mask)
        anc, anc_standup = self._device_anchors(anchors, gt.device)
        gt = gt.to(torch.float32).contiguous()
        mask = mask.to(torch.float32).contiguous()
        gt_standup = ops.boxes_standup(gt.reshape(-1, 7)).reshape(gt.shape[0], gt.shape[1], 4)
        t = self.params["target_args"]
        pos, neg, targets, num_pos = ops.detect_targets(anc, anc_standup, gt, gt_standup, mask, t["pos_threshold"], t["neg_threshold"])
        return {"targets": targets, "pos_equal_one": pos, "neg_equal_one": neg, "num_pos": num_pos}

    def generate_label(self, **kwargs):
        """The reference's signature: gt_box_center (max_num, 7), anchors (H, W, A, 7), mask (max_num,) -> {pos_equal_one (H, W, A),
        neg_equal_one (H, W, A), targets (H, W, 7A)}.  numpy in gives numpy float64 out (it drops into the reference's dataset code;
        one host read); tensors in give device tensors.  The kernel works in fp32: the targets carry fp32 precision."""
        if self.params["order"] != "hwl":
            raise CobevtHipError("VoxelPostprocessor: generate_label supports the 'hwl' bbx order only, got %r" % (self.params["order"],))
        gt, anchors, mask = kwargs["gt_box_center"], kwargs["anchors"], kwargs["mask"]
        as_numpy = isinstance(gt, np.ndarray)
        if np.ndim(gt) != 2 or np.ndim(mask) != 1:
            raise CobevtHipError("VoxelPostprocessor: gt_box_center must be (max_num, 7) with mask (max_num,), got %s and %s"
                                 % (tuple(np.shape(gt)), tuple(np.shape(mask))))
        if as_numpy:
            if not torch.cuda.is_available():
                raise CobevtHipError("VoxelPostprocessor: generate_label runs on a ROCm device; there is no CPU fallback")
            dev = torch.device("cuda", torch.cuda.current_device())
            gt, mask = torch.from_numpy(np.ascontiguousarray(gt)).to(dev), torch.from_numpy(np.ascontiguousarray(mask)).to(dev)
        else:
            ops._need_cuda(gt)
            mask = torch.as_tensor(mask).to(gt.device)
        out = self.generate_label_batch(gt[None], mask[None], anchors)
        out = {k: out[k][0] for k in ("pos_equal_one", "neg_equal_one", "targets")}
        if as_numpy:
            out = {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}
        return out

    @staticmethod
    def collate_batch(label_batch_list):
        """[{pos_equal_one, neg_equal_one, targets}] per frame (arrays or tensors) -> the three stacked as tensors"""
        def stack(key):
            items = [d[key] for d in label_batch_list]
            if all(isinstance(i, np.ndarray) for i in items):
                return torch.from_numpy(np.array(items))
            return torch.stack([torch.as_tensor(i) for i in items])
        return {"targets": stack("targets"), "pos_equal_one": stack("pos_equal_one"), "neg_equal_one": stack("neg_equal_one")}
