"""LidarBevPostprocessor — mirror of opv2v/opencood/data_utils/post_processor/lidar_bev_postprocessor.py, the anchor-free (PIXOR)
per-pixel formulation: `generate_label` rasterises rotated ground-truth boxes into a 7-channel label map, `post_process` decodes a
per-pixel cls / reg output into rotated 2-D boxes in the ego frame, runs the rotated NMS and the range mask.

Both run on the device.  Labels: ONE launch for a whole batch (ops.bev_labels, csrc/bev_labels.hip) where the reference loops over
the boxes and tests every pixel on the host.  Output: ONE operator call (ops.bev_post_process) - a decode launch in front of the
select / mask / greedy launches VoxelPostprocessor uses (csrc/detect_post.hip); the host reads the count once.
`post_process_device` is the same call without that read (fixed-capacity tensors plus a count: graph-capturable).

anchor_params: {'order': 'lwh', 'nms_thresh', 'target_args': {'score_threshold'}, 'geometry_param': {L1, L2, W1, W2, H1, H2, res,
input_shape, label_shape (lx, ly, 7), downsample_rate}}.  target_mean / target_std_dev are the reference's hard-coded values.

`generate_label` keeps the reference's signature (numpy in gives numpy out with one host read; tensors in give device tensors);
`generate_label_batch` takes the collated batch and returns device tensors without a synchronisation.  Not mirrored:
post_process_debug, visualize."""
import numpy as np
import torch

from .. import ops
from ..lib import CobevtHipError


class LidarBevPostprocessor(object):
    def __init__(self, anchor_params, train):
        self.params = anchor_params
        self.bbx_dict = {}
        self.train = train
        g = self.geometry_param = anchor_params["geometry_param"]
        missing = [k for k in ("L1", "L2", "W1", "W2", "res", "label_shape", "downsample_rate") if k not in g]
        if missing:
            raise CobevtHipError("LidarBevPostprocessor: geometry_param lacks %s" % ", ".join(missing))
        self.target_mean = np.array(ops.BEV_TARGET_MEAN)
        self.target_std_dev = np.array(ops.BEV_TARGET_STD_DEV)
        shape = tuple(int(v) for v in g["label_shape"])
        if len(shape) != 3 or shape[2] != 7 or shape[0] < 1 or shape[1] < 1:
            raise CobevtHipError("LidarBevPostprocessor: label_shape must be (lx, ly, 7), got %r" % (g["label_shape"],))
        self.label_shape = shape
        self._origin = (float(g["L1"]), float(g["W1"]))
        self._stats = {}                # (device, dtype) -> (mean, std) tensors for normalize_targets / denormalize_reg_map

    def generate_anchor_box(self):
        return None

    def _check_order(self):
        if self.params["order"] != "lwh":
            raise CobevtHipError("LidarBevPostprocessor: currently BEV only supports the 'lwh' bbx order, got %r" % (self.params["order"],))

    # ------------------------------------------------------------------------------------------ training targets
    def generate_label_batch(self, gt_box_center, mask, out=None):
        """gt_box_center (B, max_num, 7), mask (B, max_num) on the device (any float / integer type), max_num <= 128 ->
        {label_map (B, 7, lx, ly), bev_corners (B, max_num, 4, 2) fp32 (valid boxes first, zero rows behind), num_valid (B,) int32}"""
        self._check_order()
        gt, mask = torch.as_tensor(gt_box_center), torch.as_tensor(mask)
        if gt.dim() != 3 or gt.shape[2] != 7 or tuple(mask.shape) != tuple(gt.shape[:2]):
            raise CobevtHipError("LidarBevPostprocessor: gt_box_center must be (B, max_num, 7) with mask (B, max_num), got %s and %s"
                                 % (tuple(gt.shape), tuple(mask.shape)))
        ops._need_cuda(gt, mask)
        g = self.geometry_param
        label_map, corners, num_valid = ops.bev_labels(gt.to(torch.float32).contiguous(), mask.to(torch.float32).contiguous(),
                                                       self._origin, g["res"], g["downsample_rate"], self.label_shape,
                                                       self.target_mean, self.target_std_dev, out=out)
        return {"label_map": label_map, "bev_corners": corners, "num_valid": num_valid}

    def generate_label(self, **kwargs):
        """The reference's signature: gt_box_center (max_num, 7), mask (max_num,) -> {label_map (7, lx, ly) fp32, bev_corners (n, 4, 2)
        fp32 of the n valid boxes}.  numpy in gives numpy out (one host read); tensors in give device tensors (one host read of n)."""
        self._check_order()
        gt, mask = kwargs["gt_box_center"], kwargs["mask"]
        as_numpy = isinstance(gt, np.ndarray)
        if np.ndim(gt) != 2 or np.ndim(mask) != 1:
            raise CobevtHipError("LidarBevPostprocessor: gt_box_center must be (max_num, 7) with mask (max_num,), got %s and %s"
                                 % (tuple(np.shape(gt)), tuple(np.shape(mask))))
        if as_numpy:
            if not torch.cuda.is_available():
                raise CobevtHipError("LidarBevPostprocessor: generate_label runs on a ROCm device; there is no CPU fallback")
            dev = torch.device("cuda", torch.cuda.current_device())
            gt, mask = torch.from_numpy(np.ascontiguousarray(gt)).to(dev), torch.from_numpy(np.ascontiguousarray(mask)).to(dev)
        else:
            ops._need_cuda(gt)
            mask = torch.as_tensor(mask).to(gt.device)
        out = self.generate_label_batch(gt[None], mask[None])
        n = int(out["num_valid"][0].item())
        out = {"label_map": out["label_map"][0], "bev_corners": out["bev_corners"][0, :n]}
        if as_numpy:
            out = {k: v.cpu().numpy() for k, v in out.items()}
        return out

    def _stat_tensors(self, t):
        key = (t.device, t.dtype)
        if key not in self._stats:
            self._stats[key] = (torch.from_numpy(self.target_mean).to(device=t.device, dtype=t.dtype),
                                torch.from_numpy(self.target_std_dev).to(device=t.device, dtype=t.dtype))
        return self._stats[key]

    def normalize_targets(self, label_map):
        """label_map (..., 7) on the device -> channels 1 .. 6 as (v - target_mean) / target_std_dev (a new tensor; the label kernel
        already delivers normalised maps - this is the reference's helper for maps made elsewhere)"""
        ops._need_cuda(label_map)
        mean, std = self._stat_tensors(label_map)
        out = label_map.clone()
        out[..., 1:] = (label_map[..., 1:] - mean) / std
        return out

    def denormalize_reg_map(self, reg_map):
        """reg_map (..., 6) on the device -> reg_map * target_std_dev + target_mean"""
        ops._need_cuda(reg_map)
        mean, std = self._stat_tensors(reg_map)
        return reg_map * std + mean

    @staticmethod
    def collate_batch(label_batch_list):
        """[{label_map (7, lx, ly), bev_corners (n, 4, 2)}] per frame (arrays or tensors) -> {label_map (B, 7, lx, ly), bev_corners: the
        list of per-frame tensors}"""
        maps = [torch.as_tensor(x["label_map"]) for x in label_batch_list]
        return {"label_map": torch.stack(maps), "bev_corners": [torch.as_tensor(x["bev_corners"]) for x in label_batch_list]}

    # ------------------------------------------------------------------------------------------ detection output
    def _cavs(self, data_dict, output_dict):
        cavs = []
        for cav_id, cav_content in data_dict.items():
            if cav_id not in output_dict:
                raise CobevtHipError("LidarBevPostprocessor: cav %r has no model output" % (cav_id,))
            cls, reg = output_dict[cav_id]["cls"], output_dict[cav_id]["reg"]
            if cls.shape[0] != 1 or reg.shape[0] != 1:
                raise CobevtHipError("LidarBevPostprocessor: during validation / testing the batch size is 1 per cav, got %d for %r"
                                     % (reg.shape[0], cav_id))
            cavs.append((cls.float().contiguous(), reg.float().contiguous(), cav_content["transformation_matrix"]))
        return cavs

    def _post(self, cavs, out=None, workspace=None):
        g = self.geometry_param
        return ops.bev_post_process(cavs, self._origin, g["res"], g["downsample_rate"], self.params["target_args"]["score_threshold"],
                                    self.params["nms_thresh"], self.target_mean, self.target_std_dev, out=out, workspace=workspace)

    def post_process_device(self, data_dict, output_dict, out=None, workspace=None):
        """-> boxes (1000, 4, 2), scores (1000), index (1000) int32, count (1) int32 on the device, without a host read"""
        return self._post(self._cavs(data_dict, output_dict), out=out, workspace=workspace)

    def post_process(self, data_dict, output_dict):
        """-> (pred_box2d_tensor (K, 4, 2), scores (K,)) in the ego frame after NMS and the range mask, best score first; (None, None)
        when no pixel passes the score threshold; when pixels pass it but none survives NMS and the range mask both tensors are empty"""
        cavs = self._cavs(data_dict, output_dict)
        boxes, scores, _, count = self._post(cavs)
        k = int(count.item())                                  # the one host read
        if k == 0:
            # rare: tell "nothing above the threshold" (None, None) from "nothing survived" (empty tensors), as the reference does
            thr = self.params["target_args"]["score_threshold"]
            if not any(bool((torch.sigmoid(c[0]) > thr).any()) for c in cavs):
                return None, None
        return boxes[:k].clone(), scores[:k].clone()

    def reg_map_to_bbx_corners(self, reg_map, mask):
        """reg_map (lx, ly, 6) DE-NORMALISED and mask (lx, ly) bool on the device -> the corners (n, 4, 2) fp32 of the masked pixels in
        (i, j) order, in the map's own frame: ops.bev_post_process with an identity matrix, equal scores and an NMS threshold no IoU
        exceeds.  The values are rounded to fp32 on the way in; a masked pixel whose box is not finite or leaves GT_RANGE raises.
        One host read per 1000 masked pixels."""
        ops._need_cuda(reg_map, mask)
        if reg_map.dim() != 3 or reg_map.shape[2] != 6 or tuple(mask.shape) != tuple(reg_map.shape[:2]):
            raise CobevtHipError("LidarBevPostprocessor: only support shape of label_shape i.e. (*, *, 6) with a (*, *) mask, got %s and %s"
                                 % (tuple(reg_map.shape), tuple(mask.shape)))
        lx, ly = reg_map.shape[:2]
        n_pix = lx * ly
        sel = torch.nonzero(mask.reshape(-1)).reshape(-1)
        out = torch.empty((sel.numel(), 4, 2), device=reg_map.device, dtype=torch.float32)
        reg = reg_map.to(torch.float32).permute(2, 0, 1).contiguous()[None]
        eye = torch.eye(4, device=reg_map.device)
        g = self.geometry_param
        zeros, ones = np.zeros(6), np.ones(6)
        # every masked pixel becomes a candidate with the same score, so they come out in pixel order (equal scores: lower index
        # first); NMS threshold 2 suppresses nothing (iou <= 1).  The operator's capacity is 1000: the pixels go through in groups
        for s0 in range(0, sel.numel(), ops.DETECT_TOP):
            part = sel[s0:s0 + ops.DETECT_TOP]
            cls = torch.full((n_pix,), -100.0, device=reg_map.device)
            cls[part] = 4.0
            boxes, _, index, _ = ops.bev_post_process([(cls.reshape(1, 1, lx, ly), reg, eye)], self._origin, g["res"],
                                                      g["downsample_rate"], 0.5, 2.0, zeros, ones)
            out[s0:s0 + part.numel()] = boxes[:part.numel()]
            if not torch.equal(index[:part.numel()].long(), part):
                raise CobevtHipError("LidarBevPostprocessor: reg_map_to_bbx_corners: a masked pixel decodes to a non-finite or "
                                     "out-of-range box")
        return out
