"""Detection scores — mirror of opv2v/opencood/utils/eval_utils.py: voc_ap, caluclate_tp_fp (the reference's spelling),
calculate_ap, eval_final_results.

The reference builds one shapely polygon per box and intersects each detection with every remaining ground-truth box in a Python loop;
here the whole detection x ground-truth IoU matrix comes from ONE launch (ops.rotated_iou, the fp64 quad clip of csrc/detect_post.hip)
and only the greedy matching - a detection takes the remaining ground-truth box it overlaps most, which then leaves the list - runs on
the host, on that matrix.  The tp / fp lists and the AP arithmetic are the reference's plain Python."""
import os

import numpy as np
import torch

from .. import ops
from ..lib import CobevtHipError


def voc_ap(rec, prec):
    """VOC 2010 average precision: the precision envelope (running maximum from the right) summed over the recall steps;
    -> (ap, mrec, mpre); like the reference it extends the two lists it is given in place"""
    rec.insert(0, 0.0)
    rec.append(1.0)
    prec.insert(0, 0.0)
    prec.append(0.0)
    mrec, mpre = rec[:], prec[:]
    for i in reversed(range(len(mpre) - 1)):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = 0.0
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            ap += (mrec[i] - mrec[i - 1]) * mpre[i]
    return ap, mrec, mpre


def caluclate_tp_fp(det_boxes, det_score, gt_boxes, result_stat, iou_thresh):
    """Appends this frame's true / false positive flags (detections in descending score order) and its ground-truth count to
    result_stat[iou_thresh].  det_boxes (N, 8, 3) or (N, 4, 2) and det_score (N) on the device, or None for a frame without
    detections; gt_boxes (M, 8, 3) or (M, 4, 2), tensor or array."""
    fp, tp = [], []
    gt = gt_boxes.shape[0]
    if det_boxes is not None:
        if not torch.is_tensor(det_boxes) or not det_boxes.is_cuda:
            raise CobevtHipError("caluclate_tp_fp: det_boxes must be a tensor on a ROCm device (the IoU matrix is a HIP kernel)")
        n = det_boxes.shape[0]
        gt_dev = torch.as_tensor(gt_boxes).to(det_boxes.device)
        # compute_iou returns float32 arrays: the threshold comparison and the arg-max run on the rounded values
        iou = ops.rotated_iou(det_boxes, gt_dev).cpu().numpy().astype(np.float32) if n and gt else np.zeros((n, gt), np.float32)
        order = np.argsort(-torch.as_tensor(det_score).detach().cpu().numpy())
        remaining = list(range(gt))
        for d in order:
            row = iou[d, remaining]
            if len(remaining) == 0 or np.max(row) < iou_thresh:
                fp.append(1)
                tp.append(0)
                continue
            fp.append(0)
            tp.append(1)
            remaining.pop(int(np.argmax(row)))
    result_stat[iou_thresh]["fp"] += fp
    result_stat[iou_thresh]["tp"] += tp
    result_stat[iou_thresh]["gt"] += gt


def calculate_ap(result_stat, iou):
    """-> (ap, mrec, mprec) from the accumulated flags of result_stat[iou]; like the reference it turns the stored fp / tp lists into
    their running sums in place"""
    stat = result_stat[iou]
    fp, tp = stat["fp"], stat["tp"]
    if len(fp) != len(tp):
        raise CobevtHipError("calculate_ap: %d fp flags and %d tp flags" % (len(fp), len(tp)))
    gt_total = stat["gt"]
    for flags in (fp, tp):
        running = 0
        for idx, val in enumerate(flags):
            flags[idx] += running
            running += val
    rec = [float(t) / gt_total for t in tp]
    prec = [float(t) / (f + t) for f, t in zip(fp, tp)]
    return voc_ap(rec[:], prec[:])


def eval_final_results(result_stat, save_path=None):
    """-> {'ap30', 'ap_50', 'ap_70', 'mpre_50', 'mrec_50', 'mpre_70', 'mrec_70'} (the reference's keys); written to
    save_path/eval.yaml only when a path is given"""
    ap_30, _, _ = calculate_ap(result_stat, 0.30)
    ap_50, mrec_50, mpre_50 = calculate_ap(result_stat, 0.50)
    ap_70, mrec_70, mpre_70 = calculate_ap(result_stat, 0.70)
    dump = {"ap30": ap_30, "ap_50": ap_50, "ap_70": ap_70, "mpre_50": mpre_50, "mrec_50": mrec_50, "mpre_70": mpre_70,
            "mrec_70": mrec_70}
    if save_path is not None:
        import yaml
        with open(os.path.join(save_path, "eval.yaml"), "w") as f:
            yaml.dump(dump, f, default_flow_style=False)
    return dump
