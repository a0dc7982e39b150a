"""Generate gv24_voxel_postprocess.npz by running the REFERENCE's detection output on the procedural cases of cases_detect.py, in the
build container like make_golden.py:

    python tests/golden/make_golden_detect.py

Run are the reference's VoxelPostprocessor.generate_anchor_box / delta_to_boxes3d / post_process, box_utils.nms_rotated and
eval_utils.caluclate_tp_fp / calculate_ap.  Stored are only their outputs (anchors, boxes, scores, picked indices, tp / fp lists, AP)
and, per case and quantity, how far the reference's fp32 result lies from the float64 restatement (tests/detect_ref.py): the GPU
test's gate is derived from that deviation.  Inputs are procedural and never stored.

shapely is not installed: tests/golden/_standin_shapely.py provides a working float64 Polygon (third-party arithmetic, parity
unpinned) and is installed BEFORE make_golden is imported, whose _standins.install() would otherwise add an inert one.  The Cython
extension opencood.utils.box_overlaps (only generate_label uses it) and, where they do not import, the visualisation and dataset
modules' third-party packages are inert mocks: nothing replayed here calls into them.

The reference returns boxes, not anchor indices: a picked box is identified with the candidate whose fp32 score it carries (the
ladder keeps all scores distinct)."""
import importlib
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

import _standin_shapely

_standin_shapely.install()

import make_golden as mg                      # noqa: E402  puts the repository, this directory and the reference on the path
import cases_detect as cd                     # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import detect_ref as dr                       # noqa: E402

sys.modules["opencood.utils.box_overlaps"] = types.SimpleNamespace(bbox_overlaps=None)
for name in ("cv2", "timm", "timm.scheduler", "timm.scheduler.cosine_lr", "open3d", "matplotlib", "matplotlib.pyplot", "matplotlib.cm",
             "tensorboardX"):
    try:
        importlib.import_module(name)
    except Exception:
        sys.modules[name] = mock.MagicMock(name=name)
try:
    importlib.import_module("opencood.visualization.vis_utils")
except Exception:
    sys.modules["opencood.visualization.vis_utils"] = mock.MagicMock(name="vis_utils")

from opencood.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor as R_Post  # noqa: E402
from opencood.utils import box_utils as R_box  # noqa: E402
from opencood.utils import eval_utils as R_eval  # noqa: E402

assert getattr(sys.modules["shapely"], "_cobevt_standin", False)


def _tensors(cavs):
    data, output = {}, {}
    for c, (psm, rm, anchors, matrix) in enumerate(cavs):
        data[c] = {"transformation_matrix": torch.from_numpy(matrix), "anchor_box": torch.from_numpy(anchors)}
        output[c] = {"psm": torch.from_numpy(psm), "rm": torch.from_numpy(rm)}
    return data, output


def _run_case(name, post, cavs, order, out, expect_none=False):
    """reference post_process on one case -> stores boxes / scores / index and the deviations; returns the restatement's fp32 run"""
    data, output = _tensors(cavs)
    boxes, scores = post.post_process(data, output)
    ref32 = dr.post_process(cavs, cd.SCORE_THRESHOLD, cd.NMS_THRESH, order, torch.float32)
    ref64 = dr.post_process(cavs, cd.SCORE_THRESHOLD, cd.NMS_THRESH, order, torch.float64)
    cd.conditions(ref64, require_candidates=not expect_none)
    out[name + "_none"] = np.array(boxes is None)
    if boxes is None:
        assert expect_none and ref32["none"] and ref64["none"], name
        print("%-10s reference returns (None, None)" % name)
        return ref32
    assert not expect_none
    boxes, scores = boxes.numpy(), scores.numpy()
    # identify each returned box by its score among the fp32 candidates' scores
    cand_scores = []
    for psm, _, _, _ in cavs:
        cand_scores.append(torch.sigmoid(torch.from_numpy(psm).permute(0, 2, 3, 1)).reshape(-1).numpy())
    cand_scores = np.concatenate(cand_scores)
    index = np.array([int(np.nonzero(cand_scores == s)[0][0]) for s in scores], dtype=np.int32)
    assert len(set(index.tolist())) == len(index) and all(int((cand_scores == s).sum()) == 1 for s in scores)
    assert np.array_equal(index, ref32["index"]), "%s: the fp32 restatement picks differently from the reference" % name
    assert np.array_equal(index, ref64["index"]), "%s: the float64 restatement picks differently from the reference" % name
    dev_box = float(np.abs(boxes.astype(np.float64) - ref64["boxes"]).max())
    dev_score = float(np.abs(scores.astype(np.float64) - ref64["scores"]).max())
    out[name + "_boxes"], out[name + "_scores"], out[name + "_index"] = boxes.astype(np.float32), scores.astype(np.float32), index
    out[name + "_dev"] = np.array([dev_box, dev_score])
    out[name + "_maxcoord"] = np.array(float(np.abs(boxes).max()))
    print("%-10s %4d boxes of %4d candidates; reference fp32 vs float64 restatement: corners %.3e  scores %.3e; margins: score %.1e gap %.1e "
          "filter %.1e iou %.1e range %.1e" % (name, len(index), len(ref64["candidates"]), dev_box, dev_score, ref64["score_margin"],
                                               ref64["score_gap"], ref64["filter_margin"], ref64["iou_margin"], ref64["range_margin"]))
    return ref32


def main():
    out = {}
    # ---- A
    pa = R_Post(cd.anchor_params(cd.A_GRID, "hwl", 6.0, 4.0), train=False)
    anchors_a = pa.generate_anchor_box()
    out["A_anchors"] = anchors_a
    cavs, where = cd.case_a(anchors_a)
    ra = _run_case("A", pa, cavs, "hwl", out)
    assert ra["index"].tolist() == [where[i] for i in cd.A_EXPECTED]
    d2b = R_Post.delta_to_boxes3d(torch.from_numpy(cavs[0][1]), torch.from_numpy(cavs[0][2]))
    out["A_boxes3d"] = d2b.numpy()
    assert np.abs(d2b.numpy() - dr.delta_to_boxes3d(cavs[0][1], cavs[0][2], torch.float32).numpy()).max() <= 1e-6
    cavs, _ = cd.case_a(anchors_a, nothing=True)
    _run_case("A_nothing", pa, cavs, "hwl", out, expect_none=True)
    # ---- B
    for order in ("hwl", "lhw"):
        pb = R_Post(cd.anchor_params(cd.B_GRID, order, *cd.B_HALF), train=False)
        anchors_b = pb.generate_anchor_box()
        out["B_%s_anchors" % order] = anchors_b
        for reflect in ((False, True) if order == "hwl" else (False,)):
            name = "B_%s%s" % (order, "_reflect" if reflect else "")
            cavs, where = cd.case_b(anchors_b, order, reflect)
            rb = _run_case(name, pb, cavs, order, out)
            assert len(rb["candidates"]) > 64 and rb["suppressors_out_of_range"] >= 2
            picked = rb["index"].tolist()
            assert where[cd.B_SUPPRESSED] in rb["candidates"].tolist() and where[cd.B_SUPPRESSED] not in picked
            if name == "B_hwl":
                det = (torch.from_numpy(out[name + "_boxes"]), torch.from_numpy(out[name + "_scores"]))
    # a stride-4 grid through feature_stride (the default of 2 is what every other case takes)
    out["stride4_anchors"] = R_Post(cd.anchor_params((4, 5), "lhw", 20.0, 16.0, stride=4), train=False).generate_anchor_box()
    # ---- C
    pc = R_Post(cd.anchor_params(cd.C_GRID, "hwl", *cd.C_HALF), train=False)
    cavs = cd.case_c(pc.generate_anchor_box())
    rc = _run_case("C", pc, cavs, "hwl", out)
    assert len(rc["candidates"]) >= 1100
    # box_utils.nms_rotated on its own: given corners with scores of both signs, and an empty input
    nb, ns = cd.case_nms()
    keep = R_box.nms_rotated(torch.from_numpy(nb), torch.from_numpy(ns), cd.NMS_THRESH)
    mine, margin = dr.nms_rotated(nb, ns, cd.NMS_THRESH)
    assert margin >= 1e-3 and np.array_equal(keep, mine) and 0 < len(keep) < len(ns), (margin, len(keep))
    assert np.array_equal(keep, R_box.nms_rotated(torch.from_numpy(cd.case_nms(flat=True)[0]), torch.from_numpy(ns), cd.NMS_THRESH))
    out["nms_keep"] = keep.astype(np.int32)
    assert len(R_box.nms_rotated(torch.zeros(0, 8, 3), torch.zeros(0), cd.NMS_THRESH)) == 0
    # ---- E
    gt = cd.case_e_gt()
    stat = {t: {"tp": [], "fp": [], "gt": 0} for t in cd.EVAL_IOUS}
    for t in cd.EVAL_IOUS:
        R_eval.caluclate_tp_fp(det[0], det[1], torch.from_numpy(gt), stat, t)
        fp, tp, n_gt, margin = dr.tp_fp(det[0].numpy(), det[1].numpy(), gt, t)
        assert margin >= 1e-3, (t, margin)
        assert fp == stat[t]["fp"] and tp == stat[t]["tp"] and n_gt == stat[t]["gt"]
        out["E_tp_%d" % round(100 * t)] = np.array(stat[t]["tp"], dtype=np.int32)
        out["E_fp_%d" % round(100 * t)] = np.array(stat[t]["fp"], dtype=np.int32)
        ap, mrec, mpre = R_eval.calculate_ap(stat, t)
        ap2, mrec2, mpre2 = dr.average_precision(fp, tp, n_gt)
        assert abs(ap - ap2) < 1e-12 and np.allclose(mrec, mrec2) and np.allclose(mpre, mpre2)
        out["E_ap_%d" % round(100 * t)] = np.array([ap])
        out["E_mrec_%d" % round(100 * t)], out["E_mpre_%d" % round(100 * t)] = np.array(mrec), np.array(mpre)
        print("E  iou %.1f: tp %d fp %d of %d gt, AP %.4f (margin %.1e)" % (t, sum(tp), sum(fp), n_gt, ap, margin))
    # ---- D: the float64 IoU of the stand-in against the restatement's (two independent clips), nothing stored but the agreement
    a, b = cd.case_d()
    ref = dr.iou_matrix(a, b)
    pa_, pb_ = [_standin_shapely.Polygon(q) for q in a], [_standin_shapely.Polygon(q) for q in b]
    alt = np.array([[p.intersection(q).area / p.union(q).area for q in pb_] for p in pa_])
    print("D  stand-in vs restatement IoU: max |diff| %.3e" % np.abs(ref - alt).max())
    assert np.abs(ref - alt).max() < 1e-12
    mg.save("gv24_voxel_postprocess", **out)


if __name__ == "__main__":
    main()
