"""The LiDAR detection output without a GPU: the test-side restatement tests/detect_ref.py (fp32, as the reference computes)
reproduces every case of tests/golden/gv24_voxel_postprocess.npz - the reference's own run (tests/golden/make_golden_detect.py) - in its
picked anchor indices, their order, the (None, None) case, the tp / fp lists and the AP; the host mirrors' CPU sides (anchor generator,
AP arithmetic) match the reference's outputs; the cases' input conditions hold (no decision on a rounding edge); the detection head's
keys appear in PointPillarFuseBEVT's state_dict only with anchor_number; argument checks raise CobevtHipError."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import cases_detect as cd
import cases_pillar as cp
import detect_ref as dr
from cobevt_amd import host, lib, ops
from cobevt_amd.lib import CobevtHipError
from util import golden


@pytest.fixture(scope="module")
def gv():
    return golden("gv24_voxel_postprocess")


def _post(grid, order, half, **kw):
    return host.VoxelPostprocessor(cd.anchor_params(grid, order, *half, **kw), train=False)


def test_anchor_generator_matches_the_reference(gv):
    """both orders, the default feature_stride of 2 and an explicit 4: bit for bit (host numpy on both sides)"""
    for name, post in (("A_anchors", _post(cd.A_GRID, "hwl", (6.0, 4.0))), ("B_hwl_anchors", _post(cd.B_GRID, "hwl", cd.B_HALF)),
                       ("B_lhw_anchors", _post(cd.B_GRID, "lhw", cd.B_HALF)), ("stride4_anchors", _post((4, 5), "lhw", (20.0, 16.0), stride=4))):
        got = post.generate_anchor_box()
        assert got.dtype == np.float64 and got.shape == gv[name].shape and np.array_equal(got, gv[name]), name
    assert gv["stride4_anchors"].shape == (4, 5, 2, 7) and gv["A_anchors"].shape == (2, 3, 2, 7)
    bad = cd.anchor_params(cd.A_GRID, "whl", 6.0, 4.0)
    with pytest.raises(CobevtHipError):
        host.VoxelPostprocessor(bad, train=False).generate_anchor_box()


def _check_case(gv, name, cavs, order):
    out = dr.post_process(cavs, cd.SCORE_THRESHOLD, cd.NMS_THRESH, order, torch.float32)
    cd.conditions(dr.post_process(cavs, cd.SCORE_THRESHOLD, cd.NMS_THRESH, order, torch.float64), require_candidates=not bool(gv[name + "_none"]))
    assert out["none"] == bool(gv[name + "_none"])
    if out["none"]:
        return out
    assert np.array_equal(out["index"], gv[name + "_index"]), name               # same anchors, same order
    dev_box, dev_score = gv[name + "_dev"]
    assert np.abs(out["boxes"].astype(np.float64) - gv[name + "_boxes"]).max() <= 2 * dev_box + 1e-6
    assert np.abs(out["scores"].astype(np.float64) - gv[name + "_scores"]).max() <= 2 * dev_score + 1e-7
    return out


def test_case_a_by_hand(gv):
    cavs, where = cd.case_a(gv["A_anchors"])
    out = _check_case(gv, "A", cavs, "hwl")
    assert out["index"].tolist() == [where[i] for i in cd.A_EXPECTED] and len(out["candidates"]) == 4
    got = dr.delta_to_boxes3d(cavs[0][1], cavs[0][2], torch.float32).numpy()
    assert got.shape == gv["A_boxes3d"].shape == (1, 12, 7) and np.abs(got - gv["A_boxes3d"]).max() <= 1e-6
    cavs, _ = cd.case_a(gv["A_anchors"], nothing=True)
    assert _check_case(gv, "A_nothing", cavs, "hwl")["none"]


@pytest.mark.parametrize("order,reflect", [("hwl", False), ("hwl", True), ("lhw", False)])
def test_case_b(gv, order, reflect):
    name = "B_%s%s" % (order, "_reflect" if reflect else "")
    cavs, where = cd.case_b(gv["B_%s_anchors" % order], order, reflect)
    out = _check_case(gv, name, cavs, order)
    # more than 64 candidates (several ballot words); filtered boxes; an out-of-range box that suppressed an in-range one
    assert len(out["candidates"]) > 64 and out["suppressors_out_of_range"] >= 2
    assert len(out["candidates"]) == len(cd.b_designed()) - 4
    assert where[cd.B_SUPPRESSED] in out["candidates"].tolist() and where[cd.B_SUPPRESSED] not in out["index"].tolist()
    assert where[cd.B_SUPPRESSOR] in out["candidates"].tolist() and where[cd.B_SUPPRESSOR] not in out["index"].tolist()
    assert not np.array_equal(cavs[0][3], cavs[1][3])


def test_case_c_cut_at_1000(gv):
    post = _post(cd.C_GRID, "hwl", cd.C_HALF)
    cavs = cd.case_c(post.generate_anchor_box())
    out = _check_case(gv, "C", cavs, "hwl")
    assert cavs[0][0].size == 1536 and len(out["candidates"]) == cd.C_CANDIDATES >= 1100 and len(out["index"]) > 64


def test_nms_rotated_and_eval(gv):
    boxes, scores = cd.case_nms()
    keep, margin = dr.nms_rotated(boxes, scores, cd.NMS_THRESH)
    assert margin >= 1e-3 and np.array_equal(keep, gv["nms_keep"]) and float(scores.min()) < 0 < float(scores.max())
    assert np.array_equal(dr.nms_rotated(cd.case_nms(flat=True)[0], scores, cd.NMS_THRESH)[0], gv["nms_keep"])
    gt = cd.case_e_gt()
    assert gt.shape == (10, 8, 3)
    stat = {t: {"tp": [], "fp": [], "gt": 0} for t in cd.EVAL_IOUS}
    for t in cd.EVAL_IOUS:
        fp, tp, n_gt, margin = dr.tp_fp(gv["B_hwl_boxes"], gv["B_hwl_scores"], gt, t)
        assert margin >= 1e-3, (t, margin)
        k = "%d" % round(100 * t)
        assert tp == gv["E_tp_" + k].tolist() and fp == gv["E_fp_" + k].tolist() and n_gt == 10
        ap, mrec, mpre = dr.average_precision(fp, tp, n_gt)
        assert abs(ap - float(gv["E_ap_" + k][0])) < 1e-12
        # the host mirror's AP arithmetic on the reference's flags
        stat[t]["tp"], stat[t]["fp"], stat[t]["gt"] = list(tp), list(fp), n_gt
        ap_h, mrec_h, mpre_h = host.calculate_ap(copy.deepcopy(stat), t)
        assert ap_h == float(gv["E_ap_" + k][0]) and mrec_h == gv["E_mrec_" + k].tolist() and mpre_h == gv["E_mpre_" + k].tolist()
    assert 0 < sum(gv["E_tp_70"]) < sum(gv["E_tp_50"]) < sum(gv["E_tp_30"])
    res = host.eval_final_results(copy.deepcopy(stat))
    assert res["ap30"] == float(gv["E_ap_30"][0]) and res["ap_50"] == float(gv["E_ap_50"][0]) and res["ap_70"] == float(gv["E_ap_70"][0])
    assert host.voc_ap([0.5, 1.0], [1.0, 0.5])[0] == 0.75


def test_eval_final_results_writes_only_with_a_path(tmp_path):
    stat = {t: {"tp": [1, 0, 1], "fp": [0, 1, 0], "gt": 4} for t in (0.3, 0.5, 0.7)}
    host.eval_final_results(copy.deepcopy(stat))
    assert list(tmp_path.iterdir()) == []
    res = host.eval_final_results(copy.deepcopy(stat), str(tmp_path))
    import yaml
    with open(tmp_path / "eval.yaml") as f:
        assert yaml.safe_load(f)["ap_50"] == res["ap_50"]


def test_case_d_covers_the_special_pairs():
    a, b = cd.case_d()
    assert a.shape == (40, 4, 2) and b.shape == (24, 4, 2) and a.dtype == np.float32
    iou = dr.iou_matrix(a, b)
    assert abs(iou[0, 0] - 1.0) < 1e-12 and abs(iou[1, 1] - 1.0) < 1e-12        # identical, and identical with the other winding
    assert iou[2, 2] == 0.0 and float(a[2, :, 0].max()) == float(b[2, :, 0].min())   # touching along an edge
    assert abs(iou[3, 3] - 0.25) < 1e-6 and abs(iou[4, 4] - 1.0 / 9.0) < 1e-6      # contained / containing: area ratios
    assert iou[5, 5] == 0.0 and int(((iou > 0.05) & (iou < 0.95)).sum()) >= 15
    signed = [dr._signed_area(q.astype(np.float64)) for q in np.concatenate([a, b])]
    assert min(signed) < -1.0 and max(signed) > 1.0 and min(abs(s) for s in signed) > 1.0 and float(np.abs(a).max()) < 200


def _model_args(anchor_number=None):
    args = cp.model_args()
    if anchor_number is not None:
        args["anchor_number"] = anchor_number
    return args


def test_head_keys_only_with_anchor_number():
    plain = host.PointPillarFuseBEVT(_model_args())
    det = host.PointPillarFuseBEVT(_model_args(2))
    extra = {"cls_head.weight": (2, 64, 1, 1), "cls_head.bias": (2,), "reg_head.weight": (14, 64, 1, 1), "reg_head.bias": (14,)}
    sd_plain, sd_det = plain.state_dict(), det.state_dict()
    assert not any(k.startswith(("cls_head", "reg_head")) for k in sd_plain)
    assert list(sd_det)[:len(sd_plain)] == list(sd_plain) and set(sd_det) - set(sd_plain) == set(extra)
    assert all(tuple(sd_det[k].shape) == s for k, s in extra.items())
    with pytest.raises(CobevtHipError, match="inference only"):
        det.train()({"processed_lidar": {}, "record_len": torch.tensor([1])})
    with pytest.raises(CobevtHipError):
        host.PointPillarFuseBEVT(_model_args(0))


def test_argument_checks():
    """CPU tensors and wrong shapes are rejected before anything is launched; the C entry points reject null pointers (1) and
    unsupported shapes (2)"""
    psm, rm, anc, m = torch.zeros(1, 2, 2, 3), torch.zeros(1, 14, 2, 3), torch.zeros(2, 3, 2, 7), torch.eye(4)
    with pytest.raises(CobevtHipError):
        ops.detect_post_process([(psm, rm, anc, m)], 0.2, 0.15, "hwl")
    with pytest.raises(CobevtHipError):
        ops.detect_post_process([], 0.2, 0.15, "hwl")
    with pytest.raises(CobevtHipError):
        ops.delta_to_boxes3d(rm, anc)
    with pytest.raises(CobevtHipError):
        ops.rotated_iou(torch.zeros(3, 4, 2), torch.zeros(2, 4, 2))
    with pytest.raises(CobevtHipError):
        ops.nms_rotated(torch.zeros(3, 8, 3), torch.zeros(3), 0.15)
    post = _post(cd.A_GRID, "hwl", (6.0, 4.0))
    with pytest.raises(CobevtHipError, match="batch size"):
        post.post_process({0: {"anchor_box": anc, "transformation_matrix": m}}, {0: {"psm": psm.repeat(2, 1, 1, 1), "rm": rm.repeat(2, 1, 1, 1)}})
    with pytest.raises(CobevtHipError):
        post.post_process({0: {"anchor_box": anc, "transformation_matrix": m}}, {})
    l = lib.load()
    need = ctypes.c_long(0)
    assert l.cobevt_detect_scratch(1536, ctypes.byref(need)) == 0
    assert need.value == 8 * 1536 + 8 * 1000 * 16 + 4 * 1000 * 24 + 4 * 1000 + 4 * 1000 + 16 == ops.detect_workspace_bytes(1536)
    assert l.cobevt_detect_scratch(10, None) == 1 and l.cobevt_detect_scratch(-1, ctypes.byref(need)) == 2
    assert l.cobevt_detect_post(None, None, None, None, None, 1, 1, 0.2, 0.15, None, None, None, None, None, None) == 1
    buf = (ctypes.c_double * 8)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    one = (ctypes.c_void_p * 1)(ptr.value)
    dims = (ctypes.c_int * 3)(2, 3, 2)
    assert l.cobevt_detect_post(one, one, one, ptr, dims, 0, 1, 0.2, 0.15, ptr, ptr, ptr, ptr, ptr, None) == 2       # no cav
    assert l.cobevt_detect_post(one, one, one, ptr, dims, 17, 1, 0.2, 0.15, ptr, ptr, ptr, ptr, ptr, None) == 2      # more than 16
    bad = (ctypes.c_int * 3)(2, 0, 2)
    assert l.cobevt_detect_post(one, one, one, ptr, bad, 1, 1, 0.2, 0.15, ptr, ptr, ptr, ptr, ptr, None) == 2
    assert l.cobevt_nms_rotated(ptr, ptr, 4, 12, 0.15, ptr, ptr, ptr, ptr, ptr, None) == 2                          # corner_floats
    assert l.cobevt_nms_rotated(None, None, 4, 24, 0.15, ptr, ptr, ptr, ptr, ptr, None) == 1
    assert l.cobevt_delta_to_boxes3d(None, ptr, ptr, 1, 2, 3, 2, None) == 1 and l.cobevt_delta_to_boxes3d(ptr, ptr, ptr, 0, 2, 3, 2, None) == 2
    assert l.cobevt_rotated_iou(None, None, None, 0, 5, None) == 0 and l.cobevt_rotated_iou(None, ptr, ptr, 2, 2, None) == 1
