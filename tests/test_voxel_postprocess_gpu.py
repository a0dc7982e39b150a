"""The LiDAR detection output on the GPU: csrc/detect_post.hip through ops.detect_post_process / delta_to_boxes3d / rotated_iou /
nms_rotated, host.VoxelPostprocessor and host.eval_utils, against the reference's own run (tests/golden/gv24_voxel_postprocess.npz,
cases A - E of tests/golden/cases_detect.py).

Picked anchor indices and their order are compared EXACTLY: the cases keep every decision off a rounding edge (asserted on the CPU
by tests/test_voxel_postprocess.py and by the generator).  Corner coordinates and scores are gated at 4 x the deviation the generator
measured between the reference's fp32 result and the float64 restatement (stored per case in the fixture), with a floor of 4 ulp of
the case's largest coordinate (for scores: 4 ulp of a score below 1, 4 * 2^-24): the reference and the kernel both sit within one such
deviation of the float64 value, and the factor covers the device's exp / sin / cos / sigmoid differing from the host's by a few ulp.
rotated_iou is gated at 1e-9 absolute against the float64 IoU (about 50 float64 operations on coordinates below 200 and areas above
1: 200^2 * 1e-16 * 50 = 2e-10)."""
import copy

import numpy as np
import pytest
import torch

import cases_detect as cd
import cases_pillar as cp
import detect_ref as dr
from cobevt_amd import host, ops
from cobevt_amd.synth import fill_module_
from util import assert_close, bf16_gate, golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gv():
    return golden("gv24_voxel_postprocess")


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _gates(gv, name):
    dev_box, dev_score = [float(v) for v in gv[name + "_dev"]]
    return max(4 * dev_box, 4 * _ulp32(float(gv[name + "_maxcoord"]))), max(4 * dev_score, 4 * 2.0 ** -24)


def _dicts(cavs, dev, device_side=False):
    """the reference's data_dict / output_dict; device_side: anchors and matrices as fp32 device tensors (graph capture)"""
    data, output = {}, {}
    for c, (psm, rm, anchors, matrix) in enumerate(cavs):
        a, m = torch.from_numpy(anchors), torch.from_numpy(matrix)
        data["cav%d" % c] = {"transformation_matrix": m.to(dev) if device_side else m, "anchor_box": a.to(dev) if device_side else a}
        output["cav%d" % c] = {"psm": torch.from_numpy(psm).to(dev), "rm": torch.from_numpy(rm).to(dev)}
    return data, output


def _check(got, gv, name):
    """fixed-capacity device tensors against the fixture: exact indices and order, gated corners and scores, zeros past count"""
    boxes, scores, index, count = [g.cpu() for g in got]
    k = int(count[0])
    ref_index = gv[name + "_index"]
    assert k == len(ref_index), "%s: %d boxes, the reference has %d" % (name, k, len(ref_index))
    assert np.array_equal(index[:k].numpy(), ref_index), name
    box_gate, score_gate = _gates(gv, name)
    d_box = float((boxes[:k].double() - torch.from_numpy(gv[name + "_boxes"]).double()).abs().max())
    d_score = float((scores[:k].double() - torch.from_numpy(gv[name + "_scores"]).double()).abs().max())
    print("%s: corners max |diff| %.3e (gate %.3e)  scores %.3e (gate %.3e)" % (name, d_box, box_gate, d_score, score_gate))
    assert d_box <= box_gate and d_score <= score_gate, (name, d_box, box_gate, d_score, score_gate)
    assert tuple(boxes.shape) == (1000, 8, 3) and tuple(scores.shape) == (1000,) and index.dtype == torch.int32
    assert not bool(boxes[k:].any()) and not bool(scores[k:].any()) and not bool(index[k:].any())
    return k


def _run_both(gv, name, post, cavs, dev):
    """through the host mirror (one host read) and through the operator"""
    data, output = _dicts(cavs, dev)
    boxes, scores = post.post_process(data, output)
    got = post.post_process_device(data, output)
    torch.cuda.synchronize()
    k = _check(got, gv, name)
    assert tuple(boxes.shape) == (k, 8, 3) and torch.equal(boxes, got[0][:k]) and torch.equal(scores, got[1][:k])
    dev_cavs = [(o["psm"], o["rm"], d["anchor_box"], d["transformation_matrix"]) for d, o in zip(data.values(), output.values())]
    again = ops.detect_post_process(dev_cavs, cd.SCORE_THRESHOLD, cd.NMS_THRESH, post.params["order"])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    return got


def _post(grid, order, half):
    return host.VoxelPostprocessor(cd.anchor_params(grid, order, *half), train=False)


# ---------------------------------------------------------------------------------------------- A
def test_case_a(cuda, gv):
    post = _post(cd.A_GRID, "hwl", (6.0, 4.0))
    anchors = post.generate_anchor_box()
    cavs, where = cd.case_a(anchors)
    got = _run_both(gv, "A", post, cavs, cuda)
    assert got[2][:3].tolist() == [where[i] for i in cd.A_EXPECTED]
    # nothing above the score threshold: (None, None), count 0 and all-zero outputs
    cavs, _ = cd.case_a(anchors, nothing=True)
    data, output = _dicts(cavs, cuda)
    assert bool(gv["A_nothing_none"]) and post.post_process(data, output) == (None, None)
    dev_out = post.post_process_device(data, output)
    assert int(dev_out[3][0]) == 0 and not bool(dev_out[0].any())


def test_delta_to_boxes3d(cuda, gv):
    post = _post(cd.A_GRID, "hwl", (6.0, 4.0))
    cavs, _ = cd.case_a(post.generate_anchor_box())
    rm = torch.from_numpy(cavs[0][1]).to(cuda)
    ref = torch.from_numpy(gv["A_boxes3d"])
    got = host.VoxelPostprocessor.delta_to_boxes3d(rm, cavs[0][2]).cpu()
    gate = 4 * _ulp32(float(ref.abs().max()))          # a few fp32 operations per value, exp within a few ulp
    d = float((got - ref).abs().max())
    print("delta_to_boxes3d: max |diff| %.3e (gate %.3e)" % (d, gate))
    assert tuple(got.shape) == (1, 12, 7) and d <= gate
    # N = 2: the second sample's deltas negated
    both = ops.delta_to_boxes3d(torch.cat([rm, -rm]).contiguous(), torch.from_numpy(cavs[0][2]).to(cuda)).cpu()
    ref2 = dr.delta_to_boxes3d(np.concatenate([cavs[0][1], -cavs[0][1]]), cavs[0][2], torch.float64)
    assert tuple(both.shape) == (2, 12, 7) and torch.equal(both[0], got[0]) and float((both.double() - ref2).abs().max()) <= gate


# ---------------------------------------------------------------------------------------------- B, E
@pytest.mark.parametrize("order,reflect", [("hwl", False), ("hwl", True), ("lhw", False)])
def test_case_b(cuda, gv, order, reflect):
    name = "B_%s%s" % (order, "_reflect" if reflect else "")
    post = _post(cd.B_GRID, order, cd.B_HALF)
    anchors = post.generate_anchor_box()
    assert np.array_equal(anchors, gv["B_%s_anchors" % order])
    cavs, where = cd.case_b(anchors, order, reflect)
    got = _run_both(gv, name, post, cavs, cuda)
    assert where[cd.B_SUPPRESSED] not in got[2].tolist() and where[cd.B_SUPPRESSOR] not in got[2].tolist()


def test_case_e_eval(cuda, gv):
    """caluclate_tp_fp / calculate_ap on case B's detections (from the device) against 10 ground-truth boxes"""
    post = _post(cd.B_GRID, "hwl", cd.B_HALF)
    cavs, _ = cd.case_b(post.generate_anchor_box(), "hwl")
    boxes, scores = post.post_process(*_dicts(cavs, cuda))
    gt = torch.from_numpy(cd.case_e_gt())
    stat = {t: {"tp": [], "fp": [], "gt": 0} for t in cd.EVAL_IOUS}
    for t in cd.EVAL_IOUS:
        host.caluclate_tp_fp(boxes, scores, gt, stat, t)
        k = "%d" % round(100 * t)
        assert stat[t]["tp"] == gv["E_tp_" + k].tolist() and stat[t]["fp"] == gv["E_fp_" + k].tolist() and stat[t]["gt"] == 10
    # a frame without detections only adds its ground truth
    host.caluclate_tp_fp(None, None, gt, stat, 0.5)
    assert stat[0.5]["gt"] == 20 and len(stat[0.5]["tp"]) == len(gv["E_tp_50"])
    stat[0.5]["gt"] = 10
    res = host.eval_final_results(stat)
    assert res["ap30"] == float(gv["E_ap_30"][0]) and res["ap_50"] == float(gv["E_ap_50"][0]) and res["ap_70"] == float(gv["E_ap_70"][0])
    assert res["mrec_70"] == gv["E_mrec_70"].tolist() and res["mpre_50"] == gv["E_mpre_50"].tolist()


# ---------------------------------------------------------------------------------------------- C
def test_case_c_cut_at_1000(cuda, gv):
    post = _post(cd.C_GRID, "hwl", cd.C_HALF)
    cavs = cd.case_c(post.generate_anchor_box())
    k = _check(_run_both(gv, "C", post, cavs, cuda), gv, "C")
    assert k > 64 and cavs[0][0].size == 1536


# ---------------------------------------------------------------------------------------------- D
def test_rotated_iou(cuda):
    a, b = cd.case_d()
    ref = dr.iou_matrix(a, b)
    got = ops.rotated_iou(torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda)).cpu().numpy()
    d = float(np.abs(got - ref).max())
    print("rotated_iou: max |diff| %.3e (gate 1e-9)" % d)
    assert got.dtype == np.float64 and got.shape == (40, 24) and d <= 1e-9
    assert got[2, 2] == 0.0 and got[5, 5] == 0.0 and abs(got[0, 0] - 1.0) <= 1e-9 and abs(got[1, 1] - 1.0) <= 1e-9
    # (N, 8, 3) boxes: corners 0 .. 3 in xy; and an empty side
    a3 = np.zeros((40, 8, 3), dtype=np.float32)
    a3[:, :4, :2] = a
    a3[:, 4:, :] = 7.0
    assert np.array_equal(ops.rotated_iou(torch.from_numpy(a3).to(cuda), torch.from_numpy(b).to(cuda)).cpu().numpy(), got)
    assert tuple(ops.rotated_iou(torch.zeros(0, 4, 2, device=cuda), torch.from_numpy(b).to(cuda)).shape) == (0, 24)


def test_nms_rotated(cuda, gv):
    boxes, scores = cd.case_nms()
    keep = ops.nms_rotated(torch.from_numpy(boxes).to(cuda), torch.from_numpy(scores).to(cuda), cd.NMS_THRESH)
    assert keep.dtype == torch.int32 and np.array_equal(keep.cpu().numpy(), gv["nms_keep"])
    flat = cd.case_nms(flat=True)[0]
    out = ops.nms_rotated_device(torch.from_numpy(flat).to(cuda), torch.from_numpy(scores).to(cuda), cd.NMS_THRESH)
    k = int(out[3][0])
    assert np.array_equal(out[2][:k].cpu().numpy(), gv["nms_keep"]) and torch.equal(out[1][:k].cpu(), torch.from_numpy(scores[gv["nms_keep"]]))
    assert torch.equal(out[0][:k, :4, :2].cpu(), torch.from_numpy(flat[gv["nms_keep"]])) and not bool(out[0][:k, 4:].any())
    assert ops.nms_rotated(torch.zeros(0, 8, 3, device=cuda), torch.zeros(0, device=cuda), cd.NMS_THRESH).numel() == 0


# ---------------------------------------------------------------------------------------------- determinism, garbage, graph replay
def test_reproducible_garbage_and_graph_replay(cuda, gv):
    """two eager runs are bit-identical; outputs and workspace filled with garbage before a call read zero past count afterwards; a
    third run as a graph replay equals the eager result, with count read only after the replay"""
    post = _post(cd.B_GRID, "hwl", cd.B_HALF)
    cavs, _ = cd.case_b(post.generate_anchor_box(), "hwl")
    data, output = _dicts(cavs, cuda, device_side=True)
    first = [t.clone() for t in post.post_process_device(data, output)]
    outs = [torch.full((1000, 8, 3), 7.5, device=cuda), torch.full((1000,), -3.0, device=cuda),
            torch.full((1000,), 77, device=cuda, dtype=torch.int32), torch.full((1,), 77, device=cuda, dtype=torch.int32)]
    total = sum(c[0].size for c in cavs)
    ws = torch.full(((ops.detect_workspace_bytes(total) + 7) // 8 + 64,), -1, device=cuda, dtype=torch.int64)
    second = post.post_process_device(data, output, out=outs, workspace=ws[:-64])
    torch.cuda.synchronize()
    assert all(s.data_ptr() == o.data_ptr() for s, o in zip(second, outs))
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert bool((ws[-64:] == -1).all())
    k = _check(second, gv, "B_hwl")
    # graph replay on garbage-filled outputs
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        post.post_process_device(data, output, out=outs, workspace=ws[:-64])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        post.post_process_device(data, output, out=outs, workspace=ws[:-64])
    outs[0].fill_(9.25)
    outs[1].fill_(5.0)
    outs[2].fill_(-5)
    outs[3].fill_(-5)
    ws[:-64].fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, outs))
    assert int(outs[3][0]) == k                                 # the count is read only now
    del graph
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the model's head
@pytest.mark.parametrize("mode", ["bf16", "fp32", "fp32_split"])
def test_model_head(cuda, mode):
    """anchor_number = 2 on a 32 x 32 grid, one sample of 2 agents: psm / rm equal conv2d of the returned fused_feature with the head
    weights (the project's gate of the compute dtype), and the model without the argument gives a bit-identical fused_feature"""
    fusion = copy.deepcopy(cp.FUSION)
    fusion.update(agent_size=2, depth=1, drop_out=0.0)
    args = cp.model_args(grid=(32, 32), max_cav=2, fusion=fusion)
    plain = fill_module_(host.PointPillarFuseBEVT(copy.deepcopy(args)), cp.SEED).eval().to(cuda)
    args["anchor_number"] = 2
    det = fill_module_(host.PointPillarFuseBEVT(args), cp.SEED).eval().to(cuda)
    vox = {k: v.to(cuda) for k, v in cp.voxels(counts=[300, 260], grid=(32, 32), tag="gv24").items()}
    batch = {"processed_lidar": vox, "record_len": torch.tensor([2], dtype=torch.int32, device=cuda)}
    with torch.no_grad(), host.compute_dtype(mode):
        out = det(batch)
        ref_out = plain(batch)
    torch.cuda.synchronize()
    assert set(out) == {"fused_feature", "psm", "rm"} and set(ref_out) == {"fused_feature"}
    ref_fused = ref_out["fused_feature"]
    fused = out["fused_feature"]
    assert torch.equal(fused, ref_fused) and tuple(fused.shape) == (1, 64, 32, 32) and float(fused.abs().max()) > 0
    assert tuple(out["psm"].shape) == (1, 2, 32, 32) and tuple(out["rm"].shape) == (1, 14, 32, 32)
    assert out["psm"].dtype == out["rm"].dtype == torch.float32 and out["psm"].is_contiguous() and out["rm"].is_contiguous()
    tol = bf16_gate()[0] if mode == "bf16" else 1e-3
    with torch.no_grad():
        assert_close(out["psm"], torch.nn.functional.conv2d(fused, det.cls_head.weight, det.cls_head.bias), tol, "detection head psm " + mode)
        assert_close(out["rm"], torch.nn.functional.conv2d(fused, det.reg_head.weight, det.reg_head.bias), tol, "detection head rm " + mode)
    # the maps feed the post-processor as they are
    post = _post((32, 32), "hwl", (25.6, 25.6))
    data = {0: {"anchor_box": post.generate_anchor_box(), "transformation_matrix": torch.eye(4)}}
    boxes, scores, index, count = post.post_process_device(data, {0: {"psm": out["psm"], "rm": out["rm"]}})
    assert 0 <= int(count[0]) <= 1000
