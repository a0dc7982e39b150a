"""The detection targets and the PointPillar detection loss on the GPU: csrc/detect_targets.hip through ops.boxes_standup /
detect_targets / pointpillar_loss, host.VoxelPostprocessor.generate_label / generate_label_batch and host.PointPillarLoss, against
the reference's own run (tests/golden/gv27_detect_labels.npz, cases of tests/golden/cases_labels.py) and, for the loss, against
float64 autograd of the restatement (tests/labels_ref.py).

Label maps and num_pos are decisions and are compared EXACTLY.  At kernel level the kernel is fed the reference's own fp32 standup
boxes, so its IoU must have the compiled reference's bits and the maps are exact on every case, the tie-heavy case T included; at
host level the standup boxes are the device's own and the cases keep every decision off a rounding edge (asserted on the CPU by
tests/test_detect_targets.py and by the generator).  Targets, standup boxes, the loss and its gradients are gated at 4 x the
deviation the generator recorded for the fp32 restatement, relative to |ref| + the quantity's scale (cases_labels.gate,
tests/golden/README_gv27.md).  Every test prints its worst |err| / gate.

Measured on an MI355X (worst |err| / gate per test): DESIGN.md section 3m."""
import copy

import numpy as np
import pytest
import torch

import att_backbone_ref as ar
import cases_labels as cl
import labels_ref as lr
from cobevt_amd import host, ops
from cobevt_amd.registry import create_loss
from cobevt_amd.synth import fill_module_
from util import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gv():
    return golden("gv27_detect_labels")


def _case(name):
    post = host.VoxelPostprocessor(cl.anchor_params(name), train=True)
    anchors = post.generate_anchor_box()
    gt, mask = cl.case(name, anchors)
    return post, anchors, gt, mask


def _ratio(what, got, ref, scale, gate_rel):
    """worst |got - ref| / (gate_rel (|ref| + scale)), printed and returned"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    r = float((np.abs(got - ref) / (gate_rel * (np.abs(ref) + scale))).max()) if ref.size else 0.0
    print("%s: worst |err| / gate %.3f (relative gate %.3e, scale %.3e)" % (what, r, gate_rel, scale))
    return r


def _f32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


# ---------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("name", cl.HOST_CASES + ("T",))
def test_detect_targets_on_the_reference_standup_boxes(cuda, gv, name):
    _, anchors, gt, mask = _case(name)
    b, g = mask.shape
    gst = np.zeros((b, g, 4), dtype=np.float32)
    for s in range(b):
        gst[s, mask[s] == 1] = gv["%s_gt_standup_%d" % (name, s)]
    args = (_f32(anchors, cuda), _f32(gv[name + "_anchor_standup"], cuda), _f32(gt, cuda), _f32(gst, cuda), _f32(mask, cuda), cl.POS_T, cl.NEG_T)
    pos, neg, targets, num_pos = ops.detect_targets(*args)
    again = ops.detect_targets(*args)
    torch.cuda.synchronize()
    assert np.array_equal(pos.cpu().numpy(), gv[name + "_pos"].astype(np.float32)), "pos_equal_one differs from the reference"
    assert np.array_equal(neg.cpu().numpy(), gv[name + "_neg"].astype(np.float32)), "neg_equal_one differs from the reference"
    assert num_pos.cpu().tolist() == [int(gv[name + "_pos"][s].sum()) for s in range(b)]
    assert _ratio("detect_targets %s targets" % name, targets.cpu().numpy(), gv[name + "_targets"], 1.0, cl.gate(gv[name + "_dev"][0])) <= 1.0
    for x, y in zip((pos, neg, targets, num_pos), again):
        assert torch.equal(x, y), "two calls differ"


def test_detect_targets_without_ground_truth_slots(cuda, gv):
    """G = 0: one launch, everything negative"""
    _, anchors, _, _ = _case("c1")
    z = lambda *s: torch.zeros(*s, device=cuda)                                                  # noqa: E731
    pos, neg, targets, num_pos = ops.detect_targets(_f32(anchors, cuda), _f32(gv["c1_anchor_standup"], cuda), z(2, 0, 7), z(2, 0, 4),
                                                    z(2, 0), cl.POS_T, cl.NEG_T)
    assert not pos.any() and neg.all() and not targets.any() and num_pos.tolist() == [0, 0]


@pytest.mark.parametrize("name", cl.HOST_CASES + ("T",))
def test_boxes_standup_against_the_reference(cuda, gv, name):
    _, anchors, gt, mask = _case(name)
    gate = cl.gate(gv[name + "_dev"][1])
    ref = gv[name + "_anchor_standup"]
    scale = float(max(np.abs(ref).max(), max(np.abs(gv["%s_gt_standup_%d" % (name, s)]).max(initial=0.0) for s in range(len(gt)))))
    got = ops.boxes_standup(_f32(anchors.reshape(-1, 7), cuda))
    worst = _ratio("boxes_standup %s anchors" % name, got.cpu().numpy(), ref, scale, gate)
    for s in range(len(gt)):
        got = ops.boxes_standup(_f32(gt[s][mask[s] == 1].reshape(-1, 7), cuda))
        worst = max(worst, _ratio("boxes_standup %s gt %d" % (name, s), got.cpu().numpy(), gv["%s_gt_standup_%d" % (name, s)].reshape(-1, 4), scale, gate))
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------- host level
@pytest.mark.parametrize("name", cl.HOST_CASES)
def test_generate_label_matches_the_reference(cuda, gv, name):
    """numpy in / numpy float64 out per sample, the batch call on device tensors, both from the device's own standup boxes"""
    post, anchors, gt, mask = _case(name)
    batch = post.generate_label_batch(torch.from_numpy(gt).to(cuda), torch.from_numpy(mask).to(cuda), anchors)
    again = post.generate_label_batch(torch.from_numpy(gt).to(cuda), torch.from_numpy(mask).to(cuda), anchors)
    assert sorted(batch) == ["neg_equal_one", "num_pos", "pos_equal_one", "targets"] and batch["num_pos"].dtype == torch.int32
    assert all(torch.equal(batch[k], again[k]) for k in batch), "two calls differ"
    assert post._anchor_cache[1] is anchors                                          # the anchor set was uploaded once
    assert batch["num_pos"].cpu().tolist() == [int(gv[name + "_pos"][s].sum()) for s in range(len(gt))]
    worst = 0.0
    for s in range(len(gt)):
        one = post.generate_label(gt_box_center=gt[s], anchors=anchors, mask=mask[s])
        assert sorted(one) == ["neg_equal_one", "pos_equal_one", "targets"]
        assert all(isinstance(v, np.ndarray) and v.dtype == np.float64 for v in one.values())
        assert np.array_equal(one["pos_equal_one"], gv[name + "_pos"][s]) and np.array_equal(one["neg_equal_one"], gv[name + "_neg"][s])
        for k in one:
            assert np.array_equal(one[k], batch[k][s].cpu().numpy().astype(np.float64)), "the batch differs from the per-sample call"
        worst = max(worst, _ratio("generate_label %s sample %d targets" % (name, s), one["targets"], gv[name + "_targets"][s], 1.0,
                                  cl.gate(gv[name + "_dev"][0])))
    assert worst <= 1.0
    dev = post.generate_label(gt_box_center=torch.from_numpy(gt[0]).to(cuda), anchors=anchors, mask=torch.from_numpy(mask[0]))
    assert all(v.is_cuda and torch.equal(v, batch[k][0]) for k, v in dev.items())


def test_generate_label_takes_the_lower_gt_index_not_the_max_iou_gt(cuda, gv):
    post, anchors, gt, mask = _case("c2")
    ref64 = lr.generate_label(gt[0], anchors, mask[0], cl.POS_T, cl.NEG_T, np.float64)
    weak, pair = cl.c2_designed(ref64, anchors)
    other = lr.generate_label(gt[0], anchors, mask[0], cl.POS_T, cl.NEG_T, np.float64, rule="max")
    got = post.generate_label(gt_box_center=gt[0], anchors=anchors, mask=mask[0])
    t = got["targets"].reshape(-1, 7)
    assert np.abs(t[pair] - ref64["targets"].reshape(-1, 7)[pair]).max() < 1e-5 < 1e-2 < np.abs(t[pair] - other["targets"].reshape(-1, 7)[pair]).max()
    assert got["pos_equal_one"].reshape(-1)[weak] == 1 and got["neg_equal_one"].reshape(-1)[weak] == 0


# ---------------------------------------------------------------------------------------------- loss
@pytest.fixture(scope="module")
def loss_refs(gv):
    """per loss case: the inputs and the float64 autograd of the restatement, computed once"""
    out = {}
    for name in cl.LOSS_CASES:
        pos = gv[name + "_pos"].astype(np.float32)
        psm, rm, tg = cl.loss_inputs(name, pos, gv[name + "_targets"])
        out[name] = (psm, rm, pos, tg) + lr.loss_and_grads(psm, rm, pos, tg, **cl.LOSS_ARGS)
    return out


@pytest.mark.parametrize("name", cl.LOSS_CASES)
def test_pointpillar_loss_and_gradients(cuda, gv, loss_refs, name):
    """B = 1 and B = 3 with a sample without positives; logits of +-30, |d| on both sides of beta, yaw differences beyond +-pi and one
    NaN target are in the inputs (cases_labels.loss_inputs)"""
    psm, rm, pos, tg, l64, gp64, gr64 = loss_refs[name]
    assert np.abs(l64 - gv["loss_%s_ref" % name]).max() <= 1e-12 * abs(l64[0])
    d_loss, d_psm, d_rm = [float(v) for v in gv["loss_%s_dev" % name]]
    t = [_f32(x, cuda) for x in (psm, rm, pos, tg)]
    num_pos = torch.tensor([int(pos[s].sum()) for s in range(len(pos))], dtype=torch.int32, device=cuda)
    assert 0 in num_pos.tolist() or len(pos) == 1
    loss, dpsm, drm = ops.pointpillar_loss(*t, num_pos=num_pos, want_grad=True, **cl.LOSS_ARGS)
    counted = ops.pointpillar_loss(*t, num_pos=None, want_grad=True, **cl.LOSS_ARGS)
    plain, none_p, none_r = ops.pointpillar_loss(*t, num_pos=num_pos, want_grad=False, **cl.LOSS_ARGS)
    torch.cuda.synchronize()
    assert none_p is None and none_r is None and torch.equal(plain, loss), "the loss depends on whether gradients are asked for"
    for x, y in zip((loss, dpsm, drm), counted):
        assert torch.equal(x, y), "num_pos given and counted differ"
    worst = _ratio("pointpillar_loss %s [total, conf, reg]" % name, loss.cpu().numpy(), l64, abs(l64[0]), cl.gate(d_loss))
    worst = max(worst, _ratio("pointpillar_loss %s d psm" % name, dpsm.cpu().numpy(), gp64, float(np.abs(gp64).max()), cl.gate(d_psm)))
    worst = max(worst, _ratio("pointpillar_loss %s d rm" % name, drm.cpu().numpy(), gr64, float(np.abs(gr64).max()), cl.gate(d_rm)))
    assert worst <= 1.0


@pytest.mark.parametrize("name", cl.LOSS_CASES)
def test_point_pillar_loss_module_backward(cuda, loss_refs, name):
    """through create_loss and .backward(): the head maps receive the kernel's gradients; the reference's float64 label dict works"""
    psm, rm, pos, tg, l64, _, _ = loss_refs[name]
    crit = create_loss({"loss": {"core_method": "point_pillar_loss", "args": dict(cl.LOSS_ARGS)}})
    p, r = _f32(psm, cuda).requires_grad_(True), _f32(rm, cuda).requires_grad_(True)
    labels = {"pos_equal_one": torch.from_numpy(pos.astype(np.float64)).to(cuda), "targets": torch.from_numpy(tg.astype(np.float64)).to(cuda)}
    with torch.enable_grad():                                                         # whatever grad mode an earlier test left behind
        total = crit({"psm": p, "rm": r}, labels)
        assert total.dim() == 0 and total.requires_grad
        (3.0 * total).backward()
    loss, dpsm, drm = ops.pointpillar_loss(p.detach(), r.detach(), _f32(pos, cuda), _f32(tg, cuda), want_grad=True, **cl.LOSS_ARGS)
    assert torch.equal(total.detach(), loss[0]) and torch.equal(p.grad, dpsm * 3.0) and torch.equal(r.grad, drm * 3.0)
    assert sorted(crit.loss_dict) == ["conf_loss", "reg_loss", "total_loss"] and not crit.loss_dict["total_loss"].requires_grad
    assert torch.equal(crit.loss_dict["total_loss"], loss[0]) and torch.equal(crit.loss_dict["conf_loss"], loss[1]) and torch.equal(crit.loss_dict["reg_loss"], loss[2])
    with torch.no_grad():
        assert torch.equal(crit({"psm": p, "rm": r}, labels), loss[0])                # validation: no graph, same bits


# ---------------------------------------------------------------------------------------------- end to end
def test_point_pillar_intermediate_validation_loss(cuda, gv):
    """OpenCOOD's validation pass: criterion(model(batch), label_dict) under model.eval(), labels from generate_label_batch on the
    head maps' own 8 x 12 x 2 grid; the loss is finite and equals the float64 restatement applied to the model's own outputs"""
    args, vox = ar.pillar_args(), ar.pillar_voxels()
    model = fill_module_(host.PointPillarIntermediate(copy.deepcopy(args)), 0).eval().to(cuda)
    batch = {"processed_lidar": {k: v.to(cuda) for k, v in vox.items()}, "record_len": torch.tensor(ar.PILLAR_RECORD_LEN)}
    post, anchors, gt, mask = _case("e2e")
    labels = post.generate_label_batch(torch.from_numpy(gt).to(cuda), torch.from_numpy(mask).to(cuda), anchors)
    crit = host.PointPillarLoss(dict(cl.LOSS_ARGS))
    with torch.no_grad(), host.compute_dtype("fp32"):
        out = model(batch)
        total = crit(out, labels)
    torch.cuda.synchronize()
    assert tuple(out["psm"].shape) == (1, 2, 8, 12) and int(labels["num_pos"][0]) == 4 and bool(torch.isfinite(total))
    l64, _, _ = lr.loss_and_grads(out["psm"].cpu().numpy(), out["rm"].cpu().numpy(), labels["pos_equal_one"].cpu().numpy(),
                                  labels["targets"].cpu().numpy(), **cl.LOSS_ARGS)
    got = np.array([float(crit.loss_dict[k]) for k in ("total_loss", "conf_loss", "reg_loss")])
    gate = cl.gate(max(float(gv["loss_%s_dev" % n][0]) for n in cl.LOSS_CASES))
    assert _ratio("PointPillarIntermediate -> PointPillarLoss [total, conf, reg]", got, l64, abs(l64[0]), gate) <= 1.0
