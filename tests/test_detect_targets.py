"""CPU: the detection targets and loss without a GPU - the restatement (tests/labels_ref.py) against the reference's own run
(tests/golden/gv27_detect_labels.npz, cases of tests/golden/cases_labels.py), the conditions that keep every decision of a
host-level case off a rounding edge, and the host API's checks (which all come before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

import cases_labels as cl
import labels_ref as lr
from cobevt_amd import host, lib, ops
from cobevt_amd.lib import CobevtHipError
from cobevt_amd.registry import create_loss
from util import golden


@pytest.fixture(scope="module")
def gv():
    return golden("gv27_detect_labels")


def _case(name):
    post = host.VoxelPostprocessor(cl.anchor_params(name), train=True)
    anchors = post.generate_anchor_box()
    gt, mask = cl.case(name, anchors)
    return post, anchors, gt, mask


@pytest.mark.parametrize("name", cl.HOST_CASES)
def test_float64_restatement_reproduces_the_reference(gv, name):
    """exact label maps, targets to 1e-12, from the restatement's own float64 standup boxes; the case's conditions hold"""
    _, anchors, gt, mask = _case(name)
    for b in range(len(gt)):
        out = lr.generate_label(gt[b], anchors, mask[b], cl.POS_T, cl.NEG_T, np.float64)
        cl.conditions(out)
        assert np.array_equal(out["pos_equal_one"], gv[name + "_pos"][b])
        assert np.array_equal(out["neg_equal_one"], gv[name + "_neg"][b])
        assert np.abs(out["targets"] - gv[name + "_targets"][b]).max() <= 1e-12
        assert out["num_pos"] == int(gv[name + "_pos"][b].sum())
        assert not (out["pos_equal_one"] * out["neg_equal_one"]).any()


@pytest.mark.parametrize("name", cl.HOST_CASES + ("T",))
def test_fp32_restatement_on_the_reference_standup_boxes_decides_as_the_reference(gv, name):
    """what the kernel-level GPU test asks of the kernel, asked of the fp32 restatement: fed the reference's fp32 standup boxes its
    IoU has the compiled reference's bits, so the label maps are exact on every case, the tie-heavy one included"""
    _, anchors, gt, mask = _case(name)
    for b in range(len(gt)):
        out = lr.generate_label(gt[b], anchors, mask[b], cl.POS_T, cl.NEG_T, np.float32, anchor_standup=gv[name + "_anchor_standup"],
                                gt_standup=gv["%s_gt_standup_%d" % (name, b)])
        assert np.array_equal(out["pos_equal_one"], gv[name + "_pos"][b])
        assert np.array_equal(out["neg_equal_one"], gv[name + "_neg"][b])
        assert cl.rel_dev(out["targets"], gv[name + "_targets"][b], 1.0) <= cl.gate(gv[name + "_dev"][0])


def test_case_shapes_cover_what_the_table_promises(gv):
    assert gv["c1_pos"].size == 70 and gv["c2_pos"].size == 1536 and gv["c3_pos"].size == 3034
    assert gv["c4_pos"].shape[-1] == 1 and gv["c5_pos"].shape[0] == 3
    assert [int(gv["c5_pos"][b].sum()) for b in range(3)] == [0, 1, 100]
    assert gv["c5_neg"][0].all()                                   # no valid gt: every anchor is negative
    _, anchors, gt, mask = _case("c5")
    assert mask[1].sum() == 1 and mask[1, 0] == 0                  # the non-prefix mask
    assert 9 <= gv["c3_gt_standup_0"].shape[0] <= 12


def test_c2_designed_boxes_and_the_matching_rule(gv):
    """beyond: unassigned; weak: positive below neg_threshold and not negative; pair: the anchor takes the LOWER gt index although
    the higher one overlaps it more - matching to the max-IoU gt instead changes the reference's targets"""
    _, anchors, gt, mask = _case("c2")
    out = lr.generate_label(gt[0], anchors, mask[0], cl.POS_T, cl.NEG_T, np.float64)
    weak, pair = cl.c2_designed(out, anchors)
    ref_t = gv["c2_targets"][0].reshape(-1, 7)
    assert gv["c2_pos"][0].reshape(-1)[weak] == 1 and gv["c2_neg"][0].reshape(-1)[weak] == 0
    other = lr.generate_label(gt[0], anchors, mask[0], cl.POS_T, cl.NEG_T, np.float64, rule="max")
    assert np.abs(out["targets"].reshape(-1, 7)[pair] - ref_t[pair]).max() <= 1e-12
    assert np.abs(other["targets"].reshape(-1, 7)[pair] - ref_t[pair]).max() > 1e-2
    assert np.array_equal(other["pos_equal_one"], out["pos_equal_one"])


def test_loss_restatement_matches_the_recorded_float64_values(gv):
    for name in cl.LOSS_CASES:
        psm, rm, tg = cl.loss_inputs(name, gv[name + "_pos"], gv[name + "_targets"])
        assert np.isnan(tg).sum() == 1
        l64, gp, gr = lr.loss_and_grads(psm, rm, gv[name + "_pos"].astype(np.float32), tg, **cl.LOSS_ARGS)
        assert np.abs(l64 - gv["loss_%s_ref" % name]).max() <= 1e-12 * abs(l64[0])
        assert np.isfinite(gp).all() and np.isfinite(gr).all() and abs(l64[0] - (l64[1] + l64[2])) <= 1e-12 * abs(l64[0])
    # a sample without positives is normalised by 1, not by 0
    assert int(gv["c5_pos"][0].sum()) == 0


def test_generate_label_refuses_what_it_does_not_support():
    post, anchors, gt, mask = _case("c1")
    lhw = host.VoxelPostprocessor(cl.anchor_params("c1", order="lhw"), train=True)
    with pytest.raises(CobevtHipError, match="hwl"):
        lhw.generate_label(gt_box_center=gt[0], anchors=anchors, mask=mask[0])
    with pytest.raises(CobevtHipError, match="hwl"):
        lhw.generate_label_batch(torch.zeros(1, 5, 7), torch.zeros(1, 5), anchors)
    with pytest.raises(CobevtHipError, match="at most 128"):
        post.generate_label_batch(torch.zeros(1, 129, 7), torch.zeros(1, 129), anchors)
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        post.generate_label_batch(torch.zeros(1, 5, 7), torch.zeros(1, 5), anchors)
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        post.generate_label(gt_box_center=torch.zeros(5, 7), anchors=anchors, mask=torch.zeros(5))
    with pytest.raises(CobevtHipError, match=r"\(B, max_num, 7\)"):
        post.generate_label_batch(torch.zeros(1, 5, 6), torch.zeros(1, 5), anchors)
    with pytest.raises(CobevtHipError, match=r"\(B, max_num, 7\)"):
        post.generate_label_batch(torch.zeros(1, 5, 7), torch.zeros(1, 4), anchors)
    with pytest.raises(CobevtHipError, match=r"\(max_num, 7\)"):
        post.generate_label(gt_box_center=torch.zeros(1, 5, 7), anchors=anchors, mask=torch.zeros(5))


def test_operator_wrappers_check_before_they_launch():
    a = torch.zeros(2, 3, 2, 7)
    with pytest.raises(CobevtHipError, match="at most 128"):
        ops.detect_targets(a, torch.zeros(12, 4), torch.zeros(1, 129, 7), torch.zeros(1, 129, 4), torch.zeros(1, 129), 0.6, 0.45)
    with pytest.raises(CobevtHipError, match=r"\(H, W, A, 7\)"):
        ops.detect_targets(torch.zeros(12, 7), torch.zeros(12, 4), torch.zeros(1, 5, 7), torch.zeros(1, 5, 4), torch.zeros(1, 5), 0.6, 0.45)
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        ops.detect_targets(a, torch.zeros(12, 4), torch.zeros(1, 5, 7), torch.zeros(1, 5, 4), torch.zeros(1, 5), 0.6, 0.45)
    with pytest.raises(CobevtHipError, match=r"\(n, 7\)"):
        ops.boxes_standup(torch.zeros(4, 8))
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        ops.boxes_standup(torch.zeros(4, 7))
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        ops.pointpillar_loss(torch.zeros(1, 2, 3, 4), torch.zeros(1, 14, 3, 4), torch.zeros(1, 3, 4, 2), torch.zeros(1, 3, 4, 14), 1.0, 2.0)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    l = lib.load()
    assert l.cobevt_boxes_standup(None, None, 4, None) == 1
    assert l.cobevt_boxes_standup(None, None, 0, None) == 0         # nothing to do, nothing read
    assert l.cobevt_boxes_standup(None, None, -1, None) == 2
    nulls = [None] * 5
    assert l.cobevt_detect_targets(*nulls, 0.6, 0.45, None, None, None, None, None, 1, 2, 3, 2, 5, None) == 1
    assert l.cobevt_pointpillar_loss(*([None] * 9), 1, 2, 3, 2, 1.0, 2.0, None) == 1
    # more than 128 slots: code 2, decided on the numbers alone (the pointers only have to be non-null and aligned)
    buf = (ctypes.c_double * 8)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    assert l.cobevt_detect_targets(p, p, p, p, p, 0.6, 0.45, p, p, p, p, p, 1, 2, 3, 2, 129, None) == 2
    assert l.cobevt_detect_targets(p, p, p, p, p, 0.6, 0.45, p, p, p, p, p, 1, 0, 3, 2, 5, None) == 2
    # gradients: both or neither
    assert l.cobevt_pointpillar_loss(p, p, p, p, None, p, p, None, p, 1, 2, 3, 2, 1.0, 2.0, None) == 1
    assert l.cobevt_abi_version() == 1


def test_create_loss_finds_point_pillar_loss():
    crit = create_loss({"loss": {"core_method": "point_pillar_loss", "args": {"cls_weight": 1.0, "reg": 2.0}}})
    assert type(crit) is host.PointPillarLoss and crit.cls_weight == 1.0 and crit.reg_coe == 2.0 and crit.loss_dict == {}
    out = {"psm": torch.zeros(1, 2, 3, 4), "rm": torch.zeros(1, 14, 3, 4)}
    with pytest.raises(CobevtHipError, match="no CPU fallback"):
        crit(out, {"pos_equal_one": torch.zeros(1, 3, 4, 2), "targets": torch.zeros(1, 3, 4, 14)})


def test_collate_batch_mirrors_the_reference(gv):
    frames = [{"pos_equal_one": gv["c5_pos"][b].astype(np.float64), "neg_equal_one": gv["c5_neg"][b].astype(np.float64),
               "targets": gv["c5_targets"][b]} for b in range(3)]
    out = host.VoxelPostprocessor.collate_batch(frames)
    assert sorted(out) == ["neg_equal_one", "pos_equal_one", "targets"]
    assert out["targets"].dtype == torch.float64 and tuple(out["targets"].shape) == tuple(gv["c5_targets"].shape)
    assert np.array_equal(out["pos_equal_one"].numpy(), gv["c5_pos"]) and np.array_equal(out["neg_equal_one"].numpy(), gv["c5_neg"])
    assert np.array_equal(out["targets"].numpy(), gv["c5_targets"])
    tens = host.VoxelPostprocessor.collate_batch([{k: torch.from_numpy(v) for k, v in f.items()} for f in frames])
    assert all(torch.equal(tens[k], out[k]) for k in out)
