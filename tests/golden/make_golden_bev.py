"""Generate gv28_lidar_bev.npz by running the REFERENCE's BevPreprocessor.preprocess, LidarBevPostprocessor.generate_label and
post_process on the procedural cases of cases_bev.py, in the build container like make_golden_detect.py:

    python tests/golden/make_golden_bev.py

Stored are only outputs (bev_input, label maps, corners, boxes, scores, picked pixel indices) and, per case and quantity, how far
the reference lies from the float64 restatement (tests/bev_ref.py): the GPU tests' gates are derived from that deviation.  Inputs are
procedural and never stored.

Stand-ins as in make_golden_detect.py: tests/golden/_standin_shapely.py is installed BEFORE make_golden is imported, the Cython
extension and the visualisation / dataset modules' third-party packages are inert mocks, and `np.int = int` restores the alias numpy
removed (bev_preprocessor.py :30 uses it).

The reference's preprocessor has no rule for points outside its map (a negative index wraps, a large one raises): it is given the
points the project's documented rule keeps (bev_ref.kept_mask), which is also where the optional masks are applied - the reference's
dataset applies pcd_utils' masks before the preprocessor, and pcd_utils' own functions are checked against that rule here.

The reference returns boxes, not pixel indices: a picked box is identified with the candidate whose fp32 score it carries (the
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
import cases_bev as cb                        # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import bev_ref as br                          # noqa: E402

if not hasattr(np, "int"):
    np.int = int
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

from opencood.data_utils.pre_processor.bev_preprocessor import BevPreprocessor as R_Pre  # noqa: E402
from opencood.data_utils.post_processor.lidar_bev_postprocessor import LidarBevPostprocessor as R_Post  # noqa: E402
from opencood.utils import pcd_utils as R_pcd  # noqa: E402

assert getattr(sys.modules["shapely"], "_cobevt_standin", False)


def _pre_case(name, clouds, range_mask, ego_mask, designed, out):
    pre = R_Pre(cb.pre_params(range_mask, ego_mask), train=False)
    maps, margin = [], np.inf
    for p in clouds:
        keep, _, m = br.kept_mask(p, cb.GEOM, cb.LIDAR_RANGE, range_mask, ego_mask)
        margin = min(margin, m)
        # pcd_utils' own masks on the points the map rule keeps: the same selection
        base = br.kept_mask(p, cb.GEOM, cb.LIDAR_RANGE)[0]
        q = p[base]
        if range_mask:
            q = R_pcd.mask_points_by_range(q, cb.LIDAR_RANGE)
        if ego_mask:
            q = R_pcd.mask_ego_points(q)
        assert np.array_equal(q, p[keep]), name
        maps.append(pre.preprocess(p[keep])["bev_input"])
    cb.pre_conditions(margin, designed)
    ref = np.stack(maps).astype(np.float32)
    mine = br.bev_points(clouds, cb.GEOM, cb.LIDAR_RANGE, range_mask, ego_mask)
    assert np.array_equal(ref[:, :-1], mine[:, :-1]), "%s: occupancy differs from the restatement" % name
    dev = float(np.abs(ref[:, -1].astype(np.float64) - mine[:, -1]).max())
    assert dev <= 1e-3 * max(1.0, float(np.abs(mine[:, -1]).max())), (name, dev)
    out[name + "_bev"], out[name + "_dev"] = ref, np.array(dev)
    print("%-16s %6d occupied, %5d intensity cells; reference fp32 running mean vs float64 mean %.3e (margin %.1e cells)"
          % (name, int(ref[:, :-1].sum()), int((mine[:, -1] != 0).sum()), dev, margin))


def _label_case(name, gt, mask, axis_aligned, out):
    post = R_Post(cb.post_params(), train=True)
    maps, devs, nvalid = [], [], []
    corners = np.zeros(gt.shape[:2] + (4, 2), dtype=np.float32)
    for b in range(gt.shape[0]):
        ref = post.generate_label(gt_box_center=gt[b].astype(np.float64), mask=mask[b])
        mine = br.generate_label(gt[b], mask[b], cb.GEOM, cb.TARGET_MEAN, cb.TARGET_STD_DEV, faithful=True)
        if int(mask[b].sum()):
            cb.label_conditions(mine, axis_aligned)
        n = int((mask[b] == 1).sum())
        rc = np.asarray(ref["bev_corners"])
        assert rc.dtype == np.float32 and rc.shape == (n, 4, 2)
        assert np.array_equal(rc, mine["bev_corners"]), "%s: the reference's fp32 corners differ from the restatement's bits" % name
        corners[b, :n] = rc
        lm = ref["label_map"]
        assert lm.dtype == np.float32 and np.array_equal(lm[0], mine["label_map"][0])
        devs.append(float(np.abs(lm.astype(np.float64) - mine["label_map"]).max()))
        maps.append(lm)
        nvalid.append(n)
    out[name + "_label_map"], out[name + "_corners"], out[name + "_num_valid"] = np.stack(maps), corners, np.array(nvalid, dtype=np.int32)
    out[name + "_dev"] = np.array(max(devs))
    print("%-16s valid %s, %d positive pixels; reference vs float64 restatement %.3e" % (name, nvalid, int(np.stack(maps)[:, 0].sum()),
                                                                                      max(devs)))


def _post_case(name, cavs, geom, out, expect_none=False, expect_empty=False):
    post = R_Post(cb.post_params(geom), train=False)
    data = {c: {"transformation_matrix": torch.from_numpy(m)} for c, (_, _, m) in enumerate(cavs)}
    output = {c: {"cls": torch.from_numpy(cl), "reg": torch.from_numpy(rg)} for c, (cl, rg, _) in enumerate(cavs)}
    boxes, scores = post.post_process(data, output)
    ref32 = br.post_process(cavs, geom, cb.TARGET_MEAN, cb.TARGET_STD_DEV, cb.SCORE_THRESHOLD, cb.NMS_THRESH, faithful=True)
    ref64 = br.post_process(cavs, geom, cb.TARGET_MEAN, cb.TARGET_STD_DEV, cb.SCORE_THRESHOLD, cb.NMS_THRESH, faithful=False)
    cb.post_conditions(ref64, expect_none)
    cb.post_conditions(ref32, expect_none)
    out[name + "_none"] = np.array(boxes is None)
    if boxes is None:
        assert expect_none
        print("%-16s reference returns (None, None)" % name)
        return
    assert not expect_none
    boxes, scores = boxes.numpy(), scores.numpy()
    assert boxes.dtype == np.float32 and scores.dtype == np.float32
    cand = np.concatenate([torch.sigmoid(torch.from_numpy(cl)).reshape(-1).numpy() for cl, _, _ in cavs])
    index = np.array([int(np.nonzero(cand == s)[0][0]) for s in scores], dtype=np.int32)
    assert len(set(index.tolist())) == len(index) and all(int((cand == s).sum()) == 1 for s in scores)
    assert np.array_equal(index, ref32["index"]) and np.array_equal(index, ref64["index"]), "%s: the restatement picks differently" % name
    assert (len(index) == 0) == expect_empty
    out[name + "_boxes"], out[name + "_scores"], out[name + "_index"] = boxes.reshape(-1, 4, 2), scores, index
    dev_box = float(np.abs(boxes.astype(np.float64) - ref64["boxes"]).max()) if len(index) else 0.0
    dev_score = float(np.abs(scores.astype(np.float64) - ref64["scores"]).max()) if len(index) else 0.0
    out[name + "_dev"] = np.array([dev_box, dev_score])
    out[name + "_maxcoord"] = np.array(float(np.abs(boxes).max()) if len(index) else 0.0)
    print("%-16s %4d boxes of %4d candidates (%d picked before the range mask); reference vs float64 restatement: corners %.3e scores "
          "%.3e; margins: score %.1e gap %.1e iou %.1e range %.1e"
          % (name, len(index), len(ref64["candidates"]), len(ref64["picked_all"]), dev_box, dev_score, ref64["score_margin"],
             ref64["score_gap"], ref64["iou_margin"], ref64["range_margin"]))
    return ref64


def main():
    out = {}
    main_clouds, boundary = cb.points_main(), cb.points_boundary()
    _pre_case("pre_main", main_clouds, False, False, False, out)
    _pre_case("pre_main_masks", main_clouds, True, True, False, out)
    for rm in (False, True):
        for em in (False, True):
            _pre_case("pre_boundary_r%d_e%d" % (rm, em), boundary, rm, em, True, out)
    gt, mask = cb.labels_main()
    _label_case("label_main", gt, mask, False, out)
    gt, mask = cb.labels_axis()
    _label_case("label_axis", gt, mask, True, out)
    _post_case("post_two", cb.post_two_cavs(), cb.GEOM, out)
    _post_case("post_none", cb.post_nothing(), cb.GEOM, out, expect_none=True)
    _post_case("post_range", cb.post_out_of_range(), cb.GEOM, out, expect_empty=True)
    r = _post_case("post_cut", cb.post_cut(), cb.GEOM_CUT, out)
    assert len(r["candidates"]) == cb.CUT_CANDIDATES > 1000
    mg.save("gv28_lidar_bev", **out)


if __name__ == "__main__":
    main()
