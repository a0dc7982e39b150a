"""Generate gv29_cloud_prep.npz by running the REFERENCE's pcd_utils.mask_ego_points / lidar_project / mask_points_by_range,
augment_utils.random_flip_along_x / _y / global_rotation / global_scaling and DataAugmentor.forward (seeded) on the procedural cases of
cases_cloud.py, in the build container like make_golden_bev.py:

    python tests/golden/make_golden_cloud.py

Stored are only outputs (the fp32 cloud, its offsets, the boxes, the parameters the reference drew) and, per case, how far the
reference lies from the restatement (tests/cloud_ref.py) where the two may differ: the number of projected coordinates that differ
after rounding to fp32, of how many (`<case>_proj_diff`).  The largest |reference - restatement| of the rotated coordinates is printed,
not stored: the CPU test measures it against its bound from the stored points.  Inputs are procedural and never stored.  Stand-ins as in
make_golden_bev.py (open3d and shapely are absent and mocked)."""
import importlib
import os
import sys
from unittest import mock

import numpy as np

import _standin_shapely

_standin_shapely.install()

import make_golden as mg                      # noqa: E402  puts the repository, this directory and the reference on the path
import cases_cloud as cc                      # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import cloud_ref as cr                        # noqa: E402

for name in ("cv2", "open3d", "matplotlib", "matplotlib.pyplot", "matplotlib.cm"):
    try:
        importlib.import_module(name)
    except Exception:
        sys.modules[name] = mock.MagicMock(name=name)

from opencood.data_utils.augmentor import augment_utils as R_aug            # noqa: E402
from opencood.data_utils.augmentor.data_augmentor import DataAugmentor as R_Augmentor  # noqa: E402
from opencood.utils import pcd_utils as R_pcd                                # noqa: E402


def ulps32(a, b):
    """distance in fp32 units in the last place between two fp32 arrays of finite values"""
    ia, ib = (np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(v < 0, -(v & 0x7fffffff), v) for v in (ia, ib))
    return np.abs(ia - ib)


def _augment(case, points, seed):
    """the reference's augmentation of one cloud and the case's boxes -> points, boxes, the parameters it drew"""
    aug = cc.GOLDEN[case["name"]]["aug"]
    b, m = case["boxes"].copy(), case["box_mask"].copy()
    drawn = []
    choice, uniform = np.random.choice, np.random.uniform

    def rec_choice(*a, **k):
        drawn.append(float(choice(*a, **k)))
        return bool(drawn[-1])

    def rec_uniform(*a, **k):
        drawn.append(float(uniform(*a, **k)))
        return drawn[-1]
    np.random.seed(seed)
    with mock.patch.object(np.random, "choice", rec_choice), mock.patch.object(np.random, "uniform", rec_uniform):
        if aug == "full":
            d = R_Augmentor(cc.AUG_CONFIG, train=True).forward({"lidar_np": points, "object_bbx_center": b, "object_bbx_mask": m})
            points, b = d["lidar_np"], d["object_bbx_center"]
            assert np.array_equal(d["object_bbx_mask"], case["box_mask"])
        else:
            valid = b[m == 1]
            if aug == "flips":
                valid, points = R_aug.random_flip_along_x(valid, points)
                valid, points = R_aug.random_flip_along_y(valid, points)
            elif aug == "rot":
                valid, points = R_aug.global_rotation(valid, points, cc.ROT_RANGE)
            else:
                valid, points = R_aug.global_scaling(valid, points, cc.SCALE_RANGE)
            b[:len(valid)] = valid
    return points, b, np.asarray(drawn, dtype=np.float64)


def _case(name, out):
    case = dict(cc.golden_case(name), name=name)
    world, masks = case["world"], case["masks"]
    c, s = cc.cos_sin(world)
    per_agent, proj_diff, proj_total = [], 0, 0
    for a, p in enumerate(case["clouds"]):
        q = p.copy()
        if masks:
            assert float(cc.margin(p, case["transforms"][a], True, world).min()) >= cc.MARGIN
            q = R_pcd.mask_ego_points(q)
            assert np.array_equal(q, p[cr.ego_keep(p)]), "%s: the ego mask differs from the restatement" % name
            q = R_pcd.lidar_project(q, case["transforms"][a])
            assert q.dtype == np.float64
            mine = cr.project(p[cr.ego_keep(p)][:, :3].astype(np.float64), case["transforms"][a])
            u = ulps32(q[:, :3].astype(np.float32), mine.astype(np.float32))
            assert int(u.max(initial=0)) <= 1, "%s: a projected coordinate is more than one fp32 ulp from the restatement" % name
            proj_diff, proj_total = proj_diff + int((u != 0).sum()), proj_total + u.size
        per_agent.append(q)
    assert proj_diff <= 1e-4 * max(proj_total, 1), (name, proj_diff, proj_total)
    counts = [len(q) for q in per_agent]
    stack = R_pcd.projected_lidar_stack(per_agent)
    drawn = np.zeros(0)
    if world is not None:
        stack, b, drawn = _augment(case, stack, case["seed"])
        out[name + "_boxes"] = b
    if masks:
        parts = np.split(stack, np.cumsum(counts)[:-1])
        parts = [R_pcd.mask_points_by_range(q, cc.LIDAR_RANGE) for q in parts]
        assert np.array_equal(np.concatenate(parts), R_pcd.mask_points_by_range(stack, cc.LIDAR_RANGE))
        counts, stack = [len(q) for q in parts], np.concatenate(parts)
    ref = stack.astype(np.float32)
    ref_offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    mine, mine_offs, keep, mine_boxes = cc.restated(case)
    assert np.array_equal(ref_offs, mine_offs), "%s: the kept sets differ from the restatement's (%s / %s)" % (name, ref_offs, mine_offs)
    assert np.array_equal(ref[:, 3], mine[:, 3]), "%s: intensity" % name
    frac = 0.0
    if world is None or world.get("rot") is None:
        if masks:
            assert int(ulps32(ref[:, :3], mine[:, :3]).max(initial=0)) <= 1
        else:
            assert np.array_equal(ref, mine), "%s: the restatement is not bit-exact" % name
    else:
        frac = float(np.abs(ref[:, :3].astype(np.float64) - mine[:, :3]).max())          # checked against its bound by the CPU test
    if mine_boxes is not None:
        assert np.array_equal(b[:, 3:], mine_boxes[:, 3:]), "%s: box sizes / headings" % name
        assert np.array_equal(b[cc.VALID_BOXES:], mine_boxes[cc.VALID_BOXES:])
    out[name + "_points"], out[name + "_offsets"], out[name + "_drawn"] = ref, ref_offs, drawn
    out[name + "_proj_diff"] = np.array([proj_diff, proj_total], dtype=np.int64)
    print("%-10s %5d of %5d points kept, offsets %s; projection: %d of %d coordinates one fp32 ulp off; max |ref - mine| %.3e; drew %s"
          % (name, len(ref), sum(len(p) for p in case["clouds"]), ref_offs.tolist(), proj_diff, proj_total, frac, drawn.tolist()))


def main():
    out = {}
    for name in cc.GOLDEN:
        _case(name, out)
    mg.save("gv29_cloud_prep", **out)


if __name__ == "__main__":
    main()
